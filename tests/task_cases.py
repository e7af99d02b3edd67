"""The models, entries, states and the host build shared by tests/test_taskspace_host.py and tests/test_gpu_taskspace.py (not product code).

  screw_chain   revolute -> prismatic -> screw (random joint frames on both sides) and a `tip` welded to the last body at an offset.
                Entries: spatial on the last body, linear on the tip (a linear entry with a non-zero offset), angular on the last body,
                linear on the FIRST body (its columns of the two later coordinates are zero).
  free_ball     free root -> ball -> revolute: the Sdot v terms.  Entries: spatial on the last body, linear on the ball-jointed body,
                angular on the root.
  atlas20       a spatial entry on each foot, a linear entry on the pelvis.
States: |q| <= 1, |v| <= 2, |a| <= 5, uniform; the rotation vectors of ball and free joints have |theta| <= sqrt(3) < 2."""
import ctypes as C
import os
import subprocess

import numpy as np

import nimblephysics_amd as na
import task_numpy
from nimblephysics_amd.mapping import resolve_body

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SPATIAL, LINEAR, ANGULAR = 0, 1, 2
B_MAX = 130           # two full wavefronts and a tail of 2; the smaller batches are its first worlds
SEED = 5200


def screw_chain():
    from test_ball_joint import _T
    rng = np.random.default_rng(SEED)

    def body(name, parent, jt, **kw):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        return na.BodySpec(name, parent, jt, name + "_joint", axis=tuple(ax), T_pj=_T(rng, 0.25), T_cj=_T(rng, 0.1), mass=1.0, **kw)
    bodies = [body("base", -1, "revolute"), body("slide", 0, "prismatic"), body("bolt", 1, "screw", pitch=0.4),
              na.BodySpec("tip", 2, "weld", "tip_joint", T_pj=_T(rng, 0.3), mass=0.1)]
    return na.ModelDescription("screw_chain", bodies, [], max_contacts=0)


def free_ball():
    from test_ball_joint import _T
    rng = np.random.default_rng(SEED + 1)

    def body(name, parent, jt):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        root = parent < 0
        return na.BodySpec(name, parent, jt, name + "_joint", axis=tuple(ax) if jt == "revolute" else (0.0, 0.0, 1.0),
                           T_pj=np.eye(4) if root else _T(rng, 0.25), T_cj=_T(rng, 0.1), mass=1.0)
    return na.ModelDescription("free_ball", [body("root", -1, "free"), body("upper", 0, "ball"), body("fore", 1, "revolute")], [], max_contacts=0)


def cases():
    """name -> (model, entries [(kind, body index of the model)])"""
    atlas = na.atlas("atlas20")
    idx = {b.name: i for i, b in enumerate(atlas.bodies)}
    return {"screw_chain": (screw_chain(), [(SPATIAL, 2), (LINEAR, 3), (ANGULAR, 2), (LINEAR, 0)]),
            "free_ball": (free_ball(), [(SPATIAL, 2), (LINEAR, 1), (ANGULAR, 0)]),
            "atlas20": (atlas, [(SPATIAL, idx["l_foot"]), (SPATIAL, idx["r_foot"]), (LINEAR, idx["pelvis"])])}


def rows(entries):
    return sum(task_numpy.ROWS[k] for k, _ in entries)


def zero_mask(md, entries):
    """[R, n] bool: the coordinate moves no ancestor of the row's body - that entry of J and Jdot is zero by structure"""
    m = task_numpy.Model(md)
    out = []
    for k, i in entries:
        own = {d for c in m.ancestors(i) for d in range(m.off[c], m.off[c] + task_numpy.NDOF[m.jt[c]])}
        out += [[d not in own for d in range(m.n)]] * task_numpy.ROWS[k]
    return np.array(out, dtype=bool)


def numpy_entries(entries):
    return [(k, i, None) for k, i in entries]


def states(md, B, seed=SEED):
    """(q, v, a) [B, n] each"""
    rng = np.random.default_rng(seed)
    n = md.num_dofs
    return rng.uniform(-1, 1, (B, n)), rng.uniform(-2, 2, (B, n)), rng.uniform(-5, 5, (B, n))


def err(x, ref):
    """per world: max |x - ref| / max(1, |ref|) over everything but the leading dimension"""
    ax = tuple(range(1, np.ndim(ref)))
    return np.abs(x - ref).max(axis=ax) / np.maximum(1.0, np.abs(ref).max(axis=ax))


# ---- the host build of csrc/taskspace_dev.hpp ----------------------------------------------------------------------------------------------
def _build(out, src, extra=()):
    csrc = os.path.join(ROOT, "nimblephysics_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "nimble_amd.h")] + \
        [os.path.join(HERE, "host_shim", f) for f in ("task_shim.cpp", "wrench_shim.cpp", "fdyn_shim.cpp", "dyn_shim.cpp")] + \
        [os.path.join(csrc, f) for f in ("taskspace_dev.hpp", "sensors_dev.hpp", "centroidal_dev.hpp", "dynamics_dev.hpp", "kinematics_dev.hpp",
                                         "spatial_dev.hpp", "model_dev.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", *extra, "-I", os.path.join(HERE, "host_shim"), "-I", csrc,
                               "-I", os.path.join(ROOT, "include"), "-o", out, src])


def load_shim():
    out = os.path.join(HERE, "host_shim", "libtask_shim.so")
    _build(out, os.path.join(HERE, "host_shim", "task_shim.cpp"), ("-shared",))
    lib = C.CDLL(out)
    vp, i64, ci = C.c_void_p, C.c_int64, C.c_int
    lib.shim_dyn_model.argtypes = [vp]
    lib.shim_dyn_model.restype = vp
    lib.shim_dyn_free.argtypes = [vp]
    lib.shim_task_set.argtypes = [vp, ci, vp, vp, vp]
    lib.shim_task_set.restype = vp
    lib.shim_wrench_set_free.argtypes = [vp]
    lib.shim_task_rows.argtypes = [vp]
    lib.shim_task_rows.restype = ci
    lib.shim_task_jacobian.argtypes = [vp, vp, i64, vp, vp, vp]
    lib.shim_task_jacobian.restype = None
    lib.shim_task_jacobian_vjp.argtypes = [vp, vp, i64, vp, vp, vp, ci]
    lib.shim_task_jacobian_vjp.restype = None
    lib.shim_task_accel.argtypes = [vp, vp, i64, vp, vp, vp]
    lib.shim_task_accel.restype = None
    lib.shim_task_accel_vjp.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, ci]
    lib.shim_task_accel_vjp.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _soa(x):
    """[B, ...] -> [prod(...)][B], contiguous"""
    return None if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(x.shape[0], -1).T)


class ShimTask:
    """The host build of the device code for the entries of md, resolved as IKMapping resolves them.  Takes and returns [B, ...] arrays."""

    def __init__(self, lib, md, entries):
        from test_dynamics_host import ShimDynamics
        self.lib, self.dyn = lib, ShimDynamics(lib, md)
        self.h, self.n, self.R = self.dyn.h, md.num_dofs, rows(entries)
        res = [resolve_body(md, i) for _, i in entries]
        kind = np.array([k for k, _ in entries], dtype=np.int32)
        body = np.array([mb for mb, _ in res], dtype=np.int32)
        T = np.ascontiguousarray(np.stack([np.concatenate([t[:3, :3].reshape(9), t[:3, 3]]) for _, t in res]), dtype=np.float64)
        self.set = lib.shim_task_set(self.h, len(entries), _p(kind), _p(body), _p(T))
        assert lib.shim_task_rows(self.set) == self.R

    def __del__(self):
        self.lib.shim_wrench_set_free(self.set)

    def _mat(self, q, v, which):
        S = _soa(np.concatenate([q, v], 1))
        out = np.full((self.R * self.n, q.shape[0]), np.nan)            # NaN: an entry the code does not write shows
        self.lib.shim_task_jacobian(self.h, self.set, q.shape[0], _p(S), _p(out) if which == 0 else None, _p(out) if which == 1 else None)
        return out.T.reshape(q.shape[0], self.R, self.n)

    def jacobian(self, q):
        return self._mat(q, np.zeros_like(q), 0)

    def jacobian_deriv(self, q, v):
        return self._mat(q, v, 1)

    def jacobian_vjp(self, q, G):
        S, Gs = _soa(np.concatenate([q, np.zeros_like(q)], 1)), _soa(G)
        gq = np.full((self.n, q.shape[0]), np.nan)
        self.lib.shim_task_jacobian_vjp(self.h, self.set, q.shape[0], _p(S), _p(Gs), _p(gq), 0)
        return gq.T.copy()

    def accel(self, q, v, a=None):
        S, A = _soa(np.concatenate([q, v], 1)), _soa(a)
        out = np.full((self.R, q.shape[0]), np.nan)
        self.lib.shim_task_accel(self.h, self.set, q.shape[0], _p(S), _p(A), _p(out))
        return out.T.copy()

    def accel_vjp(self, q, v, a, cot):
        """(g_q, g_v, g_a or None) [B, n]"""
        S, A, g = _soa(np.concatenate([q, v], 1)), _soa(a), _soa(cot)
        gs = np.full((2 * self.n, q.shape[0]), np.nan)
        ga = None if a is None else np.full((self.n, q.shape[0]), np.nan)
        self.lib.shim_task_accel_vjp(self.h, self.set, q.shape[0], _p(S), _p(A), _p(g), _p(gs), _p(ga), 0)
        return gs[:self.n].T.copy(), gs[self.n:].T.copy(), None if ga is None else ga.T.copy()
