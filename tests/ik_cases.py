"""The models, entries, targets and seeds shared by tests/test_ik_host.py and tests/test_gpu_ik.py (not product code).  The GPU tests
compare the device with the host build on exactly the problems the CPU tests compare the host build with tests/ik_numpy.py on."""
import ctypes as C
import os
import subprocess

import numpy as np

import nimblephysics_amd as na
from kin_numpy import ROWS
from nimblephysics_amd.mapping import resolve_body

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
B_TEST = 130          # two full wavefronts and a tail of 2
SEED = 4100
ATLAS_REFERENCE_RESIDUAL = 1.533673   # worst per-row residual the reference's solve leaves on Atlas-20's targets (test_ik_host.py measures it)


def _tr(x, y, z):
    T = np.eye(4); T[:3, 3] = (x, y, z); return T


_AXES = [(0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0)]


def arm(k, lengths, limit=None, name="arm"):
    """k revolute links in a chain; a link's body frame sits at its tip (so the last joint moves the last frame's origin)"""
    bodies = []
    for i in range(k):
        kw = {} if limit is None else {"pos_lo": (-limit,), "pos_hi": (limit,)}
        bodies.append(na.BodySpec(f"link{i}", i - 1, "revolute", f"joint{i}", axis=_AXES[i], T_pj=_tr(0, 0, 0.1) if i == 0 else np.eye(4),
                                  T_cj=_tr(-lengths[i], 0.03 * (i % 2), -0.02 * (i % 3)), **kw))
    return na.ModelDescription(f"{name}{k}", bodies, [], max_contacts=0)


def free_ball_tree():
    """free root -> revolute -> ball wrist, and a revolute branch on the root"""
    bodies = [na.BodySpec("root", -1, "free", "root_joint", T_cj=_tr(0.02, -0.03, 0.01)),
              na.BodySpec("upper", 0, "revolute", "shoulder", axis=(0, 1, 0), T_pj=_tr(0.1, 0.2, 0), T_cj=_tr(-0.3, 0, 0.02), pos_lo=(-2.0,), pos_hi=(2.0,)),
              na.BodySpec("wrist", 1, "ball", "wrist_joint", T_pj=_tr(0.05, 0, 0), T_cj=_tr(-0.1, 0.02, 0)),
              na.BodySpec("leg", 0, "revolute", "hip", axis=(1, 0, 0), T_pj=_tr(0, -0.2, 0.05), T_cj=_tr(0, 0.4, 0), pos_lo=(-1.5,), pos_hi=(1.5,))]
    return na.ModelDescription("free_ball_tree", bodies, [], max_contacts=0)


def cases():
    """name -> (model, entries [(kind, body index)])"""
    atlas = na.atlas("atlas20")
    idx = {b.name: i for i, b in enumerate(atlas.bodies)}
    return {
        "arm3_linear": (arm(3, (0.4, 0.3, 0.3)), [(1, 2)]),
        "arm7_spatial": (arm(7, (0.2, 0.15, 0.15, 0.15, 0.12, 0.12, 0.1)), [(0, 6)]),
        "arm2_two_spatial": (arm(2, (0.5, 0.4)), [(0, 0), (0, 1)]),
        "free_ball_tree": (free_ball_tree(), [(0, 2), (2, 3)]),
        "atlas20": (atlas, [(0, idx["pelvis"]), (0, idx["l_foot"]), (0, idx["r_foot"]), (0, idx["l_hand"])]),
    }


def limited_arm3():
    return arm(3, (0.4, 0.3, 0.3), limit=0.3, name="limited_arm")


def random_poses(md, ow, entries, B, seed):
    """[B, n] configurations inside the limits (0.9 of a finite range, N(0, 0.35) on an unlimited coordinate) whose entry rotations stay
    at least 0.3 rad below pi"""
    rng = np.random.default_rng(seed)
    flat = md.flat()
    lo, hi = flat["pos_lo"], flat["pos_hi"]
    fin = np.isfinite(lo) & np.isfinite(hi)
    out = []
    while len(out) < B:
        q = rng.normal(0, 0.35, md.num_dofs)
        u = rng.uniform(-0.9, 0.9, md.num_dofs)
        q[fin] = (0.5 * (lo + hi) + 0.5 * (hi - lo) * u)[fin]
        if all(np.arccos(np.clip(0.5 * (np.trace(ow.body_world_transform(q, e)[:3, :3]) - 1), -1, 1)) < np.pi - 0.3 for _, e in entries):
            out.append(q)
    return np.stack(out)


def load_ik_shim():
    src = os.path.join(HERE, "host_shim", "ik_shim.cpp")
    out = os.path.join(HERE, "host_shim", "libik_shim.so")
    csrc = os.path.join(ROOT, "nimblephysics_amd", "csrc")
    deps = [src, os.path.join(HERE, "host_shim", "model_shim.hpp"), os.path.join(ROOT, "include", "nimble_amd.h")] + [os.path.join(csrc, f) for f in ("ik_dev.hpp", "kinematics_dev.hpp", "spatial_dev.hpp", "model_dev.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", os.path.join(HERE, "host_shim"),
                               "-I", csrc, "-I", os.path.join(ROOT, "include"), "-o", out, src])
    lib = C.CDLL(out)
    vp = C.c_void_p
    lib.shim_ik_model.argtypes = [vp]
    lib.shim_ik_model.restype = vp
    lib.shim_ik_free.argtypes = [vp]
    lib.shim_ik_solve.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp, C.c_int]
    lib.shim_ik_solve.restype = C.c_int
    lib.shim_ik_eval.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp]
    lib.shim_ik_eval.restype = C.c_int
    lib.shim_ik_clamp.argtypes = [vp, C.c_int64, vp]
    lib.shim_ik_clamp.restype = None
    return lib


class CConfig(C.Structure):          # nbl_ik_config
    _fields_ = [("convergence_threshold", C.c_double), ("max_step_count", C.c_int32), ("least_squares_damping", C.c_double),
                ("start_clamped", C.c_int32), ("line_search", C.c_int32), ("dont_exit_transpose", C.c_int32)]


def c_config(max_step_count=100, convergence_threshold=1e-7, least_squares_damping=0.01, start_clamped=False, line_search=True,
             dont_exit_transpose=False):
    return CConfig(convergence_threshold, max_step_count, least_squares_damping, int(start_clamped), int(line_search), int(dont_exit_transpose))


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class HostIK:
    """The host build of csrc/ik_dev.hpp on the entries [(kind, body index of md)] of md.  Arrays are [B, .] here, SoA inside."""

    def __init__(self, lib, md, entries):
        self.lib, self.md, self.entries = lib, md, entries
        dev = md.merge_welds() if md.has_welds() else md
        self.desc, self.keep = dev.to_desc()
        self.h = lib.shim_ik_model(C.addressof(self.desc))
        res = [resolve_body(md, e) for _, e in entries]
        self.kind = np.array([k for k, _ in entries], dtype=np.int32)
        self.body = np.array([r[0] for r in res], dtype=np.int32)
        self.T = np.ascontiguousarray(np.stack([np.concatenate([r[1][:3, :3].reshape(9), r[1][:3, 3]]) for r in res]))
        self.P = sum(ROWS[k] for k, _ in entries)
        self.n = md.num_dofs

    def __del__(self):
        self.lib.shim_ik_free(self.h)

    def solve(self, targets, init=None, threads=1, **cfg):
        """targets [B, P], init [B, n] or None -> (q [B, n], loss [B], steps [B])"""
        t = np.ascontiguousarray(np.asarray(targets, dtype=np.float64).T)
        B = t.shape[1]
        qi = None if init is None else np.ascontiguousarray(np.asarray(init, dtype=np.float64).T)
        q = np.full((self.n, B), np.nan); loss = np.full(B, np.nan); steps = np.zeros(B, dtype=np.int32)
        c = c_config(**cfg)
        P = self.lib.shim_ik_solve(self.h, len(self.entries), _p(self.kind), _p(self.body), _p(self.T), B, _p(t), _p(qi), C.addressof(c), _p(q),
                                   _p(loss), _p(steps), threads)
        assert P == self.P
        return q.T.copy(), loss, steps

    def evaluate(self, q, targets):
        """q [B, n], targets [B, P] -> (diff [B, P], J [B, P, n], err [B])"""
        qs = np.ascontiguousarray(np.asarray(q, dtype=np.float64).T)
        t = np.ascontiguousarray(np.asarray(targets, dtype=np.float64).T)
        B = qs.shape[1]
        diff = np.full((self.P, B), np.nan); J = np.full((self.P * self.n, B), np.nan); err = np.full(B, np.nan)
        self.lib.shim_ik_eval(self.h, len(self.entries), _p(self.kind), _p(self.body), _p(self.T), B, _p(qs), _p(t), _p(diff), _p(J), _p(err))
        return diff.T.copy(), J.T.reshape(B, self.P, self.n).copy(), err

    def clamp(self, q):
        qs = np.ascontiguousarray(np.asarray(q, dtype=np.float64).T)
        self.lib.shim_ik_clamp(self.h, qs.shape[1], _p(qs))
        return qs.T.copy()
