"""The models, poses, case classes and the tolerance rule shared by tests/test_ik_grad_host.py and tests/test_gpu_ik_grad.py (not product
code).  A problem is (q [B, n], grad_q [B, n]) on a model with entries; its reference is tests/ik_grad_numpy.py on the dense Jacobian the
host build of csrc/ik_dev.hpp gives at q (tests/test_ik_host.py holds that Jacobian to the numpy restatement of the reference).

THE TOLERANCE RULE: on a problem, d = the largest absolute disagreement of the two NumPy forms (|F| x |F| and P x P, numpy.linalg.solve on
each).  The product factors the smaller form with its own summation order and is allowed 10 d from the NumPy result of that same form.
Where every coordinate is clamped both forms are exactly 0, d = 0, and the product must be exactly 0.  Every pose has cond(J_F) <= 1e3
(asserted), so d measures round-off of the two solves and not the conditioning of a pose."""
import ctypes as C
import json
import os
import subprocess

import numpy as np

import ik_cases as ic
import ik_grad_numpy as ign
import nimblephysics_amd as na
from oracle import OracleWorld

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MUS = (1e-9, 1e-2)
COND_MAX = 1e3
SEED = 5200


def load_grad_shim():
    src = os.path.join(HERE, "host_shim", "ik_grad_shim.cpp")
    out = os.path.join(HERE, "host_shim", "libik_grad_shim.so")
    csrc = os.path.join(ROOT, "nimblephysics_amd", "csrc")
    deps = [src, os.path.join(HERE, "host_shim", "model_shim.hpp"), os.path.join(ROOT, "include", "nimble_amd.h")] + \
           [os.path.join(csrc, f) for f in ("ik_grad_dev.hpp", "ik_dev.hpp", "kinematics_dev.hpp", "spatial_dev.hpp", "model_dev.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(HERE, "host_shim"),
                               "-I", csrc, "-I", os.path.join(ROOT, "include"), "-o", out, src])
    lib = C.CDLL(out)
    vp = C.c_void_p
    lib.shim_ikg_model.argtypes = [vp]
    lib.shim_ikg_model.restype = vp
    lib.shim_ikg_free.argtypes = [vp]
    lib.shim_ikg_vjp.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int64, vp, vp, C.c_double, vp, C.c_int, vp]
    lib.shim_ikg_vjp.restype = C.c_int
    return lib


class HostIKGrad(ic.HostIK):
    """The host build of csrc/ik_grad_dev.hpp next to HostIK's solver and Jacobian (two libraries, one model description)."""

    def __init__(self, solver_lib, grad_lib, md, entries):
        super().__init__(solver_lib, md, entries)
        self.glib = grad_lib
        self.gh = grad_lib.shim_ikg_model(C.addressof(self.desc))

    def __del__(self):
        self.glib.shim_ikg_free(self.gh)
        super().__del__()

    def vjp(self, q, grad_q, mu, accumulate_into=None):
        """q, grad_q [B, n] -> (grad_target [B, P], free_count [B])"""
        qs = np.ascontiguousarray(np.asarray(q, dtype=np.float64).T)
        gs = np.ascontiguousarray(np.asarray(grad_q, dtype=np.float64).T)
        B = qs.shape[1]
        out = np.full((self.P, B), np.nan) if accumulate_into is None else np.ascontiguousarray(np.asarray(accumulate_into, dtype=np.float64).T)
        cnt = np.full(B, -1, dtype=np.int32)
        P = self.glib.shim_ikg_vjp(self.gh, len(self.entries), ic._p(self.kind), ic._p(self.body), ic._p(self.T), B, ic._p(qs), ic._p(gs),
                                   float(mu), ic._p(out), 0 if accumulate_into is None else 1, ic._p(cnt))
        assert P == self.P
        return out.T.copy(), cnt


def _json_model(name):
    return na.ModelDescription.from_json(json.load(open(os.path.join(ROOT, "nimblephysics_amd", "data", name + ".json"))))


def models():
    """name -> (model, entries [(kind, body index)]): P = n, P < n (redundant), P > n (over-determined), with and without limits"""
    base = ic.cases()
    return {
        "arm3_linear": base["arm3_linear"],                                                                         # P = n = 3, no limits
        "limited_arm3": (ic.limited_arm3(), [(1, 2)]),                                                              # P = n = 3, every coordinate limited
        "arm7_spatial": base["arm7_spatial"],                                                                       # P = 6 < n = 7, no limits
        "limited_arm7": (ic.arm(7, (0.2, 0.15, 0.15, 0.15, 0.12, 0.12, 0.1), limit=1.2, name="limited_arm"), [(0, 6)]),   # P = 6 < n = 7, limited
        "arm2_two_spatial": base["arm2_two_spatial"],                                                               # P = 12 > n = 2
        "free_ball_tree": base["free_ball_tree"],                                                                   # P = 9 < n = 11, free + ball joints
        "atlas20": base["atlas20"],                                                                                 # P = 24 > n = 20
    }


def limited_pendulum():
    """the pendulum with its coordinate limited to [-1, 1], so that the clamped classes exist on it"""
    md = na.single_pendulum()
    md.bodies[0].pos_lo, md.bodies[0].pos_hi = (-1.0,), (1.0,)
    return md


def device_models():
    """the three models of the device test: the pendulum, a chain of ball joints, Atlas-20 with two spatial entries"""
    atlas = na.atlas("atlas20")
    idx = {b.name: i for i, b in enumerate(atlas.bodies)}
    chain = _json_model("serial_chain_ball_joint")
    return {
        "pendulum": (limited_pendulum(), [(0, 0)]),                                     # P = 6 > n = 1, limited
        "ball_chain": (chain, [(0, len(chain.bodies) - 1), (1, len(chain.bodies) // 2)]),   # P = 9 < n = 30
        "atlas20_two": (atlas, [(0, idx["l_foot"]), (0, idx["l_hand"])]),               # P = 12 < n = 20
    }


def limits(md):
    flat = md.flat()
    return np.asarray(flat["pos_lo"], dtype=np.float64), np.asarray(flat["pos_hi"], dtype=np.float64)


def case_classes(md, P):
    """The classes a model can show: 'interior' always; 'one_at_limit' with a finite limit; 'all_at_limit' when every limit is finite;
    'fewer_free_than_rows' (|F| < P <= n through clamping) when P <= n and enough coordinates have limits."""
    lo, hi = limits(md)
    fin = np.isfinite(lo) | np.isfinite(hi)
    n = md.num_dofs
    out = ["interior"]
    if fin.any():
        out.append("one_at_limit")
    if fin.all():
        out.append("all_at_limit")
    if P <= n and fin.sum() >= n - P + 1 and P > 1:
        out.append("fewer_free_than_rows")
    return out


def clamp_pattern(md, P, cls, b, dead=()):
    """indices of the coordinates world b of class `cls` puts on a limit, and which side (True: upper).  `dead`: coordinates no entry
    depends on (zero columns of J); 'fewer_free_than_rows' clamps those first, since one left free would make J_F singular."""
    lo, hi = limits(md)
    cand = np.flatnonzero(np.isfinite(lo) | np.isfinite(hi))
    n = md.num_dofs
    if cls == "interior":
        pick = cand[:0]
    elif cls == "one_at_limit":
        pick = cand[[b % len(cand)]]
    elif cls == "all_at_limit":
        pick = cand
    else:
        k = n - P + 1                                    # leaves |F| = P - 1
        first = np.array([j for j in cand if j in set(dead)], dtype=cand.dtype)
        rest = np.array([j for j in cand if j not in set(dead)], dtype=cand.dtype)
        assert len(first) <= k
        pick = np.concatenate([first, np.roll(rest, -(b % max(len(rest), 1)))])[:k]
    side = np.array([(b + int(j)) % 2 == 0 for j in pick], dtype=bool)
    side = np.where(np.isfinite(hi[pick]), side, False)
    side = np.where(np.isfinite(lo[pick]), side, True)
    return pick, side


def problem(host, md, entries, cls, B, seed):
    """(q [B, n], grad_q [B, n]) of class `cls` with cond(J_F) <= COND_MAX in every world: random poses inside the limits
    (ik_cases.random_poses), the class's coordinates put exactly on their limits, poses above the bound drawn again."""
    lo, hi = limits(md)
    ow = OracleWorld(md)
    rng = np.random.default_rng(seed)
    qs = []
    draw = 0
    J0 = host.evaluate(ic.random_poses(md, ow, entries, 1, seed + 7), np.zeros((1, host.P)))[1][0]
    dead = [int(j) for j in np.flatnonzero(~J0.any(0))]
    while len(qs) < B:
        assert draw < 40, "no well-conditioned poses found"
        pool = ic.random_poses(md, ow, entries, 2 * B, seed + 1000 * draw)
        draw += 1
        for q in pool:
            b = len(qs)
            if b == B:
                break
            pick, side = clamp_pattern(md, host.P, cls, b, dead)
            q = q.copy()
            q[pick] = np.where(side, hi[pick], lo[pick])
            free = ign.free_set(q, lo, hi)
            if free.any():
                J = host.evaluate(q[None], np.zeros((1, host.P)))[1][0]
                s = np.linalg.svd(J[:, free], compute_uv=False)
                if not (s[-1] > 0 and s[0] / s[-1] <= COND_MAX):
                    continue
            qs.append(q)
    q = np.stack(qs)
    return q, rng.normal(0, 1, q.shape)


def reference(host, md, q, g, mu):
    """-> (the NumPy result of the form the product factors [B, P], d of the tolerance rule, free_count [B], worst cond(J_F))"""
    lo, hi = limits(md)
    J = host.evaluate(q, np.zeros((len(q), host.P)))[1]
    pr, du, cnt, cond = ign.vjp_batch(J, g, q, lo, hi, mu)
    assert (cond <= COND_MAX).all(), cond.max()
    small = np.where((host.P < cnt)[:, None], du, pr)       # P < |F|: the P x P form, else the |F| x |F| one (csrc/ik_grad_dev.hpp)
    return small, float(np.abs(pr - du).max()), cnt, float(cond.max())
