"""The PRODUCT's joint-space dynamics (nimblephysics_amd/csrc/dynamics_dev.hpp: recursive Newton-Euler inverse dynamics, its reverse pass
and the composite-rigid-body mass matrix - the code k_inverse_dynamics / k_inverse_dynamics_vjp / k_mass_matrix run per lane) compiled
for the host with g++ -O2 -ffp-contract=off (tests/host_shim/dyn_shim.cpp) and checked on every joint type of the device model against
the CPU oracle's mass_matrix, coriolis_gravity, forward_dynamics, jac_C and jac_Mx:
  1  M = ow.mass_matrix(q), bitwise symmetric;  2  C = ow.coriolis_gravity(q, v);  3  tau = M a + C;
  4  with joint forces, tau fed to ow.forward_dynamics reproduces a (compared in force space like tests/test_ball_joint.py:76-80, 1e-10);
  5  the reverse pass: grad_q = (jac_Mx(q, a) + jac_C(q, v, 0))^T g, grad_v = jac_C(q, v, 1)^T g (+ the diagonal joint-force terms),
     grad_a = M^T g;
  6  the reverse pass against central differences of the shim's own forward pass (eps 1e-6, 2e-7 max(1, |C|), tests/test_ball_joint.py:81-85).
Items 1 - 3 and 5 are held to max|x - ref| / max(1, |ref|) <= 1e-10 (both sides are fp64 recursions of the same depth).
Positions are N(0, 0.5^2) (rotation-vector coordinates stay at sigma <= 0.6), velocities N(0, 1), accelerations N(0, 2^2)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nimblephysics_amd as na
from oracle import OracleWorld
from util import rel_err

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NO_VELOCITY, NO_GRAVITY, JOINT_FORCES = 1, 2, 4          # NBL_ID_* of include/nimble_amd.h
TOL = 1e-10


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def load_shim():
    src = os.path.join(HERE, "host_shim", "dyn_shim.cpp")
    out = os.path.join(HERE, "host_shim", "libdyn_shim.so")
    csrc = os.path.join(ROOT, "nimblephysics_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "nimble_amd.h")] + [os.path.join(csrc, f) for f in ("dynamics_dev.hpp", "kinematics_dev.hpp", "spatial_dev.hpp", "model_dev.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(HERE, "host_shim"),
                               "-I", csrc, "-I", os.path.join(ROOT, "include"), "-o", out, src])
    lib = C.CDLL(out)
    vp = C.c_void_p
    lib.shim_dyn_model.argtypes = [vp]
    lib.shim_dyn_model.restype = vp
    lib.shim_dyn_free.argtypes = [vp]
    lib.shim_dyn_run.argtypes = [vp, C.c_int64, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp]
    lib.shim_dyn_run.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class ShimDynamics:
    """The host build of the device code on [2n][B] states of the model `md`."""

    def __init__(self, lib, md):
        self.lib, self.md = lib, md
        dev = md.merge_welds() if md.has_welds() else md
        self.desc, self.keep = dev.to_desc()
        self.h = lib.shim_dyn_model(C.addressof(self.desc))
        self.n = md.num_dofs

    def __del__(self):
        self.lib.shim_dyn_free(self.h)

    def tau(self, S, A=None, flags=0):
        S = np.ascontiguousarray(S); A = None if A is None else np.ascontiguousarray(A)
        out = np.full((self.n, S.shape[1]), np.nan)
        self.lib.shim_dyn_run(self.h, S.shape[1], _p(S), _p(A), flags, _p(out), None, None, None, 0, None)
        return out

    def vjp(self, S, A, g, flags=0, init=None):
        """(grad_state [2n][B], grad_accel [n][B]); init = (gs, ga): accumulate onto them"""
        S = np.ascontiguousarray(S); A = None if A is None else np.ascontiguousarray(A); g = np.ascontiguousarray(g)
        B = S.shape[1]
        gs = np.full((2 * self.n, B), np.nan) if init is None else init[0].copy()
        ga = np.full((self.n, B), np.nan) if init is None else init[1].copy()
        self.lib.shim_dyn_run(self.h, B, _p(S), _p(A), flags, None, _p(g), _p(gs), _p(ga), 0 if init is None else 1, None)
        return gs, ga

    def mass(self, S):
        S = np.ascontiguousarray(S)
        M = np.full((self.n * self.n, S.shape[1]), np.nan)
        self.lib.shim_dyn_run(self.h, S.shape[1], _p(S), None, 0, None, None, None, None, 0, _p(M))
        return M.reshape(self.n, self.n, -1)


def free_below_root(seed=0):
    """revolute root -> FREE joint -> revolute -> ball, and a prismatic branch on the free-jointed body"""
    from test_ball_joint import _T
    rng = np.random.default_rng(700 + seed)

    def body(name, parent, jt, **kw):
        A = rng.normal(size=(3, 3)); I = A @ A.T * 0.02 + 0.03 * np.eye(3)
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        return na.BodySpec(name, parent, jt, name + "_joint", axis=tuple(ax), T_pj=_T(rng, 0.25), T_cj=_T(rng, 0.1), mass=float(rng.uniform(0.5, 2.0)),
                           com=tuple(rng.normal(0, 0.04, 3)), inertia=(I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]), **kw)
    bodies = [body("base", -1, "revolute", damping=(0.3,)), body("floater", 0, "free", damping=tuple(rng.uniform(0.1, 1, 6)), spring=tuple(rng.uniform(0.5, 2, 6)), rest=tuple(rng.normal(0, 0.1, 6))),
              body("arm", 1, "revolute"), body("wrist", 2, "ball", spring=(1.0, 2.0, 0.5)), body("slider", 1, "prismatic")]
    return na.ModelDescription("free_below_root", bodies, [], gravity=(0.3, -9.81, 0.2), dt=1e-3, max_contacts=0)


def _models():
    from test_ball_joint import ball_model
    from test_kinematics_host import MODELS as KIN_MODELS
    out = list(KIN_MODELS)                          # pendulum, cartpole, Atlas-20 / -33, the ball-joint files, box_stack, the compound-joint skel, screws, random trees
    out += [("ball_arm", ball_model(2, True)), ("ball_arm_fixed_root", ball_model(2, False)), ("free_below_root", free_below_root())]
    return out


MODELS = _models()


def _draw(md, B, seed):
    rng = np.random.default_rng(seed)
    n = md.num_dofs
    return np.concatenate([rng.normal(0, 0.5, (n, B)), rng.normal(0, 1.0, (n, B))]), rng.normal(0, 2.0, (n, B)), rng.normal(0, 1.0, (n, B))


def _err(x, ref):
    return float(np.abs(x - ref).max() / max(1.0, np.abs(ref).max()))


def test_the_models_cover_every_joint_type_of_the_device_model():
    kinds = set()
    for _, md in MODELS:
        dev = md.merge_welds() if md.has_welds() else md
        for b in dev.bodies:
            kinds.add(("free_below_root" if b.parent >= 0 else "free_root") if b.joint_type == "free" else b.joint_type)
    assert {"revolute", "prismatic", "screw", "ball", "free_root", "free_below_root"} <= kinds, kinds


@pytest.mark.parametrize("name,md", MODELS, ids=[m[0] for m in MODELS])
def test_mass_matrix_coriolis_and_inverse_dynamics_equal_the_oracle(shim, name, md):
    ow = OracleWorld(md)
    d = ShimDynamics(shim, md)
    n, B = md.num_dofs, 4
    S, A, _ = _draw(md, B, 21)
    fl = md.flat()
    M = d.mass(S)
    Cv = d.tau(S, None)
    tau = d.tau(S, A)
    tau_jf = d.tau(S, A, JOINT_FORCES)
    C_nog = d.tau(S, None, NO_GRAVITY | NO_VELOCITY)
    Ma = d.tau(S, A, NO_GRAVITY | NO_VELOCITY)
    assert not C_nog.any()
    for b in range(B):
        q, v, a = S[:n, b], S[n:, b], A[:, b]
        Mo, Co = ow.mass_matrix(q), ow.coriolis_gravity(q, v)
        assert np.array_equal(M[:, :, b], M[:, :, b].T), name                      # the same bits in both triangles
        e = {"M": _err(M[:, :, b], Mo), "C": _err(Cv[:, b], Co), "tau": _err(tau[:, b], Mo @ a + Co), "M a": _err(Ma[:, b], Mo @ a)}
        print(name, b, e)
        assert max(e.values()) <= TOL, (name, b, e)
        # joint forces: tau reproduces a in the oracle's forward dynamics (the step's right-hand side), compared in force space
        qdd = ow.forward_dynamics(q, v, tau_jf[:, b])
        rhs = tau_jf[:, b] - Co - fl["damping"] * v - fl["spring"] * (q - fl["rest"] + md.dt * v)
        assert rel_err(Mo @ qdd, rhs) < 1e-10, (name, b)
        assert rel_err(Mo @ a, rhs) < 1e-10, (name, b)


@pytest.mark.parametrize("name,md", MODELS, ids=[m[0] for m in MODELS])
def test_the_reverse_pass_equals_the_oracles_jacobians(shim, name, md):
    ow = OracleWorld(md)
    d = ShimDynamics(shim, md)
    n, B = md.num_dofs, 3
    S, A, g = _draw(md, B, 22)
    fl = md.flat()
    gs, ga = d.vjp(S, A, g)
    gs_jf, ga_jf = d.vjp(S, A, g, JOINT_FORCES)
    gs_m, ga_m = d.vjp(S, A, g, NO_VELOCITY | NO_GRAVITY)
    gs_c, _ = d.vjp(S, None, g)
    acc = (np.random.default_rng(1).normal(size=gs.shape), np.random.default_rng(2).normal(size=ga.shape))
    gs_acc, ga_acc = d.vjp(S, A, g, 0, init=acc)
    assert np.abs(gs_acc - (acc[0] + gs)).max() <= 1e-12 * max(1.0, np.abs(gs).max()) and np.abs(ga_acc - (acc[1] + ga)).max() <= 1e-12 * max(1.0, np.abs(ga).max())
    for b in range(B):
        q, v, a, gb = S[:n, b], S[n:, b], A[:, b], g[:, b]
        Jq, Jv, JM, Mo = ow.jac_C(q, v, 0), ow.jac_C(q, v, 1), ow.jac_Mx(q, a), ow.mass_matrix(q)
        e = {"q": _err(gs[:n, b], (JM + Jq).T @ gb), "v": _err(gs[n:, b], Jv.T @ gb), "a": _err(ga[:, b], Mo.T @ gb),
             "q jf": _err(gs_jf[:n, b], (JM + Jq).T @ gb + fl["spring"] * gb),
             "v jf": _err(gs_jf[n:, b], Jv.T @ gb + (fl["damping"] + md.dt * fl["spring"]) * gb), "a jf": _err(ga_jf[:, b], Mo.T @ gb),
             "Mx q": _err(gs_m[:n, b], JM.T @ gb), "C q": _err(gs_c[:n, b], Jq.T @ gb), "C v": _err(gs_c[n:, b], Jv.T @ gb)}
        print(name, b, e)
        assert max(e.values()) <= TOL, (name, b, e)
        assert not gs_m[n:, b].any()                                               # v taken as 0: nothing flows to it


@pytest.mark.parametrize("name,md", MODELS, ids=[m[0] for m in MODELS])
def test_the_reverse_pass_equals_central_differences_of_the_forward_pass(shim, name, md):
    d = ShimDynamics(shim, md)
    n = md.num_dofs
    S, A, _ = _draw(md, 2, 23)
    eps = 1e-6
    for flags in (0, JOINT_FORCES):
        for b in range(2):
            s, a = S[:, b], A[:, b]
            scale = max(1.0, np.abs(d.tau(s[:, None], None)).max())
            # dense Jacobians of the device code: the reverse pass with unit cotangents, n worlds at the same state
            gs, ga = d.vjp(np.repeat(s[:, None], n, 1), np.repeat(a[:, None], n, 1), np.eye(n), flags)
            X = np.concatenate([s, a])
            P = X[:, None] + eps * np.eye(3 * n)
            Q = X[:, None] - eps * np.eye(3 * n)
            fd = (d.tau(P[:2 * n], P[2 * n:], flags) - d.tau(Q[:2 * n], Q[2 * n:], flags)) / (2 * eps)       # [n, 3n]: d tau_i / d x_j
            J = np.concatenate([gs, ga]).T                                                                 # row i: cotangent e_i
            assert np.abs(J - fd).max() < 2e-7 * scale, (name, flags, b, np.abs(J - fd).max())


def test_results_do_not_depend_on_the_batch(shim):
    md = na.atlas("atlas20")
    d = ShimDynamics(shim, md)
    S, A, g = _draw(md, 5, 3)
    tau, M, (gs, ga) = d.tau(S, A), d.mass(S), d.vjp(S, A, g)
    for b in range(5):
        assert np.array_equal(d.tau(S[:, b:b + 1], A[:, b:b + 1])[:, 0], tau[:, b])
        assert np.array_equal(d.mass(S[:, b:b + 1])[:, :, 0], M[:, :, b])
        one = d.vjp(S[:, b:b + 1], A[:, b:b + 1], g[:, b:b + 1])
        assert np.array_equal(one[0][:, 0], gs[:, b]) and np.array_equal(one[1][:, 0], ga[:, b])
