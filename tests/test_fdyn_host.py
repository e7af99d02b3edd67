"""The PRODUCT's forward dynamics and inverse mass matrix (second half of nimblephysics_amd/csrc/dynamics_dev.hpp: the articulated-body
sweeps k_forward_dynamics / k_forward_dynamics_lambda / k_minv_apply run per lane) compiled for the host with g++ -O2 -ffp-contract=off
(tests/host_shim/fdyn_shim.cpp) and checked on every joint type of the device model (the models of tests/test_dynamics_host.py):
  1  FD under NBL_ID_JOINT_FORCES = ow.forward_dynamics(q, v, tau) (the oracle's has the spring and damping terms);
  2  FD without the flag = solve(ow.mass_matrix(q), tau - ow.coriolis_gravity(q, v));
  3  round trips with the host build of inverse dynamics, FD(q, v, ID(q, v, a)) = a and ID(q, v, FD(q, v, tau)) = tau, under every flag
     combination;
  4  Minv M = I, Minv = its transpose bit for bit, inv_mass_apply with R = 3 = Minv @ X;
  5  the reverse pass: grad_tau = lambda = solve(M, g), grad_q = -(jac_Mx(q, a) + jac_C(q, v, 0))^T lambda, grad_v = -jac_C(q, v, 1)^T lambda
     (+ the diagonal joint-force terms under the flag), and against central differences of the shim's own forward pass (eps 1e-6,
     2e-7 max(1, |a|), as tests/test_dynamics_host.py has them for tau);
  6  results do not depend on B or on the lane, bit for bit.

TOLERANCE.  max|x - ref| / max(1, |ref|) <= TOL = 1e-10 as in tests/test_dynamics_host.py, after the check the inverse asks for: M^-1
amplifies rounding by the condition number of M, so the oracle's own two routes to the acceleration (its articulated-body
forward_dynamics against numpy's solve(mass_matrix, tau - C - joint forces)) were compared on the exact inputs of items 1 and 2 - every
model, B = 4, seed 31.  Worst disagreement over all models and worlds: 1.7e-12 (serial_chain_ball_joint, where cond(M) reaches 4.7e5;
every other model is below 5e-14), below 1e-11, so 1e-10 stands.  test_the_oracles_own_two_routes_agree holds the oracle to that figure."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import OracleWorld
from test_dynamics_host import JOINT_FORCES, MODELS, NO_GRAVITY, NO_VELOCITY, ShimDynamics, _draw, _err, _p
from test_dynamics_host import load_shim as load_dyn_shim

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOL = 1e-10
ORACLE_ROUTES_MAX = 1e-11          # measured 1.7e-12: see the head of this file
IDS = [m[0] for m in MODELS]


def load_shim():
    src = os.path.join(HERE, "host_shim", "fdyn_shim.cpp")
    out = os.path.join(HERE, "host_shim", "libfdyn_shim.so")
    csrc = os.path.join(ROOT, "nimblephysics_amd", "csrc")
    deps = [src, os.path.join(HERE, "host_shim", "dyn_shim.cpp"), os.path.join(ROOT, "include", "nimble_amd.h")]
    deps += [os.path.join(csrc, f) for f in ("dynamics_dev.hpp", "kinematics_dev.hpp", "spatial_dev.hpp", "model_dev.hpp")]
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
    lib.shim_fdyn_forward.argtypes = [vp, C.c_int64, vp, vp, C.c_int, vp]
    lib.shim_fdyn_forward.restype = None
    lib.shim_fdyn_backward.argtypes = [vp, C.c_int64, vp, vp, C.c_int, vp, vp, vp, C.c_int]
    lib.shim_fdyn_backward.restype = None
    lib.shim_fdyn_minv.argtypes = [vp, C.c_int64, C.c_int, vp, vp, vp]
    lib.shim_fdyn_minv.restype = None
    return lib


@pytest.fixture(scope="module")
def shim():
    return load_shim()


class ShimForwardDynamics(ShimDynamics):
    """The host build of the forward-dynamics code (and, inherited, of inverse dynamics and the mass matrix) on [2n][B] states."""

    def accel(self, S, T=None, flags=0):
        S = np.ascontiguousarray(S); T = None if T is None else np.ascontiguousarray(T)
        out = np.full((self.n, S.shape[1]), np.nan)
        self.lib.shim_fdyn_forward(self.h, S.shape[1], _p(S), _p(T), flags, _p(out))
        return out

    def fd_vjp(self, S, T, g, flags=0, init=None):
        """(grad_state [2n][B], grad_tau [n][B]); init = (gs, gt): accumulate onto them"""
        S = np.ascontiguousarray(S); T = None if T is None else np.ascontiguousarray(T); g = np.ascontiguousarray(g)
        B = S.shape[1]
        gs = np.full((2 * self.n, B), np.nan) if init is None else init[0].copy()
        gt = np.full((self.n, B), np.nan) if init is None else init[1].copy()
        self.lib.shim_fdyn_backward(self.h, B, _p(S), _p(T), flags, _p(g), _p(gs), _p(gt), 0 if init is None else 1)
        return gs, gt

    def minv(self, S):
        S = np.ascontiguousarray(S)
        out = np.full((self.n * self.n, S.shape[1]), np.nan)
        self.lib.shim_fdyn_minv(self.h, S.shape[1], self.n, _p(S), None, _p(out))
        return out.reshape(self.n, self.n, -1)

    def minv_apply(self, S, X):
        """X [R][n][B] -> M^-1 X"""
        S = np.ascontiguousarray(S); X = np.ascontiguousarray(X)
        out = np.full(X.shape, np.nan)
        self.lib.shim_fdyn_minv(self.h, S.shape[1], X.shape[0], _p(S), _p(X), _p(out))
        return out


def _joint_forces(md, q, v):
    fl = md.flat()
    return fl["damping"] * v + fl["spring"] * (q - fl["rest"] + md.dt * v)


@pytest.mark.parametrize("name,md", MODELS, ids=IDS)
def test_the_oracles_own_two_routes_agree(name, md):
    """What fixes TOL (head of this file): forward_dynamics against solve(mass_matrix, tau - C - joint forces) on the inputs of the next test."""
    ow = OracleWorld(md)
    n, B = md.num_dofs, 4
    S, T, _ = _draw(md, B, 31)
    worst = 0.0
    for b in range(B):
        q, v, tau = S[:n, b], S[n:, b], T[:, b]
        ref = np.linalg.solve(ow.mass_matrix(q), tau - ow.coriolis_gravity(q, v) - _joint_forces(md, q, v))
        worst = max(worst, _err(ow.forward_dynamics(q, v, tau), ref))
    print(name, "oracle forward_dynamics vs solve(M, .):", worst)
    assert worst <= ORACLE_ROUTES_MAX, (name, worst)


@pytest.mark.parametrize("name,md", MODELS, ids=IDS)
def test_forward_dynamics_equals_the_oracle(shim, name, md):
    ow = OracleWorld(md)
    d = ShimForwardDynamics(shim, md)
    n, B = md.num_dofs, 4
    S, T, _ = _draw(md, B, 31)
    a_jf, a, a0 = d.accel(S, T, JOINT_FORCES), d.accel(S, T), d.accel(S, None)
    a_m = d.accel(S, T, NO_VELOCITY | NO_GRAVITY)
    a_nov = d.accel(S, T, NO_VELOCITY)
    for b in range(B):
        q, v, tau = S[:n, b], S[n:, b], T[:, b]
        Mo, Co = ow.mass_matrix(q), ow.coriolis_gravity(q, v)
        e = {"jf": _err(a_jf[:, b], ow.forward_dynamics(q, v, tau)), "plain": _err(a[:, b], np.linalg.solve(Mo, tau - Co)),
             "tau 0": _err(a0[:, b], np.linalg.solve(Mo, -Co)), "M^-1 tau": _err(a_m[:, b], np.linalg.solve(Mo, tau)),
             "no v": _err(a_nov[:, b], np.linalg.solve(Mo, tau - ow.coriolis_gravity(q, 0 * v)))}
        print(name, b, e)
        assert max(e.values()) <= TOL, (name, b, e)


@pytest.mark.parametrize("name,md", MODELS, ids=IDS)
def test_forward_and_inverse_dynamics_are_inverse_functions(shim, name, md):
    d = ShimForwardDynamics(shim, md)
    S, A, _ = _draw(md, 3, 32)
    T = A[::-1].copy()
    for flags in range(8):                                   # every combination of NO_VELOCITY, NO_GRAVITY, JOINT_FORCES
        back = d.accel(S, d.tau(S, A, flags), flags)
        forth = d.tau(S, d.accel(S, T, flags), flags)
        e = {"FD(ID(a))": _err(back, A), "ID(FD(tau))": _err(forth, T)}
        print(name, flags, e)
        assert max(e.values()) <= TOL, (name, flags, e)


@pytest.mark.parametrize("name,md", MODELS, ids=IDS)
def test_inverse_mass_matrix(shim, name, md):
    ow = OracleWorld(md)
    d = ShimForwardDynamics(shim, md)
    n, B = md.num_dofs, 4
    S, _, _ = _draw(md, B, 33)
    X = np.random.default_rng(34).normal(size=(3, n, B))
    Mi, Y = d.minv(S), d.minv_apply(S, X)
    y1 = d.minv_apply(S, X[:1])
    assert np.array_equal(y1[0], Y[0])                       # a right-hand side's bits do not depend on R
    for b in range(B):
        Mo = ow.mass_matrix(S[:n, b])
        assert np.array_equal(Mi[:, :, b], Mi[:, :, b].T), name                    # the same bits in both triangles
        e = {"Minv M": _err(Mi[:, :, b] @ Mo, np.eye(n)), "M Minv": _err(Mo @ Mi[:, :, b], np.eye(n)),
             "Minv": _err(Mi[:, :, b], np.linalg.inv(Mo)), "apply": _err(Y[:, :, b].T, np.linalg.solve(Mo, X[:, :, b].T)),
             "apply vs Minv": _err(Y[:, :, b].T, Mi[:, :, b] @ X[:, :, b].T)}
        print(name, b, e)
        assert max(e.values()) <= TOL, (name, b, e)


@pytest.mark.parametrize("name,md", MODELS, ids=IDS)
def test_the_reverse_pass_equals_the_closed_form_of_the_oracle(shim, name, md):
    ow = OracleWorld(md)
    d = ShimForwardDynamics(shim, md)
    n, B = md.num_dofs, 3
    S, T, g = _draw(md, B, 35)
    fl = md.flat()
    gs, gt = d.fd_vjp(S, T, g)
    gs_jf, gt_jf = d.fd_vjp(S, T, g, JOINT_FORCES)
    gs_m, gt_m = d.fd_vjp(S, T, g, NO_VELOCITY | NO_GRAVITY)
    acc = (np.random.default_rng(1).normal(size=gs.shape), np.random.default_rng(2).normal(size=gt.shape))
    gs_acc, gt_acc = d.fd_vjp(S, T, g, 0, init=acc)
    assert np.abs(gs_acc - (acc[0] + gs)).max() <= 1e-12 * max(1.0, np.abs(gs).max()) and np.abs(gt_acc - (acc[1] + gt)).max() <= 1e-12 * max(1.0, np.abs(gt).max())
    only_t = d.fd_vjp(S, T, g)[1]
    assert np.array_equal(only_t, gt)
    for b in range(B):
        q, v, tau, gb = S[:n, b], S[n:, b], T[:, b], g[:, b]
        Mo, Co = ow.mass_matrix(q), ow.coriolis_gravity(q, v)
        lam = np.linalg.solve(Mo, gb)
        a = np.linalg.solve(Mo, tau - Co)
        a_jf = np.linalg.solve(Mo, tau - Co - _joint_forces(md, q, v))
        a_m = np.linalg.solve(Mo, tau)
        Jq, Jv = ow.jac_C(q, v, 0), ow.jac_C(q, v, 1)
        e = {"tau": _err(gt[:, b], lam), "q": _err(gs[:n, b], -(ow.jac_Mx(q, a) + Jq).T @ lam), "v": _err(gs[n:, b], -Jv.T @ lam),
             "tau jf": _err(gt_jf[:, b], lam), "q jf": _err(gs_jf[:n, b], -(ow.jac_Mx(q, a_jf) + Jq).T @ lam - fl["spring"] * lam),
             "v jf": _err(gs_jf[n:, b], -Jv.T @ lam - (fl["damping"] + md.dt * fl["spring"]) * lam),
             "tau m": _err(gt_m[:, b], lam), "q m": _err(gs_m[:n, b], -ow.jac_Mx(q, a_m).T @ lam)}
        print(name, b, e)
        assert max(e.values()) <= TOL, (name, b, e)
        assert not gs_m[n:, b].any()                                               # v taken as 0: nothing flows to it


@pytest.mark.parametrize("name,md", MODELS, ids=IDS)
def test_the_reverse_pass_equals_central_differences_of_the_forward_pass(shim, name, md):
    d = ShimForwardDynamics(shim, md)
    n = md.num_dofs
    S, T, _ = _draw(md, 2, 36)
    eps = 1e-6
    for flags in (0, JOINT_FORCES):
        for b in range(2):
            s, t = S[:, b], T[:, b]
            scale = max(1.0, np.abs(d.accel(s[:, None], t[:, None], flags)).max())
            # dense Jacobians of the device code: the reverse pass with unit cotangents, n worlds at the same state
            gs, gt = d.fd_vjp(np.repeat(s[:, None], n, 1), np.repeat(t[:, None], n, 1), np.eye(n), flags)
            X = np.concatenate([s, t])
            P = X[:, None] + eps * np.eye(3 * n)
            Q = X[:, None] - eps * np.eye(3 * n)
            fd = (d.accel(P[:2 * n], P[2 * n:], flags) - d.accel(Q[:2 * n], Q[2 * n:], flags)) / (2 * eps)     # [n, 3n]: d a_i / d x_j
            J = np.concatenate([gs, gt]).T                                                                 # row i: cotangent e_i
            print(name, flags, b, np.abs(J - fd).max(), scale)
            assert np.abs(J - fd).max() < 2e-7 * scale, (name, flags, b, np.abs(J - fd).max(), scale)


def test_results_do_not_depend_on_the_batch(shim):
    import nimblephysics_amd as na
    md = na.atlas("atlas20")
    d = ShimForwardDynamics(shim, md)
    n = md.num_dofs
    S, T, g = _draw(md, 5, 3)
    X = np.random.default_rng(4).normal(size=(2, n, 5))
    a, Mi, Y, (gs, gt) = d.accel(S, T), d.minv(S), d.minv_apply(S, X), d.fd_vjp(S, T, g)
    for b in range(5):
        assert np.array_equal(d.accel(S[:, b:b + 1], T[:, b:b + 1])[:, 0], a[:, b])
        assert np.array_equal(d.minv(S[:, b:b + 1])[:, :, 0], Mi[:, :, b])
        assert np.array_equal(d.minv_apply(S[:, b:b + 1], X[:, :, b:b + 1])[:, :, 0], Y[:, :, b])
        one = d.fd_vjp(S[:, b:b + 1], T[:, b:b + 1], g[:, b:b + 1])
        assert np.array_equal(one[0][:, 0], gs[:, b]) and np.array_equal(one[1][:, 0], gt[:, b])
    # the lane: world 0 of S as the last world of a reordered batch
    R = S[:, ::-1].copy()
    assert np.array_equal(d.accel(R, T[:, ::-1].copy())[:, -1], a[:, 0]) and np.array_equal(d.minv(R)[:, :, -1], Mi[:, :, 0])


def test_the_header_still_builds_the_inverse_dynamics_shim():
    """dynamics_dev.hpp serves both shims: the existing one compiles and loads with the forward-dynamics half in the header."""
    assert load_dyn_shim().shim_dyn_slots() == 48
