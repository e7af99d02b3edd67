"""The PRODUCT's wrench code (nimblephysics_amd/csrc/dynamics_dev.hpp: inverse and forward dynamics with wrenches on body frames, their
reverse passes and contact inverse dynamics - the code k_inverse_dynamics_wrench, k_inverse_dynamics_wrench_vjp, k_forward_dynamics_wrench,
k_forward_dynamics_wrench_lambda and k_contact_inverse_dynamics run per lane) compiled for the host with g++ -O2 -ffp-contract=off
(tests/host_shim/wrench_shim.cpp) and checked on every model of test_dynamics_host.MODELS, i.e. on every joint type of the device model.

The reference for tau_ext = sum_e J_e^T W_e is built from code older than the wrench calls only: the world Jacobian of kin_numpy.body_jacobians
moved to the entry's origin, OracleWorld.body_world_transform for the frames, and the oracle's M a + C for the plain inverse dynamics.
  1  tau_wrench = tau_plain - J_vel^T W_world in both frames of expression (1e-10 of max(1, |ref|), the bound test_dynamics_host.py holds
     the same recursions to);
  2  forward dynamics of that tau with the same wrenches returns a (compared in force space, 1e-10, as item 4 there);
  3  grad_wrench = -J g against the same numpy Jacobian, grad_state and grad_accel against central differences of the shim's own forward
     pass (eps 1e-6, 2e-7 max(1, |C|), as item 6 there), in both frames - the world frame is the one with a new position term; the reverse
     pass of forward dynamics likewise;
  4  a set without entries and an all-zero wrench array give the wrench-free results bit for bit;
  5  contact inverse dynamics against tests/cid_numpy.py, the numpy restatement of Skeleton.cpp:9705-9949.
Every set has 2 - 3 entries on distinct bodies where the model has that many, one of them with an offset frame that is not the identity.

THE TOLERANCE OF ITEM 5 is measured, not chosen: on these very inputs the restatement's route (lstsq / the QR solve of the KKT matrix) and
the normal-equations closed form of the same answer disagree by at most 5.3e-14 relative to max(1, |ref|) (wrenches and torques)
over all models, sets, modes and worlds below (printed by the test; the device code is within 3.7e-14 of the restatement).  The kernel is a third route of the same conditioning (an LDL^T of
A D A^T), so it is held to 100 x that measured disagreement per case, floored at 1e-12.  cond(A A^T) stays below 1e8 for every drawn
world (asserted; the largest is about 6): no world is left out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nimblephysics_amd as na
from cid_numpy import contact_inverse_dynamics, multiple_contact_inverse_dynamics, multiple_contact_inverse_dynamics_normal
from kin_numpy import body_jacobians, dof_offsets
from nimblephysics_amd.mapping import resolve_body
from oracle import OracleWorld
from test_dynamics_host import MODELS, ShimDynamics, _draw, _err
from util import rel_err

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
JOINT_FORCES, WORLD = 4, 8                               # NBL_ID_JOINT_FORCES, NBL_WRENCH_WORLD
SINGLE, NEAREST, MIN_TORQUE = 0, 1, 2                    # NBL_CID_*
TOL = 1e-10


def load_shim():
    src = os.path.join(HERE, "host_shim", "wrench_shim.cpp")
    out = os.path.join(HERE, "host_shim", "libwrench_shim.so")
    csrc = os.path.join(ROOT, "nimblephysics_amd", "csrc")
    deps = [src, os.path.join(HERE, "host_shim", "dyn_shim.cpp"), os.path.join(HERE, "host_shim", "fdyn_shim.cpp"), os.path.join(ROOT, "include", "nimble_amd.h")] + \
        [os.path.join(csrc, f) for f in ("dynamics_dev.hpp", "kinematics_dev.hpp", "spatial_dev.hpp", "model_dev.hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(HERE, "host_shim"),
                               "-I", csrc, "-I", os.path.join(ROOT, "include"), "-o", out, src])
    lib = C.CDLL(out)
    vp, i64, ci = C.c_void_p, C.c_int64, C.c_int
    lib.shim_dyn_model.argtypes = [vp]
    lib.shim_dyn_model.restype = vp
    lib.shim_dyn_free.argtypes = [vp]
    lib.shim_dyn_run.argtypes = [vp, i64, vp, vp, ci, vp, vp, vp, vp, ci, vp]
    lib.shim_dyn_run.restype = None
    lib.shim_fdyn_forward.argtypes = [vp, i64, vp, vp, ci, vp]
    lib.shim_fdyn_forward.restype = None
    lib.shim_wrench_set.argtypes = [vp, ci, vp, vp]
    lib.shim_wrench_set.restype = vp
    lib.shim_wrench_set_free.argtypes = [vp]
    lib.shim_wrench_id.argtypes = [vp, vp, i64, vp, vp, vp, ci, vp]
    lib.shim_wrench_id.restype = None
    lib.shim_wrench_id_vjp.argtypes = [vp, vp, i64, vp, vp, vp, ci, vp, vp, vp, vp, ci]
    lib.shim_wrench_id_vjp.restype = None
    lib.shim_wrench_fd.argtypes = [vp, vp, i64, vp, vp, vp, ci, vp]
    lib.shim_wrench_fd.restype = None
    lib.shim_wrench_fd_vjp.argtypes = [vp, vp, i64, vp, vp, vp, ci, vp, vp, vp, vp, ci]
    lib.shim_wrench_fd_vjp.restype = None
    lib.shim_wrench_cid_root.argtypes = [vp, vp]
    lib.shim_wrench_cid_root.restype = ci
    lib.shim_wrench_cid.argtypes = [vp, vp, i64, vp, vp, vp, ci, ci, vp, vp]
    lib.shim_wrench_cid.restype = None
    return lib


@pytest.fixture(scope="module")
def shim():
    return load_shim()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


class ShimWrench(ShimDynamics):
    """The host build of the device code with the wrench set `entries` = [(body index of md, frame in that body, 4 x 4)]."""

    def __init__(self, lib, md, entries):
        super().__init__(lib, md)
        self.entries = entries
        res = [resolve_body(md, e) for e, _ in entries]
        self.E = len(entries)
        body = np.array([r[0] for r in res], dtype=np.int32)
        T = [r[1] @ Tx for r, (_, Tx) in zip(res, entries)]
        T12 = np.ascontiguousarray(np.stack([np.concatenate([t[:3, :3].reshape(9), t[:3, 3]]) for t in T])) if entries else None
        self.set = lib.shim_wrench_set(self.h, self.E, _p(body), _p(T12))

    def __del__(self):
        self.lib.shim_wrench_set_free(self.set)
        super().__del__()

    def wtau(self, S, A, W, flags=0):
        S, A, W = _c(S), _c(A), _c(W)
        out = np.full((self.n, S.shape[1]), np.nan)
        self.lib.shim_wrench_id(self.h, self.set, S.shape[1], _p(S), _p(A), _p(W), flags, _p(out))
        return out

    def wvjp(self, S, A, W, g, flags=0):
        S, A, W, g = _c(S), _c(A), _c(W), _c(g)
        B = S.shape[1]
        gs, ga, gw = np.full((2 * self.n, B), np.nan), np.full((self.n, B), np.nan), np.full((6 * self.E, B), np.nan)
        self.lib.shim_wrench_id_vjp(self.h, self.set, B, _p(S), _p(A), _p(W), flags, _p(g), _p(gs), _p(ga), _p(gw), 0)
        return gs, ga, gw

    def waccel(self, S, T, W, flags=0):
        S, T, W = _c(S), _c(T), _c(W)
        out = np.full((self.n, S.shape[1]), np.nan)
        self.lib.shim_wrench_fd(self.h, self.set, S.shape[1], _p(S), _p(T), _p(W), flags, _p(out))
        return out

    def wfd_vjp(self, S, T, W, g, flags=0):
        S, T, W, g = _c(S), _c(T), _c(W), _c(g)
        B = S.shape[1]
        gs, gt, gw = np.full((2 * self.n, B), np.nan), np.full((self.n, B), np.nan), np.full((6 * self.E, B), np.nan)
        self.lib.shim_wrench_fd_vjp(self.h, self.set, B, _p(S), _p(T), _p(W), flags, _p(g), _p(gs), _p(gt), _p(gw), 0)
        return gs, gt, gw

    def accel(self, S, T, flags=0):
        S, T = _c(S), _c(T)
        out = np.full((self.n, S.shape[1]), np.nan)
        self.lib.shim_fdyn_forward(self.h, S.shape[1], _p(S), _p(T), flags, _p(out))
        return out

    def cid_root(self):
        return self.lib.shim_wrench_cid_root(self.h, self.set)

    def cid(self, S, A, mode, guess=None, flags=JOINT_FORCES):
        S, A, guess = _c(S), _c(A), _c(guess)
        B = S.shape[1]
        W, tau = np.full((6 * self.E, B), np.nan), np.full((self.n, B), np.nan)
        self.lib.shim_wrench_cid(self.h, self.set, B, _p(S), _p(A), _p(guess), mode, flags, _p(W), _p(tau))
        return W, tau


def _offset(seed):
    """a frame that is not the identity: a rotation of about 0.6 rad per axis and a shift of a few centimetres"""
    from test_ball_joint import _T
    return _T(np.random.default_rng(seed), 0.05)


def wrench_entries(md):
    """2 - 3 entries on distinct BodyNodes (the last, the middle and the first one that can carry one), the second with an offset frame; a
    model with one body gets two entries on it"""
    ok = []
    for i in range(len(md.bodies)):
        try:
            if resolve_body(md, i)[0] >= 0:
                ok.append(i)
        except ValueError:
            pass
    pick = []
    for i in (ok[-1], ok[len(ok) // 2], ok[0]):
        if i not in pick:
            pick.append(i)
    if len(pick) == 1:
        pick.append(pick[0])
    return [(i, _offset(40 + k) if k == 1 else np.eye(4)) for k, i in enumerate(pick)]


def frame_jacobian(ow, md, q, e, Tx):
    """(F = W_e Tx, the world Jacobian [6][n] of F: angular velocity, velocity of F's origin) from kin_numpy.body_jacobians"""
    W, _, Jv = body_jacobians(ow, md, q, e)
    F = W @ Tx
    J = Jv.copy()
    J[3:] += np.cross(Jv[:3].T, F[:3, 3] - W[:3, 3]).T
    return F, J


def world_wrenches(ow, md, q, entries, W, world):
    """(J_vel [6 E][n], W_world [6 E], J_local [6 E][n]) of the wrenches W [6 E] given in the entries' frames or (world) in world coordinates"""
    Js, Ws, Jl = [], [], []
    for k, (e, Tx) in enumerate(entries):
        F, J = frame_jacobian(ow, md, q, e, Tx)
        R = F[:3, :3]
        w = W[6 * k:6 * k + 6]
        Ws.append(w if world else np.concatenate([R @ w[:3], R @ w[3:]]))
        Js.append(J)
        Jl.append(np.concatenate([R.T @ J[:3], R.T @ J[3:]]))
    return np.concatenate(Js), np.concatenate(Ws), np.concatenate(Jl)


IDS = [m[0] for m in MODELS]


def test_the_offset_frame_is_not_the_identity():
    T = _offset(41)
    assert np.abs(T[:3, :3] - np.eye(3)).max() > 0.1 and np.abs(T[:3, 3]).max() > 1e-3
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-14)


@pytest.mark.parametrize("name,md", MODELS, ids=IDS)
def test_inverse_dynamics_with_wrenches_equals_the_oracle_minus_the_jacobian_term_and_forward_dynamics_inverts_it(shim, name, md):
    ow = OracleWorld(md)
    entries = wrench_entries(md)
    d = ShimWrench(shim, md, entries)
    n, B = md.num_dofs, 3
    S, A, _ = _draw(md, B, 31)
    W = np.random.default_rng(32).normal(0, 3.0, (6 * d.E, B))
    for world in (False, True):
        fl = WORLD if world else 0
        tau = d.wtau(S, A, W, fl)
        tau_jf = d.wtau(S, A, W, fl | JOINT_FORCES)
        acc = d.waccel(S, tau, W, fl)
        acc_jf = d.waccel(S, tau_jf, W, fl | JOINT_FORCES)
        for b in range(B):
            q, v, a = S[:n, b], S[n:, b], A[:, b]
            Mo, Co = ow.mass_matrix(q), ow.coriolis_gravity(q, v)
            Jv, Ww, _ = world_wrenches(ow, md, q, entries, W[:, b], world)
            ref = Mo @ a + Co - Jv.T @ Ww
            e = _err(tau[:, b], ref)
            print(name, "world" if world else "local", b, "tau", e)
            assert e <= TOL, (name, world, b, e)
            # the inverse function, compared in force space
            assert rel_err(Mo @ acc[:, b], Mo @ a) < 1e-10, (name, world, b)
            assert rel_err(Mo @ acc_jf[:, b], Mo @ a) < 1e-10, (name, world, b)


@pytest.mark.parametrize("name,md", MODELS, ids=IDS)
def test_grad_wrench_equals_minus_the_numpy_jacobian_times_the_cotangent(shim, name, md):
    ow = OracleWorld(md)
    entries = wrench_entries(md)
    d = ShimWrench(shim, md, entries)
    n, B = md.num_dofs, 3
    S, A, g = _draw(md, B, 33)
    W = np.random.default_rng(34).normal(0, 3.0, (6 * d.E, B))
    for world in (False, True):
        fl = WORLD if world else 0
        gs, ga, gw = d.wvjp(S, A, W, g, fl)
        _, ga0 = d.vjp(S, A, g)
        assert np.array_equal(ga, ga0)                                     # M^T g: the wrenches do not enter
        tau = d.wtau(S, A, W, fl)
        _, gt, gwf = d.wfd_vjp(S, tau, W, g, fl)                           # forward dynamics: grad_tau = lambda = M^-1 g, grad_wrench = J lambda
        for b in range(B):
            q = S[:n, b]
            Jv, _, Jl = world_wrenches(ow, md, q, entries, W[:, b], world)
            J = Jv if world else Jl
            e = _err(gw[:, b], -J @ g[:, b])
            lam = np.linalg.solve(ow.mass_matrix(q), g[:, b])
            ef = max(_err(gt[:, b], lam), _err(gwf[:, b], J @ lam))
            print(name, "world" if world else "local", b, "grad_wrench", e, "forward dynamics", ef)
            assert e <= TOL and ef <= TOL, (name, world, b, e, ef)


@pytest.mark.parametrize("name,md", MODELS, ids=IDS)
def test_the_reverse_passes_equal_central_differences_of_the_forward_passes(shim, name, md):
    entries = wrench_entries(md)
    d = ShimWrench(shim, md, entries)
    n, E6 = md.num_dofs, 6 * d.E
    S, A, _ = _draw(md, 1, 35)
    W = np.random.default_rng(36).normal(0, 3.0, (E6, 1))
    eps = 1e-6
    s, a, w = S[:, 0], A[:, 0], W[:, 0]
    X = np.concatenate([s, a, w])
    N = X.size
    P = X[:, None] + eps * np.eye(N)
    Q = X[:, None] - eps * np.eye(N)
    rep = lambda x: np.repeat(x[:, None], n, 1)
    scale = max(1.0, np.abs(d.tau(s[:, None], None)).max())
    for flags in (0, WORLD, WORLD | JOINT_FORCES):
        # inverse dynamics: the dense Jacobian = the reverse pass with unit cotangents, n worlds at the same point
        gs, ga, gw = d.wvjp(rep(s), rep(a), rep(w), np.eye(n), flags)
        fd = (d.wtau(P[:2 * n], P[2 * n:3 * n], P[3 * n:], flags) - d.wtau(Q[:2 * n], Q[2 * n:3 * n], Q[3 * n:], flags)) / (2 * eps)
        J = np.concatenate([gs, ga, gw]).T
        err = np.abs(J - fd).max()
        print(name, flags, "inverse dynamics", err / scale)
        assert err < 2e-7 * scale, (name, flags, err)
        # forward dynamics at tau = ID(a): accelerations are forces times M^-1, so the bound is taken in units of the accelerations
        t = d.wtau(s[:, None], a[:, None], w[:, None], flags)[:, 0]
        Y = np.concatenate([s, t, w])
        P2, Q2 = Y[:, None] + eps * np.eye(N), Y[:, None] - eps * np.eye(N)
        gs, gt, gw = d.wfd_vjp(rep(s), rep(t), rep(w), np.eye(n), flags)
        fd = (d.waccel(P2[:2 * n], P2[2 * n:3 * n], P2[3 * n:], flags) - d.waccel(Q2[:2 * n], Q2[2 * n:3 * n], Q2[3 * n:], flags)) / (2 * eps)
        J = np.concatenate([gs, gt, gw]).T
        ascale = max(1.0, np.abs(fd).max())
        err = np.abs(J - fd).max()
        print(name, flags, "forward dynamics", err / ascale)
        assert err < 2e-7 * ascale, (name, flags, err)


@pytest.mark.parametrize("name,md", MODELS, ids=IDS)
def test_no_entries_and_zero_wrenches_give_the_wrench_free_bits(shim, name, md):
    d0 = ShimWrench(shim, md, [])
    d = ShimWrench(shim, md, wrench_entries(md))
    B = 3
    S, A, g = _draw(md, B, 37)
    Z = np.zeros((6 * d.E, B))
    for flags in (0, JOINT_FORCES):
        tau = d.tau(S, A, flags)
        acc = d.accel(S, tau, flags)
        gs, ga = d.vjp(S, A, g, flags)
        for dd, W, wf in ((d0, None, 0), (d, Z, 0), (d, Z, WORLD)):
            assert np.array_equal(dd.wtau(S, A, W, flags | wf), tau), (name, flags, wf)
            assert np.array_equal(dd.waccel(S, tau, W, flags | wf), acc), (name, flags, wf)
            ws, wa, _ = dd.wvjp(S, A, W, g, flags | wf)
            assert np.array_equal(ws, gs) and np.array_equal(wa, ga), (name, flags, wf)


# ---- contact inverse dynamics -----------------------------------------------------------------------------------------------------------------
def _contact_cases():
    from test_ball_joint import ball_model
    out = []
    for nm in ("atlas20", "atlas33"):
        md = na.atlas(nm)
        out += [(nm + "_one_foot", md, ["l_foot"]), (nm + "_feet", md, ["l_foot", "r_foot"]), (nm + "_feet_and_hand", md, ["l_foot", "r_foot", "r_hand"])]
    arm = ball_model(2, True)
    out += [("ball_arm_hand", arm, ["hand"]), ("ball_arm_hand_and_tail", arm, ["hand", "tail"])]
    return out


CONTACT_CASES = _contact_cases()


def _contact_entries(md, names):
    idx = [[i for i, b in enumerate(md.bodies) if b.name == nm][0] for nm in names]
    return [(i, _offset(50 + k) if k == 1 else np.eye(4)) for k, i in enumerate(idx)]


@pytest.mark.parametrize("name,md,names", CONTACT_CASES, ids=[c[0] for c in CONTACT_CASES])
def test_contact_inverse_dynamics_equals_the_numpy_restatement(shim, name, md, names):
    """Measured on these inputs: lstsq / KKT-QR against the normal equations, at most 5.3e-14 relative to max(1, |ref|) (wrenches and
    torques); the bound per case is 100 x its own measured value, floored at 1e-12.  cond(A A^T) <= 6 < 1e8 in every world."""
    ow = OracleWorld(md)
    entries = _contact_entries(md, names)
    d = ShimWrench(shim, md, entries)
    n, B, E = md.num_dofs, 4, len(entries)
    assert d.cid_root() == 0
    root = slice(dof_offsets(md)[0], dof_offsets(md)[0] + 6)
    fl = md.flat()
    S, A, _ = _draw(md, B, 41)
    G = np.random.default_rng(42).normal(0, 20.0, (6 * E, B))
    modes = ([("single", SINGLE, None)] if E == 1 else []) + [("nearest", NEAREST, G), ("min_torque", MIN_TORQUE, None)]
    for label, mode, guess in modes:
        W, tau = d.cid(S, A, mode, guess)
        assert not tau[root].any(), (name, label)                                        # exactly 0
        acc = d.waccel(S, tau, W, JOINT_FORCES)                                          # the reference's sumError: (tau, W) reproduce a
        two, dev = 0.0, 0.0
        refs = []
        for b in range(B):
            q, v, a = S[:n, b], S[n:, b], A[:, b]
            Mo = ow.mass_matrix(q)
            plain = Mo @ a + ow.coriolis_gravity(q, v) + fl["damping"] * v + fl["spring"] * (q - fl["rest"] + md.dt * v)
            _, _, Jl = world_wrenches(ow, md, q, entries, np.zeros(6 * E), False)
            Ablk = Jl[:, root].T
            cond = np.linalg.cond(Ablk @ Ablk.T)
            assert cond < 1e8, (name, b, cond)
            if mode == SINGLE:
                Wr, tr = contact_inverse_dynamics(Jl, plain, root)
            else:
                Wr, tr = multiple_contact_inverse_dynamics(Jl, plain, root, None if guess is None else guess[:, b])
            Wn, tn = multiple_contact_inverse_dynamics_normal(Jl, plain, root, None if guess is None else guess[:, b], mode == MIN_TORQUE)
            two = max(two, _err(Wn, Wr), _err(tn, tr))
            dev = max(dev, _err(W[:, b], Wr), _err(tau[:, b], tr))
            refs.append(Wr)
            assert rel_err(Mo @ acc[:, b], Mo @ a) < 1e-10, (name, label, b)
            if mode == NEAREST:                                                          # no further from the guesses than the restatement's
                assert np.linalg.norm(W[:, b] - guess[:, b]) <= np.linalg.norm(Wr - guess[:, b]) * (1 + 1e-12), (name, b)
        bound = max(100 * two, 1e-12)
        print(name, label, "two numpy routes", two, "device code vs restatement", dev, "bound", bound)
        assert dev <= bound, (name, label, dev, bound)
    if E == 1:                                                                           # one body: the three modes are one answer
        W1, t1 = d.cid(S, A, SINGLE)
        W2, t2 = d.cid(S, A, NEAREST, G)
        assert _err(W2, W1) < 1e-11 and _err(t2, t1) < 1e-11


def test_nan_in_one_world_of_the_contact_solve_stays_in_that_world(shim):
    """A block A_e of a body below a free root is invertible, so valid inputs never reach the pivot test; what can be checked here is that
    one world's trouble (NaN guesses) stays in that world: its outputs are NaN, the others keep their bits."""
    md = na.atlas("atlas20")
    d = ShimWrench(shim, md, _contact_entries(md, ["l_foot", "r_foot"]))
    S, A, _ = _draw(md, 3, 43)
    G = np.random.default_rng(44).normal(0, 20.0, (12, 3))
    W, tau = d.cid(S, A, NEAREST, G)
    G2 = G.copy(); G2[:, 1] = np.nan
    Wn, taun = d.cid(S, A, NEAREST, G2)
    assert np.isnan(Wn[:, 1]).all() and np.array_equal(Wn[:, [0, 2]], W[:, [0, 2]]) and np.array_equal(taun[:, [0, 2]], tau[:, [0, 2]])


def test_contact_inverse_dynamics_requires_one_free_root(shim):
    """the rule nbl_contact_inverse_dynamics checks on the host before it launches (cidRoot; NBL_E_UNSUPPORTED)"""
    from test_dynamics_host import free_below_root
    from test_ball_joint import ball_model
    fixed = ball_model(2, False)                                                         # no free root
    assert ShimWrench(shim, fixed, [(len(fixed.bodies) - 1, np.eye(4))]).cid_root() < 0
    fb = free_below_root()                                                               # its free joint is not at the root
    assert ShimWrench(shim, fb, [(1, np.eye(4))]).cid_root() < 0
    stack = na.box_stack()                                                               # several free roots
    roots = [i for i, b in enumerate(stack.bodies) if b.parent < 0 and b.joint_type == "free"]
    assert len(roots) >= 2
    assert ShimWrench(shim, stack, [(roots[0], np.eye(4))]).cid_root() >= 0
    assert ShimWrench(shim, stack, [(roots[0], np.eye(4)), (roots[1], np.eye(4))]).cid_root() < 0
    assert ShimWrench(shim, stack, []).cid_root() < 0


def test_results_do_not_depend_on_the_batch(shim):
    md = na.atlas("atlas20")
    d = ShimWrench(shim, md, _contact_entries(md, ["l_foot", "r_foot"]))
    S, A, g = _draw(md, 4, 45)
    W = np.random.default_rng(46).normal(0, 3.0, (12, 4))
    tau, (gs, ga, gw), (Wc, tc) = d.wtau(S, A, W, WORLD), d.wvjp(S, A, W, g, WORLD), d.cid(S, A, MIN_TORQUE)
    for b in range(4):
        sl = slice(b, b + 1)
        assert np.array_equal(d.wtau(S[:, sl], A[:, sl], W[:, sl], WORLD)[:, 0], tau[:, b])
        one = d.wvjp(S[:, sl], A[:, sl], W[:, sl], g[:, sl], WORLD)
        assert np.array_equal(one[0][:, 0], gs[:, b]) and np.array_equal(one[2][:, 0], gw[:, b])
        c1 = d.cid(S[:, sl], A[:, sl], MIN_TORQUE)
        assert np.array_equal(c1[0][:, 0], Wc[:, b]) and np.array_equal(c1[1][:, 0], tc[:, b])
