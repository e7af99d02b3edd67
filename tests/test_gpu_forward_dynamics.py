"""Forward dynamics and the inverse mass matrix on the device (k_forward_dynamics / k_forward_dynamics_lambda / k_minv_apply of
csrc/dynamics.hip through nimblephysics_amd/dynamics.py): forward_dynamics, multiply_by_inv_mass_matrix, inv_mass_matrix and their
vector-Jacobian products against the CPU oracle on every world, torch.autograd.gradcheck, the host build of the same header, composition
with timestep(), bit identity, deferred join, World.getInvMassMatrix, setMasses, immobile skeletons, argument errors, the plain-C driver.

TOLERANCE AGAINST THE ORACLE: TOL = 1e-10 (max error over max(1, |ref|), _rel of tests/test_gpu_dynamics.py), after this check: M^-1
amplifies rounding by the condition number of M, so the oracle's own two routes to the acceleration - its articulated-body
forward_dynamics and numpy's solve(mass_matrix, tau - C - joint forces) - were compared on the CPU on the exact inputs of the parity
test (_reference: B = 131, seed 11).  Measured disagreement: atlas20 1.6e-14 (cond(M) up to 3.7e4), ball_arm 4.0e-15 (3.0e2),
free_below_root 1.2e-13 (2.7e3), cartpole 7.3e-16 (2.2) - all below 1e-11, so 1e-10 stands (it would have been ten times the measured
value otherwise).  test_the_oracles_own_two_routes_agree_on_the_parity_inputs (no GPU) repeats the measurement.

DEVICE AGAINST HOST BUILD: 1e-13 relative, for the reasons at the head of tests/test_gpu_dynamics.py (hipcc contracts a * b + c into
fused multiply-adds, its sincos is not glibc's)."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_dynamics import _rel, _states

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10                       # measured oracle disagreement <= 1.2e-13: see the head of this file
ORACLE_ROUTES_MAX = 1e-11
BLOCK = 64                        # DYN_BLOCK of csrc/dynamics.hip
B_PARITY = 2 * BLOCK + 3          # two full workgroups and a partial one
PARITY_MODELS = ["atlas20", "ball_arm", "free_below_root", "cartpole", "screw_arm", "screw_root"]


def _model(name):
    import nimblephysics_amd as na
    from test_ball_joint import ball_model
    from test_dynamics_host import free_below_root
    from test_screw_joint import screw_arm
    return {"atlas20": lambda: na.atlas("atlas20"), "ball_arm": lambda: ball_model(2, True), "free_below_root": free_below_root,
            "cartpole": na.cartpole, "screw_arm": lambda: screw_arm(2, True), "screw_root": lambda: screw_arm(2, False)}[name]()


def _joint_forces(md, q, v):
    fl = md.flat()
    return fl["damping"] * v + fl["spring"] * (q - fl["rest"] + md.dt * v)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The inputs of the parity test and what the oracle says about every world of them; computed once, never written to."""
    from oracle import OracleWorld
    md = _model(name)
    ow = OracleWorld(md)
    n, B = md.num_dofs, B_PARITY
    S, T, g = _states(md, B, 11)
    rng = np.random.default_rng(12)
    X, GY, GM = rng.normal(size=(B, n, 3)), rng.normal(size=(B, n, 3)), rng.normal(size=(B, n, n))
    fl = md.flat()
    r = {k: [] for k in ("a", "a_jf", "a_aba", "Minv", "Y", "fd_gq", "fd_gv", "fd_gt", "mul_gq", "mul_gx", "inv_gq")}
    for b in range(B):
        q, v, tau = S[b, :n], S[b, n:], T[b]
        M, Cv = ow.mass_matrix(q), ow.coriolis_gravity(q, v)
        Mi = np.linalg.inv(M)
        K = np.stack([ow.jac_Mx(q, e) for e in np.eye(n)])            # jac_Mx(q, x) = sum_k x_k K[k]: M x is linear in x
        jmx = lambda x: np.tensordot(x, K, 1)
        a = np.linalg.solve(M, tau - Cv)
        lam = np.linalg.solve(M, g[b])
        Y, L = np.linalg.solve(M, X[b]), np.linalg.solve(M, GY[b])
        LM = np.linalg.solve(M, GM[b])
        r["a"].append(a); r["a_jf"].append(np.linalg.solve(M, tau - Cv - _joint_forces(md, q, v))); r["a_aba"].append(ow.forward_dynamics(q, v, tau))
        r["Minv"].append(Mi); r["Y"].append(Y)
        r["fd_gt"].append(lam); r["fd_gq"].append(-(jmx(a) + ow.jac_C(q, v, 0)).T @ lam); r["fd_gv"].append(-ow.jac_C(q, v, 1).T @ lam)
        r["mul_gx"].append(L); r["mul_gq"].append(-sum(jmx(Y[:, k]).T @ L[:, k] for k in range(3)))
        r["inv_gq"].append(-sum(jmx(Mi[:, j]).T @ LM[:, j] for j in range(n)))
    out = {k: np.stack(v) for k, v in r.items()}
    out.update(md=md, S=S, T=T, g=g, X=X, GY=GY, GM=GM)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize("name", PARITY_MODELS)
def test_the_oracles_own_two_routes_agree_on_the_parity_inputs(name):
    """What fixes TOL (head of this file); runs without a GPU."""
    ref = _reference(name)
    worst = max(_rel(ref["a_aba"][b], ref["a_jf"][b]) for b in range(B_PARITY))
    print(name, "oracle forward_dynamics vs solve(mass_matrix, .):", worst)
    assert worst <= ORACLE_ROUTES_MAX, (name, worst)


@gpu
@pytest.mark.parametrize("name", PARITY_MODELS)
def test_parity_with_the_oracle_on_every_world(name):
    import nimblephysics_amd as na
    ref = _reference(name)
    md, S, B = ref["md"], ref["S"], B_PARITY
    n = md.num_dofs
    w = na.World(md, device=DEV)
    t = lambda x: torch.tensor(np.array(x), device=DEV)
    st, tt = t(S).requires_grad_(True), t(ref["T"]).requires_grad_(True)
    a = na.forward_dynamics(w, st, tt)
    assert a.shape == (B, n) and a.device == DEV
    a.backward(t(ref["g"]))
    a_jf = na.forward_dynamics(w, t(S), t(ref["T"]), joint_forces=True)
    Mi_in = t(S).requires_grad_(True)
    Mi = na.inv_mass_matrix(w, Mi_in)
    assert Mi.shape == (B, n, n)
    Mi.backward(t(ref["GM"]))
    sx, xx = t(S).requires_grad_(True), t(ref["X"]).requires_grad_(True)
    Y = na.multiply_by_inv_mass_matrix(w, sx, xx)
    assert Y.shape == (B, n, 3)
    Y.backward(t(ref["GY"]))
    y1 = na.multiply_by_inv_mass_matrix(w, t(S), t(ref["X"][:, :, 0]))
    assert y1.shape == (B, n)
    c = lambda x: x.detach().cpu().numpy()
    got = {"a": c(a), "a_jf": c(a_jf), "a_aba": c(a_jf), "Minv": c(Mi), "Y": c(Y), "fd_gq": c(st.grad)[:, :n], "fd_gv": c(st.grad)[:, n:], "fd_gt": c(tt.grad),
           "mul_gq": c(sx.grad)[:, :n], "mul_gx": c(xx.grad), "inv_gq": c(Mi_in.grad)[:, :n]}
    assert np.array_equal(c(y1), got["Y"][:, :, 0])                      # R = 1: the same bits as the first of three right-hand sides
    assert not c(sx.grad)[:, n:].any() and not c(Mi_in.grad)[:, n:].any()   # M^-1 does not depend on the velocities
    worst = {k: 0.0 for k in got}
    for b in range(B):                                                    # every world
        assert np.array_equal(got["Minv"][b], got["Minv"][b].T), b
        e = {k: _rel(got[k][b], ref[k][b]) for k in got}
        for k, x in e.items():
            worst[k] = max(worst[k], x)
        assert max(e.values()) <= TOL, (name, b, e)
    print(name, "worst relative errors over", B, "worlds:", worst)


@gpu
@pytest.mark.parametrize("name", ["cartpole", "ball_arm"])
def test_gradcheck(name):
    import nimblephysics_amd as na
    md = _model(name)
    n = md.num_dofs
    w = na.World(md, device=DEV)
    S, T, _ = _states(md, 3, 4)
    st = torch.tensor(S, device=DEV, requires_grad=True)
    tt = torch.tensor(T, device=DEV, requires_grad=True)
    xv = torch.tensor(np.random.default_rng(5).normal(size=(3, n)), device=DEV, requires_grad=True)
    xm = torch.tensor(np.random.default_rng(6).normal(size=(3, n, 2)), device=DEV, requires_grad=True)
    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda s, u: na.forward_dynamics(w, s, u), (st, tt), **kw)
    assert torch.autograd.gradcheck(lambda s, u: na.forward_dynamics(w, s, u, joint_forces=True), (st, tt), **kw)
    assert torch.autograd.gradcheck(lambda s, x: na.multiply_by_inv_mass_matrix(w, s, x), (st, xv), **kw)
    assert torch.autograd.gradcheck(lambda s, x: na.multiply_by_inv_mass_matrix(w, s, x), (st, xm), **kw)
    assert torch.autograd.gradcheck(lambda s: na.inv_mass_matrix(w, s), (st,), **kw)


@gpu
@pytest.mark.parametrize("name", ["atlas20", "ball_arm", "free_below_root", "screw_arm", "screw_root"])
def test_the_device_kernels_equal_the_host_build_to_1e_13(name):
    """See the head of this file: 1e-13 relative, not bit for bit."""
    import nimblephysics_amd as na
    from test_fdyn_host import ShimForwardDynamics, load_shim
    from nimblephysics_amd.dynamics import ID_JOINT_FORCES, forward_dynamics_soa, forward_dynamics_vjp_soa, inv_mass_apply_soa, inv_mass_matrix_soa
    md = _model(name)
    n = md.num_dofs
    host = ShimForwardDynamics(load_shim(), md)
    w = na.World(md, device=DEV)
    S, T, g = _states(md, 128, 6)
    X = np.random.default_rng(7).normal(size=(3, n, 128))
    s, tq, gg = (torch.tensor(np.ascontiguousarray(x.T), device=DEV) for x in (S, T, g))
    worst = {}
    for flags in (0, ID_JOINT_FORCES):
        acc = forward_dynamics_soa(w, s, tq, flags).cpu().numpy()
        gs, gt = forward_dynamics_vjp_soa(w, s, tq, gg, flags)
        hgs, hgt = host.fd_vjp(S.T, T.T, g.T, flags)
        for key, x, ref in (("accel", acc, host.accel(S.T, T.T, flags)), ("grad_state", gs.cpu().numpy(), hgs), ("grad_tau", gt.cpu().numpy(), hgt)):
            worst[(key, flags)] = _rel(x, ref)
    worst["Minv"] = _rel(inv_mass_matrix_soa(w, s).cpu().numpy().reshape(n, n, -1), host.minv(S.T))
    worst["Minv X"] = _rel(inv_mass_apply_soa(w, s, torch.tensor(X, device=DEV)).cpu().numpy(), host.minv_apply(S.T, X))
    print(name, "device vs host build:", worst)
    assert max(worst.values()) <= 1e-13, worst


@gpu
def test_the_acceleration_of_a_contact_free_step_is_forward_dynamics_with_joint_forces():
    """(v' - v) / dt of timestep() on a model without colliders whose joints have damping and springs = forward_dynamics(joint_forces=True):
    the step solves the same equation and integrates v' = v + dt a.  Bound: 1e-9 max(1, scale) as the pendulum test of
    tests/test_gpu_dynamics.py has it for the same quotient (v' - v cancels digits of v: 1e-16 / dt), scale = the quotient's own size."""
    import nimblephysics_amd as na
    from nimblephysics_amd.timestep import timestep
    md = _model("free_below_root")
    fl = md.flat()
    assert md.max_contacts == 0 and np.any(fl["damping"]) and np.any(fl["spring"])
    n, B = md.num_dofs, 64
    w = na.World(md, device=DEV)
    assert w.k == n
    S, T, _ = _states(md, B, 13)
    st, tt = torch.tensor(S, device=DEV), torch.tensor(T, device=DEV)
    nxt = timestep(w, st, tt)
    quot = (nxt[:, n:] - st[:, n:]) / md.dt
    a = na.forward_dynamics(w, st, tt, joint_forces=True)
    scale = float(quot.abs().max())
    err = float((a - quot).abs().max())
    plain = float((na.forward_dynamics(w, st, tt) - quot).abs().max())
    print("step quotient vs forward_dynamics:", err, "scale", scale, "(without joint forces:", plain, ")")
    assert err <= 1e-9 * max(1.0, scale)
    assert plain > 1e-3                                                   # the springs and dampers matter here


def _run(na, world, s, t, g, X):
    x, y = s.clone().requires_grad_(True), t.clone().requires_grad_(True)
    a = na.forward_dynamics(world, x, y, joint_forces=True)
    a.backward(g)
    return a.detach(), x.grad, y.grad, na.inv_mass_matrix(world, s), na.multiply_by_inv_mass_matrix(world, s, X)


@gpu
def test_bit_identity_over_batch_lane_and_rollout_shape():
    import nimblephysics_amd as na
    md = _model("atlas20")
    n, B = md.num_dofs, B_PARITY
    S, T, g = _states(md, B, 9)
    X = np.random.default_rng(10).normal(size=(B, n, 2))
    w = na.World(md, device=DEV)
    st, tt, gt, xt = (torch.tensor(x, device=DEV) for x in (S, T, g, X))
    first, second = _run(na, w, st, tt, gt, xt), _run(na, w, st, tt, gt, xt)
    for u, v in zip(first, second):
        assert torch.equal(u, v)
    assert torch.equal(first[3], first[3].transpose(1, 2))                 # Minv = its transpose, bit for bit
    for b in (0, B - 1):                                                   # B = 1 against the first and the last lane of the large batch
        for u, v in zip(_run(na, w, st[b:b + 1], tt[b:b + 1], gt[b:b + 1], xt[b:b + 1]), first):
            assert torch.equal(u[0], v[b]), b
    last_first = torch.cat([st[B - 1:], st[:B - 1]]), torch.cat([tt[B - 1:], tt[:B - 1]]), torch.cat([gt[B - 1:], gt[:B - 1]]), torch.cat([xt[B - 1:], xt[:B - 1]])
    for u, v in zip(_run(na, w, *last_first), first):                      # the last world in the first lane
        assert torch.equal(u[0], v[B - 1]) and torch.equal(u[1], v[0])
    # a [T+1, B, 2n] rollout-shaped call: one launch over (T+1) x B worlds
    T1, Bs = 3, 5
    roll = _run(na, w, st[:T1 * Bs].reshape(T1, Bs, -1), tt[:T1 * Bs].reshape(T1, Bs, -1), gt[:T1 * Bs].reshape(T1, Bs, -1), xt[:T1 * Bs].reshape(T1, Bs, n, 2))
    assert roll[0].shape == (T1, Bs, n) and roll[1].shape == (T1, Bs, 2 * n) and roll[3].shape == (T1, Bs, n, n) and roll[4].shape == (T1, Bs, n, 2)
    for u, v in zip(roll, first):
        assert torch.equal(u.reshape((T1 * Bs,) + u.shape[2:]), v[:T1 * Bs])
    # CPU float64 in -> CPU out, one world as a 1-D vector
    one = na.forward_dynamics(w, st[0].cpu(), tt[0].cpu(), joint_forces=True)
    assert one.device.type == "cpu" and one.shape == (n,) and torch.equal(one, first[0][0].cpu())
    assert na.inv_mass_matrix(w, st[0].cpu()).shape == (n, n) and na.multiply_by_inv_mass_matrix(w, st[0].cpu(), xt[0, :, 0].cpu()).shape == (n,)
    with pytest.raises(ValueError):
        na.forward_dynamics(w, st[:, :-1], tt)
    with pytest.raises(ValueError):
        na.forward_dynamics(w, st, tt[:3])
    with pytest.raises(ValueError):
        na.multiply_by_inv_mass_matrix(w, st, xt[:3])


@gpu
def test_deferred_join_gives_the_same_bits():
    """The state comes straight out of a step whose slices are still in flight (as test_bit_identity_deferred_join_getters_and_errors of
    tests/test_gpu_dynamics.py does for inverse dynamics)."""
    import nimblephysics_amd as na
    md = na.atlas("atlas20", ground=True)
    n, B = md.num_dofs, 4096
    S, T, _ = _states(md, B, 9)
    S[:, 0] = -np.pi / 2; S[:, 4] += 1.0
    st, tt = torch.tensor(S, device=DEV), torch.tensor(T, device=DEV)
    ref, dw = na.World(md, device=DEV), na.World(md, device=DEV)
    s_soa = ref.to_soa(st); a_soa = ref.to_soa(torch.zeros((B, ref.k), dtype=torch.float64, device=DEV))
    want_next, _, _ = ref.step_soa(s_soa, a_soa, want_saved=True)
    want = na.forward_dynamics(ref, want_next.t(), tt), na.inv_mass_matrix(ref, want_next.t()[:64])
    dw.set_deferred_join(True)
    assert dw.slices_for(B) > 1
    buf = {"nxt": torch.empty_like(s_soa), "saved": torch.empty(dw.saved_bytes(B), dtype=torch.uint8, device=DEV),
           "status": torch.empty(B, dtype=torch.int32, device=DEV), "cache": torch.empty((dw.m, B), dtype=torch.float64, device=DEV)}
    dw.step_into(s_soa, a_soa, buf["nxt"], buf["saved"], buf["status"], None, buf["cache"])
    got = na.forward_dynamics(dw, buf["nxt"].t(), tt), na.inv_mass_matrix(dw, buf["nxt"].t()[:64])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    dw.join()
    torch.cuda.synchronize()


@gpu
def test_world_get_inv_mass_matrix_times_get_mass_matrix_is_the_identity():
    import nimblephysics_amd as na
    md = _model("atlas20")
    n = md.num_dofs
    w = na.World(md, device=DEV)
    S, _, _ = _states(md, 8, 14)
    st = torch.tensor(S, device=DEV)
    w.setState(st)
    Mi, M = w.getInvMassMatrix(), w.getMassMatrix()
    assert Mi.shape == (8, n, n) and torch.equal(Mi, na.inv_mass_matrix(w, st)) and torch.equal(w.getState(), st)
    eye = np.eye(n)
    for b in range(8):
        assert _rel((Mi[b] @ M[b]).cpu().numpy(), eye) <= TOL and _rel((M[b] @ Mi[b]).cpu().numpy(), eye) <= TOL
    w.setState(st[3])
    assert w.getInvMassMatrix().shape == (n, n) and torch.equal(w.getInvMassMatrix(), Mi[3])


@gpu
def test_set_masses_changes_the_results_like_the_oracle():
    import nimblephysics_amd as na
    from nimblephysics_amd.mass import WrtMassBodyNodeEntryType as MT
    from oracle import OracleWorld
    md = _model("atlas20")
    n = md.num_dofs
    w = na.World(md, device=DEV)
    S, T, _ = _states(md, 16, 8)
    st, tt = torch.tensor(S, device=DEV), torch.tensor(T, device=DEV)
    before = na.inv_mass_matrix(w, st).cpu().numpy()
    w.tuneMass(0, MT.INERTIA_MASS); w.tuneMass(4, MT.INERTIA_FULL)
    x = w.getMasses().numpy().copy()
    x[0] *= 1.3; x[1] *= 0.7; x[2:5] += 0.01; x[5:8] *= 1.2
    w.setMasses(x)
    after = na.inv_mass_matrix(w, st).cpu().numpy()
    acc = na.forward_dynamics(w, st, tt).cpu().numpy()
    ow = OracleWorld(w.description)                                       # setMasses edited the World's description
    for b in range(16):
        Mo = ow.mass_matrix(S[b, :n])
        assert _rel(after[b], np.linalg.inv(Mo)) <= TOL
        assert _rel(acc[b], np.linalg.solve(Mo, T[b] - ow.coriolis_gravity(S[b, :n], S[b, n:]))) <= TOL
    assert np.abs(after - before).max() > 1e-3                            # the edit matters


@gpu
def test_immobile_skeletons_take_the_references_layout(tmp_path):
    import nimblephysics_amd as na
    from test_ref_layout import load
    md = load(tmp_path)
    w = na.World(md, device=DEV)
    assert w.ref_layout is not None and w.getStateSize() == 24 and w.n == 6
    rng = np.random.default_rng(1)
    full = np.zeros((8, 24)); full[:, 6:12] = rng.normal(0, 0.3, (8, 6)); full[:, 18:] = rng.normal(0, 1, (8, 6))
    tfull = rng.normal(0, 1, (8, 12))                                     # forces on the frozen coordinates too: they move nothing
    x = torch.tensor(full, device=DEV, requires_grad=True)
    y = torch.tensor(tfull, device=DEV, requires_grad=True)
    a = na.forward_dynamics(w, x, y)
    w2 = na.World(md, device=DEV); w2.ref_layout = None                   # the device's own (shorter) layout
    xs = torch.tensor(np.concatenate([full[:, 6:12], full[:, 18:]], 1), device=DEV)
    ys = torch.tensor(tfull[:, 6:], device=DEV)
    assert a.shape == (8, 12) and not a[:, :6].any() and torch.equal(a.detach()[:, 6:], na.forward_dynamics(w2, xs, ys))
    a.sum().backward()
    assert not x.grad[:, :6].any() and not x.grad[:, 12:18].any() and x.grad[:, 6:12].abs().sum() > 0
    assert not y.grad[:, :6].any() and y.grad[:, 6:].abs().sum() > 0
    Mi = na.inv_mass_matrix(w, x.detach())
    assert Mi.shape == (8, 12, 12) and not Mi[:, :6].any() and not Mi[:, :, :6].any() and torch.equal(Mi[:, 6:, 6:], na.inv_mass_matrix(w2, xs))
    z = torch.tensor(rng.normal(0, 1, (8, 12, 2)), device=DEV, requires_grad=True)
    x2 = torch.tensor(full, device=DEV, requires_grad=True)
    Y = na.multiply_by_inv_mass_matrix(w, x2, z)
    assert Y.shape == (8, 12, 2) and not Y[:, :6].any() and torch.equal(Y.detach()[:, 6:], na.multiply_by_inv_mass_matrix(w2, xs, z.detach()[:, 6:]))
    Y.sum().backward()
    assert not z.grad[:, :6].any() and z.grad[:, 6:].abs().sum() > 0 and not x2.grad[:, :6].any() and not x2.grad[:, 12:].any()
    x3 = torch.tensor(full, device=DEV, requires_grad=True)
    wt = torch.tensor(rng.normal(0, 1, (8, 12, 12)), device=DEV)
    (na.inv_mass_matrix(w, x3) * wt).sum().backward()
    x4 = xs.clone().requires_grad_(True)
    (na.inv_mass_matrix(w2, x4) * wt[:, 6:, 6:]).sum().backward()
    # the mobile block is the device layout's gradient, bit for bit.  (Its value is zero in this model: the mass matrix of a
    # single free body is its constant spatial inertia, so no "> 0" here; forward_dynamics above covers a non-zero one.)
    assert not x3.grad[:, :6].any() and not x3.grad[:, 12:].any() and torch.equal(x3.grad[:, 6:12], x4.grad[:, :6])


@gpu
def test_argument_errors_return_their_codes_and_launch_nothing():
    import ctypes as C
    import nimblephysics_amd as na
    from nimblephysics_amd._lib import check
    from nimblephysics_amd.dynamics import _fd_workspace, forward_dynamics_soa
    md = _model("atlas20")
    n = md.num_dofs
    w = na.World(md, device=DEV)
    S, T, _ = _states(md, 8, 15)
    L, h = w._L, w._h
    s8, t8 = w.to_soa(torch.tensor(S, device=DEV)), w.to_soa(torch.tensor(T, device=DEV))
    SENT = -12345.0
    out = torch.full((n * n, 8), SENT, dtype=torch.float64, device=DEV)   # nothing may be written on an error
    ws = _fd_workspace(w, 8)
    need = L.nbl_forward_dynamics_workspace_bytes(h, 8)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert need > 0 and L.nbl_forward_dynamics_workspace_bytes(None, 8) == 0 and L.nbl_forward_dynamics_workspace_bytes(h, 0) == 0
    nb, rem = divmod(need // (8 * 8) - 2 * n, 84)                         # 84 doubles per body and world + 2 n per world
    assert rem == 0 and nb >= 1
    assert L.nbl_dynamics_workspace_bytes(h, 8) == nb * 48 * 8 * 8        # the size of the existing calls is what it was: 48 doubles per body
    BAD, WSP = -1, -4
    cases = ((BAD, lambda: L.nbl_forward_dynamics_forward(None, 8, p(s8), p(t8), 0, p(out), p(ws), need, None)),
             (BAD, lambda: L.nbl_forward_dynamics_forward(h, -1, p(s8), p(t8), 0, p(out), p(ws), need, None)),
             (BAD, lambda: L.nbl_forward_dynamics_forward(h, 8, None, p(t8), 0, p(out), p(ws), need, None)),
             (BAD, lambda: L.nbl_forward_dynamics_forward(h, 8, p(s8), p(t8), 0, None, p(ws), need, None)),
             (BAD, lambda: L.nbl_forward_dynamics_forward(h, 8, p(s8), p(t8), 0, p(out), None, need, None)),
             (BAD, lambda: L.nbl_forward_dynamics_forward(h, 8, p(s8), p(t8), 8, p(out), p(ws), need, None)),
             (WSP, lambda: L.nbl_forward_dynamics_forward(h, 8, p(s8), p(t8), 0, p(out), p(ws), need - 1, None)),
             (BAD, lambda: L.nbl_forward_dynamics_backward(None, 8, p(s8), p(t8), 0, p(t8), p(out), p(out), 0, p(ws), need, None)),
             (BAD, lambda: L.nbl_forward_dynamics_backward(h, 8, p(s8), p(t8), 0, None, p(out), p(out), 0, p(ws), need, None)),
             (BAD, lambda: L.nbl_forward_dynamics_backward(h, 8, p(s8), p(t8), 16, p(t8), p(out), p(out), 0, p(ws), need, None)),
             (WSP, lambda: L.nbl_forward_dynamics_backward(h, 8, p(s8), p(t8), 0, p(t8), p(out), p(out), 0, p(ws), 8, None)),
             (BAD, lambda: L.nbl_inv_mass_apply(None, 8, 1, p(s8), p(t8), p(out), p(ws), need, None)),
             (BAD, lambda: L.nbl_inv_mass_apply(h, 8, 0, p(s8), p(t8), p(out), p(ws), need, None)),
             (BAD, lambda: L.nbl_inv_mass_apply(h, -2, 1, p(s8), p(t8), p(out), p(ws), need, None)),
             (BAD, lambda: L.nbl_inv_mass_apply(h, 8, 1, None, p(t8), p(out), p(ws), need, None)),
             (BAD, lambda: L.nbl_inv_mass_apply(h, 8, 1, p(s8), p(t8), None, p(ws), need, None)),
             (BAD, lambda: L.nbl_inv_mass_apply(h, 8, 1, p(s8), None, p(out), p(ws), need, None)),      # X may be null only with R = n
             (WSP, lambda: L.nbl_inv_mass_apply(h, 8, 1, p(s8), p(t8), p(out), p(ws), need // 2, None)),
             (BAD, lambda: L.nbl_inv_mass_matrix(None, 8, p(s8), p(out), p(ws), need, None)),
             (BAD, lambda: L.nbl_inv_mass_matrix(h, 8, None, p(out), p(ws), need, None)),
             (BAD, lambda: L.nbl_inv_mass_matrix(h, 8, p(s8), None, p(ws), need, None)),
             (BAD, lambda: L.nbl_inv_mass_matrix(h, 8, p(s8), p(out), None, need, None)),
             (WSP, lambda: L.nbl_inv_mass_matrix(h, 8, p(s8), p(out), p(ws), 0, None)))
    for rc_want, call in cases:
        rc = call()
        assert rc == rc_want, (rc, rc_want)
        with pytest.raises(na.NimbleAmdError):
            check(rc, "forward dynamics")
        assert L.nbl_last_error()
    assert bool((out == SENT).all())                                      # no kernel ran
    for call in (lambda: L.nbl_forward_dynamics_forward(h, 0, None, None, 0, None, None, 0, None),        # B = 0: a no-op
                 lambda: L.nbl_forward_dynamics_backward(h, 0, None, None, 0, None, None, None, 0, None, 0, None),
                 lambda: L.nbl_inv_mass_apply(h, 0, 1, None, None, None, None, 0, None), lambda: L.nbl_inv_mass_matrix(h, 0, None, None, None, 0, None)):
        assert call() == 0
    with pytest.raises(na.NimbleAmdError, match="flag"):
        forward_dynamics_soa(w, s8, t8, 8)


@gpu
def test_plain_c_forward_dynamics_driver(tmp_path):
    """tests/c_abi_example/forward_dynamics.c: the four entry points from pure C99 on the Atlas-20 model header; ID(FD(tau)) == tau and
    Minv M == I from the library's own outputs, Minv bitwise symmetric, grad_tau == Minv g, the argument errors."""
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/lib/libamdhip64.so"):
        pytest.skip("no gcc / ROCm runtime")
    libdir = os.path.join(ROOT, "nimblephysics_amd")
    exe = str(tmp_path / "forward_dynamics")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_abi_example", "forward_dynamics.c"), "-o", exe, "-L" + libdir, "-lnimble_amd",
                           "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath," + libdir])
    out = subprocess.check_output([exe, "64"]).decode()
    print(out)
    assert "max residuals" in out and "asymmetric 0" in out
