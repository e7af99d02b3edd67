"""Joint-space dynamics on the device (csrc/dynamics.hip through nimblephysics_amd/dynamics.py): inverse_dynamics, coriolis_and_gravity and
mass_matrix and their vector-Jacobian products against the CPU oracle (mass_matrix, coriolis_gravity, jac_C, jac_Mx; 1e-10 on every
world, no world skipped), torch.autograd.gradcheck, the host build of the same header, shapes and devices, composition with rollout(),
setMasses, bit-reproducibility, deferred join, the World getters, argument errors and the plain-C driver.

DEVICE AGAINST HOST BUILD: to 1e-13 relative, not bit for bit.  The host shim is compiled with -ffp-contract=off; hipcc contracts a * b + c
into fused multiply-adds (one rounding instead of two) and its sincos is not glibc's, so single results differ in the last bits."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


def _states(md, B, seed):
    """[B, 2n], [B, n], [B, n]: positions N(0, 0.5^2) (rotation vectors at sigma <= 0.6), velocities N(0, 1), accelerations N(0, 2^2), cotangents N(0, 1)"""
    rng = np.random.default_rng(seed)
    n = md.num_dofs
    return np.concatenate([rng.normal(0, 0.5, (B, n)), rng.normal(0, 1.0, (B, n))], 1), rng.normal(0, 2.0, (B, n)), rng.normal(0, 1.0, (B, n))


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


@pytest.mark.parametrize("variant", ["atlas20", "atlas33"])
def test_parity_with_the_oracle_on_4096_worlds(variant):
    import nimblephysics_amd as na
    from oracle import OracleWorld
    md = na.atlas(variant)
    ow = OracleWorld(md)
    B, n = 4096, md.num_dofs
    S, A, g = _states(md, B, 1)
    w = na.World(md, device=DEV)
    st = torch.tensor(S, device=DEV, requires_grad=True)
    at = torch.tensor(A, device=DEV, requires_grad=True)
    tau = na.inverse_dynamics(w, st, at)
    assert tau.shape == (B, n) and tau.device == DEV
    tau.backward(torch.tensor(g, device=DEV))
    sc = torch.tensor(S, device=DEV, requires_grad=True)
    Cv = na.coriolis_and_gravity(w, sc)
    Cv.backward(torch.tensor(g, device=DEV))
    sm = torch.tensor(S, device=DEV, requires_grad=True)
    M = na.mass_matrix(w, sm)
    assert M.shape == (B, n, n)
    G = np.random.default_rng(2).normal(size=(B, n, n))
    M.backward(torch.tensor(G, device=DEV))
    tau, Cv, M = tau.detach().cpu().numpy(), Cv.detach().cpu().numpy(), M.detach().cpu().numpy()
    gs, ga, gc, gm = st.grad.cpu().numpy(), at.grad.cpu().numpy(), sc.grad.cpu().numpy(), sm.grad.cpu().numpy()
    worst = {"M": 0.0, "C": 0.0, "tau": 0.0, "gq": 0.0, "gv": 0.0, "ga": 0.0, "gCq": 0.0, "gCv": 0.0, "gMq": 0.0}
    for b in range(B):                                                    # every world
        q, v, a = S[b, :n], S[b, n:], A[b]
        Mo, Co = ow.mass_matrix(q), ow.coriolis_gravity(q, v)
        e = {"M": _rel(M[b], Mo), "C": _rel(Cv[b], Co), "tau": _rel(tau[b], Mo @ a + Co)}
        assert np.array_equal(M[b], M[b].T), b
        if b % 16 == 0:                                                   # the VJPs on every 16th world
            Jq, Jv, JM = ow.jac_C(q, v, 0), ow.jac_C(q, v, 1), ow.jac_Mx(q, a)
            e.update({"gq": _rel(gs[b, :n], (JM + Jq).T @ g[b]), "gv": _rel(gs[b, n:], Jv.T @ g[b]), "ga": _rel(ga[b], Mo.T @ g[b]),
                      "gCq": _rel(gc[b, :n], Jq.T @ g[b]), "gCv": _rel(gc[b, n:], Jv.T @ g[b])})
            # d <G, M(q)> / dq = sum_j jac_Mx(q, e_j)^T G[:, j]
            ref = sum(ow.jac_Mx(q, np.eye(n)[j]).T @ G[b][:, j] for j in range(n))
            e["gMq"] = _rel(gm[b, :n], ref)
            assert not gm[b, n:].any()
        for k, x in e.items():
            worst[k] = max(worst[k], x)
        assert max(e.values()) <= TOL, (variant, b, e)
    print(variant, "worst relative errors over", B, "worlds:", worst)


def _small_models():
    import nimblephysics_amd as na
    from test_ball_joint import ball_model
    return [("cartpole", na.cartpole()), ("ball_arm", ball_model(2, True))]


@pytest.mark.parametrize("which", [0, 1], ids=["cartpole", "ball_arm"])
def test_gradcheck(which):
    import nimblephysics_amd as na
    name, md = _small_models()[which]
    w = na.World(md, device=DEV)
    S, A, _ = _states(md, 3, 4)
    st = torch.tensor(S, device=DEV, requires_grad=True)
    at = torch.tensor(A, device=DEV, requires_grad=True)
    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda s, a: na.inverse_dynamics(w, s, a), (st, at), **kw)
    assert torch.autograd.gradcheck(lambda s, a: na.inverse_dynamics(w, s, a, joint_forces=True), (st, at), **kw)
    assert torch.autograd.gradcheck(lambda s: na.coriolis_and_gravity(w, s), (st,), **kw)
    assert torch.autograd.gradcheck(lambda s: na.mass_matrix(w, s), (st,), **kw)


@pytest.mark.parametrize("name", ["atlas20", "ball_arm", "free_below_root", "screw_arm", "screw_root"])
def test_the_device_kernels_equal_the_host_build_to_1e_13(name):
    """See the head of this file: 1e-13 relative (fused multiply-adds and sincos differ from the host build), not bit for bit."""
    import nimblephysics_amd as na
    from test_ball_joint import ball_model
    from test_dynamics_host import ShimDynamics, free_below_root, load_shim
    from test_screw_joint import screw_arm
    from nimblephysics_amd.dynamics import ID_JOINT_FORCES, inverse_dynamics_soa, inverse_dynamics_vjp_soa, mass_matrix_soa
    md = {"atlas20": lambda: na.atlas("atlas20"), "ball_arm": lambda: ball_model(2, True), "free_below_root": free_below_root,
          "screw_arm": lambda: screw_arm(2, True), "screw_root": lambda: screw_arm(2, False)}[name]()
    host = ShimDynamics(load_shim(), md)
    w = na.World(md, device=DEV)
    S, A, g = _states(md, 128, 6)
    s, a, gg = (torch.tensor(np.ascontiguousarray(x.T), device=DEV) for x in (S, A, g))
    worst = {}
    for flags in (0, ID_JOINT_FORCES):
        tau = inverse_dynamics_soa(w, s, a, flags).cpu().numpy()
        gs, ga = inverse_dynamics_vjp_soa(w, s, a, gg, flags)
        hgs, hga = host.vjp(S.T, A.T, g.T, flags)
        for key, x, ref in (("tau", tau, host.tau(S.T, A.T, flags)), ("grad_state", gs.cpu().numpy(), hgs), ("grad_accel", ga.cpu().numpy(), hga)):
            worst[(key, flags)] = _rel(x, ref)
    n = md.num_dofs
    worst["M"] = _rel(mass_matrix_soa(w, s).cpu().numpy().reshape(n, n, -1), host.mass(S.T))
    print(name, "device vs host build:", worst)
    assert max(worst.values()) <= 1e-13, worst


def test_shapes_and_devices():
    import nimblephysics_amd as na
    md = na.atlas("atlas20")
    n = md.num_dofs
    w = na.World(md, device=DEV)
    S, A, _ = _states(md, 6, 5)
    T1, B = 3, 2
    rows, acc = torch.tensor(S), torch.tensor(A)                          # CPU float64 in -> CPU out
    one = na.inverse_dynamics(w, rows[0], acc[0])
    assert one.shape == (n,) and one.device.type == "cpu"
    batch = na.inverse_dynamics(w, rows, acc)
    assert batch.shape == (6, n) and batch.device.type == "cpu" and torch.equal(batch[0], one)
    roll = na.inverse_dynamics(w, rows.reshape(B, T1, -1), acc.reshape(B, T1, -1))     # [B, T+1, 2n]
    assert roll.shape == (B, T1, n) and torch.equal(roll.reshape(6, n), batch)
    dev = na.inverse_dynamics(w, rows.to(DEV), acc.to(DEV))
    assert dev.device == DEV and torch.equal(dev.cpu(), batch)
    assert na.coriolis_and_gravity(w, rows[0]).shape == (n,) and na.coriolis_and_gravity(w, rows.reshape(B, T1, -1)).shape == (B, T1, n)
    M1 = na.mass_matrix(w, rows[0])
    Mb = na.mass_matrix(w, rows.reshape(B, T1, -1))
    assert M1.shape == (n, n) and M1.device.type == "cpu" and Mb.shape == (B, T1, n, n) and torch.equal(Mb[0, 0], M1)
    assert na.mass_matrix(w, rows.to(DEV)).device == DEV
    x = rows.clone().requires_grad_(True)
    y = acc.clone().requires_grad_(True)
    na.inverse_dynamics(w, x.reshape(B, T1, -1), y.reshape(B, T1, -1)).sum().backward()
    assert x.grad.device.type == "cpu" and x.grad.shape == x.shape and y.grad.device.type == "cpu" and y.grad.shape == y.shape
    z = rows.clone().requires_grad_(True)
    na.mass_matrix(w, z).sum().backward()
    import nimblephysics_amd.dynamics as dyn
    cap = dyn.MASS_BACKWARD_WORLDS
    try:                                                                  # cut into launches of whole columns: the same bits
        dyn.MASS_BACKWARD_WORLDS = 4 * 6
        z2 = rows.clone().requires_grad_(True)
        na.mass_matrix(w, z2).sum().backward()
    finally:
        dyn.MASS_BACKWARD_WORLDS = cap
    assert torch.equal(z2.grad, z.grad)
    assert z.grad.shape == z.shape and z.grad.device.type == "cpu" and not z.grad[:, n:].any() and z.grad[:, :n].abs().sum() > 0
    with pytest.raises(ValueError):
        na.inverse_dynamics(w, rows[:, :-1], acc)
    with pytest.raises(ValueError):
        na.inverse_dynamics(w, rows, acc[:3])


def test_a_residual_loss_over_a_pendulum_rollout_is_zero_and_reaches_state0():
    """tau = inverse_dynamics(states[t], (v[t+1] - v[t]) / dt) over a contact-free rollout with zero actions and no damping: ~0 (the step
    solves M a = -C and integrates v' = v + dt a), and the loss's gradient flows back to state0 through rollout()."""
    import copy
    import dataclasses
    import nimblephysics_amd as na
    from nimblephysics_amd.timestep import rollout
    md = copy.deepcopy(na.single_pendulum())
    md.bodies[0] = dataclasses.replace(md.bodies[0], damping=())
    assert not np.any(md.flat()["damping"])
    n, B, T = md.num_dofs, 32, 16
    w = na.World(md, device=DEV)
    rng = np.random.default_rng(7)
    s0 = torch.tensor(np.concatenate([rng.normal(0, 0.8, (B, n)), rng.normal(0, 1.0, (B, n))], 1), device=DEV, requires_grad=True)
    actions = torch.zeros((B, T, w.k), dtype=torch.float64, device=DEV)
    states = rollout(w, s0, actions)
    assert states.shape == (B, T + 1, 2 * n)
    acc = (states[:, 1:, n:] - states[:, :-1, n:]) / md.dt
    tau = na.inverse_dynamics(w, states[:, :-1], acc)
    assert tau.shape == (B, T, n)
    scale = float(na.coriolis_and_gravity(w, states.detach()).abs().max())
    print("pendulum residual", float(tau.detach().abs().max()), "against |C| =", scale)
    assert float(tau.detach().abs().max()) <= 1e-9 * max(1.0, scale)            # v' - v cancels ~1e-3 of v: 1e-16 / dt in the quotient
    # a loss with a known minimum elsewhere: the residual against a constant measured torque
    loss = ((tau - 0.3) ** 2).sum()
    loss.backward()
    assert s0.grad is not None and s0.grad.shape == s0.shape and torch.isfinite(s0.grad).all() and float(s0.grad.abs().max()) > 0
    # the damped pendulum with joint_forces=True: the same identity with the step's own damping term
    wd = na.World(na.single_pendulum(), device=DEV)
    sd = rollout(wd, s0.detach(), actions)
    td = na.inverse_dynamics(wd, sd[:, :-1], (sd[:, 1:, n:] - sd[:, :-1, n:]) / md.dt, joint_forces=True)
    assert float(td.abs().max()) <= 1e-9 * max(1.0, scale)


def test_set_masses_changes_the_mass_matrix_like_the_oracle():
    import nimblephysics_amd as na
    from nimblephysics_amd.mass import WrtMassBodyNodeEntryType as T
    from oracle import OracleWorld
    md = na.atlas("atlas20")
    n = md.num_dofs
    w = na.World(md, device=DEV)
    S, A, _ = _states(md, 16, 8)
    st = torch.tensor(S, device=DEV)
    before = na.mass_matrix(w, st).cpu().numpy()
    w.tuneMass(0, T.INERTIA_MASS); w.tuneMass(4, T.INERTIA_FULL)
    x = w.getMasses().numpy().copy()
    x[0] *= 1.3; x[1] *= 0.7; x[2:5] += 0.01; x[5:8] *= 1.2
    w.setMasses(x)
    after = na.mass_matrix(w, st).cpu().numpy()
    tau = na.inverse_dynamics(w, st, torch.tensor(A, device=DEV)).cpu().numpy()
    ow = OracleWorld(w.description)                                       # setMasses edited the World's description
    for b in range(16):
        Mo = ow.mass_matrix(S[b, :n])
        assert _rel(after[b], Mo) <= TOL
        assert _rel(tau[b], Mo @ A[b] + ow.coriolis_gravity(S[b, :n], S[b, n:])) <= TOL
    assert np.abs(after - before).max() > 1e-3                            # the edit matters


def test_bit_identity_deferred_join_getters_and_errors():
    import ctypes as C
    import nimblephysics_amd as na
    from nimblephysics_amd.dynamics import _workspace
    md = na.atlas("atlas20", ground=True)
    n, B = md.num_dofs, 4096
    S, A, g = _states(md, B, 9)
    S[:, 0] = -np.pi / 2; S[:, 4] += 1.0                                  # standing above the ground: the step below is contact-free or not, no matter
    w = na.World(md, device=DEV)
    st, at, gt = torch.tensor(S, device=DEV), torch.tensor(A, device=DEV), torch.tensor(g, device=DEV)

    def run(world, s, a, gg):
        x, y = s.clone().requires_grad_(True), a.clone().requires_grad_(True)
        t = na.inverse_dynamics(world, x, y)
        t.backward(gg)
        return t.detach(), x.grad, y.grad, na.mass_matrix(world, s), na.coriolis_and_gravity(world, s)
    first, second = run(w, st, at, gt), run(w, st, at, gt)
    for u, v in zip(first, second):
        assert torch.equal(u, v)
    for Bs in (1, 64):                                                    # a world's bits do not depend on B or on its place in the batch
        for off in (0, B - Bs):
            for u, v in zip(run(w, st[off:off + Bs], at[off:off + Bs], gt[off:off + Bs]), first):
                assert torch.equal(u, v[off:off + Bs])
    # the World getters on the current state; the state is left alone
    w.setState(st[:8])
    assert torch.equal(w.getMassMatrix(), first[3][:8]) and torch.equal(w.getCoriolisAndGravityForces(), first[4][:8])
    assert torch.equal(w.getState(), st[:8])
    w.setState(st[3])
    assert w.getMassMatrix().shape == (n, n) and torch.equal(w.getMassMatrix(), first[3][3])
    assert w.getCoriolisAndGravityForces().shape == (n,) and torch.equal(w.getCoriolisAndGravityForces(), first[4][3])
    # deferred join: the state comes straight out of a step whose slices are still in flight
    ref, dw = na.World(md, device=DEV), na.World(md, device=DEV)
    s_soa = ref.to_soa(st); a_soa = ref.to_soa(torch.zeros((B, ref.k), dtype=torch.float64, device=DEV))
    want_next, _, _ = ref.step_soa(s_soa, a_soa, want_saved=True)
    want = na.inverse_dynamics(ref, want_next.t(), at), na.mass_matrix(ref, want_next.t())
    dw.set_deferred_join(True)
    assert dw.slices_for(B) > 1
    buf = {"nxt": torch.empty_like(s_soa), "saved": torch.empty(dw.saved_bytes(B), dtype=torch.uint8, device=DEV),
           "status": torch.empty(B, dtype=torch.int32, device=DEV), "cache": torch.empty((dw.m, B), dtype=torch.float64, device=DEV)}
    dw.step_into(s_soa, a_soa, buf["nxt"], buf["saved"], buf["status"], None, buf["cache"])
    got = na.inverse_dynamics(dw, buf["nxt"].t(), at), na.mass_matrix(dw, buf["nxt"].t())
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    dw.join()
    torch.cuda.synchronize()
    # argument errors of the C ABI surface as NimbleAmdError
    L, h = w._L, w._h
    s8, a8 = w.to_soa(st[:8]), w.to_soa(at[:8])
    out = torch.empty((n, 8), dtype=torch.float64, device=DEV)
    ws = _workspace(w, 8)
    p = lambda t: C.c_void_p(t.data_ptr())
    from nimblephysics_amd._lib import check
    assert L.nbl_dynamics_workspace_bytes(h, 8) > 0 and L.nbl_dynamics_workspace_bytes(None, 8) == 0
    for rc_want, call in ((-1, lambda: L.nbl_inverse_dynamics_forward(None, 8, p(s8), p(a8), 0, p(out), p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_inverse_dynamics_forward(h, -1, p(s8), p(a8), 0, p(out), p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_inverse_dynamics_forward(h, 8, p(s8), p(a8), 8, p(out), p(ws), ws.numel(), None)),
                          (-4, lambda: L.nbl_inverse_dynamics_forward(h, 8, p(s8), p(a8), 0, p(out), p(ws), L.nbl_dynamics_workspace_bytes(h, 8) - 1, None)),
                          (-1, lambda: L.nbl_inverse_dynamics_backward(h, 8, p(s8), p(a8), 16, p(out), None, p(out), 0, p(ws), ws.numel(), None)),
                          (-4, lambda: L.nbl_inverse_dynamics_backward(h, 8, p(s8), p(a8), 0, p(out), None, p(out), 0, p(ws), 8, None)),
                          (-1, lambda: L.nbl_mass_matrix(h, 8, None, p(out), p(ws), ws.numel(), None)),
                          (-4, lambda: L.nbl_mass_matrix(h, 8, p(s8), p(out), p(ws), 0, None))):
        rc = call()
        assert rc == rc_want, (rc, rc_want)
        with pytest.raises(na.NimbleAmdError):
            check(rc, "dynamics")
        assert L.nbl_last_error()
    # ... and through dynamics.py itself: unknown flag bits and a batch that does not fit the state's
    from nimblephysics_amd.dynamics import InverseDynamicsLayer, inverse_dynamics_soa, inverse_dynamics_vjp_soa
    with pytest.raises(na.NimbleAmdError, match="flag"):
        inverse_dynamics_soa(w, s8, a8, 8)
    with pytest.raises(na.NimbleAmdError, match="flag"):
        inverse_dynamics_vjp_soa(w, s8, a8, a8, 32)
    with pytest.raises(na.NimbleAmdError, match="flag"):
        InverseDynamicsLayer.apply(w, st[:8], at[:8], 64)


def test_immobile_skeletons_take_the_references_layout(tmp_path):
    import nimblephysics_amd as na
    from test_ref_layout import load
    md = load(tmp_path)
    w = na.World(md, device=DEV)
    assert w.ref_layout is not None and w.getStateSize() == 24 and w.n == 6
    rng = np.random.default_rng(1)
    full = np.zeros((8, 24)); full[:, 6:12] = rng.normal(0, 0.3, (8, 6)); full[:, 18:] = rng.normal(0, 1, (8, 6))
    afull = np.zeros((8, 12)); afull[:, 6:] = rng.normal(0, 1, (8, 6))
    x = torch.tensor(full, device=DEV, requires_grad=True)
    y = torch.tensor(afull, device=DEV, requires_grad=True)
    tau = na.inverse_dynamics(w, x, y)
    w2 = na.World(md, device=DEV); w2.ref_layout = None                   # the device's own (shorter) layout
    xs = torch.tensor(np.concatenate([full[:, 6:12], full[:, 18:]], 1), device=DEV)
    assert tau.shape == (8, 6) and torch.equal(tau.detach(), na.inverse_dynamics(w2, xs, torch.tensor(afull[:, 6:], device=DEV)))
    tau.sum().backward()
    assert not x.grad[:, :6].any() and not x.grad[:, 12:18].any() and x.grad[:, 6:12].abs().sum() > 0 and not y.grad[:, :6].any()
    M = na.mass_matrix(w, x.detach())
    assert M.shape == (8, 6, 6) and torch.equal(M, na.mass_matrix(w2, xs))


def test_plain_c_dynamics_driver(tmp_path):
    """tests/c_abi_example/dynamics.c: the three entry points from pure C99 on the Atlas-20 model header; M a + C == tau from the library's
    own outputs, grad_accel == M^T g, the argument errors."""
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/lib/libamdhip64.so"):
        pytest.skip("no gcc / ROCm runtime")
    libdir = os.path.join(ROOT, "nimblephysics_amd")
    exe = str(tmp_path / "dynamics")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_abi_example", "dynamics.c"), "-o", exe, "-L" + libdir, "-lnimble_amd",
                           "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath," + libdir])
    out = subprocess.check_output([exe, "64"]).decode()
    print(out)
    assert "max residuals" in out and "asymmetric 0" in out
