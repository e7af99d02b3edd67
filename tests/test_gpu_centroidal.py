"""The centre-of-mass family on the device (csrc/centroidal.hip through nimblephysics_amd/centroidal.py): every output and every gradient
against tests/cen_numpy.py at the bounds of tests/test_centroidal_host.py (forward outputs and closed-form gradients 1e-10 of max(1, |ref|);
the other gradients 100 x the disagreement of the reference's own central differences at 1e-5 and 1e-6, floored at 1e-8), the host build of
the same header (1e-13 relative, not bit for bit: fused multiply-adds and sincos differ, as test_gpu_dynamics.py's header explains),
torch.autograd.gradcheck, Newton's law through forward_dynamics, d pe / dq = C(q, 0), d ke / dv = M v, Jcom v = com_vel, the reference's
potential-energy rule, rollout shapes and bit-reproducibility, composition with rollout(), setMasses, deferred join, CPU tensors, argument
errors.  Batches B in {1, 63, 65, 130}: the lane tails around a wavefront and a block."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-10
NAMES = ("com", "com_vel", "com_acc", "momentum", "ke", "pe")
ROWS = (3, 3, 3, 6, 1, 1)


def _states(md, B, seed):
    from test_gpu_dynamics import _states as draw
    S, A, _ = draw(md, B, seed)
    return S, A


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def _model(name):
    import nimblephysics_amd as na
    from test_ball_joint import ball_model
    from test_screw_joint import screw_arm
    return {"screw_arm": lambda: screw_arm(2, True), "screw_root": lambda: screw_arm(2, False),
            "cartpole": na.cartpole, "ball_arm": lambda: ball_model(2, True), "atlas20_ground": lambda: na.atlas("atlas20", ground=True),
            "atlas33": lambda: na.atlas("atlas33"), "atlas20": lambda: na.atlas("atlas20"), "pendulum": na.single_pendulum}[name]()


_REF = {}


def _reference(name, md, S, A, cots, fd_worlds):
    """cen_numpy on every world (outputs, closed-form gradients) and its central differences on `fd_worlds`; computed once per model"""
    import cen_numpy
    from oracle import OracleWorld
    if name in _REF:
        return _REF[name]
    ow = OracleWorld(md)
    sel, n = cen_numpy.default_set(md), md.num_dofs
    out = {"fwd": [], "cf": [], "fd": {}}
    for b in range(S.shape[0]):
        q, v, a = S[b, :n], S[b, n:], A[b]
        cot = {nm: c[b] for nm, c in zip(NAMES, cots)}
        out["fwd"].append(cen_numpy.outputs(ow, md, sel, q, v, a))
        out["cf"].append(cen_numpy.closed_form_vjp(ow, md, sel, q, v, cot, True))
        if b in fd_worlds:
            out["fd"][b] = (cen_numpy.fd_vjp(ow, md, sel, q, v, a, cot, 1e-5), cen_numpy.fd_vjp(ow, md, sel, q, v, a, cot, 1e-6))
    _REF[name] = out
    return out


@pytest.mark.parametrize("B", [1, 63, 65, 130])
@pytest.mark.parametrize("name", ["cartpole", "ball_arm", "atlas20_ground", "atlas33", "screw_arm", "screw_root"])
def test_device_equals_cen_numpy_and_the_host_build(name, B):
    """Every world is checked.  The states of the smaller batches are the first worlds of the largest one, so the reference is computed once
    per model.  Forward outputs, closed-form gradients and the comparison with the host build cover EVERY world; the finite-difference
    reference (numpy, 12 n evaluations per world: the slow part) covers worlds 0, 62, 64 and 129 - the first lane, the first lane of the
    second block and the last world of every batch size, so each B has its tail world checked."""
    import nimblephysics_amd as na
    from nimblephysics_amd.centroidal import centroidal_soa, centroidal_vjp_soa, _body_set
    from test_centroidal_host import ShimCentroidal, load_shim
    md = _model(name)
    n = md.num_dofs
    S, A = _states(md, 130, 71)
    rng = np.random.default_rng(72)
    cots = [rng.normal(0, 1.0, (130, r)) for r in ROWS]
    ref = _reference(name, md, S, A, cots, (0, 62, 64, 129))
    S, A, cots = S[:B], A[:B], [c[:B] for c in cots]
    w = na.World(md, device=DEV)
    out = na.centroidal(w, torch.tensor(S, device=DEV), torch.tensor(A, device=DEV))
    J = na.com_jacobian(w, torch.tensor(S, device=DEV)).cpu().numpy()
    assert out.com.shape == (B, 3) and out.momentum.shape == (B, 6) and out.ke.shape == (B,) and J.shape == (B, 3, n)
    grads = {}
    for k, nm in enumerate(NAMES):
        st = torch.tensor(S, device=DEV, requires_grad=True)
        at = torch.tensor(A, device=DEV, requires_grad=True)
        o = na.centroidal(w, st, at)[k]
        o.backward(torch.tensor(cots[k].reshape(o.shape), device=DEV))
        grads[nm] = np.concatenate([st.grad.cpu().numpy(), at.grad.cpu().numpy()], 1)
    dev = {nm: getattr(out, nm).cpu().numpy().reshape(B, -1) for nm in NAMES}
    mass = w.getMass()
    worst = {}
    for b in range(B):
        r = ref["fwd"][b]
        e = {nm: _rel(dev[nm][b], r[nm]) for nm in NAMES}
        e["Jcom"], e["mass"] = _rel(J[b], r["Jcom"]), abs(mass - r["mass"]) / r["mass"]
        g = {"com_q": grads["com"][b, :n], "com_vel_v": grads["com_vel"][b, n:2 * n], "com_acc_a": grads["com_acc"][b, 2 * n:],
             "pe_q": grads["pe"][b, :n], "ke_v": grads["ke"][b, n:2 * n], "ke_q": grads["ke"][b, :n]}
        e.update({kk: _rel(g[kk], x) for kk, x in ref["cf"][b].items()})
        assert _rel(dev["momentum"][b, 3:], mass * dev["com_vel"][b]) <= 1e-13, (name, b)
        if b in ref["fd"]:
            fd5, fd6 = ref["fd"][b]
            for nm in NAMES:
                bound = max(100.0 * _rel(fd5[nm], fd6[nm]), 1e-8)
                x = _rel(grads[nm][b], fd6[nm])
                worst["fd " + nm] = max(worst.get("fd " + nm, 0.0), x)
                assert x <= bound, (name, b, nm, x, bound)
        for kk, x in e.items():
            worst[kk] = max(worst.get(kk, 0.0), x)
        assert max(e.values()) <= TOL, (name, b, e)
    # the host build of the same header
    host = ShimCentroidal(load_shim(), md)
    houts, hJ = host.forward(S.T, A.T, jac=True)
    hgs, hga = host.vjp(S.T, A.T, [c.T for c in cots])
    s, a = w.to_soa(torch.tensor(S, device=DEV)), w.to_soa(torch.tensor(A, device=DEV))
    bset = _body_set(w)
    douts, dJ = centroidal_soa(w, bset, s, a, 0, (True,) * 6, True)
    dcots = [torch.tensor(np.ascontiguousarray(c.T if r > 1 else c[:, 0]), device=DEV) for c, r in zip(cots, ROWS)]
    dgs, dga = centroidal_vjp_soa(w, bset, s, a, dcots)
    pairs = [(nm, o.cpu().numpy().reshape(h.shape), h) for nm, o, h in zip(NAMES, douts, houts)]
    pairs += [("Jcom", dJ.cpu().numpy(), hJ), ("grad_state", dgs.cpu().numpy(), hgs), ("grad_accel", dga.cpu().numpy(), hga)]
    vs_host = {nm: _rel(x, h) for nm, x, h in pairs}
    print(name, B, "worst vs cen_numpy:", worst, "| device vs host build:", vs_host)
    assert max(vs_host.values()) <= 1e-13, vs_host


@pytest.mark.parametrize("name", ["cartpole", "ball_arm"])
def test_gradcheck(name):
    import nimblephysics_amd as na
    md = _model(name)
    w = na.World(md, device=DEV)
    S, A = _states(md, 3, 73)
    st = torch.tensor(S, device=DEV, requires_grad=True)
    at = torch.tensor(A, device=DEV, requires_grad=True)
    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda s, a: tuple(na.centroidal(w, s, a)), (st, at), **kw)
    assert torch.autograd.gradcheck(lambda s: tuple(x for x in na.centroidal(w, s, at_com=False) if x is not None), (st,), **kw)


def test_newtons_law_the_com_accelerates_with_gravity_plus_the_external_forces_over_the_mass():
    import nimblephysics_amd as na
    md = _model("atlas20")
    n, B = md.num_dofs, 64
    w = na.World(md, device=DEV)
    S, _ = _states(md, B, 74)
    rng = np.random.default_rng(75)
    tau = rng.normal(0, 5.0, (B, n)); tau[:, :6] = 0.0
    st, tt = torch.tensor(S, device=DEV), torch.tensor(tau, device=DEV)
    g = np.asarray(md.gravity, dtype=np.float64)
    gn = np.linalg.norm(g)
    acc = na.forward_dynamics(w, st, tt)
    cdd = na.com_acceleration(w, st, acc).cpu().numpy()
    e0 = np.abs(cdd - g).max() / gn
    W = rng.normal(0, 30.0, (B, 12))
    acc = na.forward_dynamics(w, st, tt, wrenches=torch.tensor(W, device=DEV), bodies=["l_foot", "r_foot"], world_frame=True)
    cdd = na.com_acceleration(w, st, acc).cpu().numpy()
    e1 = np.abs(cdd - (g + (W[:, 3:6] + W[:, 9:12]) / w.getMass())).max() / gn
    print("Newton's law, relative to |g|:", e0, e1)
    assert e0 <= TOL and e1 <= TOL and np.abs(W[:, 3:6] + W[:, 9:12]).max() / w.getMass() > 0.1


@pytest.mark.parametrize("name", ["cartpole", "pendulum"])
def test_energy_gradients_are_the_gravity_force_and_the_momentum_and_jcom_is_the_jacobian_of_the_com(name):
    import nimblephysics_amd as na
    from nimblephysics_amd.dynamics import ID_NO_GRAVITY, ID_NO_VELOCITY, InverseDynamicsLayer
    md = _model(name)
    n, B = md.num_dofs, 65
    w = na.World(md, device=DEV)
    S, _ = _states(md, B, 76)
    st = torch.tensor(S, device=DEV, requires_grad=True)
    na.potential_energy(w, st, at_com=True, springs=False).sum().backward()
    zero_v = torch.tensor(np.concatenate([S[:, :n], np.zeros((B, n))], 1), device=DEV)
    Cg = na.coriolis_and_gravity(w, zero_v)
    assert _rel(st.grad[:, :n].cpu().numpy(), Cg.cpu().numpy()) <= TOL and not st.grad[:, n:].any()
    sk = torch.tensor(S, device=DEV, requires_grad=True)
    na.kinetic_energy(w, sk).sum().backward()
    Mv = InverseDynamicsLayer.apply(w, torch.tensor(S, device=DEV), torch.tensor(S[:, n:], device=DEV), ID_NO_VELOCITY | ID_NO_GRAVITY)
    assert _rel(sk.grad[:, n:].cpu().numpy(), Mv.cpu().numpy()) <= TOL
    J = na.com_jacobian(w, torch.tensor(S, device=DEV))
    assert not J.requires_grad
    cv = na.com_velocity(w, torch.tensor(S, device=DEV))
    assert _rel(torch.einsum("bij,bj->bi", J, torch.tensor(S[:, n:], device=DEV)).cpu().numpy(), cv.cpu().numpy()) <= 1e-13
    rows = []
    for r in range(3):                                              # revolute / prismatic coordinates only: d com / dq IS the velocity Jacobian
        sr = torch.tensor(S, device=DEV, requires_grad=True)
        na.center_of_mass(w, sr)[:, r].sum().backward()
        rows.append(sr.grad[:, :n])
    assert _rel(torch.stack(rows, 1).cpu().numpy(), J.cpu().numpy()) <= TOL


def test_the_worlds_potential_energy_follows_the_references_body_origin_rule():
    import cen_numpy
    import nimblephysics_amd as na
    from oracle import OracleWorld
    md = _model("atlas20")                                           # non-zero local centres of mass, welded hands, joint springs or not
    n, B = md.num_dofs, 5
    w = na.World(md, device=DEV)
    S, A = _states(md, B, 77)
    w.setState(torch.tensor(S, device=DEV))
    pe_ref = w.computePotentialEnergy().cpu().numpy()
    pe_com = na.potential_energy(w, torch.tensor(S, device=DEV)).cpu().numpy()
    ow, sel = OracleWorld(md), cen_numpy.default_set(md)
    for b in range(B):
        k = cen_numpy.Kin(ow, md, S[b, :n], sel)
        assert _rel(pe_ref[b], k.pe(md.gravity, at_com=False)) <= TOL and _rel(pe_com[b], k.pe(md.gravity, at_com=True)) <= TOL
    assert np.abs(pe_ref - pe_com).min() > 1e-3                      # the flag is not a no-op
    # the other getters on the current state, detached, and the 1-D convention
    full = na.centroidal(w, torch.tensor(S, device=DEV), torch.tensor(A, device=DEV))
    assert torch.equal(w.getCOM(), full.com) and torch.equal(w.getCOMLinearVelocity(), full.com_vel) and torch.equal(w.computeKineticEnergy(), full.ke)
    assert torch.equal(w.getCOMLinearAcceleration(torch.tensor(A, device=DEV)), full.com_acc)
    assert torch.equal(w.getCOMLinearJacobian(), na.com_jacobian(w, torch.tensor(S, device=DEV)))
    assert torch.equal(w.getState(), torch.tensor(S, device=DEV))
    w.setState(torch.tensor(S[2], device=DEV))
    assert w.getCOM().shape == (3,) and torch.equal(w.getCOM(), full.com[2]) and w.getCOMLinearJacobian().shape == (3, n)
    assert w.computeKineticEnergy().shape == () and abs(w.getMass() - sum(b.mass for b in md.bodies)) <= 1e-12 * w.getMass()


def test_rollout_shape_batch_independence_and_reproducibility():
    import nimblephysics_amd as na
    md = _model("atlas20_ground")
    n, T1, B = md.num_dofs, 3, 130
    w = na.World(md, device=DEV)
    S, A = _states(md, T1 * B, 78)
    rng = np.random.default_rng(79)

    def run(s, a, cot):
        x, y = s.clone().requires_grad_(True), a.clone().requires_grad_(True)
        out = na.centroidal(w, x, y)
        torch.autograd.backward(list(out), [c.reshape(o.shape) for c, o in zip(cot, out)])
        return [o.detach() for o in out] + [x.grad, y.grad]
    st, at = torch.tensor(S, device=DEV).reshape(T1, B, 2 * n), torch.tensor(A, device=DEV).reshape(T1, B, n)
    cot = [torch.tensor(rng.normal(0, 1.0, (T1, B, r)), device=DEV) for r in ROWS]
    whole, again = run(st, at, cot), run(st, at, cot)
    assert whole[0].shape == (T1, B, 3) and whole[4].shape == (T1, B) and whole[6].shape == (T1, B, 2 * n) and whole[7].shape == (T1, B, n)
    assert all(torch.equal(u, v) for u, v in zip(whole, again))                          # two runs: the same bits
    for t in range(T1):                                                                  # one launch over the rollout = the per-step calls
        step = run(st[t], at[t], [c[t] for c in cot])
        assert all(torch.equal(u, v[t]) for u, v in zip(step, whole))
    one = run(st[0, 77:78], at[0, 77:78], [c[0, 77:78] for c in cot])                    # B = 1 against slot 77 of B = 130
    assert all(torch.equal(u[0], v[0, 77]) for u, v in zip(one, whole))


def test_a_loss_on_the_com_after_a_rollout_reaches_state0_like_the_chained_oracle():
    import cen_numpy
    import nimblephysics_amd as na
    from nimblephysics_amd.timestep import rollout
    from oracle import OracleWorld
    md = _model("cartpole")
    n, k, B, T = md.num_dofs, len(md.action_map), 4, 3
    w = na.World(md, device=DEV)
    S, _ = _states(md, B, 80)
    a = np.random.default_rng(81).normal(0, 0.5, (B, T, k))
    goal = np.array([0.3, -0.2, 0.1])
    s0 = torch.tensor(S, device=DEV, requires_grad=True)
    at = torch.tensor(a, device=DEV, requires_grad=True)
    c = na.center_of_mass(w, rollout(w, s0, at)[:, -1])
    ((c - torch.tensor(goal, device=DEV)) ** 2).sum().backward()
    ow, sel = OracleWorld(md), cen_numpy.default_set(md)
    states = [S]
    for t in range(T):
        states.append(ow.step_batch(states[-1], a[:, t], None)["next"])
    g = np.zeros((B, 2 * n))
    for b in range(B):
        kin = cen_numpy.Kin(ow, md, states[-1][b, :n], sel)
        g[b, :n] = kin.jcom(position=True).T @ (2 * (kin.com() - goal))
    ga = np.zeros((B, T, k))
    for t in reversed(range(T)):
        r = ow.step_batch(states[t], a[:, t], g)
        g, ga[:, t] = r["grad_state"], r["grad_action"]
    e = _rel(c.detach().cpu().numpy(), np.stack([cen_numpy.Kin(ow, md, states[-1][b, :n], sel).com() for b in range(B)]))
    es, ea = _rel(s0.grad.cpu().numpy(), g), _rel(at.grad.cpu().numpy(), ga)
    print("com after the rollout", e, "grad_state0", es, "grad_actions", ea)
    assert e <= 1e-7 and es <= 1e-7 and ea <= 1e-7 and np.abs(g).max() > 1e-3


def test_set_masses_moves_the_mass_and_the_com():
    import cen_numpy
    import nimblephysics_amd as na
    from nimblephysics_amd.mass import WrtMassBodyNodeEntryType as T
    from oracle import OracleWorld
    md = _model("atlas20")
    n = md.num_dofs
    w = na.World(md, device=DEV)
    S, _ = _states(md, 4, 82)
    st = torch.tensor(S, device=DEV)
    m0, c0 = w.getMass(), na.center_of_mass(w, st).cpu().numpy()
    w.tuneMass(0, T.INERTIA_MASS); w.tuneMass(4, T.INERTIA_FULL)
    x = w.getMasses().numpy().copy()
    x[0] *= 1.3; x[1] *= 0.7; x[2:5] += 0.01
    w.setMasses(x)
    m1, c1 = w.getMass(), na.center_of_mass(w, st).cpu().numpy()
    ow, sel = OracleWorld(w.description), cen_numpy.default_set(w.description)
    for b in range(4):
        kin = cen_numpy.Kin(ow, w.description, S[b, :n], sel)
        assert _rel(c1[b], kin.com()) <= TOL and abs(m1 - kin.M) <= 1e-12 * kin.M
    assert abs(m1 - m0) > 1e-3 and np.abs(c1 - c0).max() > 1e-4


def test_deferred_join_cpu_tensors_body_sets_and_argument_errors():
    import nimblephysics_amd as na
    from nimblephysics_amd._lib import check
    from nimblephysics_amd.centroidal import CentroidalLayer, _body_set, _workspace
    md = _model("atlas20_ground")
    n, B = md.num_dofs, 4096
    S, A = _states(md, B, 83)
    S[:, 0] = -np.pi / 2; S[:, 4] += 1.0
    st, at = torch.tensor(S, device=DEV), torch.tensor(A, device=DEV)
    # deferred join: the state comes straight out of a step whose slices are still in flight
    ref, dw = na.World(md, device=DEV), na.World(md, device=DEV)
    s_soa = ref.to_soa(st); a_soa = ref.to_soa(torch.zeros((B, ref.k), dtype=torch.float64, device=DEV))
    want_next, _, _ = ref.step_soa(s_soa, a_soa, want_saved=True)
    want = na.centroidal(ref, want_next.t(), at)
    dw.set_deferred_join(True)
    assert dw.slices_for(B) > 1
    buf = {"nxt": torch.empty_like(s_soa), "saved": torch.empty(dw.saved_bytes(B), dtype=torch.uint8, device=DEV),
           "status": torch.empty(B, dtype=torch.int32, device=DEV), "cache": torch.empty((dw.m, B), dtype=torch.float64, device=DEV)}
    dw.step_into(s_soa, a_soa, buf["nxt"], buf["saved"], buf["status"], None, buf["cache"])
    got = na.centroidal(dw, buf["nxt"].t(), at)
    assert all(torch.equal(u, v) for u, v in zip(got, want))
    dw.join()
    torch.cuda.synchronize()
    # CPU float64 tensors in and out, [2n] and [B, 2n]; gradients come back on the CPU
    w = ref
    full = na.centroidal(w, st[:6], at[:6])
    x, y = torch.tensor(S[:6], requires_grad=True), torch.tensor(A[:6], requires_grad=True)
    cpu = na.centroidal(w, x, y)
    assert all(o.device.type == "cpu" and torch.equal(o, f.cpu()) for o, f in zip(cpu, full))
    (cpu.ke.sum() + cpu.com_acc.sum()).backward()
    assert x.grad.device.type == "cpu" and x.grad.shape == x.shape and y.grad.shape == y.shape and float(y.grad.abs().max()) > 0
    one = na.center_of_mass(w, torch.tensor(S[0]))
    assert one.shape == (3,) and one.device.type == "cpu" and torch.equal(one, full.com[0].cpu())
    assert na.centroidal(w, st[:6]).com_acc is None and na.kinetic_energy(w, torch.tensor(S[0])).shape == ()
    # sets: a skeleton, the feet; each output alone is the same bits as in the joint call
    sk = md.body_skeletons()[[b.name for b in md.bodies].index("l_foot")]
    assert torch.equal(na.center_of_mass(w, st[:6], skeleton=sk), full.com) and abs(w.getMass(sk) - w.getMass()) == 0
    feet = na.centroidal(w, st[:6], at[:6], bodies=["l_foot", "r_foot"])
    assert float((feet.com - full.com).abs().max()) > 1e-2
    assert torch.equal(na.com_velocity(w, st[:6]), full.com_vel) and torch.equal(na.centroidal_momentum(w, st[:6]), full.momentum)
    assert torch.equal(na.com_acceleration(w, st[:6], at[:6]), full.com_acc) and torch.equal(na.potential_energy(w, st[:6]), full.pe)
    targets, _ = md.weld_targets()
    welded = [i for i, b in enumerate(md.bodies) if b.joint_type == "weld" and targets[i] >= 0]
    with pytest.raises(na.NimbleAmdError, match="welded into one body"):
        na.center_of_mass(w, st[:6], bodies=[md.bodies[welded[0]].name])
    with pytest.raises(na.NimbleAmdError, match="accelerations"):
        CentroidalLayer.apply(w, st[:6], None, _body_set(w), 0, (False, False, True, False, False, False))
    with pytest.raises(na.NimbleAmdError, match="flag"):
        CentroidalLayer.apply(w, st[:6], None, _body_set(w), 8, (True,) + (False,) * 5)
    with pytest.raises(ValueError):
        na.centroidal(w, st[:6], at[:5])
    # the C ABI's own refusals
    other = na.World(_model("cartpole"), device=DEV)                  # a set belongs to the model it was made for
    wc_other = lambda: other
    L, h = w._L, w._h
    p = lambda t: C.c_void_p(t.data_ptr())
    s8, a8 = w.to_soa(st[:8]), w.to_soa(at[:8])
    o3 = torch.empty((3, 8), dtype=torch.float64, device=DEV)
    gs = torch.empty((2 * n, 8), dtype=torch.float64, device=DEV)
    ws, bs = _workspace(w, 8), _body_set(w).ptr
    need = L.nbl_centroidal_workspace_bytes(h, 8)
    assert need == 8 * L.nbl_centroidal_workspace_bytes(h, 1) and need % (8 * 54 * 8) == 0 and L.nbl_centroidal_workspace_bytes(None, 8) == 0
    N = None
    for rc_want, call in ((-1, lambda: L.nbl_centroidal_forward(None, bs, 8, p(s8), N, 0, p(o3), N, N, N, N, N, N, p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_centroidal_forward(h, None, 8, p(s8), N, 0, p(o3), N, N, N, N, N, N, p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_centroidal_forward(h, bs, 8, None, N, 0, p(o3), N, N, N, N, N, N, p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_centroidal_forward(h, bs, -1, p(s8), N, 0, p(o3), N, N, N, N, N, N, p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_centroidal_forward(h, bs, 8, p(s8), N, 4, p(o3), N, N, N, N, N, N, p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_centroidal_forward(h, bs, 8, p(s8), N, 0, N, N, p(o3), N, N, N, N, p(ws), ws.numel(), None)),
                          (-4, lambda: L.nbl_centroidal_forward(h, bs, 8, p(s8), N, 0, p(o3), N, N, N, N, N, N, p(ws), need - 1, None)),
                          (-1, lambda: L.nbl_centroidal_backward(h, bs, 8, p(s8), N, 0, N, N, p(o3), N, N, N, p(gs), N, 0, p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_centroidal_backward(h, bs, 8, p(s8), p(a8), 16, p(o3), N, N, N, N, N, p(gs), N, 0, p(ws), ws.numel(), None)),
                          (-4, lambda: L.nbl_centroidal_backward(h, bs, 8, p(s8), p(a8), 0, p(o3), N, N, N, N, N, p(gs), N, 0, p(ws), 8, None))):
        rc = call()
        assert rc == rc_want, (rc, rc_want)
        with pytest.raises(na.NimbleAmdError):
            check(rc, "centroidal")
        assert L.nbl_last_error()
    assert L.nbl_centroidal_forward(h, bs, 0, None, N, 0, N, N, N, N, N, N, N, None, 0, None) == 0          # B = 0 is a no-op
    assert L.nbl_body_set_mass(h, bs) == w.getMass() > 0 and L.nbl_body_set_mass(wc_other()._h, bs) == 0.0 and b"another model" in L.nbl_last_error()
    out = C.c_void_p()
    two = np.asarray([1, 1], dtype=np.int32)
    assert L.nbl_body_set_create(h, 2, two.ctypes.data_as(C.c_void_p), C.byref(out)) == -1                  # a body named twice
    far = np.asarray([10 ** 6], dtype=np.int32)
    assert L.nbl_body_set_create(h, 1, far.ctypes.data_as(C.c_void_p), C.byref(out)) == -1
    # a set without mass: the massless links of a compound joint are bodies of the model description
    import os
    cj = na.load_skel(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "compound_joints.skel"))
    wc = na.World(cj, device=DEV)
    massless = [i for i, b in enumerate(wc.model.bodies) if float(b.mass) == 0.0]
    assert massless, "the compound-joint fixture has massless links"
    arr = np.asarray(massless[:1], dtype=np.int32)
    assert wc._L.nbl_body_set_create(wc._h, 1, arr.ctypes.data_as(C.c_void_p), C.byref(out)) == -1 and b"mass" in wc._L.nbl_last_error()
    # the kernels are registered with the per-kernel timers
    names = [L.nbl_kernel_name(i).decode() for i in range(L.nbl_kernel_count())]
    assert "k_centroidal" in names and "k_centroidal_vjp" in names
