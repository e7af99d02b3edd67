"""World-space body kinematics on the device (csrc/kinematics.hip through nimblephysics_amd/mapping.py): IKMapping rows, map_to_pos /
map_to_vel and their vector-Jacobian products against the CPU oracle and the numpy statement of the reference's Jacobians
(tests/kin_numpy.py); shapes and devices; composition with rollout() and timestep(); bit-reproducibility, handle changes, deferred join
and the reference's state layout of worlds with immobile skeletons."""
import numpy as np
import pytest
import torch

from kin_numpy import mapping_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LIMBS = ("l_hand", "r_hand", "l_foot", "r_foot")           # atlas: the hands are welded to the forearms (offset entries)


def _atlas_states(md, B, seed, sigma=0.3):
    rng = np.random.default_rng(seed)
    n = md.num_dofs
    q = rng.normal(0, sigma, (B, n)); q[:, 0] = -np.pi / 2 + rng.normal(0, 0.1, B)
    q[:, 3:6] = rng.normal(0, 0.5, (B, 3))
    v = rng.normal(0, 1.0, (B, n))
    return np.concatenate([q, v], 1)


def _away_from_pi(md, ow, S, B, names=LIMBS):
    """the first B states of S whose entry rotations all stay at least 0.3 rad below theta = pi (the reference's dLogMap takes a special
    branch above pi - 1e-6 that the device does not restate; near it logMap itself loses digits)"""
    ent = _entries(md, names)
    n = md.num_dofs
    keep = [b for b in range(S.shape[0])
            if all(np.arccos(np.clip(0.5 * (np.trace(ow.body_world_transform(S[b, :n], e)[:3, :3]) - 1), -1, 1)) < np.pi - 0.3 for _, e in ent)]
    assert len(keep) >= B
    return S[keep[:B]]


def _mapping(world, names=LIMBS, kind="spatial"):
    import nimblephysics_amd as na
    m = na.neural.IKMapping(world)
    for nm in names:
        {"spatial": m.addSpatialBodyNode, "linear": m.addLinearBodyNode, "angular": m.addAngularBodyNode}[kind](nm)
    return m


def _entries(md, names=LIMBS, kind=0):
    return [(kind, [b.name for b in md.bodies].index(nm)) for nm in names]


def _rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


@pytest.mark.parametrize("variant", ["atlas20", "atlas33"])
def test_rows_and_vjps_equal_the_oracle(variant):
    import nimblephysics_amd as na
    from oracle import OracleWorld
    md = na.atlas(variant)
    ow = OracleWorld(md)
    B, n = 4096, md.num_dofs
    S = _away_from_pi(md, ow, _atlas_states(md, 2 * B, 1), B)
    w = na.World(md, device=DEV)
    m = _mapping(w)
    st = torch.tensor(S, device=DEV, requires_grad=True)
    pos = na.map_to_pos(w, m, st)
    vel = na.map_to_vel(w, m, torch.tensor(S, device=DEV))
    assert pos.shape == (B, 24) and pos.device == DEV
    g = torch.tensor(np.random.default_rng(2).normal(size=(B, 24)), device=DEV)
    pos.backward(g)
    pos, vel, grad, g = pos.detach().cpu().numpy(), vel.cpu().numpy(), st.grad.cpu().numpy(), g.cpu().numpy()
    ent = _entries(md)
    for b in range(B):                                        # positions of every world: the oracle's transforms + logMap
        T = [ow.body_world_transform(S[b, :n], e) for _, e in ent]
        ref = np.concatenate([np.concatenate([_logmap(t[:3, :3]), t[:3, 3]]) for t in T])
        assert np.abs(pos[b] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), b
    for b in range(0, B, 16):                                 # velocities and VJPs: the numpy Jacobians on every 16th world
        _, Jp, Jv = mapping_rows(ow, md, S[b, :n], ent)
        assert _rel(vel[b], Jv @ S[b, n:]) <= 1e-10, b
        assert _rel(grad[b, :n], Jp.T @ g[b]) <= 1e-10, b
        assert not grad[b, n:].any()


def _logmap(R):
    from kin_numpy import logmap
    return logmap(R)


def test_gradcheck_and_the_dense_getters():
    import nimblephysics_amd as na
    from oracle import OracleWorld
    md = na.atlas("atlas20")
    ow = OracleWorld(md)
    n = md.num_dofs
    S = _away_from_pi(md, ow, _atlas_states(md, 32, 4), 3, LIMBS + ("pelvis",))
    w = na.World(md, device=DEV)
    m = _mapping(w)
    m.addLinearBodyNode("utorso"); m.addAngularBodyNode("pelvis")
    st = torch.tensor(S, device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda s: na.map_to_pos(w, m, s), (st,), eps=1e-6, atol=1e-6, rtol=1e-5)
    # map_to_vel: the reference's layer keeps d(J v)/dq out, so the check runs on the velocity coordinates only
    q0 = torch.tensor(S[:, :n], device=DEV)
    v0 = torch.tensor(S[:, n:], device=DEV, requires_grad=True)
    assert torch.autograd.gradcheck(lambda v: na.map_to_vel(w, m, torch.cat([q0, v], 1)), (v0,), eps=1e-6, atol=1e-6, rtol=1e-5)
    w.setState(torch.tensor(S, device=DEV))
    Jp, Jv = m.getRealPosToMappedPosJac(w).cpu().numpy(), m.getRealVelToMappedVelJac(w).cpu().numpy()
    P = m.getPosDim()
    assert Jp.shape == (3, P, n) and Jv.shape == (3, P, n)
    ent = _entries(md) + [(1, [b.name for b in md.bodies].index("utorso")), (2, 0)]
    for b in range(3):
        x, rp, rv = mapping_rows(ow, md, S[b, :n], ent)
        assert _rel(Jp[b], rp) <= 1e-10 and _rel(Jv[b], rv) <= 1e-10
        assert _rel(m.getPositions(w)[b].cpu().numpy(), x) <= 1e-12
        assert _rel(m.getVelocities(w)[b].cpu().numpy(), rv @ S[b, n:]) <= 1e-10
    assert np.array_equal(w.getState().cpu().numpy(), S)                  # the getters leave the World's state alone


def test_shapes_and_devices():
    import nimblephysics_amd as na
    md = na.atlas("atlas20")
    w = na.World(md, device=DEV)
    m = _mapping(w, ("l_hand", "r_foot"), "linear")
    S = _atlas_states(md, 6, 5)
    T1, B = 3, 2
    rows = torch.tensor(S)                                               # CPU float64 in -> CPU out
    one = na.map_to_pos(w, m, rows[0])
    assert one.shape == (6,) and one.device.type == "cpu"
    batch = na.map_to_pos(w, m, rows)
    assert batch.shape == (6, 6) and batch.device.type == "cpu" and torch.equal(batch[0], one)
    roll = na.map_to_pos(w, m, rows.reshape(T1, B, -1))                  # [T+1, B, 2n]
    assert roll.shape == (T1, B, 6) and torch.equal(roll.reshape(6, 6), batch)
    dev = na.map_to_vel(w, m, rows.to(DEV))
    assert dev.device == DEV and torch.equal(dev.cpu(), na.map_to_vel(w, m, rows))
    x = rows.clone().requires_grad_(True)
    na.map_to_pos(w, m, x.reshape(T1, B, -1)).sum().backward()
    assert x.grad.device.type == "cpu" and x.grad.shape == x.shape and not x.grad[:, md.num_dofs:].any()


def test_composition_with_rollout_and_timestep():
    import nimblephysics_amd as na
    from nimblephysics_amd.timestep import rollout, timestep
    from oracle import OracleWorld
    from parity import assert_match_or_reference_unstable, world_errors
    md = na.atlas("atlas20", ground=True)
    ow = OracleWorld(md)
    n, k, B, T = md.num_dofs, len(md.action_map), 256, 8
    rng = np.random.default_rng(0)
    q = np.zeros((B, n)); q[:, 0] = -np.pi / 2; q[:, 4] = -0.01
    q[:, 6:] = rng.normal(0, 0.02, (B, n - 6))
    s = np.concatenate([q, rng.normal(0, 0.01, (B, n))], 1)
    a = rng.normal(0, 0.5, (B, T, k))
    w = na.World(md, device=DEV)
    m = _mapping(w)
    goal = torch.tensor(rng.normal(0, 0.3, 24), device=DEV)
    s0 = torch.tensor(s, device=DEV, requires_grad=True)
    at = torch.tensor(a, device=DEV, requires_grad=True)
    states = rollout(w, s0, at)
    x = na.map_to_pos(w, m, states)[:, -1]
    ((x - goal) ** 2).sum().backward()
    # the same gradient through the raw rollout backward, fed with J^T g built on the host
    ent = _entries(md)
    last = states[:, -1].detach().cpu().numpy()
    gl = 2 * (x.detach() - goal).cpu().numpy()
    gs = np.zeros((T + 1, 2 * n, B))
    for b in range(B):
        _, Jp, _ = mapping_rows(ow, md, last[b, :n], ent)
        gs[T, :n, b] = Jp.T @ gl[b]
    g0, ga = w.rollout_backward_soa(w.rollout_record, torch.tensor(gs, device=DEV))
    g0, ga = w.from_soa(g0).cpu().numpy(), ga.permute(2, 0, 1).cpu().numpy()
    assert _rel(s0.grad.cpu().numpy(), g0) <= 1e-12 and _rel(at.grad.cpu().numpy(), ga) <= 1e-12
    # one timestep + map_to_pos against the oracle's backprop fed with J^T g (the per-world parity rule of tests/parity.py)
    a1 = np.zeros((B, k))
    w.reset_lcp_cache()                                        # a cold LCP start, like the oracle's
    st = torch.tensor(s, device=DEV, requires_grad=True)
    at1 = torch.tensor(a1, device=DEV, requires_grad=True)
    nxt = timestep(w, st, at1)
    y = na.map_to_pos(w, m, nxt)
    ((y - goal) ** 2).sum().backward()
    torch.cuda.synchronize()
    ref0 = OracleWorld(md).step_batch(s, a1, None, threads=4)
    gref = np.zeros((B, 2 * n))
    for b in range(B):
        xb, Jp, _ = mapping_rows(ow, md, ref0["next"][b, :n], ent)
        gref[b, :n] = Jp.T @ (2 * (xb - goal.cpu().numpy()))
    # The reference central-differences the position integration of the free root (FreeJoint.cpp:950-1007): with a cotangent on the next
    # POSITIONS only, the velocity block of the state gradient (dt x the position block) carries that error at ~1e-6 of its size.  The
    # device differentiates exactly, so it is held to the oracle with its exact-derivative instrument (oracle.set_exact_position_jacobians).
    ow = OracleWorld(md)
    fd = ow.step_batch(s, a1, gref, threads=4)
    ow.set_exact_position_jacobians(True)
    ref = ow.step_batch(s, a1, gref, threads=4)
    ow.set_exact_position_jacobians(False)
    assert world_errors(fd, ref)[0]["grad_state"].max() < 1e-5
    dev = {"next": nxt.detach().cpu().numpy(), "grad_state": st.grad.cpu().numpy(), "grad_action": at1.grad.cpu().numpy()}
    errs, _ = world_errors(dev, ref)
    print("timestep + map_to_pos vs oracle:", {kk: float(v.max()) for kk, v in errs.items()})
    assert_match_or_reference_unstable("timestep + map_to_pos", ow, s, a1, gref, dev, ref, 1e-7, max_unstable=3)


def test_bit_identity_handles_and_deferred_join():
    import nimblephysics_amd as na
    md = na.atlas("atlas20", ground=True)
    B = 4096
    S = torch.tensor(_atlas_states(md, B, 9), device=DEV)
    w = na.World(md, device=DEV)
    m = _mapping(w)
    m.addLinearBodyNode("utorso")
    g = torch.tensor(np.random.default_rng(3).normal(size=(B, m.getPosDim())), device=DEV)

    def run(world, x, gg):
        xs = x.clone().requires_grad_(True)
        p = na.map_to_pos(world, m, xs)
        p.backward(gg)
        return p.detach(), na.map_to_vel(world, m, x), xs.grad
    first, second = run(w, S, g), run(w, S, g)
    for u, v in zip(first, second):
        assert torch.equal(u, v)
    for Bs in (1, 64):                                        # a world's bits do not depend on B or on its place in the batch
        for off in (0, B - Bs):
            got = run(w, S[off:off + Bs], g[off:off + Bs])
            for u, v in zip(got, first):
                assert torch.equal(u, v[off:off + Bs])
    w.setActionSpace(list(range(6, md.num_dofs)))            # a new handle: the mapping makes its device map again
    for u, v in zip(run(w, S, g), first):
        assert torch.equal(u, v)
    # deferred join: the state comes straight out of a step whose slices are still in flight
    ref, dw = na.World(md, device=DEV), na.World(md, device=DEV)
    st = ref.to_soa(S); at = ref.to_soa(torch.zeros((B, ref.k), dtype=torch.float64, device=DEV))
    want_next, _, _ = ref.step_soa(st, at, want_saved=True)
    want = na.map_to_pos(ref, m, want_next.t())
    dw.set_deferred_join(True)
    assert dw.slices_for(B) > 1
    buf = {"nxt": torch.empty_like(st), "saved": torch.empty(dw.saved_bytes(B), dtype=torch.uint8, device=DEV),
           "status": torch.empty(B, dtype=torch.int32, device=DEV), "cache": torch.empty((dw.m, B), dtype=torch.float64, device=DEV)}
    dw.step_into(st, at, buf["nxt"], buf["saved"], buf["status"], None, buf["cache"])
    got = na.map_to_pos(dw, m, buf["nxt"].t())
    assert torch.equal(got, want)
    dw.join()
    torch.cuda.synchronize()


def test_immobile_skeletons_take_the_references_layout(tmp_path):
    import nimblephysics_amd as na
    from test_ref_layout import load
    md = load(tmp_path)
    w = na.World(md, device=DEV)
    assert w.ref_layout is not None and w.getStateSize() == 24
    m = na.neural.IKMapping(w)
    with pytest.raises(ValueError, match="immobile"):
        m.addSpatialBodyNode("ground")
    m.addSpatialBodyNode("box")
    rng = np.random.default_rng(1)
    full = np.zeros((8, 24)); full[:, 6:12] = rng.normal(0, 0.3, (8, 6)); full[:, 18:] = rng.normal(0, 1, (8, 6))
    x = torch.tensor(full, device=DEV, requires_grad=True)
    p = na.map_to_pos(w, m, x)
    dev_state = torch.tensor(np.concatenate([full[:, 6:12], full[:, 18:]], 1), device=DEV)
    w2 = na.World(md, device=DEV); w2.ref_layout = None           # the device's own (shorter) layout
    m2 = na.neural.IKMapping(w2); m2.addSpatialBodyNode("box")
    assert torch.equal(p.detach(), na.map_to_pos(w2, m2, dev_state))
    p.sum().backward()
    assert not x.grad[:, :6].any() and not x.grad[:, 12:].any() and x.grad[:, 6:12].abs().sum() > 0
    v = na.map_to_vel(w, m, x.detach())
    assert torch.equal(v, na.map_to_vel(w2, m2, dev_state))
    w.setState(torch.tensor(full, device=DEV))
    J = m.getRealVelToMappedVelJac(w)
    assert J.shape == (8, 6, 12) and not J[:, :, :6].any()


def test_a_port_of_the_references_arm_ik_loop():
    """python/new_examples/arm_ik.py:41-53 with `nimble` replaced by nimblephysics_amd and a loader model instead of the GUI: a 1-D CPU state,
    a linear entry on a hand, plain gradient descent on the squared distance to a goal."""
    import nimblephysics_amd as na
    world = na.World(na.atlas("atlas20"), device=DEV)
    ikMap = na.neural.IKMapping(world)
    ikMap.addLinearBodyNode("l_hand")
    torch.manual_seed(0)
    state = (0.1 * torch.randn(world.getStateSize(), dtype=torch.float64)).requires_grad_(True)
    goal = torch.tensor([0.3, 0.4, 0.2], dtype=torch.float64)
    learning_rate = 0.01
    losses = []
    for _ in range(200):
        hand_pos = na.map_to_pos(world, ikMap, state)
        loss = (hand_pos - goal).square().sum()
        loss.backward()
        with torch.no_grad():
            state -= learning_rate * state.grad
            state.grad = None
        losses.append(float(loss.detach()))
    assert hand_pos.shape == (3,) and hand_pos.device.type == "cpu"
    assert losses[-1] < 0.05 * losses[0], (losses[0], losses[-1])
