"""Screw joints through the device paths that tests/test_screw_joint.py's free step does not reach: contact rows and the dense contact
kernels of the three builds with a collider on a screw-jointed body, the one-world-per-lane tree kernels, the mass gradient, the rollout
and the contact read-out.  A screw whose pitch is dropped is a hinge - plausible motion, finite gradients - so every comparison here is
against the CPU oracle (itself held to finite differences and a derived statement of the physics in tests/test_screw_joint.py) or pins
the linear part of the joint axis end to end.  The scenes and their conditions (share in contact, share resolved at stage 0) are
checked on the CPU in tests/test_screw_joint.py."""
import numpy as np
import pytest

from test_screw_joint import CONTACT_SCENES, contact_scene, screw_arm

pytestmark = pytest.mark.gpu
TOL = 1e-7                            # tests/test_gpu_capsules.py
DEV = "cuda:0"
BUILDS = {8: 8, 16: 16, 24: 64}       # max_contacts of the description -> nbl_model_max_contacts of the build that serves it


def _step_and_compare(tag, md, s, a, seed, min_contact=0.9):
    """timestep + backward against the oracle's step_batch: EVERY world (tests/parity.py), as tests/test_gpu_capsules.py::_compare"""
    import torch
    import nimblephysics_amd as na
    from nimblephysics_amd.timestep import timestep
    from oracle import OracleWorld
    from parity import assert_match_or_reference_unstable
    s, a = np.array(s), np.array(a)
    world = na.World(md, device=DEV); ow = OracleWorld(md)
    g = np.random.default_rng(seed).normal(0, 1, s.shape)
    st = torch.tensor(s, device=DEV, requires_grad=True); at = torch.tensor(a, device=DEV, requires_grad=True)
    world.set_timing(True)
    out = timestep(world, st, at)
    status = world.last_status.cpu().numpy().astype(np.uint32)
    out.backward(torch.tensor(g, device=DEV))
    ref = ow.step_batch(s, a, g, threads=8)
    if md.max_contacts:
        assert np.array_equal(status & 0x81, ref["status"] & 0x81)          # the same worlds in contact
        assert (status & 0x1).mean() >= min_contact, (status & 0x1).mean()
    dev = {"next": out.detach().cpu().numpy(), "grad_state": st.grad.cpu().numpy(), "grad_action": at.grad.cpu().numpy()}
    assert_match_or_reference_unstable(tag, ow, s, a, g, dev, ref, TOL, max_unstable=0.02 * len(s))
    return world


# ---- (a) a collider on a screw-jointed body, all three builds of the contact stage -------------------------------------------------------
@pytest.mark.parametrize("max_contacts", sorted(BUILDS))
@pytest.mark.parametrize("name", CONTACT_SCENES)
def test_contacts_on_screw_jointed_bodies_equal_the_oracle(name, max_contacts):
    md, s, a = contact_scene(name, max_contacts)
    world = _step_and_compare(f"{name}, {max_contacts} slots", md, s, a, 11)
    assert world._L.nbl_model_max_contacts(world._h) == BUILDS[max_contacts]


# ---- (b) the tree kernels of every mode ----------------------------------------------------------------------------------------------------
def _modes():
    from test_gpu_tree_modes import IDS, MODES
    return [pytest.param(m, id=i) for m, i in zip(MODES, IDS)]


@pytest.mark.parametrize("mode", _modes())
@pytest.mark.parametrize("model", ["screw_arm", "screw_root", "screw_walker"])
def test_screw_joints_in_every_tree_mode(model, mode, monkeypatch):
    """kernels.hip's JT_SCREW branch (one world per lane) runs only under NBL_COOP_TREE=0 / NBL_SAVE_TREE=0: assert that it really ran there."""
    for k, v in mode.items():
        monkeypatch.setenv(k, v)
    if model == "screw_walker":
        md, s, a = contact_scene("screw_walker", 8)
        s, a = s[:128], a[:128]
    else:
        md = screw_arm(2, model == "screw_arm")
        B = 96; rng = np.random.default_rng(3); n = md.num_dofs
        s = np.concatenate([rng.normal(0, 0.6, (B, n)), rng.normal(0, 1.5, (B, n))], 1); a = rng.normal(0, 1, (B, len(md.action_map)))
    world = _step_and_compare(f"{model} {mode}", md, s, a, 5)
    kernels = world.get_timing()["kernels"]
    lanes = mode.get("NBL_COOP_TREE") == "0" or mode.get("NBL_SAVE_TREE") == "0"
    if lanes:
        assert "k_step_forward" in kernels, (mode, sorted(kernels))


# ---- (d) mass gradient of screw-jointed bodies ---------------------------------------------------------------------------------------------
def test_mass_gradient_of_screw_jointed_bodies_in_free_fall():
    import copy
    from nimblephysics_amd.mass import WrtMassBodyNodeEntryType as T
    from test_gpu_mass import _check
    md = screw_arm(2, True)
    B = 32; rng = np.random.default_rng(31); n = md.num_dofs
    s = np.concatenate([rng.normal(0, 0.6, (B, n)), rng.normal(0, 1.0, (B, n))], 1); a = rng.normal(0, 1, (B, len(md.action_map)))
    for t in (T.INERTIA_MASS, T.INERTIA_COM, T.INERTIA_DIAGONAL, T.INERTIA_OFF_DIAGONAL, T.INERTIA_FULL):
        _check(md, [(3, t)], s, a, 32)                                   # "nut": pitch -1.5 behind a revolute joint and another screw
    _check(md, [(1, T.INERTIA_MASS), (4, T.INERTIA_FULL)], s, a, 33)
    mu = copy.deepcopy(md); mu.bodies[1].beta = (0.5, -1.5, 0.25); mu.bodies[1].com = (0.1, -0.3, 0.05)   # COM = beta * 0.2
    _check(mu, [(1, T.INERTIA_COM_MU)], s, a, 34)


def test_mass_gradient_of_screw_jointed_bodies_in_contact():
    import copy
    from nimblephysics_amd.mass import WrtMassBodyNodeEntryType as T
    from test_gpu_mass import _check
    md, s, a = contact_scene("screw_walker", 8)
    s, a = np.array(s[:32]), np.array(a[:32])
    _check(md, [(1, T.INERTIA_MASS), (2, T.INERTIA_COM), (3, T.INERTIA_FULL)], s, a, 35, tol=2e-4, second_eps=1e-5)
    _check(md, [(1, T.INERTIA_DIAGONAL), (2, T.INERTIA_OFF_DIAGONAL)], s, a, 36, tol=2e-4, second_eps=1e-5)
    mu = copy.deepcopy(md); mu.bodies[4].beta = (0.5, -1.5, 0.25); mu.bodies[4].com = (0.1, -0.3, 0.05)   # the free tail; COM = beta * 0.2
    _check(mu, [(4, T.INERTIA_COM_MU), (0, T.INERTIA_MASS)], s, a, 37, tol=2e-4, second_eps=1e-5)


# ---- (f) rollout ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("checkpoint_every", [0, 2])
def test_rollout_of_the_screw_walker_equals_the_chain_of_timesteps(checkpoint_every):
    """Device against itself (states bit for bit, gradients to 1e-12 as tests/test_gpu_rollout.py): does not see a dropped pitch, only
    that the rollout and its checkpointed form run the same screw-joint step as timestep()."""
    import torch
    import nimblephysics_amd as na
    from nimblephysics_amd.timestep import rollout
    from test_gpu_rollout import _chain
    md, s0, a0 = contact_scene("screw_walker", 8)
    s0, a0 = np.array(s0), np.array(a0)
    B, T = len(s0), 5
    rng = np.random.default_rng(3)
    acts = np.repeat(a0[:, None, :], T, 1) + rng.normal(0, 0.005, (B, T, a0.shape[1]))
    w = torch.tensor(rng.normal(0, 1, (B, T + 1, s0.shape[1])), device=DEV)
    world = na.World(md, device=DEV)
    st, at, xs = _chain(world, s0, acts, True)
    (xs * w).sum().backward()
    world2 = na.World(md, device=DEV)
    st2 = torch.tensor(s0, device=DEV, requires_grad=True); at2 = torch.tensor(acts, device=DEV, requires_grad=True)
    ys = rollout(world2, st2, at2, warm_start=True, checkpoint_every=checkpoint_every)
    (ys * w).sum().backward()
    assert torch.equal(ys, xs.detach())
    worst = 0.0
    for x, y in ((st2.grad, st.grad), (at2.grad, at.grad)):
        e = (x - y).abs().max().item() / max(y.abs().max().item(), 1.0)
        worst = max(worst, e)
        assert e <= 1e-12
    assert np.all(world2.rollout_status.cpu().numpy() & 0x1)
    print(f"[screw_walker rollout, checkpoint_every={checkpoint_every}] states bit-identical, worst gradient error {worst:.2e}")


# ---- (g) the read-out wrenches reproduce the step --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONTACT_SCENES)
def test_read_out_wrenches_on_screw_jointed_bodies_reproduce_the_step(name):
    """v' - v = dt forward_dynamics(state, tau, joint_forces=True, wrenches=W, world_frame=True) with W the read-out contact wrenches
    (tests/test_gpu_contact_readout.py, test 4): the ground's force does work on a screw coordinate through h axis, so this pins the sign,
    the point of action and the screw's linear part end to end; without the wrenches the step is NOT reproduced."""
    import torch
    import nimblephysics_amd as na
    from nimblephysics_amd.contacts import body_contact_wrenches
    from test_gpu_contact_readout import _close, _collider_bodies, _err, _step
    md, s, a = contact_scene(name, 8)
    s, a = np.array(s[:70]), np.array(a[:70])
    world, saved, nxt, status = _step(md, s, a)
    n, B = md.num_dofs, len(s)
    assert list(md.action_map) == list(range(n)) and not world.getPenetrationCorrectionEnabled()
    bodies = _collider_bodies(md)
    W = body_contact_wrenches(world, saved, B, bodies)
    st, tau = torch.tensor(s, device=DEV), torch.tensor(a, device=DEV)
    acc = na.forward_dynamics(world, st, tau, joint_forces=True, wrenches=W.reshape(B, 6 * len(bodies)), bodies=bodies, world_frame=True).cpu().numpy()
    free = na.forward_dynamics(world, st, tau, joint_forces=True).cpu().numpy()
    dv = nxt[:, n:] - s[:, n:]
    print(f"[{name}] max |dv - dt a| / max(1, |dv|) = {_err(md.dt * acc, dv):.2e} (without the wrenches {_err(md.dt * free, dv):.2e})")
    assert np.abs(dv - md.dt * free).max() > 1e-4
    assert _close(md.dt * acc, dv), _err(md.dt * acc, dv)
    # the same statement with nothing of the device's but the wrenches and the step: the oracle's mass matrix and bias forces, the bodies'
    # world Jacobians of tests/kin_numpy.py (which builds the screws' twists from `pitch` itself).  The device's forward_dynamics above shares
    # its joint axes with the step, so alone it would also hold for a library that runs every screw as a hinge.
    from kin_numpy import body_jacobians
    from oracle import OracleWorld
    ow = OracleWorld(md); Wn = W.cpu().numpy()
    assert not md.flat()["damping"].any() and not md.flat()["spring"].any()
    ref = np.zeros_like(dv)
    for b in range(B):
        q, v = s[b, :n], s[b, n:]
        gen = a[b] - ow.coriolis_gravity(q, v)
        for e, body in enumerate(bodies):
            gen = gen + body_jacobians(ow, md, q, body)[2].T @ Wn[b, e]
        ref[b] = md.dt * np.linalg.solve(ow.mass_matrix(q), gen)
    print(f"[{name}] max |dv - dt M^-1 (tau - C + J^T W)| / max(1, |dv|) with the oracle's M, C and kin_numpy's J = {_err(ref, dv):.2e}")
    assert _close(ref, dv), _err(ref, dv)


# ---- (c) joint limits and joint Coulomb friction on screw coordinates ----------------------------------------------------------------------
def limited_screw_arm(ground=True):
    """tests/util.py::limited_arm with its hinges turned into screw joints (pitches 0.25 and -1.5): limits [-0.5, 0.4] enforced on every
    screw coordinate, the base's box on the ground next to them.  The library refuses neither limits nor friction on a screw coordinate
    (it refuses them on a free-joint root only), so both are tested."""
    from util import limited_arm
    md = limited_arm(ground=ground)
    for k, b in enumerate(md.bodies[1:]):
        b.joint_type, b.pitch = "screw", (0.25, -1.5)[k % 2]
    md.name = "limited_screw_arm"
    return md


def test_position_limits_on_screw_coordinates_next_to_contacts():
    """Every limited screw coordinate above, on or inside its limit, moving inwards or outwards (tests/test_gpu_joint_limits.py::_states),
    the base on the ground in most worlds: every world against the oracle (its _compare)."""
    import test_gpu_joint_limits as tl
    md = limited_screw_arm()
    s, a = tl._states(md, 256, 5, at_limit=0.35)
    s[:, 0] = np.random.default_rng(6).uniform(-0.025, 0.008, len(s))
    tl._compare("limited screw arm on the ground", md, s, a, 7, min_limit=0.5, min_contact=0.3)


def test_coulomb_friction_on_screw_coordinates_sticks_and_slides():
    """tests/test_gpu_joint_friction.py::test_friction_only_unique_solution on a chain of screw joints: A = M^-1 on the moving coordinates is
    positive definite, so the boxed LCP has one solution: v' = v_pre + M^-1 x with |x| <= f dt, v'_d = 0 where x_d is inside its bounds and
    opposing the bound otherwise.  v_pre and M are the oracle's (friction off)."""
    import copy
    import torch
    import nimblephysics_amd as na
    from oracle import OracleWorld
    md = screw_arm(2, False)
    for i, b in enumerate(md.bodies):
        b.coulomb_friction = (0.5 + 0.4 * i,)
    md = na.ModelDescription("screw_friction_chain", md.bodies, gravity=md.gravity, dt=md.dt)
    off = copy.deepcopy(md)
    for b in off.bodies:
        b.coulomb_friction = ()
    n, B = md.num_dofs, 256
    rng = np.random.default_rng(10)
    q = rng.normal(0, 0.3, (B, n))
    v = rng.normal(0, 1, (B, n)) * 10.0 ** rng.uniform(-4, 0, (B, 1))        # some worlds stick, some slide
    a = rng.normal(0, 0.5, (B, len(md.action_map)))
    s = np.concatenate([q, v], 1)
    ow = OracleWorld(off)
    vpre = ow.step_batch(s, a)["next"][:, n:]
    w = na.World(md, device=DEV)
    nxt, _saved, status = w.step_soa(torch.tensor(s.T.copy(), device=DEV), torch.tensor(a.T.copy(), device=DEV), want_saved=False)
    nxt = nxt.cpu().numpy().T
    status = status.cpu().numpy().astype(np.uint32)
    cache = w.lcp_cache.cpu().numpy()
    bound = md.flat()["coulomb_friction"] * md.dt
    assert (status & 0x800).all() and not (status & (0x80 | 0x40 | 0x1)).any()
    stuck = slid = 0
    worst = 0.0
    for b in range(B):
        act = np.nonzero(vpre[b] != 0.0)[0]
        assert int(cache[-1, b]) == 3 * len(act)
        x = np.zeros(n)
        x[act] = cache[0:3 * len(act):3, b]
        assert np.all(np.abs(x) <= bound * (1 + 1e-12))
        v1 = vpre[b] + np.linalg.solve(ow.mass_matrix(q[b]), x)
        worst = max(worst, float(np.abs(nxt[b, n:] - v1).max()))
        assert np.allclose(nxt[b, n:], v1, rtol=0, atol=1e-9), np.abs(nxt[b, n:] - v1).max()
        inside = np.abs(x) < bound * (1 - 1e-7)
        assert np.all(np.abs(nxt[b, n:][inside]) <= 1e-9)
        assert np.all(nxt[b, n:][x >= bound * (1 - 1e-7)] <= 1e-9) and np.all(nxt[b, n:][x <= -bound * (1 - 1e-7)] >= -1e-9)
        stuck += inside.any(); slid += (~inside).any()
    print(f"[screw friction chain] worst |v' - (v_pre + M^-1 x)| {worst:.2e}; worlds with a sticking / a sliding coordinate: {stuck} / {slid} of {B}")
    assert stuck > B // 10 and slid > B // 10, (stuck, slid)


# ---- (h) kinematics and inverse kinematics -------------------------------------------------------------------------------------------------
KIN_ENTRIES = [(0, 1), (1, 3), (2, 4), (0, 3)]       # (kind: 0 spatial, 1 linear, 2 angular; body): bolt, nut, dflt - all behind screw joints


@pytest.mark.parametrize("free_root", [True, False])
def test_map_to_pos_and_map_to_vel_on_screw_jointed_bodies(free_root):
    """kinematics_dev.hpp's JT_SCREW branch in the kinematics kernels against tests/kin_numpy.py (which builds the screw's transform and
    twist from `pitch` itself) at the bars of tests/test_gpu_kinematics.py: positions 1e-12, velocities and VJPs 1e-10."""
    import torch
    import nimblephysics_amd as na
    import ik_cases as ic
    from kin_numpy import mapping_rows
    from oracle import OracleWorld
    from test_gpu_kinematics import _rel
    md = screw_arm(2, free_root)
    ow = OracleWorld(md); n = md.num_dofs; B = 130
    Q = ic.random_poses(md, ow, KIN_ENTRIES, B, 41)
    S = np.concatenate([Q, np.random.default_rng(42).normal(0, 1.0, (B, n))], 1)
    w = na.World(md, device=DEV)
    m = na.IKMapping(w)
    for kind, body in KIN_ENTRIES:
        (m.addSpatialBodyNode, m.addLinearBodyNode, m.addAngularBodyNode)[kind](body)
    st = torch.tensor(S, device=DEV, requires_grad=True)
    pos = na.map_to_pos(w, m, st)
    vel = na.map_to_vel(w, m, torch.tensor(S, device=DEV))
    P = 6 + 3 + 3 + 6
    assert pos.shape == (B, P) and vel.shape == (B, P)
    g = np.random.default_rng(43).normal(size=(B, P))
    pos.backward(torch.tensor(g, device=DEV))
    sv = torch.tensor(S, device=DEV, requires_grad=True)
    na.map_to_vel(w, m, sv).backward(torch.tensor(g, device=DEV))
    pos, vel, gp, gv = pos.detach().cpu().numpy(), vel.cpu().numpy(), st.grad.cpu().numpy(), sv.grad.cpu().numpy()
    worst = {"pos": 0.0, "vel": 0.0, "pos vjp": 0.0, "vel vjp (velocities)": 0.0}
    for b in range(B):
        ref, Jp, Jv = mapping_rows(ow, md, S[b, :n], KIN_ENTRIES)
        e = {"pos": float(np.abs(pos[b] - ref).max() / max(1.0, np.abs(ref).max())), "vel": _rel(vel[b], Jv @ S[b, n:]),
             "pos vjp": _rel(gp[b, :n], Jp.T @ g[b]), "vel vjp (velocities)": _rel(gv[b, n:], Jv.T @ g[b])}
        assert not gp[b, n:].any()
        for k, x in e.items():
            worst[k] = max(worst[k], float(x))
        assert e["pos"] <= 1e-12 and max(e["vel"], e["pos vjp"], e["vel vjp (velocities)"]) <= 1e-10, (b, e)
    print(f"[screw_arm free_root={free_root}] kinematics against kin_numpy, worst over {B} worlds: {worst}")


def test_solve_ik_turns_the_screws_like_the_host_build():
    """An arm whose every coordinate but one is a screw (screw_arm on a screw root), a point on `nut` and the pose of `dflt` as targets: the
    first steps against the host build of the same header at 1e-9 and the full run under its rule (tests/test_gpu_ik.py); the host build
    is held to tests/ik_numpy.py in tests/test_ik_host.py."""
    import torch
    import nimblephysics_amd as na
    import ik_cases as ic
    from kin_numpy import mapping_rows
    from oracle import OracleWorld
    from test_ik_host import full_run_check
    md = screw_arm(2, False)
    entries = [(1, 3), (0, 4)]
    ow = OracleWorld(md)
    poses = ic.random_poses(md, ow, entries, ic.B_TEST, 51)
    targets = np.stack([mapping_rows(ow, md, q, entries)[0] for q in poses])
    w = na.World(md, device=DEV)
    m = na.IKMapping(w)
    for kind, body in entries:
        (m.addSpatialBodyNode, m.addLinearBodyNode, m.addAngularBodyNode)[kind](body)
    h = ic.HostIK(ic.load_ik_shim(), md, entries)
    worst = 0.0
    for k in (1, 5, 500):
        q, loss, steps = (x.cpu().numpy() for x in na.solve_ik(w, m, torch.tensor(targets, device=DEV), None, na.IKConfig(max_step_count=k)))
        hq, hl, hs = h.solve(targets, max_step_count=k)
        if k < 500:
            assert np.array_equal(steps, hs), k
            worst = max(worst, float(np.abs(q - hq).max()))
        else:
            full_run_check(q, loss, steps, hq, hl, hs, "screw_root arm (device against host build)")
    print(f"[ik, screw_root arm] worst |q - host build| over max_step_count 1, 5 and {len(targets)} worlds: {worst:.3e}; "
          f"full run: median loss {np.median(loss):.2e}, worst {loss.max():.2e}")
    assert worst <= 1e-9
