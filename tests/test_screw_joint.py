"""Screw joints (dart/dynamics/ScrewJoint.cpp: one DOF, rotation about an axis coupled with `pitch` of translation per turn along it,
S = Ad(T_cj)[axis; axis pitch / 2 pi], T = T_pj expMap(S_local q) T_cj^-1): the oracle against the closed-form transform and finite
differences of its own step (CPU), the device against the oracle (GPU)."""
import functools

import numpy as np
import pytest

import nimblephysics_amd as na
from oracle import OracleWorld
from test_oracle_props import _fd_jac
from util import rel_err


def screw_arm(seed=0, free_root=True):
    from test_ball_joint import _T
    rng = np.random.default_rng(300 + seed)
    def body(name, parent, jt, **kw):
        A = rng.normal(size=(3, 3)); I = A @ A.T * 0.02 + 0.03 * np.eye(3)
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        root = parent < 0 and jt == "free"
        return na.BodySpec(name, parent, jt, name + "_joint", axis=tuple(ax) if jt in ("revolute", "screw") else (0.0, 0.0, 1.0),
                           T_pj=np.eye(4) if root else _T(rng, 0.25), T_cj=np.eye(4) if root else _T(rng, 0.1), mass=float(rng.uniform(0.5, 2.0)),
                           com=tuple(rng.normal(0, 0.04, 3)), inertia=(I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]), **kw)
    bodies = [body("root", -1, "free" if free_root else "screw", **({} if free_root else {"pitch": 0.3})),
              body("bolt", 0, "screw", pitch=0.25, damping=(0.2,)), body("link", 1, "revolute"), body("nut", 2, "screw", pitch=-1.5, spring=(2.0,), rest=(0.1,)),
              body("dflt", 0, "screw")]
    return na.ModelDescription("screw_arm", bodies, [], gravity=(0.0, -9.81, 0.0), dt=1e-3, max_contacts=0)


# ---- screw joints in contact: the scenes of the contact tests below and of tests/test_gpu_screw_joint.py --------------------------------
def _ground():
    return na.BoxSpec(-1, na.make_transform((0, -0.5, 0)), (8.0, 1.0, 8.0), 1.0)          # top face at y = 0


def lowest_point(T_body, col):
    """world height of the lowest point of the collider `col` (box or sphere) of a body with world transform T_body"""
    T = T_body @ np.asarray(col.T)
    if col.shape == "sphere":
        return T[1, 3] - col.size[0]
    return T[1, 3] - np.abs(T[1, :3]) @ (0.5 * np.asarray(col.size))


def nut_on_bolt(axis_tilt=0.0, max_contacts=8, shape="box", mu=0.8):
    """One body on a ROOT screw joint (pitch 0.25, axis vertical or tilted by `axis_tilt` rad towards a fixed horizontal direction) that
    carries a box or a sphere above a world-fixed ground box.  The ground's normal force reaches the joint only through the linear part
    h axis of S = [axis; h axis]: a hinge about the same axis could not be pushed up at all."""
    phi = np.random.default_rng(411).uniform(0, 2 * np.pi)
    axis = (np.sin(axis_tilt) * np.cos(phi), np.cos(axis_tilt), np.sin(axis_tilt) * np.sin(phi))
    nut = na.BodySpec("nut", -1, "screw", "thread", axis=axis, pitch=0.25, T_pj=na.make_transform((0.0, 0.3, 0.0)), mass=1.2, com=(0.02, -0.05, -0.01),
                      inertia=(0.011, 0.02, 0.013, 0.001, -0.002, 0.0015))
    col = na.BoxSpec(0, na.make_transform((0.03, -0.2, 0.02), rpy=(0.3, 0.0, 0.25) if axis_tilt else (0.0, 0.0, 0.0)), (0.2, 0.1, 0.16), mu) if shape == "box" else na.SphereSpec(0, na.make_transform((0.06, -0.2, 0.01)), 0.08, mu)
    return na.ModelDescription("nut_on_bolt_" + shape, [nut], [_ground(), col], gravity=(0.0, -9.81, 0.0), dt=1e-3, max_contacts=max_contacts)


WALKER_PITCH = (0.25, -1.5, 0.25)


def screw_walker(max_contacts=8, seed=0):
    """A free root above the ground with three limbs and a tail on screw joints (pitches of both signs, random joint frames on both sides as in
    screw_arm; the axes roughly horizontal in the root's frame, each limb's collider 0.3 from its joint, outwards and down, so that turning the
    screw swings it onto the ground): spheres on two limbs, a box (the box-box route) on the third."""
    from scipy.spatial.transform import Rotation as Rot
    from test_ball_joint import _T
    rng = np.random.default_rng(500 + seed)
    def inertia():
        A = rng.normal(size=(3, 3)); I = A @ A.T * 0.004 + 0.006 * np.eye(3)
        return (I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2])
    bodies = [na.BodySpec("torso", -1, "free", "root", mass=2.0, com=tuple(rng.normal(0, 0.02, 3)), inertia=inertia())]
    cols = [_ground()]
    for k, pitch in enumerate(WALKER_PITCH):
        psi = 2 * np.pi * k / 3 + rng.normal(0, 0.1)
        d = np.array([np.cos(psi + np.pi / 2), rng.normal(0, 0.1), np.sin(psi + np.pi / 2)]); d /= np.linalg.norm(d)    # the axis in the root's frame
        T_pj = _T(rng, 0.0); T_pj[:3, 3] = 0.15 * np.array([np.cos(psi), 0.0, np.sin(psi)]) + rng.normal(0, 0.01, 3)
        axis = T_pj[:3, :3].T @ d
        T_cj = _T(rng, 0.05)
        u = T_pj[:3, :3].T @ np.array([np.cos(psi) * np.sin(np.pi / 3), -np.cos(np.pi / 3), np.sin(psi) * np.sin(np.pi / 3)])   # at q = 0: outwards and down
        Tc = np.eye(4); Tc[:3, :3] = Rot.from_rotvec(rng.normal(0, 0.6, 3)).as_matrix(); Tc[:3, 3] = 0.3 * u + axis * rng.normal(0, 0.03)   # in the joint's frame
        bodies.append(na.BodySpec(f"limb{k}", 0, "screw", f"screw{k}", axis=tuple(axis), pitch=pitch, T_pj=T_pj, T_cj=T_cj, mass=float(rng.uniform(0.4, 0.9)),
                                  com=tuple((T_cj @ Tc)[:3, 3] * 0.5 + rng.normal(0, 0.02, 3)), inertia=inertia()))
        cols.append(na.BoxSpec(k + 1, T_cj @ Tc, (0.1, 0.08, 0.12), 0.9) if k == 2 else na.SphereSpec(k + 1, T_cj @ Tc, 0.05, 0.8))
    # a tail on a fourth screw joint that touches nothing: with three sticking contacts (nine rows) on the other nine coordinates the walker
    # would be fully clamped - v' = 0 whatever the action, the masses or the pitch - and its gradients trivial; the tail keeps one screw
    # coordinate free, coupled to the clamped ones through the mass matrix
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    bodies.append(na.BodySpec("tail", 0, "screw", "screw_tail", axis=tuple(ax), pitch=0.6, T_pj=_T(rng, 0.08), T_cj=_T(rng, 0.05), mass=0.5,
                              com=tuple(rng.normal(0, 0.06, 3)), inertia=inertia()))
    return na.ModelDescription("screw_walker", bodies, cols, gravity=(0.0, -9.81, 0.0), dt=1e-3, max_contacts=max_contacts)


def _screw_angle_for_depth(w, q, dof, body, col, pen, lo, hi, grid=73):
    """a value of q[dof] in [lo, hi] at which the lowest point of `col` is `pen` below the ground (the crossing of the scanned height nearest to zero, refined)"""
    from scipy.optimize import brentq
    def f(x):
        qq = q.copy(); qq[dof] = x
        return lowest_point(w.body_world_transform(qq, body), col) + pen
    xs = np.linspace(lo, hi, grid); ys = np.array([f(x) for x in xs])
    cross = np.where(ys[:-1] * ys[1:] < 0)[0]
    assert len(cross), (body, "the collider cannot reach the ground", ys.min())
    i = int(min(cross, key=lambda j: abs(xs[j])))
    return brentq(f, xs[i], xs[i + 1], xtol=1e-13)


def contact_states(md, B, seed, vel=0.05):
    """[B, 2n] states and [B, k] actions of nut_on_bolt / screw_walker with every collider 0.5 .. 3 mm in the ground (placed with the oracle's
    own forward kinematics, the way tests/test_gpu_capsules.py::_states places its capsules), velocities N(0, vel^2), actions N(0, 0.1^2)"""
    w = OracleWorld(md); n = md.num_dofs
    S, A = np.zeros((B, 2 * n)), np.zeros((B, len(md.action_map)))
    walker = md.bodies[0].joint_type == "free"
    for i in range(B):
        rng = np.random.default_rng(seed * 100003 + i)
        q = np.zeros(n)
        if walker:
            q[0:3] = rng.normal(0, 1, 3) * (0.06, 0.5, 0.06); q[3:6] = (rng.normal(0, 0.3), 0.2 + rng.normal(0, 0.01), rng.normal(0, 0.3))
        for col in md.boxes:
            if col.body >= 0:
                dof = 5 + col.body if walker else 0
                q[dof] = _screw_angle_for_depth(w, q, dof, col.body, col, rng.uniform(5e-4, 3e-3), *((-1.2, 1.2) if walker else (-4.0, 1.0)))
        if walker:
            q[9] = rng.normal(0, 0.6)                                   # the tail
        S[i, :n] = q; S[i, n:] = rng.normal(0, vel, n); A[i] = rng.normal(0, 0.1 if not walker else 0.01, A.shape[1])
        if walker:
            S[i, n + 9] = rng.normal(0, 0.5)
            A[i, 6:] += _standing_torques(md, w, q)
    return S, A


def _standing_torques(md, w, q, eps=1e-6):
    """The screw torques with which the walker STANDS on its three limbs: vertical ground forces f at the three lowest points that carry the
    weight with no moment about the centre of mass (a tripod: three equations, three forces), and on screw k
    tau_k = (gravity force on the coordinate) - f_k d(height of its lowest point) / d q_k.  With them the contacts need no friction, so the
    all-sticking guess of the LCP's stage 0 is the solution; the random part of the actions and velocities disturbs it a little."""
    cols = [c for c in md.boxes if c.body >= 0]
    mass = np.array([b.mass for b in md.bodies])
    T = [w.body_world_transform(q, k) for k in range(len(md.bodies))]
    com = sum(m * (Tb[:3, :3] @ np.asarray(b.com) + Tb[:3, 3]) for m, Tb, b in zip(mass, T, md.bodies)) / mass.sum()
    pts = []
    for c in cols:
        Tc = T[c.body] @ np.asarray(c.T)
        pts.append(Tc[:3, 3] if c.shape == "sphere" else Tc[:3, 3] - Tc[:3, :3] @ (np.sign(Tc[1, :3]) * 0.5 * np.asarray(c.size)))
    P = np.array(pts)
    f = np.linalg.solve(np.array([np.ones(3), P[:, 0] - com[0], P[:, 2] - com[2]]), [mass.sum() * 9.81, 0.0, 0.0])
    assert (f > 0).all(), ("the centre of mass is not over the tripod", f)
    G = w.coriolis_gravity(q, np.zeros_like(q))
    tau = G[6:].copy()                                               # (the tail: held against gravity)
    for k, c in enumerate(cols):
        qp, qm = q.copy(), q.copy(); qp[6 + k] += eps; qm[6 + k] -= eps
        tau[k] -= f[k] * (lowest_point(w.body_world_transform(qp, c.body), c) - lowest_point(w.body_world_transform(qm, c.body), c)) / (2 * eps)
    return tau


CONTACT_SCENES = ["nut_box", "nut_sphere", "screw_walker"]


def contact_model(name, max_contacts=8):
    return {"nut_box": lambda: nut_on_bolt(0.08, max_contacts, "box"), "nut_sphere": lambda: nut_on_bolt(0.05, max_contacts, "sphere"),
            "screw_walker": lambda: screw_walker(max_contacts)}[name]()


@functools.lru_cache(maxsize=None)
def contact_scene(name, max_contacts=8, B=256):
    """(model, states, actions) of the contact tests: the box standing on one corner on a thread tilted by 0.08 rad (flat on a
    vertical thread its four contacts on one coordinate make the reference's Dantzig solver abort on a singular pivot as soon as a
    perturbed step leaves stage 0), the sphere on a thread tilted by 0.05 rad, the walker standing on its three limbs; computed once, never written to.  The velocities are small enough for the contacts
    to stick (0.02 on the nut, 0.002 on the walker, whose 3.8 kg take an impulse of only 0.04 N s per step from the ground): what
    test_the_contact_scenes_meet_their_conditions holds them to."""
    md = contact_model(name, max_contacts)
    s, a = contact_states(md, B, 7 + CONTACT_SCENES.index(name), vel=0.002 if name == "screw_walker" else 0.02)
    s.setflags(write=False); a.setflags(write=False)
    return md, s, a


@pytest.mark.parametrize("name", CONTACT_SCENES)
def test_the_contact_scenes_meet_their_conditions(name):
    """What the device tests assume of their inputs, on the oracle alone: at least 90 % of the worlds in contact, at least 90 % resolved at
    stage 0 of the LCP, every collider 0.5 .. 3 mm in the ground, no world NaN, and the reference's own solver present."""
    md, s, a = contact_scene(name)
    w = OracleWorld(md); n = md.num_dofs
    r = w.step_batch(s, a, np.random.default_rng(1).normal(0, 1, s.shape), threads=8)
    st = r["status"]
    contact, stage0 = float((st & 1).mean()), float(((st & 2) != 0).mean())
    print(f"[{name}] in contact {contact:.3f}, resolved at stage 0 {stage0:.3f}, status words {sorted({hex(int(x)) for x in st})}")
    assert contact >= 0.9 and stage0 >= 0.9, (contact, stage0)
    assert not (st & 0x80000040).any()                                # no NaN; oracle/_ref/libodelcp_ref.so was there for the worlds past stage 0
    assert all(np.isfinite(r[k]).all() for k in ("next", "grad_state", "grad_action"))
    for i in range(0, len(s), 16):
        for col in md.boxes:
            if col.body >= 0:
                assert 4e-4 < -lowest_point(w.body_world_transform(s[i, :n], col.body), col) < 3.1e-3


@pytest.mark.parametrize("name", CONTACT_SCENES)
def test_backprop_through_a_screw_joint_in_contact_is_the_jacobian_transpose(name):
    """The oracle's backprop of one step against central differences of its own step (form and tolerance of
    tests/test_ball_joint.py::test_backprop_through_ball_joints_is_the_jacobian_transpose[ground]) on 20 worlds of each scene.  A world is
    skipped only where the difference quotients of two step sizes disagree with EACH OTHER by more than the tolerance (a kink of the LCP
    between the stencil points); at most 10 % of the worlds."""
    md, s, a = contact_scene(name)
    w = OracleWorld(md); n = w.n; rng = np.random.default_rng(4)
    tol, worlds, skipped, worst = 2e-5, range(20), 0, 0.0

    def step(x, u):                                                  # every step from the LCP's own guess, not from the previous call's solution
        w.reset_lcp_cache()
        return w.step(x, u)
    for i in worlds:
        s0, a0 = np.array(s[i]), np.array(a[i])
        g = rng.normal(0, 1, 2 * n)
        fd = []
        for eps in (1e-6, 3e-7):
            Js = _fd_jac(lambda x: step(x, a0), s0, eps); Ja = _fd_jac(lambda x: step(s0, x), a0, eps)
            fd.append((Js.T @ g, Ja.T @ g))
        step(s0, a0)
        assert w.last_status & 1
        gs, ga = w.backprop(g)
        scs, sca = max(1.0, np.abs(gs).max()), max(1.0, np.abs(ga).max())
        if np.abs(fd[0][0] - fd[1][0]).max() >= tol * scs or np.abs(fd[0][1] - fd[1][1]).max() >= tol * sca:
            skipped += 1
            continue
        e = max(np.abs(gs - fd[0][0]).max() / scs, np.abs(ga - fd[0][1]).max() / sca)
        worst = max(worst, e)
        assert e < tol, (name, i, e)
    print(f"[{name}] backprop vs central differences: worst {worst:.2e} over {len(worlds) - skipped} worlds, {skipped} skipped (quotients of two step sizes disagree)")
    assert skipped <= 0.1 * len(worlds), skipped


@pytest.mark.parametrize("shape", ["box", "sphere"])
def test_a_nut_on_a_vertical_thread_falls_at_the_screw_rate_and_is_held_by_the_ground(shape):
    """Derived, not measured.  One body on a vertical screw axis, h = pitch / 2 pi of translation per radian: the kinetic energy is
    (I_axis + m h^2) qd^2 / 2 (I_axis about the thread), the potential energy m g h q, so the free joint acceleration is
    -m g h / (I_axis + m h^2).  At rest on a frictionless ground the contact point can only move with h qd along the normal, so the step
    must leave qd >= 0 - which only the linear part of the screw makes possible."""
    md = nut_on_bolt(0.0, 8, shape, mu=0.0)
    b = md.bodies[0]
    h = b.pitch / (2 * np.pi); I_axis = b.inertia[1] + b.mass * (b.com[0] ** 2 + b.com[2] ** 2)
    want = -b.mass * 9.81 * h / (I_axis + b.mass * h * h)
    w = OracleWorld(md)
    s, _ = contact_states(md, 4, 3, vel=0.0)
    for i in range(4):
        q = s[i, :1]
        acc = w.forward_dynamics(q, np.zeros(1), np.zeros(1))[0]
        assert abs(acc - want) <= 1e-12 * abs(want), (acc, want)
        w.reset_lcp_cache()
        nxt = w.step(s[i], np.zeros(1))
        assert w.last_status & 1
        assert nxt[1] >= -1e-12, nxt[1]                                # held by the ground
    assert md.dt * want < -1e-3                                         # (without the ground the step would have ended at dt * want)


def test_screw_joint_transform_is_a_rotation_with_its_share_of_the_pitch():
    from scipy.spatial.transform import Rotation as Rot
    md = screw_arm(0, free_root=False)
    w = OracleWorld(md); rng = np.random.default_rng(1)
    q = rng.normal(0, 1.0, md.num_dofs)
    b0 = md.bodies[0]
    Q = np.eye(4); ax = np.array(b0.axis); Q[:3, :3] = Rot.from_rotvec(ax * q[0]).as_matrix(); Q[:3, 3] = ax * b0.pitch * q[0] / (2 * np.pi)
    T = np.array(b0.T_pj) @ Q @ np.linalg.inv(np.array(b0.T_cj))
    assert np.allclose(w.body_world_transform(q, 0), T, atol=1e-13)
    assert md.bodies[4].pitch == 0.1                                    # ScrewJointAspect's default


@pytest.mark.parametrize("free_root", [True, False])
def test_screw_joint_dynamics_and_backprop_vs_finite_differences(free_root):
    md = screw_arm(1, free_root)
    w = OracleWorld(md); n = w.n; rng = np.random.default_rng(2)
    q, v, a0 = rng.normal(0, 0.6, n), rng.normal(0, 1.0, n), rng.normal(0, 1.0, len(md.action_map))
    tau = np.zeros(n); tau[list(md.action_map)] = a0
    fl = md.flat()
    M = w.mass_matrix(q)
    rhs = tau - w.coriolis_gravity(q, v) - fl["damping"] * v - fl["spring"] * (q - fl["rest"] + md.dt * v)
    assert rel_err(M @ w.forward_dynamics(q, v, tau), rhs) < 1e-10
    scale = max(1.0, np.abs(w.coriolis_gravity(q, v)).max())
    assert np.abs(w.jac_C(q, v, 0) - _fd_jac(lambda x: w.coriolis_gravity(x, v), q)).max() < 2e-7 * scale
    assert np.abs(w.jac_Mx(q, v) - _fd_jac(lambda y: w.mass_matrix(y) @ v, q)).max() < 2e-7 * scale
    s0 = np.concatenate([q, v])
    Js = _fd_jac(lambda x: w.step(x, a0), s0, 1e-6); Ja = _fd_jac(lambda x: w.step(s0, x), a0, 1e-6)
    g = rng.normal(0, 1, 2 * n)
    w.step(s0, a0)
    gs, ga = w.backprop(g)
    assert np.abs(gs - Js.T @ g).max() < 1e-6 * max(1.0, np.abs(gs).max()) and np.abs(ga - Ja.T @ g).max() < 1e-6 * max(1.0, np.abs(ga).max())


@pytest.mark.gpu
@pytest.mark.parametrize("free_root", [True, False])
def test_screw_joints_on_the_device_equal_the_oracle(free_root):
    import torch
    from nimblephysics_amd.timestep import timestep
    md = screw_arm(2, free_root)
    B = 64; rng = np.random.default_rng(3); n = md.num_dofs
    s = np.concatenate([rng.normal(0, 0.6, (B, n)), rng.normal(0, 1.5, (B, n))], 1); a = rng.normal(0, 1, (B, len(md.action_map))); g = rng.normal(0, 1, s.shape)
    world = na.World(md, device="cuda:0")
    st = torch.tensor(s, device="cuda:0", requires_grad=True); at = torch.tensor(a, device="cuda:0", requires_grad=True)
    out = timestep(world, st, at); out.backward(torch.tensor(g, device="cuda:0"))
    ref = OracleWorld(md).step_batch(s, a, g, threads=8)
    sc = lambda x: max(np.abs(x).max(), 1e-30)
    assert np.abs(out.detach().cpu().numpy() - ref["next"]).max() / sc(ref["next"]) < 1e-7
    assert np.abs(st.grad.cpu().numpy() - ref["grad_state"]).max() / sc(ref["grad_state"]) < 1e-7
    assert np.abs(at.grad.cpu().numpy() - ref["grad_action"]).max() / sc(ref["grad_action"]) < 1e-7
