"""The read-out of a step's contacts, impulses and body contact wrenches (nimblephysics_amd/contacts.py, csrc/contact_readout.hip) against
the CPU oracle (OracleWorld.step per world, then last_contacts() / last_lcp()), against the step itself through forward_dynamics with
wrenches, and against itself bit for bit across layouts.  Parity bar: 1e-7 relative to max(1, |reference value|) per field (README,
DESIGN section 5).  Impulses are compared contact by contact only where the LCP solution is unique (two balls, one contact each);
redundant contact sets (cube corners, foot corners) are compared through the body wrenches, which are unique, and through the step."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from util import ball_state, ball_world, box_stack_inputs, cfg_inputs, contact_inputs, cube_tower_inputs, folding_arm, limited_arm

pytestmark = pytest.mark.gpu

TOL = 1e-7
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(dev, ref, tol=TOL):
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return bool((np.abs(dev - ref) <= tol * np.maximum(1.0, np.abs(ref))).all())


def _err(dev, ref):
    dev, ref = np.asarray(dev, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(dev - ref) / np.maximum(1.0, np.abs(ref))).max()) if dev.size else 0.0


def _step(md, s, a, world=None):
    import nimblephysics_amd as na
    world = world or na.World(md, device=DEV)
    st = world.to_soa(torch.tensor(s, device=DEV)); at = world.to_soa(torch.tensor(a, device=DEV))
    nxt, saved, status = world.step_soa(st, at, want_saved=True)
    return world, saved, world.from_soa(nxt).cpu().numpy(), status.cpu().numpy().astype(np.uint32)


def _oracle(md, s, a):
    """per world: (contacts [C, 12], lcp dict, next state)"""
    from oracle import OracleWorld
    ow = OracleWorld(md)
    out = []
    for b in range(len(s)):
        ow.reset_lcp_cache()
        nxt = ow.step(s[b], a[b])
        out.append((ow.last_contacts(), ow.last_lcp(), nxt))
    return ow, out


def _np(r):
    """ContactReadout -> dict of numpy arrays"""
    return {k: getattr(r, k).cpu().numpy() for k in r.FIELDS}


def _match(r, b, oc):
    """device slot of every oracle contact of world b: same collider pair, then the nearest point; a bijection, every point within 1e-9"""
    cnt = int(r["count"][b])
    assert cnt == len(oc), (b, cnt, len(oc))
    free, slots = set(range(cnt)), []
    for c in oc:
        cand = [k for k in free if r["collider_a"][b, k] == int(c[10]) and r["collider_b"][b, k] == int(c[11])]
        assert cand, (b, "no device contact on collider pair", c[10], c[11])
        k = min(cand, key=lambda j: np.linalg.norm(r["point"][b, j] - c[0:3]))
        assert np.linalg.norm(r["point"][b, k] - c[0:3]) < 1e-9, (b, k, r["point"][b, k], c[0:3])
        free.remove(k); slots.append(k)
    assert not free
    return slots


def _check_geometry(tag, r, oracle):
    worst = {"normal": 0.0, "depth": 0.0}
    B = len(oracle)
    assert r["count"].shape == (B,)
    for b, (oc, _, _) in enumerate(oracle):
        slots = _match(r, b, oc)
        for k, c in zip(slots, oc):
            worst["normal"] = max(worst["normal"], _err(r["normal"][b, k], c[3:6])); worst["depth"] = max(worst["depth"], _err(r["depth"][b, k], c[6]))
            assert _close(r["normal"][b, k], c[3:6]) and _close(r["depth"][b, k], c[6]), (tag, b, k)
            assert int(r["type"][b, k]) == int(c[7]), (tag, b, k, r["type"][b, k], c[7])
            assert (int(r["body_a"][b, k]), int(r["body_b"][b, k])) == (int(c[8]), int(c[9])), (tag, b, k, r["body_a"][b, k], r["body_b"][b, k], c[8:10])
        cnt = int(r["count"][b])
        for f in ("point", "normal", "depth", "type", "collider_a", "collider_b", "body_a", "body_b", "impulse", "row_class", "force"):
            assert not np.asarray(r[f][b, cnt:]).any(), (tag, b, f, "slots past the count must be zeros")
    print(f"[{tag}] {B} worlds, contacts per world {np.bincount(r['count'])}, worst relative error {worst}")


def _tangent_basis(n):
    """ContactConstraint::getTangentBasisMatrixODE (ContactConstraint.cpp:734-795)"""
    t = np.cross([0.0, 0.0, 1.0], n)
    if t @ t < 1e-12:
        t = np.cross([1.0, 0.0, 0.0], n)
        if t @ t < 1e-12:
            t = np.cross([0.0, 1.0, 0.0], n)
    t1 = t / np.linalg.norm(t)
    return t1, np.cross(n, t1)


def _oracle_forces(oc, lcp, dt):
    """Contact::force of every oracle contact (three LCP rows per contact: every collider of these scenes has friction)"""
    assert len(lcp["x"]) == 3 * len(oc)
    out = []
    for i, c in enumerate(oc):
        t1, t2 = _tangent_basis(c[3:6])
        x = lcp["x"][3 * i:3 * i + 3]
        out.append((c[3:6] * x[0] + t1 * x[1] + t2 * x[2]) / dt)
    return np.array(out).reshape(len(oc), 3)


def _oracle_wrench(ow, q, body, oc, forces):
    """sum of + force on body A, - force on body B of the oracle's contacts, with the moments about the body's origin: [torque; force]"""
    p0 = ow.body_world_transform(q, body)[:3, 3]
    w = np.zeros(6)
    for c, f in zip(oc, forces):
        sgn = (1.0 if int(c[8]) == body else 0.0) - (1.0 if int(c[9]) == body else 0.0)
        w[:3] += sgn * np.cross(c[0:3] - p0, f); w[3:] += sgn * f
    return w


def _collider_bodies(md):
    """description bodies that carry a collider and move"""
    targets, _ = md.weld_targets()
    return sorted({bx.body for bx in md.boxes if bx.body >= 0 and targets[bx.body] >= 0})


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(md, s, a, world, saved, next, status, oracle world, per-world oracle results, read-out as numpy) of the two scenes of tests 1, 3, 4"""
    from nimblephysics_amd.contacts import read_contacts
    md, s, a = box_stack_inputs(70, 21) if name == "box_stack" else contact_inputs("atlas20", 70, 22)
    world, saved, nxt, status = _step(md, s, a)
    ow, oracle = _oracle(md, s, a)
    return md, s, a, world, saved, nxt, status, ow, oracle, _np(read_contacts(world, saved, len(s)))


SCENES = ["box_stack", "atlas20"]


# ---- 1. geometry and bookkeeping against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_geometry_and_bookkeeping_match_the_oracle(name):
    md, s, a, world, saved, nxt, status, ow, oracle, r = _scene(name)
    assert r["point"].shape == (70, md.max_contacts, 3) and r["collider_a"].dtype == np.int64 and r["count"].dtype == np.int32
    assert not (status & 0x80).any() and (r["count"] == 8).mean() > 0.9
    assert not r["n_limit_rows"].any() and not r["n_friction_rows"].any()
    _check_geometry(name, r, oracle)


# ---- 2. impulses where the LCP solution is unique ---------------------------------------------------------------------------------------
def _two_balls():
    md = ball_world(n_balls=2)
    s, a = ball_state(md, [(-0.6, 0.1), (0.7, -0.2)], 5)
    s[12:] = 0.0
    s[6:9] = 0.0                                            # (ball 1 unrotated: its velocity coordinates are the world's)
    s[12 + 3:12 + 6] = (0.01, -0.05, 0.02)                  # ball 0 rests on the ground (sticking: three clamping rows)
    s[12 + 6 + 3] = 3.0; s[12 + 6 + 5] = -1.2               # ball 1 slides over the ground: its friction rows sit on their bound
    return md, s[None, :].copy(), a[None, :].copy()


def test_impulses_classes_and_forces_match_the_oracle_on_two_balls():
    from nimblephysics_amd.contacts import read_contacts
    md, s, a = _two_balls()
    world, saved, nxt, status = _step(md, s, a)
    ow, oracle = _oracle(md, s, a)
    oc, lcp, onxt = oracle[0]
    r = _np(read_contacts(world, saved, 1))
    assert len(oc) == 2 and (lcp["row_class"] == 2).sum() >= 1 and (lcp["row_class"] == 1).sum() >= 3, lcp["row_class"]
    slots = _match(r, 0, oc)
    forces = _oracle_forces(oc, lcp, md.dt)
    for i, k in enumerate(slots):
        x, rc = lcp["x"][3 * i:3 * i + 3], lcp["row_class"][3 * i:3 * i + 3]
        print(f"[two balls] contact {i}: impulse err {_err(r['impulse'][0, k], x):.2e}, force err {_err(r['force'][0, k], forces[i]):.2e}, classes {r['row_class'][0, k]} / {rc}")
        assert _close(r["impulse"][0, k], x), (i, r["impulse"][0, k], x)
        assert np.array_equal(np.abs(r["row_class"][0, k]).astype(int), rc), (i, r["row_class"][0, k], rc)
        assert _close(r["force"][0, k], forces[i]), (i, r["force"][0, k], forces[i])
    assert _close(nxt[0], onxt)


# ---- 3. body wrenches against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_body_wrenches_match_the_oracle_sums(name):
    from nimblephysics_amd.contacts import body_contact_wrenches
    md, s, a, world, saved, nxt, status, ow, oracle, r = _scene(name)
    names = [1, 2] if name == "box_stack" else ["l_foot", "r_foot"]
    idx = [b if isinstance(b, int) else [i for i, bd in enumerate(md.bodies) if bd.name == b][0] for b in names]
    W = body_contact_wrenches(world, saved, len(s), names).cpu().numpy()
    assert W.shape == (70, 2, 6)
    worst = 0.0
    for b, (oc, lcp, _) in enumerate(oracle):
        forces = _oracle_forces(oc, lcp, md.dt)
        for e, body in enumerate(idx):
            want = _oracle_wrench(ow, s[b, :md.num_dofs], body, oc, forces)
            worst = max(worst, _err(W[b, e], want))
            assert _close(W[b, e], want), (name, b, e, W[b, e], want)
    assert np.abs(W[:, :, 3:]).max() > 0.5
    print(f"[{name}] body wrenches of {names}: worst relative error {worst:.2e}")


# ---- 4. consistency with the step through forward dynamics with wrenches ----------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_read_out_wrenches_reproduce_the_step_through_forward_dynamics(name):
    """v' - v = dt forward_dynamics(state, tau, joint_forces=True, wrenches=W, bodies, world_frame=True) with W the read-out wrenches on
    every body that carries a collider: pins the sign, the point of action and the tangent basis end to end.  No oracle."""
    import nimblephysics_amd as na
    from nimblephysics_amd.contacts import body_contact_wrenches
    md, s, a, world, saved, nxt, status, ow, oracle, r = _scene(name)
    n, B = md.num_dofs, len(s)
    assert not world.getPenetrationCorrectionEnabled() and not r["n_limit_rows"].any() and not r["n_friction_rows"].any()
    assert list(md.action_map) == list(range(n))
    bodies = _collider_bodies(md)
    assert len(bodies) == 2
    W = body_contact_wrenches(world, saved, B, bodies)
    st, tau = torch.tensor(s, device=DEV), torch.tensor(a, device=DEV)
    acc = na.forward_dynamics(world, st, tau, joint_forces=True, wrenches=W.reshape(B, 12), bodies=bodies, world_frame=True).cpu().numpy()
    dv = nxt[:, n:] - s[:, n:]
    free = na.forward_dynamics(world, st, tau, joint_forces=True).cpu().numpy()
    assert np.abs(dv - md.dt * free).max() > 1e-4                      # the contacts matter: without the wrenches the step is NOT reproduced
    print(f"[{name}] max |dv - dt a| / max(1, |dv|) = {_err(md.dt * acc, dv):.2e} (without the wrenches {_err(md.dt * free, dv):.2e})")
    assert _close(md.dt * acc, dv), _err(md.dt * acc, dv)


# ---- 5. edge shapes ---------------------------------------------------------------------------------------------------------------------
def test_worlds_without_contacts_next_to_full_worlds():
    from nimblephysics_amd.contacts import body_contact_wrenches, read_contacts
    md, s, a = box_stack_inputs(70, 31)
    s[1::2, 4] += 5.0; s[1::2, 10] += 10.0                             # both cubes parked high, apart, in every other world
    world, saved, nxt, status = _step(md, s, a)
    ow, oracle = _oracle(md, s, a)
    r = _np(read_contacts(world, saved, 70))
    assert (r["count"][1::2] == 0).all() and (r["count"][0::2] == 8).all() and md.max_contacts == 8
    _check_geometry("empty next to full", r, oracle)
    W = body_contact_wrenches(world, saved, 70, [1, 2]).cpu().numpy()
    assert not W[1::2].any() and np.abs(W[0::2, :, 3:]).max() > 0.5


def test_frictionless_contacts_have_empty_tangent_slots():
    from nimblephysics_amd import _abi
    from nimblephysics_amd.contacts import read_contacts
    md, s, a = cube_tower_inputs(9, 41, 1, max_contacts=8, mu=5e-4)
    world, saved, nxt, status = _step(md, s, a)
    ow, oracle = _oracle(md, s, a)
    r = _np(read_contacts(world, saved, 9))
    _check_geometry("frictionless", r, oracle)
    for b, (oc, lcp, _) in enumerate(oracle):
        cnt = int(r["count"][b])
        assert cnt == 4 and len(lcp["x"]) == cnt                       # one LCP row per contact in the reference
        assert not r["impulse"][b, :cnt, 1:].any() and (r["row_class"][b, :cnt, 1:] == _abi.CO_CLASS_EMPTY).all()
        assert np.allclose(r["force"][b, :cnt], r["normal"][b, :cnt] * r["impulse"][b, :cnt, :1] / md.dt, rtol=1e-14, atol=0)
        assert _close(r["impulse"][b, :cnt, 0].sum(), lcp["x"].sum())   # (four corners: only the total is unique)
    assert r["impulse"][:, :, 0].max() > 1e-5


@pytest.mark.parametrize("slots,build", [(16, 16), (24, 64)])
def test_sixteen_and_twenty_four_slot_models(slots, build):
    from nimblephysics_amd.contacts import body_contact_wrenches, read_contacts
    md, s, a = cube_tower_inputs(12, 51, 3, max_contacts=slots)
    world, saved, nxt, status = _step(md, s, a)
    assert world._L.nbl_model_max_contacts(world._h) == build
    ow, oracle = _oracle(md, s, a)
    r = _np(read_contacts(world, saved, 12))
    assert r["point"].shape == (12, slots, 3) and (r["count"] == 12).mean() > 0.8
    _check_geometry(f"{slots} slots", r, oracle)
    W = body_contact_wrenches(world, saved, 12, [0, 1, 2]).cpu().numpy()
    for b, (oc, lcp, _) in enumerate(oracle):
        forces = _oracle_forces(oc, lcp, md.dt)
        for e in range(3):
            assert _close(W[b, e], _oracle_wrench(ow, s[b, :md.num_dofs], e, oc, forces)), (slots, b, e)


def test_a_joint_limit_row_is_not_a_contact():
    from nimblephysics_amd.contacts import body_contact_wrenches, read_contacts
    md = limited_arm(enforce=True, ground=True)
    n = md.num_dofs
    s = np.zeros((3, 2 * n)); a = np.zeros((3, n))
    s[:, 0] = [-0.01, -0.02, -0.015]                                  # the base's box in the ground: four corner contacts
    s[:, 1] = [0.41, 0.1, -0.5]                                       # hinge 0 above its upper limit / free / on its lower limit
    s[:, n + 1] = [1.0, 0.0, -1.0]                                    # ... and moving further out: the limit rows carry an impulse
    world, saved, nxt, status = _step(md, s, a)
    ow, oracle = _oracle(md, s, a)
    r = _np(read_contacts(world, saved, 3))
    assert list(r["n_limit_rows"]) == [1, 0, 1] and not r["n_friction_rows"].any() and (status & 0x400 != 0).tolist() == [True, False, True]
    _check_geometry("limited arm on the ground", r, oracle)            # count == the oracle's contacts: the limit row is not among them
    assert (r["count"] == 4).all()
    W = body_contact_wrenches(world, saved, 3, ["base", "link0"]).cpu().numpy()
    for b in range(3):
        f = r["force"][b, :4].sum(0) * (1.0 if r["body_a"][b, 0] == 0 else -1.0)
        assert np.allclose(W[b, 0, 3:], f, rtol=1e-13, atol=1e-13) and not W[b, 1].any()   # link 0 has the limit row and no collider: zeros
    # the live LCP rows: 12 contact rows, then the limit row (negative at the upper limit, the reference's sign)
    import nimblephysics_amd as na
    world.setState(torch.tensor(s, device=DEV)); world.setAction(torch.tensor(a, device=DEV)); world.reset_lcp_cache()
    snap = na.neural.forwardPass(world)
    assert snap.getNumContacts().tolist() == [13, 12, 13]
    imp = snap.getContactConstraintImpulses()
    assert imp[0][12] < 0.0 < imp[2][12] and [len(v) for v in imp] == [13, 12, 13]


def test_a_self_collision_gives_equal_and_opposite_forces():
    from nimblephysics_amd.contacts import body_contact_wrenches, read_contacts
    md = folding_arm()
    rng = np.random.default_rng(61)
    B = 16
    q = np.stack([rng.uniform(-0.3, 0.3, B), rng.uniform(2.05, 2.15, B), rng.uniform(1.9, 1.945, B)], 1)
    s = np.concatenate([q, rng.normal(0, 0.3, (B, 3))], 1); a = rng.normal(0, 0.1, (B, 3))
    world, saved, nxt, status = _step(md, s, a)
    ow, oracle = _oracle(md, s, a)
    r = _np(read_contacts(world, saved, B))
    _check_geometry("folding arm", r, oracle)
    touching = r["count"] > 0
    assert touching.mean() > 0.5
    W = body_contact_wrenches(world, saved, B, ["l0", "l1", "l2"]).cpu().numpy()
    assert np.array_equal(W[:, 0, 3:], -W[:, 2, 3:]) and not W[:, 1].any() and np.abs(W[touching, 0, 3:]).max() > 1e-3
    for b in np.nonzero(touching)[0]:
        assert {int(r["body_a"][b, 0]), int(r["body_b"][b, 0])} == {0, 2}


def test_a_welded_body_reports_its_own_index():
    import nimblephysics_amd as na
    from nimblephysics_amd.contacts import read_contacts
    I = (0.02, 0.02, 0.02, 0, 0, 0)
    bodies = [na.BodySpec("base", -1, "free", "root", mass=1.0, inertia=I),
              na.BodySpec("pad", 0, "weld", "pad_weld", T_pj=na.make_transform((0.0, -0.1, 0.0)), mass=0.2, inertia=I)]
    boxes = [na.BoxSpec(-1, na.make_transform((0, -0.5, 0)), (4.0, 1.0, 4.0), 1.0), na.BoxSpec(1, np.eye(4), (0.2, 0.1, 0.2), 0.9)]
    md = na.ModelDescription("welded_pad", bodies, boxes, max_contacts=8)
    s = np.zeros((2, 12)); s[:, 4] = [0.149, 0.148]; s[:, 1] = [0.2, -0.4]; a = np.zeros((2, 6))
    world, saved, nxt, status = _step(md, s, a)
    assert len(world.model.bodies) == 1                                # the device model merged the pad into the base
    ow, oracle = _oracle(md, s, a)
    r = _np(read_contacts(world, saved, 2))
    _check_geometry("welded pad", r, oracle)
    assert (r["count"] == 4).all() and (r["body_a"][:, :4] == -1).all() and (r["body_b"][:, :4] == 1).all()


def test_a_model_without_colliders_has_no_contacts():
    import nimblephysics_amd as na
    from nimblephysics_amd.contacts import body_contact_wrenches, read_constraint_rows, read_contacts
    md, s, a = cfg_inputs("cartpole", 5, 1)
    world, saved, nxt, status = _step(md, s, a)
    r = read_contacts(world, saved, 5)
    assert not r.count.any() and r.point.shape == (5, 0, 3) and not r.n_limit_rows.any()
    assert not body_contact_wrenches(world, saved, 5, [0, 1]).any()
    assert not read_constraint_rows(world, saved, 5)[0].any()
    world.setState(torch.tensor(s, device=DEV)); world.setAction(torch.tensor(a, device=DEV)); world.step()
    assert not world.getLastCollisionResult().count.any()


def test_argument_errors():
    import ctypes as C
    from nimblephysics_amd import _abi
    from nimblephysics_amd._lib import NimbleAmdError
    from nimblephysics_amd.contacts import body_contact_wrenches
    md, s, a, world, saved, *_ = _scene("box_stack")
    L, h, p = world._L, world._h, C.c_void_p(saved.data_ptr())
    out = torch.zeros(70 * 12, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(70, dtype=torch.int32, device=DEV)
    ids = lambda *v: np.asarray(v, dtype=np.int32).ctypes.data_as(C.c_void_p)   # noqa: E731
    o, c = C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr())
    BAD = _abi.NBL_E_BADARG
    assert L.nbl_contact_readout(h, 70, None, c, None, None, None, None) == BAD and L.nbl_contact_readout(h, 70, p, None, None, None, None, None) == BAD
    assert L.nbl_contact_readout(h, -1, p, c, None, None, None, None) == BAD and L.nbl_contact_readout(h, 0, None, c, None, None, None, None) == 0
    assert L.nbl_contact_body_wrenches(h, 70, p, 2, ids(0, 0), o, None) == BAD and b"twice" in L.nbl_last_error()
    assert L.nbl_contact_body_wrenches(h, 70, p, 1, ids(2), o, None) == BAD and L.nbl_contact_body_wrenches(h, 70, p, 1, ids(-1), o, None) == BAD
    assert L.nbl_contact_body_wrenches(h, 70, p, 65, ids(*range(65)), o, None) == BAD and L.nbl_contact_body_wrenches(h, 70, p, -1, None, o, None) == BAD
    assert L.nbl_contact_body_wrenches(h, 70, p, 1, ids(0), None, None) == BAD and L.nbl_contact_body_wrenches(h, 0, None, 1, ids(0), o, None) == 0
    assert L.nbl_contact_readout_rows(h, 70, p, None, None, None, None) == BAD
    with pytest.raises(NimbleAmdError, match="twice"):
        body_contact_wrenches(world, saved, 70, [1, 1])
    with pytest.raises(NimbleAmdError, match="welded to the world"):
        body_contact_wrenches(world, saved, 70, [0])


# ---- 6. layout independence -------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys, numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import nimblephysics_amd as na
from nimblephysics_amd.contacts import read_contacts, body_contact_wrenches
from util import box_stack_inputs
md, s, a = box_stack_inputs(70, 21)
w = na.World(md, device="cuda:0")
nxt, saved, status = w.step_soa(w.to_soa(torch.tensor(s, device="cuda:0")), w.to_soa(torch.tensor(a, device="cuda:0")), want_saved=True)
out = {{}}
r = read_contacts(w, saved, 70)
out.update({{"own_" + k: getattr(r, k).cpu().numpy() for k in r.FIELDS}})
# the parent's record, read by THIS handle: first block and dense block lie where this handle's do, its tree block behind them is cut off
given = torch.tensor(np.load({record!r}), device="cuda:0")[:saved.numel()].contiguous()
r = read_contacts(w, given, 70)
out.update({{k: getattr(r, k).cpu().numpy() for k in r.FIELDS}})
out["wrench"] = body_contact_wrenches(w, given, 70, [1, 2]).cpu().numpy()
out["saved_bytes"] = np.array(w.saved_bytes(70))
np.savez({out!r}, **out)
"""


def test_bit_identical_without_the_saved_tree_block(tmp_path):
    """A handle made with NBL_SAVE_TREE=0 (fresh child process: records without a tree block) reads the SAME worlds' record bit for bit
    like the default handle: contacts, impulses, classes, forces and wrenches.  The record is handed to the child, because the two modes
    run different tree kernels and their own steps agree to rounding only, not bit for bit (measured on MI355X, box stack, B = 70: every
    geometry and bookkeeping field of the child's own step is bit-identical, its impulses differ from the default mode's by up to 7.1e-14
    and its forces by 1.1e-10 of the largest force - the figures this test prints): that difference belongs to the step, which this read-out
    does not touch."""
    from nimblephysics_amd.contacts import body_contact_wrenches
    md, s, a, world, saved, nxt, status, ow, oracle, r = _scene("box_stack")
    out, record = str(tmp_path / "child.npz"), str(tmp_path / "record.npy")
    np.save(record, saved.cpu().numpy())
    env = dict(os.environ, NBL_SAVE_TREE="0")
    subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), out=out, record=record)], check=True, env=env,
                   timeout=300)
    got = np.load(out)
    assert int(got["saved_bytes"]) < world.saved_bytes(70)            # the child's records carry no tree block
    for k in r:
        assert np.array_equal(got[k], r[k]), k
    assert np.array_equal(got["wrench"], body_contact_wrenches(world, saved, 70, [1, 2]).cpu().numpy())
    for k in ("count", "point", "normal", "depth", "type", "collider_a", "collider_b", "body_a", "body_b", "n_limit_rows", "n_friction_rows"):
        assert np.array_equal(got["own_" + k], r[k]), k               # the narrow phase does not depend on the tree kernels
    print("[NBL_SAVE_TREE=0] the child's OWN step against the default mode's: impulse", _err(got["own_impulse"], r["impulse"]),
          "force", float(np.abs(got["own_force"] - r["force"]).max() / np.abs(r["force"]).max()))


def test_bit_identical_alone_and_inside_a_batch():
    from nimblephysics_amd.contacts import body_contact_wrenches, read_contacts
    md, s, a, world, saved, nxt, status, ow, oracle, r = _scene("box_stack")
    W = body_contact_wrenches(world, saved, 70, [1, 2]).cpu().numpy()
    for b in (0, 63, 64, 69):
        w1, sv1, _, _ = _step(md, s[b:b + 1], a[b:b + 1])
        r1 = _np(read_contacts(w1, sv1, 1))
        for k in r:
            assert np.array_equal(r1[k][0], r[k][b]), (b, k)
        assert np.array_equal(body_contact_wrenches(w1, sv1, 1, [1, 2]).cpu().numpy()[0], W[b])


def test_bit_identical_after_a_deferred_join_step():
    import nimblephysics_amd as na
    from nimblephysics_amd.contacts import body_contact_wrenches, read_contacts
    B = 512
    md, s, a = box_stack_inputs(B, 71)
    world, saved, nxt, status = _step(md, s, a)
    want, wantW = _np(read_contacts(world, saved, B)), body_contact_wrenches(world, saved, B, [1, 2])
    w = na.World(md, device=DEV)
    w.set_slices(2); w.set_deferred_join(True)
    assert len(w.slices(B)) == 2
    st = w.to_soa(torch.tensor(s, device=DEV)); at = w.to_soa(torch.tensor(a, device=DEV))
    bufs = dict(nxt=torch.empty_like(st), saved=torch.empty(w.saved_bytes(B), dtype=torch.uint8, device=DEV),
                status=torch.empty(B, dtype=torch.int32, device=DEV), cache=torch.empty((w.m, B), dtype=torch.float64, device=DEV))
    w.fork()
    w.step_into(st, at, bufs["nxt"], bufs["saved"], bufs["status"], None, bufs["cache"])     # returns with its slices in flight
    got = _np(read_contacts(w, bufs["saved"], B))                                             # joins by itself
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert torch.equal(body_contact_wrenches(w, bufs["saved"], B, [1, 2]), wantW)
    torch.cuda.synchronize()


# ---- 7. rollout -------------------------------------------------------------------------------------------------------------------------
def test_rollout_read_outs_equal_chained_timesteps():
    import nimblephysics_amd as na
    from nimblephysics_amd._lib import NimbleAmdError
    from nimblephysics_amd.contacts import body_contact_wrenches, rollout_body_contact_wrenches, rollout_contacts
    from nimblephysics_amd.timestep import rollout, timestep
    T, B = 3, 5
    md, s, a = box_stack_inputs(B, 81)
    acts = np.random.default_rng(82).normal(0, 0.05, (B, T, 12))
    w = na.World(md, device=DEV)
    states = rollout(w, torch.tensor(s, device=DEV), torch.tensor(acts, device=DEV))
    rc, rw = rollout_contacts(w), rollout_body_contact_wrenches(w, [1, 2])
    assert rc.point.shape == (T, B, 8, 3) and rc.count.shape == (T, B) and rw.shape == (T, B, 2, 6)
    w2 = na.World(md, device=DEV)
    x = torch.tensor(s, device=DEV)
    for t in range(T):
        x = timestep(w2, x, torch.tensor(acts[:, t], device=DEV))
        assert torch.equal(x, states[:, t + 1])
        one = w2.getLastCollisionResult()
        for k in one.FIELDS:
            assert torch.equal(getattr(one, k), getattr(rc, k)[t]), (t, k)
        assert torch.equal(body_contact_wrenches(w2, w2._last_record, B, [1, 2]), rw[t])
    assert rc.count.sum() > 0
    rollout(w, torch.tensor(s, device=DEV), torch.tensor(acts, device=DEV), checkpoint_every=2)
    with pytest.raises(NimbleAmdError, match="checkpoint_every"):
        rollout_contacts(w)
    with pytest.raises(NimbleAmdError, match="checkpoint_every"):
        rollout_body_contact_wrenches(w, [1, 2])


# ---- 8. snapshot API --------------------------------------------------------------------------------------------------------------------
def test_snapshot_counts_and_impulses_match_the_oracle_on_two_balls():
    import nimblephysics_amd as na
    md, s, a = _two_balls()
    ow, oracle = _oracle(md, s, a)
    oc, lcp, _ = oracle[0]
    world = na.World(md, device=DEV)
    world.setState(torch.tensor(s[0], device=DEV)); world.setAction(torch.tensor(a[0], device=DEV))
    snap = na.neural.forwardPass(world)
    x, rc = lcp["x"], lcp["row_class"]
    assert snap.getNumContacts() == len(x) == 6
    assert snap.getNumClamping() == int((rc == 1).sum()) and snap.getNumUpperBound() == int((rc == 2).sum()) >= 1
    imp, mp, fc = snap.getContactConstraintImpulses().cpu().numpy(), snap.getContactConstraintMappings().cpu().numpy(), snap.getClampingConstraintImpulses().cpu().numpy()
    assert imp.shape == (6,) and _close(imp, x), (imp, x)
    assert np.array_equal(mp == -1, rc == 1) and np.array_equal(mp >= 0, rc == 2) and np.array_equal(mp[mp >= 0], lcp["findex"][mp >= 0])
    assert _close(fc, x[rc == 1])
    r = snap.getContacts()
    assert int(r.count[0]) == 2 and torch.equal(world.getLastCollisionResult().force, r.force)
    W = snap.getBodyContactWrenches(["ball0", "ball1"])
    assert W.shape == (2, 6)
    for k in range(2):                                                 # one contact per ball, the ground (the world) on the other side
        ball, sgn = (int(r.body_a[0, k]), 1.0) if int(r.body_b[0, k]) < 0 else (int(r.body_b[0, k]), -1.0)
        assert torch.equal(W[ball, 3:], sgn * r.force[0, k])
