"""The contact-independent calls (csrc/nimble_amd_tree.hip: kinematics, dynamics, wrenches, IK and its reverse pass, centroidal quantities,
sensors, task-space Jacobians and accelerations) are built once and work on the capacity-independent base of a handle that one of FOUR instantiations of the contact stage owns (csrc/abi_variants.h,
csrc/tree_model_host.hpp).  Every other dynamics / kinematics test creates collider-free models, which always land in the 8-slot build; here
the same model is created in all four (NBL_MIN_VARIANT = 0..3, read at every nbl_model_create) and every call is run on all four handles.

Model: a ball joint below a free root with colliders (test_ball_joint.ball_model, ground=True: the body map of the handle is not the
identity, and nbl_model_max_contacts tells the four instantiations apart).  B = 65: the launches use 64-lane blocks, so one full block and a
one-lane tail.

ACROSS THE HANDLES: bitwise equal - one kernel, one input, the same constants.
AGAINST THE REFERENCE, on the handle of the 8-slot build, at the tolerance and with the reference of the existing GPU test of each call:
  inverse / forward dynamics, mass matrix and its inverse   the oracle, 1e-10 (_rel)   test_gpu_dynamics, test_gpu_forward_dynamics
  forward dynamics with a world-frame wrench                 the oracle, 1e-10          test_gpu_forward_dynamics (accelerations); the wrench
                                                                                        term is test_wrench_host.world_wrenches
  map_to_pos / map_to_vel / the position VJP                 kin_numpy, 1e-12 / 1e-10   test_gpu_kinematics
  centroidal outputs, sensor readings                        cen_numpy / sens_numpy, 1e-10   test_gpu_centroidal, test_gpu_sensors
  solve_ik, max_step_count = 20                              the host build, 1e-9, equal step counts (up to 25 steps: test_ik_host) test_gpu_ik
  task_jacobian, task_jacobian_deriv, map_to_acc             task_numpy, FORWARD_TOL; reverse passes: 100 x the scatter of the reference's
                                                             own central differences                     test_gpu_taskspace
  solve_ik_vjp at the solver's poses                         ik_grad_numpy, 10 d, cond(J_F) <= 1e3 in every world   test_gpu_ik_grad
The other VJPs are held bitwise to the 8-slot handle's, which is the build every existing VJP test already runs against its reference."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_dynamics import _rel, _states

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B = 65
CAPACITY = (8, 16, 64, 128)
TOL = 1e-10


def _t(x, grad=False):
    return torch.tensor(np.ascontiguousarray(x), device=DEV, requires_grad=grad)


def _worlds(md):
    """the model on a handle of each instantiation; NBL_MIN_VARIANT is set by the caller's fixture"""
    import os
    import nimblephysics_amd as na
    out = []
    for v, cap in enumerate(CAPACITY):
        os.environ["NBL_MIN_VARIANT"] = str(v)
        w = na.World(md, device=DEV)
        assert w._L.nbl_model_max_contacts(w._h) == cap
        out.append(w)
    return out


@pytest.fixture(scope="module")
def rig():
    from oracle import OracleWorld
    from test_ball_joint import ball_model
    md = ball_model(4, True, ground=True)
    n = md.num_dofs
    ball = [i for i, b in enumerate(md.bodies) if b.joint_type == "ball"][0]
    entries = [(0, ball), (1, len(md.bodies) - 1)]            # (kind, body): one spatial, one linear
    ow = OracleWorld(md)
    S, A, g = _states(md, 4 * B, 11)
    # the spatial entry's rotation at least 0.3 rad below pi, as test_gpu_kinematics keeps it (logMap loses digits there)
    pool = [b for b in range(4 * B)
            if np.arccos(np.clip(0.5 * (np.trace(ow.body_world_transform(S[b, :n], ball)[:3, :3]) - 1), -1, 1)) < np.pi - 0.3]
    keep = pool[:B]
    assert len(keep) == B
    rng = np.random.default_rng(12)
    mp = pytest.MonkeyPatch()
    mp.setenv("NBL_MIN_VARIANT", "0")
    r = {"md": md, "n": n, "ball": ball, "entries": entries, "ow": ow, "S": S[keep], "A": A[keep], "g": g[keep], "worlds": _worlds(md),
         "pool": S[pool],                                          # every pose with the log-map margin: the reverse pass of IK picks from it
         "W": rng.normal(0, 3.0, (B, 6)), "F": rng.normal(0, 1.0, (B, 3)), "G": rng.normal(0, 1.0, (B, n, n)), "gp": rng.normal(0, 1.0, (B, 9))}
    yield r
    mp.undo()


def _mapping(w, entries):
    import nimblephysics_amd as na
    m = na.IKMapping(w)
    for kind, body in entries:
        (m.addSpatialBodyNode, m.addLinearBodyNode)[kind](body)
    return m


def _on_every_handle(worlds, call):
    """call(world) -> tuple of tensors, on the four handles: bitwise equal; returns the 8-slot handle's as numpy"""
    outs = [call(w) for w in worlds]
    for cap, o in zip(CAPACITY[1:], outs[1:]):
        assert len(o) == len(outs[0])
        for k, (x, y) in enumerate(zip(outs[0], o)):
            assert torch.equal(x, y), (cap, k)
    return [x.detach().cpu().numpy() for x in outs[0]]


def test_the_four_handles_are_owned_by_four_instantiations(rig):
    assert [w._L.nbl_model_max_contacts(w._h) for w in rig["worlds"]] == list(CAPACITY)
    assert [w._L.nbl_model_num_dofs(w._h) for w in rig["worlds"]] == [rig["n"]] * 4


def test_dynamics_and_mass_matrices(rig):
    import nimblephysics_amd as na
    S, A, g, G, n, ow = rig["S"], rig["A"], rig["g"], rig["G"], rig["n"], rig["ow"]

    def call(w):
        s1, a1 = _t(S, True), _t(A, True)
        tau = na.inverse_dynamics(w, s1, a1); tau.backward(_t(g))
        s2, t2 = _t(S, True), _t(A, True)
        acc = na.forward_dynamics(w, s2, t2); acc.backward(_t(g))
        s3 = _t(S, True)
        M = na.mass_matrix(w, s3); M.backward(_t(G))
        s4 = _t(S, True)
        Mi = na.inv_mass_matrix(w, s4); Mi.backward(_t(G))
        return tau, s1.grad, a1.grad, acc, s2.grad, t2.grad, M, s3.grad, Mi, s4.grad
    tau, _, ga, acc, _, _, M, _, Mi, _ = _on_every_handle(rig["worlds"], call)
    for b in range(B):
        q, v = S[b, :n], S[b, n:]
        Mo, Co = ow.mass_matrix(q), ow.coriolis_gravity(q, v)
        e = {"tau": _rel(tau[b], Mo @ A[b] + Co), "ga": _rel(ga[b], Mo.T @ g[b]), "acc": _rel(acc[b], np.linalg.solve(Mo, A[b] - Co)),
             "M": _rel(M[b], Mo), "Minv": _rel(Mi[b], np.linalg.inv(Mo))}
        assert max(e.values()) <= TOL, (b, e)


def test_forward_dynamics_with_a_world_frame_wrench(rig):
    import nimblephysics_amd as na
    from test_wrench_host import world_wrenches
    S, A, g, W, n, ow, md, ball = rig["S"], rig["A"], rig["g"], rig["W"], rig["n"], rig["ow"], rig["md"], rig["ball"]
    maps = {id(w): _mapping(w, [(0, ball)]) for w in rig["worlds"]}

    def call(w):
        s, t, ww = _t(S, True), _t(A, True), _t(W, True)
        acc = na.forward_dynamics(w, s, t, wrenches=ww, bodies=maps[id(w)], world_frame=True)
        acc.backward(_t(g))
        return acc, s.grad, t.grad, ww.grad
    acc, _, _, gw = _on_every_handle(rig["worlds"], call)
    assert np.abs(gw).max() > 0
    for b in range(B):
        q, v = S[b, :n], S[b, n:]
        Mo, Co = ow.mass_matrix(q), ow.coriolis_gravity(q, v)
        Jv, Ww, _ = world_wrenches(ow, md, q, [(ball, np.eye(4))], W[b], True)
        assert _rel(acc[b], np.linalg.solve(Mo, A[b] - Co + Jv.T @ Ww)) <= TOL, b


def test_map_to_pos_and_map_to_vel(rig):
    import nimblephysics_amd as na
    from kin_numpy import mapping_rows
    S, gp, n, ow, md, entries = rig["S"], rig["gp"], rig["n"], rig["ow"], rig["md"], rig["entries"]
    maps = {id(w): _mapping(w, entries) for w in rig["worlds"]}

    def call(w):
        s1, s2 = _t(S, True), _t(S, True)
        pos = na.map_to_pos(w, maps[id(w)], s1); pos.backward(_t(gp))
        vel = na.map_to_vel(w, maps[id(w)], s2); vel.backward(_t(gp))
        return pos, s1.grad, vel, s2.grad
    pos, gpos, vel, _ = _on_every_handle(rig["worlds"], call)
    assert pos.shape == (B, 9)
    for b in range(B):
        rows, Jp, Jv = mapping_rows(ow, md, S[b, :n], entries)
        assert np.abs(pos[b] - rows).max() <= 1e-12 * max(1.0, np.abs(rows).max()), b
        assert _rel(vel[b], Jv @ S[b, n:]) <= 1e-10 and _rel(gpos[b, :n], Jp.T @ gp[b]) <= 1e-10, b


def test_centroidal_outputs(rig):
    import cen_numpy
    import nimblephysics_amd as na
    from test_gpu_centroidal import NAMES, ROWS
    S, A, n, ow, md = rig["S"], rig["A"], rig["n"], rig["ow"], rig["md"]
    cots = [np.random.default_rng(13 + k).normal(0, 1.0, (B, r)) for k, r in enumerate(ROWS)]

    def call(w):
        s, a = _t(S, True), _t(A, True)
        out = na.centroidal(w, s, a)
        sum((out[k].reshape(B, -1) * _t(cots[k])).sum() for k in range(6)).backward()
        return tuple(out[k] for k in range(6)) + (s.grad, a.grad)
    got = _on_every_handle(rig["worlds"], call)
    sel = cen_numpy.default_set(md)
    for b in range(B):
        r = cen_numpy.outputs(ow, md, sel, S[b, :n], S[b, n:], A[b])
        e = {nm: _rel(got[k][b].reshape(-1), np.asarray(r[nm]).reshape(-1)) for k, nm in enumerate(NAMES)}
        assert max(e.values()) <= TOL, (b, e)


def test_sensor_readings(rig):
    import nimblephysics_amd as na
    import sens_numpy
    from test_sensors_host import as_numpy_sensors, sensor_list
    S, A, F, n, ow, md = rig["S"], rig["A"], rig["F"], rig["n"], rig["ow"], rig["md"]
    sensors = sensor_list(md)
    cots = [np.random.default_rng(23 + k).normal(0, 1.0, (B, 3 * len(sensors))) for k in range(3)]

    def call(w):
        s, a, f = _t(S, True), _t(A, True), _t(F, True)
        out = na.imu_readings(w, sensors, s, a, f)
        sum((out[k] * _t(cots[k])).sum() for k in range(3)).backward()
        return out.gyro, out.acc, out.mag, s.grad, a.grad, f.grad
    got = _on_every_handle(rig["worlds"], call)
    for b in range(B):
        r = sens_numpy.readings(ow, md, as_numpy_sensors(sensors), S[b, :n], S[b, n:], A[b], F[b])
        e = {nm: _rel(got[k][b], r[nm]) for k, nm in enumerate(("gyro", "acc", "mag"))}
        assert max(e.values()) <= TOL, (b, e)


def test_solve_ik(rig):
    import ik_cases as ic
    import nimblephysics_amd as na
    from kin_numpy import mapping_rows
    S, n, ow, md, entries = rig["S"], rig["n"], rig["ow"], rig["md"], rig["entries"]
    targets = np.stack([mapping_rows(ow, md, S[b, :n], entries)[0] for b in range(B)])
    maps = {id(w): _mapping(w, entries) for w in rig["worlds"]}
    q, loss, steps = _on_every_handle(rig["worlds"], lambda w: na.solve_ik(w, maps[id(w)], _t(targets), None, na.IKConfig(max_step_count=20)))
    hq, _, hs = ic.HostIK(ic.load_ik_shim(), md, entries).solve(targets, max_step_count=20)
    assert np.array_equal(steps, hs) and float(np.abs(q - hq).max()) <= 1e-9


def test_task_space_jacobians_and_accelerations(rig):
    import nimblephysics_amd as na
    import task_cases as tc
    import task_numpy as tn
    from test_gpu_taskspace import FORWARD_TOL
    S, A, n, md, entries = rig["S"], rig["A"], rig["n"], rig["md"], rig["entries"]
    R = tc.rows(entries)
    rng = np.random.default_rng(31)
    cot, G = rng.normal(size=(B, R)), rng.normal(size=(B, R, n))
    maps = {id(w): _mapping(w, entries) for w in rig["worlds"]}

    def call(w):
        s1, a1, s2 = _t(S, True), _t(A, True), _t(S, True)
        xdd = na.map_to_acc(w, maps[id(w)], s1, a1); xdd.backward(_t(cot))
        J = na.task_jacobian(w, maps[id(w)], s2); J.backward(_t(G))
        return J, na.task_jacobian_deriv(w, maps[id(w)], _t(S)), xdd, s1.grad, a1.grad, s2.grad
    J, Jd, xdd, gs, ga, gj = _on_every_handle(rig["worlds"], call)
    assert J.shape == (B, R, n) and not gj[:, n:].any()
    m, ne, q, v = tn.Model(md), tc.numpy_entries(entries), S[:, :n], S[:, n:]
    Jr, Jdr = tn.jacobians(m, ne, q, v)
    for what, got, ref in (("J", J, Jr), ("Jdot", Jd, Jdr), ("xdd", xdd, tn.accel(m, ne, q, v, A))):
        e = tc.err(got, ref)
        print(what, "largest per-world deviation:", float(e.max()))
        assert (e <= FORWARD_TOL).all(), (what, int(e.argmax()), float(e.max()))
    fd = {eps: tn.fd_accel_vjp(m, ne, q, v, A, cot, eps) + (tn.fd_jacobian_vjp(m, ne, q, G, eps),) for eps in (1e-5, 1e-6)}
    for k, (what, got) in enumerate((("xdd q", gs[:, :n]), ("xdd v", gs[:, n:]), ("xdd a", ga), ("J q", gj[:, :n]))):
        scatter = float(tc.err(fd[1e-5][k], fd[1e-6][k]).max())
        e = tc.err(got, fd[1e-6][k])
        print(what, "device against the 1e-6 differences:", float(e.max()), "reference differences, 1e-5 against 1e-6:", scatter)
        assert (e <= 100.0 * scatter).all(), (what, int(e.argmax()), float(e.max()), 100.0 * scatter)


def test_solve_ik_and_its_reverse_pass(rig):
    """the first 65 poses of the rig's pool whose solve (20 steps from zero, the host build's) ends at a pose with cond(J_F) <= 1e3: the
    condition of ik_grad_cases' tolerance rule, met by the choice of inputs; gc.reference asserts it again at the device's own poses"""
    import ik_cases as ic
    import ik_grad_cases as gc
    import ik_grad_numpy as ign
    import nimblephysics_amd as na
    from kin_numpy import mapping_rows
    n, ow, md, entries, pool = rig["n"], rig["ow"], rig["md"], rig["entries"], rig["pool"]
    h = gc.HostIKGrad(ic.load_ik_shim(), gc.load_grad_shim(), md, entries)
    targets = np.stack([mapping_rows(ow, md, s[:n], entries)[0] for s in pool])
    hq = h.solve(targets, max_step_count=20)[0]
    gq = np.random.default_rng(32).normal(0, 1, hq.shape)
    lo, hi = gc.limits(md)
    cond = ign.vjp_batch(h.evaluate(hq, targets)[1], gq, hq, lo, hi, 1e-9)[3]
    pick = np.flatnonzero(cond <= gc.COND_MAX)[:B]
    assert len(pick) == B, (len(pool), int((cond <= gc.COND_MAX).sum()))
    targets, gq = targets[pick], gq[pick]
    maps = {id(w): _mapping(w, entries) for w in rig["worlds"]}

    def call(w):
        q, loss, steps = na.solve_ik(w, maps[id(w)], _t(targets), None, na.IKConfig(max_step_count=20))
        gt, free = na.solve_ik_vjp(w, maps[id(w)], q, _t(gq))
        return q, steps, gt, free
    q, steps, gt, free = _on_every_handle(rig["worlds"], call)
    assert float(np.abs(q - hq[pick]).max()) <= 1e-9
    want, d, cnt, worst = gc.reference(h, md, q, gq, 1e-9)
    err = float(np.abs(gt - want).max())
    print(f"solve_ik_vjp: |F| in [{cnt.min()}, {cnt.max()}], worst cond(J_F) {worst:.1f}, NumPy forms disagree by {d:.3e}, device off by {err:.3e}")
    assert np.array_equal(free, cnt) and np.isfinite(gt).all() and err <= 10.0 * d


def test_inertia_patches_reach_the_base_of_every_handle(rig):
    """nbl_set_body_inertia writes into the instantiation's handle; the mass matrix call reads the base of the same handle."""
    import nimblephysics_amd as na
    from oracle import OracleWorld
    md, S, n, ball = rig["md"], rig["S"], rig["n"], rig["ball"]
    worlds = _worlds(md)
    before = na.mass_matrix(worlds[0], _t(S))
    mass, com, ine = 2.5 * md.bodies[ball].mass, np.asarray([0.03, -0.02, 0.05]), np.asarray([0.09, 0.07, 0.08, 0.01, -0.005, 0.002])
    for w in worlds:
        assert w._L.nbl_set_body_inertia(w._h, ball, C.c_double(mass), com.ctypes.data_as(C.c_void_p), ine.ctypes.data_as(C.c_void_p)) == 0
    M, = _on_every_handle(worlds, lambda w: (na.mass_matrix(w, _t(S)),))
    assert np.abs(M - before.cpu().numpy()).max() > 1e-3
    md2 = copy.deepcopy(md)
    md2.bodies[ball].mass, md2.bodies[ball].com, md2.bodies[ball].inertia = float(mass), tuple(com), tuple(ine)
    ow2 = OracleWorld(md2)
    for b in range(B):
        assert _rel(M[b], ow2.mass_matrix(S[b, :n])) <= TOL, b


def test_registered_inertia_parameters_reach_the_base_of_every_handle(rig):
    import nimblephysics_amd as na
    from nimblephysics_amd.mass import WrtMassBodyNodeEntryType as T
    md, S, A, g, ball = rig["md"], rig["S"], rig["A"], rig["g"], rig["ball"]
    worlds = _worlds(md)
    for w in worlds:
        w.tuneMass(ball, T.INERTIA_MASS)
        w.tuneMass(0, T.INERTIA_MASS)
        assert w._L.nbl_num_inertia_params(w._h) == 2
    gm, = _on_every_handle(worlds, lambda w: (na.inverse_dynamics_mass_gradient(w, _t(S), _t(A), _t(g)),))
    assert gm.shape == (B, 2) and np.abs(gm).min(0).max() > 0


def test_a_map_or_set_of_another_instantiation_is_refused(rig):
    from nimblephysics_amd.centroidal import _body_set, _workspace
    w0, w1, S, n = rig["worlds"][0], rig["worlds"][1], rig["S"], rig["n"]
    L = w0._L
    p = lambda t: C.c_void_p(t.data_ptr())
    s = w0.to_soa(_t(S))
    pos = torch.empty((9, B), dtype=torch.float64, device=DEV)
    m0 = _mapping(w0, rig["entries"])
    km0 = m0._device_map(w0)
    assert L.nbl_kinematics_forward(w1._h, km0, B, p(s), p(pos), None, None) == -1
    assert b"the kinematics map was made for another model" in L.nbl_last_error()
    assert L.nbl_kinematics_forward(w0._h, km0, B, p(s), p(pos), None, None) == 0
    o3 = torch.empty((3, B), dtype=torch.float64, device=DEV)
    bs0, ws = _body_set(w0).ptr, _workspace(w1, B)
    N = None
    assert L.nbl_centroidal_forward(w1._h, bs0, B, p(s), N, 0, p(o3), N, N, N, N, N, N, p(ws), ws.numel(), None) == -1
    assert b"the body set was made for another model" in L.nbl_last_error()
    assert L.nbl_centroidal_forward(w0._h, bs0, B, p(s), N, 0, p(o3), N, N, N, N, N, N, p(ws), ws.numel(), None) == 0
    J = torch.empty((9 * n, B), dtype=torch.float64, device=DEV)
    assert L.nbl_task_jacobian(w1._h, km0, B, 9, n, p(s), p(J), None) == -1
    assert L.nbl_last_error() == b"the kinematics map was made for another model"
    assert L.nbl_task_jacobian(w0._h, km0, B, 9, n, p(s), p(J), None) == 0
    need = L.nbl_ik_grad_workspace_bytes(w0._h, km0, B)
    iws = torch.empty(need, dtype=torch.uint8, device=DEV)
    qz, gt = torch.zeros((n, B), dtype=torch.float64, device=DEV), torch.empty((9, B), dtype=torch.float64, device=DEV)
    assert L.nbl_ik_solve_vjp(w1._h, km0, B, p(qz), p(qz), 1e-9, p(gt), 0, None, p(iws), need, None) == -1
    assert L.nbl_last_error() == b"the kinematics map was made for another model"
    assert L.nbl_ik_solve_vjp(w0._h, km0, B, p(qz), p(qz), 1e-9, p(gt), 0, None, p(iws), need, None) == 0
    torch.cuda.synchronize()


def test_a_centroidal_launch_is_timed_on_a_handle_of_the_general_build(rig):
    from nimblephysics_amd.centroidal import _body_set, centroidal_soa
    w = _worlds(rig["md"])[2]
    w.set_timing(True)
    centroidal_soa(w, _body_set(w), w.to_soa(_t(rig["S"])), w.to_soa(_t(rig["A"])))
    torch.cuda.synchronize()
    k = w.get_timing()["kernels"]
    assert k["k_centroidal"]["count"] == 1 and k["k_centroidal"]["ms_sum"] > 0 and "k_centroidal_vjp" not in k
