"""Gyroscope, accelerometer and magnetometer readings on the device (csrc/sensors.hip through nimblephysics_amd/sensors.py): every reading
and every gradient against tests/sens_numpy.py at the bounds of tests/test_sensors_host.py (readings and closed-form blocks 1e-10 of
max(1, |ref|); the other gradients 100 x the disagreement of the reference's own central differences at 1e-5 and 1e-6, floored at 1e-8), the
host build of the same header (1e-13 relative, not bit for bit: fused multiply-adds and sincos differ), torch.autograd.gradcheck, the
reference page's linearity claims, cross-checks against com_acceleration and map_to_vel, free fall through forward_dynamics, dense
Jacobians, rollout shapes and bit-reproducibility, the World getters, immobile skeletons, deferred join, CPU tensors, argument errors.
Batches B in {1, 63, 65, 130}: the lane tails around a wavefront and a block.  The sensor lists are test_sensors_host.sensor_list's."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-10
NAMES = ("gyro", "acc", "mag")


def _states(md, B, seed):
    """[B, 2n], [B, n], [B, 3]: test_gpu_dynamics._states and a field N(0, 1)"""
    from test_gpu_dynamics import _states as draw
    S, A, _ = draw(md, B, seed)
    return S, A, np.random.default_rng(seed + 1000).normal(0, 1.0, (B, 3))


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


def _model(name):
    import nimblephysics_amd as na
    from test_ball_joint import ball_model
    from test_screw_joint import screw_arm
    return {"screw_arm": lambda: screw_arm(2, True), "screw_root": lambda: screw_arm(2, False),
            "cartpole": na.cartpole, "ball_arm": lambda: ball_model(2, True), "atlas20_ground": lambda: na.atlas("atlas20", ground=True),
            "atlas33": lambda: na.atlas("atlas33")}[name]()


def _t(x, grad=False):
    return torch.tensor(x, device=DEV, requires_grad=grad)


def _rot(r):
    """exp of the rotation vectors r [..., 3] (numpy)"""
    th = np.linalg.norm(r, axis=-1)[..., None, None]
    K = np.zeros(r.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -r[..., 2], r[..., 1], r[..., 2], -r[..., 0], -r[..., 1], r[..., 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        a, b = np.where(th > 1e-9, np.sin(th) / th, 1.0), np.where(th > 1e-9, (1 - np.cos(th)) / th ** 2, 0.5)
    return np.eye(3) + a * K + b * K @ K


_REF = {}


def _reference(name, md, sensors, S, A, F, cots, fd_worlds):
    """sens_numpy on every world (readings, closed-form Jacobians) and its central differences on `fd_worlds`; computed once per model"""
    import sens_numpy
    from oracle import OracleWorld
    if name in _REF:
        return _REF[name]
    ow, n = OracleWorld(md), md.num_dofs
    out = {"fwd": [], "cf": [], "fd": {}}
    for b in range(S.shape[0]):
        q, v, a, m = S[b, :n], S[b, n:], A[b], F[b]
        out["fwd"].append(sens_numpy.readings(ow, md, sensors, q, v, a, m))
        out["cf"].append(sens_numpy.closed_form_jacobians(ow, md, sensors, q))
        if b in fd_worlds:
            cot = {nm: c[b] for nm, c in zip(NAMES, cots)}
            out["fd"][b] = (sens_numpy.fd_vjp(ow, md, sensors, q, v, a, m, cot, 1e-5), sens_numpy.fd_vjp(ow, md, sensors, q, v, a, m, cot, 1e-6))
    _REF[name] = out
    return out


@pytest.mark.parametrize("B", [1, 63, 65, 130])
@pytest.mark.parametrize("name", ["cartpole", "ball_arm", "atlas20_ground", "atlas33", "screw_arm", "screw_root"])
def test_device_equals_sens_numpy_the_host_build_and_its_own_dense_jacobians(name, B):
    """Every world is checked.  The states of the smaller batches are the first worlds of the largest one, so the reference is computed
    once per model.  Readings, closed-form blocks and the comparison with the host build cover EVERY world; the finite-difference
    reference covers worlds 0, 62, 64 and 129 - the first lane, the first lane of the second block and the last world of every batch."""
    import nimblephysics_amd as na
    from nimblephysics_amd.sensors import _sensor_set, sensors_soa, sensors_vjp_soa
    from test_sensors_host import ShimSensors, as_numpy_sensors, load_shim, sensor_list
    md = _model(name)
    n = md.num_dofs
    sensors = sensor_list(md)
    P = 3 * len(sensors)
    S, A, F = _states(md, 130, 71)
    rng = np.random.default_rng(72)
    cots = [rng.normal(0, 1.0, (130, P)) for _ in NAMES]
    ref = _reference(name, md, as_numpy_sensors(sensors), S, A, F, cots, (0, 62, 64, 129))
    S, A, F, cots = S[:B], A[:B], F[:B], [c[:B] for c in cots]
    w = na.World(md, device=DEV)
    out = na.imu_readings(w, sensors, _t(S), _t(A), _t(F))
    assert all(o.shape == (B, P) for o in out)
    assert torch.equal(out.gyro, na.gyro_readings(w, sensors, _t(S))) and torch.equal(out.acc, na.accelerometer_readings(w, sensors, _t(S), _t(A)))
    assert torch.equal(out.mag, na.magnetometer_readings(w, sensors, _t(S), _t(F)))
    grads = {}
    for k, nm in enumerate(NAMES):
        st, at, ft = _t(S, True), _t(A, True), _t(F, True)
        o = na.imu_readings(w, sensors, st, at, ft)[k]
        o.backward(_t(cots[k]))
        z = lambda x, like: (x.grad if x.grad is not None else torch.zeros_like(like)).cpu().numpy()
        grads[nm] = np.concatenate([z(st, st), z(at, at), z(ft, ft)], 1)
    # dense Jacobians: one launch over 3 S x B worlds each; the zero blocks without a launch
    Jgv = na.gyro_jacobian(w, sensors, _t(S), "velocity")
    Jaa = na.accelerometer_jacobian(w, sensors, _t(S), _t(A), "acceleration")
    Jmf = na.magnetometer_jacobian(w, sensors, _t(S), _t(F), "field")
    dense = {("gyro", 0): na.gyro_jacobian(w, sensors, _t(S), "position"), ("gyro", 1): Jgv,
             ("acc", 0): na.accelerometer_jacobian(w, sensors, _t(S), _t(A), "position"),
             ("acc", 1): na.accelerometer_jacobian(w, sensors, _t(S), _t(A), "velocity"), ("acc", 2): Jaa,
             ("mag", 0): na.magnetometer_jacobian(w, sensors, _t(S), _t(F), "position"), ("mag", 3): Jmf}
    assert Jgv.shape == (B, P, n) and Jmf.shape == (B, P, 3)
    for J in (na.gyro_jacobian(w, sensors, _t(S), "acceleration"), na.magnetometer_jacobian(w, sensors, _t(S), _t(F), "velocity"),
              na.magnetometer_jacobian(w, sensors, _t(S), _t(F), "acceleration")):
        assert J.shape == (B, P, n) and not J.any()
    dev = {nm: getattr(out, nm).cpu().numpy() for nm in NAMES}
    worst = {}
    for b in range(B):
        r, cf = ref["fwd"][b], ref["cf"][b]
        e = {nm: _rel(dev[nm][b], r[nm]) for nm in NAMES}
        e["gyro_v"], e["acc_a"], e["mag_m"] = _rel(Jgv[b].cpu().numpy(), cf["gyro_v"]), _rel(Jaa[b].cpu().numpy(), cf["acc_a"]), _rel(Jmf[b].cpu().numpy(), cf["mag_m"])
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
    # the dense Jacobians equal stacked per-row autograd on worlds 0 and B - 1 (a world's bits do not depend on the batch)
    pick = sorted({0, B - 1})
    for k, nm in enumerate(NAMES):
        st, at, ft = _t(S[pick], True), _t(A[pick], True), _t(F[pick], True)
        o = na.imu_readings(w, sensors, st, at, ft)[k]
        rows = []
        for p in range(P):
            g = torch.autograd.grad(o[:, p].sum(), [st, at, ft], retain_graph=True, allow_unused=True)
            rows.append(torch.cat([x if x is not None else torch.zeros_like(y) for x, y in zip(g, (st, at, ft))], 1))
        rows = torch.stack(rows, 1)                                    # [2, P, 3 n + 3]
        for (nm2, block), J in dense.items():
            if nm2 == nm:
                cols = slice(3 * n, 3 * n + 3) if block == 3 else slice(block * n, (block + 1) * n)
                assert torch.equal(J[pick], rows[:, :, cols]), (name, nm, block)
    # the host build of the same header
    host = ShimSensors(load_shim(), md, sensors)
    houts = host.forward(S.T, A.T, F.T)
    hg = host.vjp(S.T, A.T, F.T, [c.T for c in cots])
    s, a, f = w.to_soa(_t(S)), w.to_soa(_t(A)), w.to_soa(_t(F))
    sset = _sensor_set(w, sensors)
    douts = sensors_soa(w, sset, s, a, f)
    dg = sensors_vjp_soa(w, sset, s, a, f, [_t(np.ascontiguousarray(c.T)) for c in cots])
    pairs = [(nm, o.cpu().numpy(), h) for nm, o, h in zip(NAMES, douts, houts)] + \
            [(nm, o.cpu().numpy(), h) for nm, o, h in zip(("grad_state", "grad_accel", "grad_field"), dg, hg)]
    vs_host = {nm: _rel(x, h) for nm, x, h in pairs}
    print(name, B, "worst vs sens_numpy:", worst, "| device vs host build:", vs_host)
    assert max(vs_host.values()) <= 1e-13, vs_host
    # two runs give the same bits; a rollout-shaped state is the same bits as its slices; world b of the batch is the same bits alone
    again = na.imu_readings(w, sensors, _t(S), _t(A), _t(F))
    assert all(torch.equal(x, y) for x, y in zip(out, again))
    assert all(torch.equal(x, y) for x, y in zip(dg, sensors_vjp_soa(w, sset, s, a, f, [_t(np.ascontiguousarray(c.T)) for c in cots])))
    T = 3
    Sr, Ar, Fr = (np.stack([np.roll(x, t, axis=0) for t in range(T + 1)]) for x in (S, A, F))
    roll = na.imu_readings(w, sensors, _t(Sr), _t(Ar), _t(Fr))
    assert roll.gyro.shape == (T + 1, B, P)
    for t in range(T + 1):
        sep = na.imu_readings(w, sensors, _t(Sr[t]), _t(Ar[t]), _t(Fr[t]))
        assert all(torch.equal(x[t], y) for x, y in zip(roll, sep)), t
    if B == 130:
        for b in (0, 64, 129):
            one = na.imu_readings(w, sensors, _t(S[b:b + 1]), _t(A[b:b + 1]), _t(F[b:b + 1]))
            assert all(torch.equal(x[b:b + 1], y) for x, y in zip(out, one)), b
            assert torch.equal(Jaa[b:b + 1], na.accelerometer_jacobian(w, sensors, _t(S[b:b + 1]), _t(A[b:b + 1]), "acceleration"))


def test_gradcheck():
    import nimblephysics_amd as na
    from test_sensors_host import sensor_list
    md = _model("cartpole")
    w = na.World(md, device=DEV)
    sensors = sensor_list(md)
    S, A, F = _states(md, 2, 73)
    st, at, ft = _t(S, True), _t(A, True), _t(F, True)
    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda s, a, f: tuple(na.imu_readings(w, sensors, s, a, f)), (st, at, ft), **kw)
    f1 = _t(F[0], True)                                                # one field for the batch: its gradient is summed over the worlds
    assert torch.autograd.gradcheck(lambda f: na.magnetometer_readings(w, sensors, st.detach(), f), (f1,), **kw)


@pytest.mark.parametrize("name", ["cartpole", "atlas20_ground"])
def test_at_rest_every_accelerometer_reads_gravity_and_the_readings_are_linear_where_the_reference_says_so(name):
    """www/docs/accs-and-gyros.rst: the gyro reading is linear in v, the accelerometer reading linear in the accelerations, and
    d acc / da = d (sensor-frame velocity of the sensor's origin) / dv."""
    import nimblephysics_amd as na
    from test_sensors_host import sensor_list
    md = _model(name)
    n, B = md.num_dofs, 65
    sensors = sensor_list(md)
    w = na.World(md, device=DEV)
    S, A, _ = _states(md, B, 74)
    rest = S.copy(); rest[:, n:] = 0.0
    acc = na.accelerometer_readings(w, sensors, _t(rest), _t(np.zeros_like(A))).cpu().numpy().reshape(B, -1, 3)
    g = np.linalg.norm(np.asarray(md.gravity, dtype=np.float64))
    assert g > 1 and np.abs(np.linalg.norm(acc, axis=2) - g).max() <= 1e-12 * g
    S2 = S.copy(); S2[:, n:] = np.random.default_rng(75).normal(0, 3.0, (B, n))
    A2 = np.random.default_rng(76).normal(0, 5.0, (B, n))
    Jg, Jg2 = na.gyro_jacobian(w, sensors, _t(S), "velocity"), na.gyro_jacobian(w, sensors, _t(S2), "velocity")
    Ja, Ja2 = na.accelerometer_jacobian(w, sensors, _t(S), _t(A), "acceleration"), na.accelerometer_jacobian(w, sensors, _t(S2), _t(A2), "acceleration")
    assert _rel(Jg2.cpu().numpy(), Jg.cpu().numpy()) <= 1e-13 and _rel(Ja2.cpu().numpy(), Ja.cpu().numpy()) <= 1e-13
    # d acc / da rebuilt from the IKMapping's velocity Jacobian of the sensors' bodies: rows [w; v] of the body origin, world coordinates
    m = na.IKMapping(w)
    on_bodies = [(k, i, T) for k, (i, T) in enumerate(sensors) if i >= 0]
    for _, i, _ in on_bodies:
        m.addSpatialBodyNode(int(i))
    w.setState(_t(S))
    Jv = m.getRealVelToMappedVelJac(w).cpu().numpy().reshape(B, len(on_bodies), 6, n)
    pos = na.map_to_pos(w, m, _t(S)).cpu().numpy().reshape(B, len(on_bodies), 6)
    R = _rot(pos[:, :, :3])
    want = np.zeros((B, 3 * len(sensors), n))
    for e, (k, i, T) in enumerate(on_bodies):
        T = np.eye(4) if T is None else T
        arm = R[:, e] @ T[:3, 3]                                        # R p_bs, world
        Jx = Jv[:, e, 3:] - np.cross(arm[:, None, :], Jv[:, e, :3].transpose(0, 2, 1)).transpose(0, 2, 1)   # v + w x arm
        want[:, 3 * k:3 * k + 3] = np.einsum("ji,bkj,bkn->bin", T[:3, :3], R[:, e], Jx)
    e = _rel(Ja.cpu().numpy(), want)
    print(name, "d acc / da against the IKMapping's velocity Jacobian:", e)
    assert e <= TOL


def test_cross_checks_against_com_acceleration_and_map_to_vel():
    import nimblephysics_amd as na
    md = _model("atlas33")
    n, B = md.num_dofs, 65
    w = na.World(md, device=DEV)
    S, A, _ = _states(md, B, 77)
    targets, _ = md.weld_targets()
    alone = [i for i, b in enumerate(md.bodies) if targets[i] >= 0 and list(targets).count(targets[i]) == 1]
    picks = [alone[0], alone[len(alone) // 2], alone[-1]]
    m = na.IKMapping(w)
    for i in picks:
        m.addSpatialBodyNode(int(i))
    R = _rot(na.map_to_pos(w, m, _t(S)).cpu().numpy().reshape(B, len(picks), 6)[:, :, :3])
    vel = na.map_to_vel(w, m, _t(S)).cpu().numpy().reshape(B, len(picks), 6)
    at_com = []
    for i in picks:
        T = np.eye(4); T[:3, 3] = np.asarray(md.bodies[i].com, dtype=np.float64)
        at_com.append((int(i), T))
    acc = na.accelerometer_readings(w, at_com, _t(S), _t(A)).cpu().numpy().reshape(B, len(picks), 3)
    gyro = na.gyro_readings(w, [(int(i), None) for i in picks], _t(S)).cpu().numpy().reshape(B, len(picks), 3)
    g = np.asarray(md.gravity, dtype=np.float64)
    for e, i in enumerate(picks):
        want = na.com_acceleration(w, _t(S), _t(A), bodies=[int(i)]).cpu().numpy()
        got = np.einsum("bij,bj->bi", R[:, e], acc[:, e]) + g
        ea = _rel(got, want)
        eg = _rel(gyro[:, e], np.einsum("bji,bj->bi", R[:, e], vel[:, e, :3]))
        print(md.bodies[i].name, "R acc + g against com_acceleration:", ea, "| gyro against R^T map_to_vel:", eg)
        assert ea <= TOL and eg <= TOL


def test_a_body_in_free_fall_reads_no_acceleration_at_its_centre_of_mass_whatever_its_spin():
    import nimblephysics_amd as na
    com = (0.03, -0.05, 0.02)
    body = na.BodySpec("rock", -1, "free", "rock_joint", mass=1.7, com=com, inertia=(0.05, 0.08, 0.06, 0.004, -0.003, 0.002))
    md = na.ModelDescription("free_fall", [body], [], gravity=(0.4, -9.81, 0.3), dt=1e-3, max_contacts=0)
    B = 65
    w = na.World(md, device=DEV)
    S, _, _ = _states(md, B, 78)
    S[:, 6:9] *= 5.0                                                   # a fast spin
    a = na.forward_dynamics(w, _t(S), _t(np.zeros((B, 6))))
    T = np.eye(4); T[:3, 3] = com
    acc = na.accelerometer_readings(w, [("rock", T)], _t(S), a).cpu().numpy()
    off = na.accelerometer_readings(w, [("rock", None)], _t(S), a).cpu().numpy()
    g = np.linalg.norm(md.gravity)
    print("free fall: |acc| / |g| at the centre of mass", np.abs(acc).max() / g, "| at the body's origin", np.abs(off).max() / g)
    assert np.abs(acc).max() <= 1e-10 * g and np.abs(off).max() > 1e-3 * g


def test_world_getters_immobile_skeletons_deferred_join_and_cpu_tensors(tmp_path):
    import nimblephysics_amd as na
    from nimblephysics_amd import neural
    from test_ref_layout import load
    from test_sensors_host import sensor_list
    md = _model("atlas20_ground")
    n, B = md.num_dofs, 6
    sensors = sensor_list(md)
    w = na.World(md, device=DEV)
    S, A, F = _states(md, B, 79)
    want = na.imu_readings(w, sensors, _t(S), _t(A), _t(F))
    w.setState(_t(S))
    assert torch.equal(w.getGyroReadings(sensors), want.gyro) and torch.equal(w.getAccelerometerReadings(sensors, _t(A)), want.acc)
    assert torch.equal(w.getMagnetometerReadings(sensors, _t(F)), want.mag)
    assert torch.equal(w.getGyroReadingsJacobianWrt(sensors, neural.WRT_POSITION), na.gyro_jacobian(w, sensors, _t(S), "position"))
    assert torch.equal(w.getAccelerometerReadingsJacobianWrt(sensors, _t(A), neural.WRT_VELOCITY), na.accelerometer_jacobian(w, sensors, _t(S), _t(A), "velocity"))
    assert torch.equal(w.getMagnetometerReadingsJacobianWrt(sensors, _t(F), neural.WRT_POSITION), na.magnetometer_jacobian(w, sensors, _t(S), _t(F), "position"))
    assert torch.equal(w.getMagnetometerReadingsJacobianWrtMagneticField(sensors, _t(F)), na.magnetometer_jacobian(w, sensors, _t(S), _t(F), "field"))
    assert not w.getGyroReadingsJacobianWrt(sensors, neural.WRT_ACCELERATION).any()
    w.setState(_t(S[0]))                                                # one world given as a 1-D vector
    assert torch.equal(w.getGyroReadings(sensors), want.gyro[0]) and w.getMagnetometerReadingsJacobianWrtMagneticField(sensors, _t(F[0])).shape == (3 * len(sensors), 3)
    # names resolve like indices; one field for the whole batch
    named = [(md.bodies[i].name if i >= 0 else -1, T) for i, T in sensors]
    assert torch.equal(na.gyro_readings(w, named, _t(S)), want.gyro)
    assert torch.equal(na.magnetometer_readings(w, sensors, _t(S), _t(F[0])), na.magnetometer_readings(w, sensors, _t(S), _t(np.tile(F[0], (B, 1)))))
    # CPU float64 tensors in and out, [2n] and [B, 2n]; gradients come back on the CPU
    x, y, z = torch.tensor(S, requires_grad=True), torch.tensor(A, requires_grad=True), torch.tensor(F, requires_grad=True)
    cpu = na.imu_readings(w, sensors, x, y, z)
    assert all(o.device.type == "cpu" and torch.equal(o, f.cpu()) for o, f in zip(cpu, want))
    (cpu.gyro.sum() + cpu.acc.sum() + cpu.mag.sum()).backward()
    assert all(t.grad.device.type == "cpu" and t.grad.shape == t.shape and float(t.grad.abs().max()) > 0 for t in (x, y, z))
    one = na.gyro_readings(w, sensors, torch.tensor(S[0]))
    assert one.shape == (3 * len(sensors),) and one.device.type == "cpu" and torch.equal(one, want.gyro[0].cpu())
    assert na.imu_readings(w, sensors, _t(S), _t(A)).mag is None
    # deferred join: the state comes straight out of a step whose slices are still in flight
    Bd = 4096
    Sd, Ad, _ = _states(md, Bd, 80)
    Sd[:, 0] = -np.pi / 2; Sd[:, 4] += 1.0
    ref, dw = na.World(md, device=DEV), na.World(md, device=DEV)
    s_soa = ref.to_soa(_t(Sd)); a_soa = ref.to_soa(torch.zeros((Bd, ref.k), dtype=torch.float64, device=DEV))
    want_next, _, _ = ref.step_soa(s_soa, a_soa, want_saved=True)
    want_d = na.imu_readings(ref, sensors, want_next.t(), _t(Ad))
    dw.set_deferred_join(True)
    assert dw.slices_for(Bd) > 1
    buf = {"nxt": torch.empty_like(s_soa), "saved": torch.empty(dw.saved_bytes(Bd), dtype=torch.uint8, device=DEV),
           "status": torch.empty(Bd, dtype=torch.int32, device=DEV), "cache": torch.empty((dw.m, Bd), dtype=torch.float64, device=DEV)}
    dw.step_into(s_soa, a_soa, buf["nxt"], buf["saved"], buf["status"], None, buf["cache"])
    got = na.imu_readings(dw, sensors, buf["nxt"].t(), _t(Ad))
    assert torch.equal(got.gyro, want_d.gyro) and torch.equal(got.acc, want_d.acc)
    dw.join()
    torch.cuda.synchronize()
    # a world with an immobile skeleton: the reference's layout in, n_ref columns out, the frozen ones zero
    mi = load(tmp_path)
    wi = na.World(mi, device=DEV)
    assert wi.ref_layout is not None and wi.getStateSize() == 24 and wi.n == 6
    mobile = [b.name for b in mi.bodies if b.skeleton not in set(mi.immobile_skeletons or ())]
    si = [(mobile[0], None), (mobile[0], sensors[1][1])]
    rng = np.random.default_rng(1)
    full = np.zeros((8, 24)); full[:, 6:12] = rng.normal(0, 0.3, (8, 6)); full[:, 18:] = rng.normal(0, 1, (8, 6))
    afull = np.zeros((8, 12)); afull[:, 6:] = rng.normal(0, 1, (8, 6))
    xs, ys = _t(full, True), _t(afull, True)
    r = na.imu_readings(wi, si, xs, ys)
    w2 = na.World(mi, device=DEV); w2.ref_layout = None                  # the device's own (shorter) layout
    short = na.imu_readings(w2, si, _t(np.concatenate([full[:, 6:12], full[:, 18:]], 1)), _t(afull[:, 6:]))
    assert torch.equal(r.gyro.detach(), short.gyro) and torch.equal(r.acc.detach(), short.acc)
    (r.gyro.sum() + r.acc.sum()).backward()
    assert xs.grad.shape == (8, 24) and not xs.grad[:, :6].any() and not xs.grad[:, 12:18].any() and xs.grad[:, 18:].abs().sum() > 0
    assert ys.grad.shape == (8, 12) and not ys.grad[:, :6].any() and ys.grad[:, 6:].abs().sum() > 0
    wi.setState(_t(full))
    J = wi.getAccelerometerReadingsJacobianWrt(si, _t(afull), neural.WRT_ACCELERATION)
    assert J.shape == (8, 6, 12) and not J[:, :, :6].any() and J[:, :, 6:].abs().sum() > 0
    assert torch.equal(J, na.accelerometer_jacobian(wi, si, _t(full), _t(afull), "acceleration"))


def test_argument_errors():
    import nimblephysics_amd as na
    from nimblephysics_amd._lib import check
    from nimblephysics_amd.sensors import _sensor_set, _workspace
    md = _model("atlas20_ground")
    n = md.num_dofs
    w = na.World(md, device=DEV)
    S, A, F = _states(md, 8, 81)
    st, at, ft = _t(S), _t(A), _t(F)
    rng = np.random.default_rng(6)
    from test_sensors_host import rigid
    many = [(int(rng.integers(0, 5)), rigid(rng, 0.1)) for _ in range(65)]
    with pytest.raises(ValueError, match="at most 64"):
        na.gyro_readings(w, many, st)
    assert na.gyro_readings(w, many[:64], st).shape == (8, 192)
    with pytest.raises(na.NimbleAmdError, match="accelerations"):
        na.imu_readings(w, many[:2], st, None)
    with pytest.raises(ValueError):
        na.accelerometer_readings(w, many[:2], st, at[:5])
    with pytest.raises(ValueError):
        na.gyro_readings(w, many[:2], st[:, :-1])
    with pytest.raises(ValueError, match="field"):
        na.magnetometer_readings(w, many[:2], st, ft[:, :2])
    with pytest.raises(ValueError, match="field"):
        na.magnetometer_readings(w, many[:2], st, ft[:5])
    with pytest.raises(ValueError, match="wrt"):
        na.gyro_jacobian(w, many[:2], st, "scales")
    with pytest.raises(ValueError, match="wrt"):
        na.gyro_jacobian(w, many[:2], st, "field")
    with pytest.raises(ValueError):
        na.gyro_readings(w, [("no_such_body", None)], st)
    with pytest.raises(ValueError):
        na.gyro_readings(w, [(0, np.eye(3))], st)
    with pytest.raises(ValueError):
        na.gyro_readings(w, [], st)
    # the C ABI's own refusals
    L, h = w._L, w._h
    p = lambda t: C.c_void_p(t.data_ptr())
    s8, a8, f8 = w.to_soa(st), w.to_soa(at), w.to_soa(ft)
    sset = _sensor_set(w, many[:2])
    o = torch.empty((6, 8), dtype=torch.float64, device=DEV)
    gs = torch.empty((2 * n, 8), dtype=torch.float64, device=DEV)
    ws, k = _workspace(w, 8), sset.ptr
    need = L.nbl_sensors_workspace_bytes(h, 8)
    assert need == 8 * L.nbl_sensors_workspace_bytes(h, 1) == L.nbl_centroidal_workspace_bytes(h, 8) and L.nbl_sensors_workspace_bytes(None, 8) == 0
    m = na.IKMapping(w)
    m.addSpatialBodyNode(0); m.addLinearBodyNode(1)
    mixed = m._device_map(w)                                           # a kinematics map with an entry that is not NBL_KIN_SPATIAL
    other = na.World(_model("cartpole"), device=DEV)
    N = None
    for rc_want, call in ((-1, lambda: L.nbl_sensors_forward(None, k, 8, p(s8), N, N, p(o), N, N, p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_sensors_forward(h, None, 8, p(s8), N, N, p(o), N, N, p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_sensors_forward(other._h, k, 8, p(s8), N, N, p(o), N, N, p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_sensors_forward(h, mixed, 8, p(s8), N, N, p(o), N, N, p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_sensors_forward(h, k, 8, None, N, N, p(o), N, N, p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_sensors_forward(h, k, -1, p(s8), N, N, p(o), N, N, p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_sensors_forward(h, k, 8, p(s8), N, N, N, p(o), N, p(ws), ws.numel(), None)),           # acc without accel
                          (-1, lambda: L.nbl_sensors_forward(h, k, 8, p(s8), p(a8), N, N, N, p(o), p(ws), ws.numel(), None)),       # mag without field
                          (-1, lambda: L.nbl_sensors_forward(h, k, 8, p(s8), N, N, p(o), N, N, None, ws.numel(), None)),
                          (-4, lambda: L.nbl_sensors_forward(h, k, 8, p(s8), N, N, p(o), N, N, p(ws), need - 1, None)),
                          (-1, lambda: L.nbl_sensors_backward(h, k, 8, p(s8), N, N, N, p(o), N, p(gs), N, N, 0, p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_sensors_backward(h, k, 8, p(s8), N, N, N, N, p(o), p(gs), N, N, 0, p(ws), ws.numel(), None)),
                          (-1, lambda: L.nbl_sensors_backward(h, mixed, 8, p(s8), N, N, p(o), N, N, p(gs), N, N, 0, p(ws), ws.numel(), None)),
                          (-4, lambda: L.nbl_sensors_backward(h, k, 8, p(s8), p(a8), p(f8), p(o), N, N, p(gs), N, N, 0, p(ws), 8, None))):
        rc = call()
        assert rc == rc_want, (rc, rc_want)
        with pytest.raises(na.NimbleAmdError):
            check(rc, "sensors")
        assert L.nbl_last_error()
    assert L.nbl_sensors_forward(h, k, 0, None, N, N, N, N, N, None, 0, None) == 0                                                   # B = 0 is a no-op
    # accumulate adds onto what is there
    cot = _t(np.random.default_rng(7).normal(size=(6, 8)))
    g0 = torch.empty_like(gs)
    assert L.nbl_sensors_backward(h, k, 8, p(s8), p(a8), N, p(cot), p(cot), N, p(g0), N, N, 0, p(ws), ws.numel(), w._stream()) == 0
    g1 = torch.ones_like(gs)
    assert L.nbl_sensors_backward(h, k, 8, p(s8), p(a8), N, p(cot), p(cot), N, p(g1), N, N, 1, p(ws), ws.numel(), w._stream()) == 0
    torch.cuda.synchronize()
    assert float((g1 - (g0 + 1.0)).abs().max()) <= 1e-12 * max(1.0, float(g0.abs().max())) and float(g0.abs().max()) > 0
