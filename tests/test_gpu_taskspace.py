"""Task-space Jacobians, their time derivative and map_to_acc on the device (csrc/taskspace.hip through nimblephysics_amd/taskspace.py)
against tests/task_numpy.py on the three models of tests/task_cases.py, at the batch sizes 1, 63, 64, 65 and 130 (the lane tails around
a wavefront and a block) and as one rollout-shaped [3, 65] call.  Every world of every batch is checked; nothing is batch-averaged.

BOUNDS.  Forward quantities are closed-form fp64 on both sides: FORWARD_TOL = 2.5e-13 = 100 x the largest per-world deviation of the HOST
build of the same header from the numpy statement (2.4e-15, measured on these models and states by tests/test_taskspace_host.py), relative
to max(1, |ref|) - room for the device's summation order and fused multiply-adds, far inside the project's 1e-7 parity bound.
Reverse passes against central differences of the NUMPY statement at the step 1e-6: 100 x the largest disagreement of the reference's own
differences at the steps 1e-5 and 1e-6 on that model (measured: at most 4.4e-9, so the bounds lie between 7.4e-8 and 4.4e-7; the host
build sits within 4.1e-9 of the 1e-6 differences).  The inner-product identity of task_jacobian's reverse pass against differences of
the DEVICE's forward kernel along 8 random directions is held to 100 x the disagreement of the same directional differences of the
reference at 1e-5 and 1e-6.

MEASURED on an MI355X (printed by the tests): see DESIGN.md, "Task-space Jacobians and accelerations"."""
import ctypes as C

import numpy as np
import pytest
import torch

import task_cases as tc
import task_numpy as tn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FORWARD_TOL = 2.5e-13
CASES = tc.cases()
IDS = list(CASES)
BATCHES = [1, 63, 64, 65, 130]
_REF, _WORLDS = {}, {}


def _t(x, grad=False):
    return torch.tensor(x, device=DEV, requires_grad=grad)


def _np(x):
    return x.detach().cpu().numpy()


def _world(name):
    """(World, IKMapping) of a case, made once"""
    import nimblephysics_amd as na
    if name not in _WORLDS:
        md, entries = CASES[name]
        w = na.World(md, device=DEV)
        m = na.IKMapping(w)
        for kind, i in entries:
            (m.addSpatialBodyNode, m.addLinearBodyNode, m.addAngularBodyNode)[kind](i)
        _WORLDS[name] = (w, m)
    return _WORLDS[name]


def _reference(name):
    """the numpy statement on the 130 worlds of a case and its central differences at 1e-5 and 1e-6; computed once per model"""
    if name in _REF:
        return _REF[name]
    md, entries = CASES[name]
    m, ne = tn.Model(md), tc.numpy_entries(entries)
    q, v, a = tc.states(md, tc.B_MAX)
    rng = np.random.default_rng(tc.SEED + 11)
    R, n = tc.rows(entries), md.num_dofs
    cot, G = rng.normal(size=(tc.B_MAX, R)), rng.normal(size=(tc.B_MAX, R, n))
    J, Jd = tn.jacobians(m, ne, q, v)
    out = {"q": q, "v": v, "a": a, "cot": cot, "G": G, "J": J, "Jdot": Jd, "bias": tn.accel(m, ne, q, v), "xdd": tn.accel(m, ne, q, v, a),
           "W": tn.kinematics(m, q)[0], "fd": {}}
    for eps in (1e-5, 1e-6):
        x = tn.fd_accel_vjp(m, ne, q, v, a, cot, eps)
        c = tn.fd_accel_vjp(m, ne, q, v, None, cot, eps)
        out["fd"][eps] = {"xdd q": x[0], "xdd v": x[1], "xdd a": x[2], "bias q": c[0], "bias v": c[1], "J q": tn.fd_jacobian_vjp(m, ne, q, G, eps)}
    out["scatter"] = {k: float(tc.err(out["fd"][1e-5][k], out["fd"][1e-6][k]).max()) for k in out["fd"][1e-6]}
    _REF[name] = out
    return out


def _check(name, what, got, ref, bound):
    e = tc.err(got, ref)
    assert np.isfinite(got).all() and (e <= bound).all(), (name, what, "world", int(e.argmax()), float(e.max()), bound)
    return float(e.max())


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", IDS)
def test_forward_quantities_equal_the_numpy_statement_in_every_world(name, B):
    import nimblephysics_amd as na
    from nimblephysics_amd.taskspace import task_jacobian_soa
    md, entries = CASES[name]
    w, m = _world(name)
    r = _reference(name)
    q, v, a = r["q"][:B], r["v"][:B], r["a"][:B]
    S, A = _t(np.concatenate([q, v], 1)), _t(a)
    R, n = tc.rows(entries), md.num_dofs
    J, Jd = na.task_jacobian(w, m, S), na.task_jacobian_deriv(w, m, S)
    bias, xdd, vel = na.task_jacobian_dot_times_v(w, m, S), na.map_to_acc(w, m, S, A), na.map_to_vel(w, m, S)
    assert J.shape == (B, R, n) and Jd.shape == (B, R, n) and bias.shape == (B, R) and xdd.shape == (B, R) and not Jd.requires_grad
    worst = {k: _check(name, k, _np(x), r[k][:B], FORWARD_TOL) for k, x in (("J", J), ("Jdot", Jd), ("bias", bias), ("xdd", xdd))}
    worst["J v - map_to_vel"] = _check(name, "J v", _np(torch.einsum("brd,bd->br", J, S[:, n:])), _np(vel), FORWARD_TOL)
    worst["Jdot v - bias"] = _check(name, "Jdot v", _np(torch.einsum("brd,bd->br", Jd, S[:, n:])), _np(bias), FORWARD_TOL)
    print(name, B, "largest per-world deviations:", worst)
    # the kernels write every entry of their outputs: a buffer poisoned with NaN comes back without one, its structural zeros exact
    zero = tc.zero_mask(md, entries)
    assert zero.any() and not _np(J)[:, zero].any() and not _np(Jd)[:, zero].any()
    s_soa = w.to_soa(S)
    for deriv, want in ((False, J), (True, Jd)):
        buf = torch.full((R * n, B), float("nan"), dtype=torch.float64, device=DEV)
        fn = w._L.nbl_task_jacobian_deriv if deriv else w._L.nbl_task_jacobian
        assert fn(w._h, m._device_map(w), B, R, n, C.c_void_p(s_soa.data_ptr()), C.c_void_p(buf.data_ptr()), w._stream()) == 0
        assert torch.equal(buf, task_jacobian_soa(w, m, s_soa, deriv)) and torch.equal(w.from_soa(buf).reshape(B, R, n), want)
    # the World's getters on its current state; getRealVelToMappedVelJac is the existing route (one reverse-mode world per row)
    w.setState(S)
    old = m.getRealVelToMappedVelJac(w)
    assert torch.equal(m.getJacobian(w), J) and torch.equal(m.getJacobianDeriv(w), Jd) and torch.equal(m.getAccelerations(w, A), xdd)
    _check(name, "getRealVelToMappedVelJac", _np(J), _np(old), FORWARD_TOL)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", ["screw_chain", "free_ball"])
def test_an_accelerometer_at_the_body_origin_reads_the_linear_acceleration_minus_gravity(name, B):
    """merged code as the yardstick: R_body accelerometer_readings + g = the linear rows of map_to_acc on the same body"""
    import nimblephysics_amd as na
    md, entries = CASES[name]
    w, _ = _world(name)
    r = _reference(name)
    body = 0 if name == "screw_chain" else 1
    m = na.IKMapping(w)
    m.addLinearBodyNode(body)
    S, A = _t(np.concatenate([r["q"][:B], r["v"][:B]], 1)), _t(r["a"][:B])
    acc = _np(na.accelerometer_readings(w, [(body, None)], S, A))
    want = np.einsum("bij,bj->bi", r["W"][body][:B, :3, :3], acc) + np.asarray(md.gravity, dtype=np.float64)
    print(name, B, "map_to_acc against the accelerometer:", _check(name, "accelerometer", _np(na.map_to_acc(w, m, S, A)), want, FORWARD_TOL))


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", IDS)
def test_reverse_passes_equal_the_references_central_differences_in_every_world(name, B):
    import nimblephysics_amd as na
    md, entries = CASES[name]
    w, m = _world(name)
    r = _reference(name)
    n = md.num_dofs
    S0, A0, cot, G = np.concatenate([r["q"][:B], r["v"][:B]], 1), r["a"][:B], _t(r["cot"][:B]), _t(r["G"][:B])
    got = {}
    S, A = _t(S0, True), _t(A0, True)
    na.map_to_acc(w, m, S, A).backward(cot)
    got["xdd q"], got["xdd v"], got["xdd a"] = _np(S.grad[:, :n]), _np(S.grad[:, n:]), _np(A.grad)
    S = _t(S0, True)
    na.task_jacobian_dot_times_v(w, m, S).backward(cot)
    got["bias q"], got["bias v"] = _np(S.grad[:, :n]), _np(S.grad[:, n:])
    S = _t(S0, True)
    na.task_jacobian(w, m, S).backward(G)
    got["J q"] = _np(S.grad[:, :n])
    assert not S.grad[:, n:].any()
    worst = {k: _check(name, k, got[k], r["fd"][1e-6][k][:B], 100.0 * r["scatter"][k]) for k in got}
    print(name, B, "reference differences, 1e-5 against 1e-6:", r["scatter"])
    print(name, B, "device against the 1e-6 differences:", worst)


@pytest.mark.parametrize("name", IDS)
def test_the_reverse_pass_of_the_jacobian_meets_the_inner_product_identity_of_the_forward_kernel(name):
    """<g_q, d> = <G, J(q + eps d) - J(q - eps d)> / 2 eps on the device's own forward kernel, 8 random directions, B = 65"""
    import nimblephysics_amd as na
    md, entries = CASES[name]
    w, m = _world(name)
    r = _reference(name)
    B, n, eps = 65, md.num_dofs, 1e-6
    mm, ne = tn.Model(md), tc.numpy_entries(entries)
    q, G = r["q"][:B], r["G"][:B]
    S = _t(np.concatenate([q, 0 * q], 1), True)
    na.task_jacobian(w, m, S).backward(_t(G))
    gq = _np(S.grad[:, :n])
    rng = np.random.default_rng(tc.SEED + 13)
    worst = 0.0
    for _ in range(8):
        d = rng.normal(size=(B, n))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        dev = lambda e: _np(na.task_jacobian(w, m, _t(np.concatenate([q + e * d, 0 * q], 1))))
        ref = lambda e: tn.jacobians(mm, ne, q + e * d)[0]
        fd_dev = np.einsum("brd,brd->b", G, dev(eps) - dev(-eps)) / (2 * eps)
        fd_ref = {e: np.einsum("brd,brd->b", G, ref(e) - ref(-e)) / (2 * e) for e in (1e-5, 1e-6)}
        scatter = float((np.abs(fd_ref[1e-5] - fd_ref[1e-6]) / np.maximum(1.0, np.abs(fd_ref[1e-6]))).max())
        e = np.abs(np.einsum("bd,bd->b", gq, d) - fd_dev) / np.maximum(1.0, np.abs(fd_dev))
        assert (e <= 100.0 * scatter).all(), (name, int(e.argmax()), float(e.max()), 100.0 * scatter)
        worst = max(worst, float(e.max()))
    print(name, "inner-product identity, largest per-world deviation:", worst)


def _everything(na, w, m, S0, A0, cot, G):
    """every output and every gradient of the four functions"""
    n = w.n
    S, A = S0.clone().requires_grad_(True), A0.clone().requires_grad_(True)
    xdd = na.map_to_acc(w, m, S, A)
    xdd.backward(cot)
    S2 = S0.clone().requires_grad_(True)
    bias = na.task_jacobian_dot_times_v(w, m, S2)
    bias.backward(cot)
    S3 = S0.clone().requires_grad_(True)
    J = na.task_jacobian(w, m, S3)
    J.backward(G)
    return [xdd.detach(), S.grad, A.grad, bias.detach(), S2.grad, J.detach(), S3.grad, na.task_jacobian_deriv(w, m, S0)]


@pytest.mark.parametrize("name", IDS)
def test_a_rollout_shaped_call_a_deferred_join_handle_and_cpu_tensors_give_the_same_bits(name):
    import nimblephysics_amd as na
    md, entries = CASES[name]
    w, m = _world(name)
    r = _reference(name)
    T1, B, n, R = 3, 65, md.num_dofs, tc.rows(entries)
    pick = np.arange(T1 * B) % tc.B_MAX                                # 195 worlds out of the 130: the first 65 come twice
    shape = lambda x: _t(x[pick].reshape((T1, B) + x.shape[1:]))
    S, A, cot, G = shape(np.concatenate([r["q"], r["v"]], 1)), shape(r["a"]), shape(r["cot"]), shape(r["G"])
    whole = _everything(na, w, m, S, A, cot, G)
    assert whole[0].shape == (T1, B, R) and whole[5].shape == (T1, B, R, n) and whole[1].shape == (T1, B, 2 * n)
    for t in range(T1):                                               # the [3, 65] call equals three [65] calls byte for byte
        for x, y in zip(_everything(na, w, m, S[t], A[t], cot[t], G[t]), whole):
            assert torch.equal(x, y[t])
    dw = na.World(md, device=DEV)                                     # a deferred-join handle is joined first: the same bytes
    dw.set_deferred_join(True)
    for x, y in zip(_everything(na, dw, m, S[0], A[0], cot[0], G[0]), whole):
        assert torch.equal(x, y[0])
    dw.join()
    torch.cuda.synchronize()
    host = _everything(na, w, m, S[0].cpu(), A[0].cpu(), cot[0].cpu(), G[0].cpu())   # CPU float64 tensors in and out
    for x, y in zip(host, whole):
        assert x.device.type == "cpu" and torch.equal(x, y[0].cpu())


def test_a_wrong_row_count_or_dof_count_is_refused_with_badarg():
    from nimblephysics_amd import _abi
    w, m = _world("screw_chain")
    md, entries = CASES["screw_chain"]
    R, n, B = tc.rows(entries), md.num_dofs, 4
    S = w.to_soa(_t(np.concatenate(tc.states(md, B)[:2], 1)))
    nan = lambda rows: torch.full((rows, B), float("nan"), dtype=torch.float64, device=DEV)
    J, out, gs, A = nan(R * n), nan(R), nan(2 * n), w.to_soa(_t(tc.states(md, B)[2]))
    ws = torch.empty(max(w._L.nbl_task_workspace_bytes(w._h, B), 1), dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    km, L, st = m._device_map(w), w._L, w._stream()
    for rows, dofs in ((R + 1, n), (R - 1, n), (R, n + 1), (R, n - 1), (0, n), (R, 0)):
        assert L.nbl_task_jacobian(w._h, km, B, rows, dofs, p(S), p(J), st) == _abi.NBL_E_BADARG
        assert L.nbl_task_jacobian_deriv(w._h, km, B, rows, dofs, p(S), p(J), st) == _abi.NBL_E_BADARG
        assert L.nbl_task_jacobian_vjp(w._h, km, B, rows, dofs, p(S), p(J), p(gs), 0, st) == _abi.NBL_E_BADARG
        assert L.nbl_task_accel(w._h, km, B, rows, dofs, p(S), p(A), None, p(out), st) == _abi.NBL_E_BADARG
        assert L.nbl_task_accel_vjp(w._h, km, B, rows, dofs, p(S), p(A), p(out), p(gs), None, 0, p(ws), ws.numel(), st) == _abi.NBL_E_BADARG
        assert b"rows" in L.nbl_last_error() or b"n = " in L.nbl_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(J).all() and torch.isnan(out).all() and torch.isnan(gs).all()      # nothing was launched
    assert L.nbl_task_jacobian(w._h, None, B, R, n, p(S), p(J), st) == _abi.NBL_E_BADARG       # a null map, state, output
    assert L.nbl_task_jacobian(w._h, km, B, R, n, None, p(J), st) == _abi.NBL_E_BADARG
    assert L.nbl_task_jacobian(w._h, km, B, R, n, p(S), None, st) == _abi.NBL_E_BADARG
    assert L.nbl_task_accel(w._h, km, B, R, n, p(S), None, None, p(out), st) == _abi.NBL_E_BADARG   # xdd without accel
    assert L.nbl_task_accel_vjp(w._h, km, B, R, n, p(S), p(A), p(out), p(gs), None, 0, p(ws), 8, st) == _abi.NBL_E_WORKSPACE
    assert L.nbl_task_jacobian(w._h, km, 0, R, n, None, None, st) == 0                              # B = 0: a no-op
