"""Batched inverse kinematics on the device (csrc/ik.hip: nbl_ik_solve, solve_ik, IKMapping.setPositions / setVelocities /
setControlForces) against the host build of the same header (tests/host_shim/ik_shim.cpp) on the models, targets and seeds of
tests/test_ik_host.py (tests/ik_cases.py) - there the host build is held to the numpy restatement of the reference -, bit-identity across
batch sizes and under divergent termination, the World setters, deferred join, immobile skeletons, argument errors and the plain-C driver.
B = 130: two full wavefronts and a tail of 2, the smallest batch with both lane divergence and a partial wave."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ik_cases as ic
from kin_numpy import mapping_rows
from oracle import OracleWorld

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CASES = list(ic.cases().keys())
_STATE = {}


def _problem(case):
    """(md, entries, targets [130, P], poses) exactly as tests/test_ik_host.py draws them"""
    if case not in _STATE:
        md, entries = ic.cases()[case]
        ow = OracleWorld(md)
        poses = ic.random_poses(md, ow, entries, ic.B_TEST, ic.SEED + CASES.index(case))
        targets = np.stack([mapping_rows(ow, md, q, entries)[0] for q in poses])
        _STATE[case] = (md, entries, targets, poses)
    return _STATE[case]


def _device(case):
    """(World, IKMapping) of a case, made once"""
    import nimblephysics_amd as na
    key = ("device", case)
    if key not in _STATE:
        md, entries, _, _ = _problem(case)
        w = na.World(md, device=DEV)
        m = na.IKMapping(w)
        for kind, body in entries:
            (m.addSpatialBodyNode, m.addLinearBodyNode, m.addAngularBodyNode)[kind](body)
        _STATE[key] = (w, m)
    return _STATE[key]


@pytest.fixture(scope="module")
def shim():
    return ic.load_ik_shim()


def _solve(case, targets, init=None, **cfg):
    import nimblephysics_amd as na
    w, m = _device(case)
    q, loss, steps = na.solve_ik(w, m, torch.tensor(targets, device=DEV), None if init is None else torch.tensor(init, device=DEV),
                                 na.IKConfig(**cfg))
    return q.cpu().numpy(), loss.cpu().numpy(), steps.cpu().numpy()


@pytest.mark.parametrize("case", CASES)
def test_the_first_steps_equal_the_host_build(shim, case):
    """max_step_count 1 and 5 after the 20-step phase, every world, 1e-9 (the reasoning of tests/test_ik_host.py: the device contracts
    a b + c into one rounding where the host build does not, which is round-off of the same size)."""
    md, entries, targets, _ = _problem(case)
    h = ic.HostIK(shim, md, entries)
    worst = 0.0
    for k in (1, 5):
        q, loss, steps = _solve(case, targets, max_step_count=k)
        hq, hl, hs = h.solve(targets, max_step_count=k)
        assert np.array_equal(steps, hs), (case, k)
        worst = max(worst, float(np.abs(q - hq).max()))
    print(f"[ik gpu] {case}: worst |q - host build| over max_step_count 1, 5 and {len(targets)} worlds: {worst:.3e}")
    assert worst <= 1e-9


@pytest.mark.parametrize("case", CASES)
def test_full_runs_equal_the_host_build(shim, case):
    """500 steps under the full-run rule of tests/test_ik_host.py (1e-7 on the worlds with the host build's `steps`, the others end with
    loss <= 1.01 x the host build's + 1e-12, at most 2 % of them)."""
    from test_ik_host import full_run_check
    md, entries, targets, _ = _problem(case)
    q, loss, steps = _solve(case, targets, max_step_count=500)
    hq, hl, hs = ic.HostIK(shim, md, entries).solve(targets, max_step_count=500)
    full_run_check(q, loss, steps, hq, hl, hs, case + " (device against host build)")


def test_a_world_does_not_depend_on_the_batch():
    _, _, targets, _ = _problem("atlas20")
    first, second = _solve("atlas20", targets, max_step_count=500), _solve("atlas20", targets, max_step_count=500)
    for u, v in zip(first, second):
        assert np.array_equal(u, v)
    for b in (0, 63, 64, 129):
        one = _solve("atlas20", targets[b:b + 1], max_step_count=500)
        for u, v in zip(one, first):
            assert np.array_equal(u[0], v[b]), b


def test_divergent_termination_lane_by_lane():
    """Trivially solved targets (the rows at q_init), reachable and unreachable ones interleaved lane by lane: each world is its own
    B = 1 solve bit for bit.  A trivially solved world takes 2 evaluations PER PHASE, 4 in all, the fewest refineIK's control flow allows:
    its ladder runs only after step 0 (IKSolver.cpp:345), so each of the two refineIK calls evaluates at i = 0, steps, and stops at
    i = 1 on currentError < 1e-21."""
    md, entries, targets, poses = _problem("arm3_linear")
    ow = OracleWorld(md)
    B = ic.B_TEST
    rng = np.random.default_rng(ic.SEED + 21)
    init = rng.uniform(-0.5, 0.5, (B, 3))
    t = targets.copy()
    for b in range(B):
        if b % 3 == 0:
            t[b] = mapping_rows(ow, md, init[b], entries)[0]
        elif b % 3 == 2:
            d = rng.normal(size=3)
            t[b] = 2.0 * d / np.linalg.norm(d)
    q, loss, steps = _solve("arm3_linear", t, init=init, max_step_count=500)
    assert (steps[0::3] == 4).all() and (loss[0::3] < 1e-21).all()
    assert (loss[2::3] > 0.5).all() and (steps[2::3] < 520).all() and np.isfinite(q).all()
    assert len(set(steps.tolist())) > 3
    for b in list(range(0, 12)) + [63, 64, 65, 127, 128, 129]:
        one = _solve("arm3_linear", t[b:b + 1], init=init[b:b + 1], max_step_count=500)
        assert np.array_equal(one[0][0], q[b]) and one[1][0] == loss[b] and one[2][0] == steps[b], b


def test_set_positions_on_atlas20():
    """getPositions after setPositions reproduces 130 reachable targets to within the worst per-row residual the reference's own solve
    leaves on them (ic.ATLAS_REFERENCE_RESIDUAL, measured by tests/test_ik_host.py on the numpy restatement) plus 10 % for the different
    branch histories; the velocities are untouched; the same on a 1-D target."""
    import nimblephysics_amd as na
    md, entries, targets, _ = _problem("atlas20")
    w, m = _device("atlas20")
    n = md.num_dofs
    rng = np.random.default_rng(3)
    state = torch.tensor(rng.normal(0, 0.3, (ic.B_TEST, 2 * n)), device=DEV)
    w.setState(state)
    m.setPositions(w, torch.tensor(targets, device=DEV))
    got = m.getPositions(w).cpu().numpy()
    resid = float(np.abs(got - targets).max())
    print(f"[ik gpu] atlas20 setPositions: worst per-row residual {resid:.6f} (the reference's own: {ic.ATLAS_REFERENCE_RESIDUAL})")
    # (the bound the issue sets; with the reference itself stopping 1.53 away it says little: the sharp checks are the equality with
    # solve_ik below and the full-run parity with the host build above)
    assert resid <= 1.1 * ic.ATLAS_REFERENCE_RESIDUAL
    after = w.getState()
    assert torch.equal(after[:, n:], state[:, n:])
    q, _, _ = na.solve_ik(w, m, torch.tensor(targets, device=DEV), None, na.IKConfig(max_step_count=500))
    assert torch.equal(after[:, :n], q)                        # setPositions = solve_ik from zero with 500 steps
    w.setState(state[5])
    m.setPositions(w, torch.tensor(targets[5]))                # a [P] target, given on the CPU
    one = w.getState()
    assert one.shape == (1, 2 * n) or one.shape == (2 * n,)
    assert torch.equal(one.reshape(-1)[:n], q[5]) and torch.equal(one.reshape(-1)[n:], state[5, n:])
    assert m.getPositions(w).shape == (m.getPosDim(),)


def test_set_velocities_and_control_forces():
    import nimblephysics_amd as na
    md, entries, targets, poses = _problem("arm7_spatial")
    w, m = _device("arm7_spatial")
    n, B = md.num_dofs, 32
    rng = np.random.default_rng(5)
    state = torch.tensor(np.concatenate([poses[:B], rng.normal(0, 1, (B, n))], 1), device=DEV)
    w.setState(state)
    v = torch.tensor(rng.normal(0, 1, (B, 6)), device=DEV)
    m.setVelocities(w, v)
    assert torch.equal(w.getState()[:, :n], state[:, :n])
    assert float((m.getVelocities(w) - v).abs().max()) <= 1e-9
    f = torch.tensor(rng.normal(0, 1, (B, 6)), device=DEV)
    m.setControlForces(w, f)
    J = m.getRealVelToMappedVelJac(w)
    want = (J.transpose(1, 2) @ f.unsqueeze(-1)).squeeze(-1)[:, list(w.model.action_map)]
    assert float((w.getAction() - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_deferred_join_with_a_step_in_flight():
    import nimblephysics_amd as na
    md = na.atlas("atlas20", ground=True)
    B = 4096
    plain, entries, targets, _ = _problem("atlas20")
    rng = np.random.default_rng(8)
    S = np.zeros((B, 2 * md.num_dofs)); S[:, 0] = -np.pi / 2; S[:, 4] = 1.0; S[:, 6:md.num_dofs] = rng.normal(0, 0.02, (B, md.num_dofs - 6))
    ref, dw = na.World(md, device=DEV), na.World(md, device=DEV)
    maps = []
    for w in (ref, dw):
        m = na.IKMapping(w)
        for kind, body in entries:
            m.addSpatialBodyNode(plain.bodies[body].name)         # (the bodies' names: the ground model lists them at other indices)
        maps.append(m)
    s_soa = ref.to_soa(torch.tensor(S, device=DEV)); a_soa = ref.to_soa(torch.zeros((B, ref.k), dtype=torch.float64, device=DEV))
    t = torch.tensor(targets[:64], device=DEV)
    want_next, _, _ = ref.step_soa(s_soa, a_soa, want_saved=True)
    init_ref = want_next.t()[:64, :md.num_dofs].contiguous()
    want = na.solve_ik(ref, maps[0], t, init_ref, na.IKConfig(max_step_count=20))
    dw.set_deferred_join(True)
    assert dw.slices_for(B) > 1
    buf = {"nxt": torch.empty_like(s_soa), "saved": torch.empty(dw.saved_bytes(B), dtype=torch.uint8, device=DEV),
           "status": torch.empty(B, dtype=torch.int32, device=DEV), "cache": torch.empty((dw.m, B), dtype=torch.float64, device=DEV)}
    dw.step_into(s_soa, a_soa, buf["nxt"], buf["saved"], buf["status"], None, buf["cache"])
    got = na.solve_ik(dw, maps[1], t, buf["nxt"].t()[:64, :md.num_dofs], na.IKConfig(max_step_count=20))
    for u, v in zip(got, want):
        assert torch.equal(u, v)
    dw.join()
    torch.cuda.synchronize()


def test_immobile_skeletons_keep_their_frozen_coordinates_zero(tmp_path):
    import nimblephysics_amd as na
    from test_ref_layout import load
    md = load(tmp_path)
    w = na.World(md, device=DEV)
    assert w.ref_layout is not None and w.getStateSize() == 24 and w.n == 6
    mobile = [b.name for b in md.bodies if b.skeleton not in set(md.immobile_skeletons or ())]
    m = na.IKMapping(w)
    m.addSpatialBodyNode(mobile[-1])
    rng = np.random.default_rng(2)
    full = np.zeros((8, 24)); full[:, 6:12] = rng.normal(0, 0.3, (8, 6)); full[:, 18:] = rng.normal(0, 1, (8, 6))
    w.setState(torch.tensor(full, device=DEV))
    target = m.getPositions(w).clone()
    w.setState(torch.tensor(np.concatenate([np.zeros((8, 12)), full[:, 12:]], 1), device=DEV))
    start = ((m.getPositions(w) - target) ** 2).sum(1)          # the loss at zero, where setPositions starts
    m.setPositions(w, target)
    s = w.getState()
    assert s.shape == (8, 24) and not s[:, :6].any() and torch.equal(s[:, 12:], torch.tensor(full[:, 12:], device=DEV))
    q, loss, steps = na.solve_ik(w, m, target, None, na.IKConfig(max_step_count=500))
    assert q.shape == (8, 6) and torch.equal(q, s[:, 6:12])
    assert (loss <= start).all() and (steps >= 2).all()
    m.setVelocities(w, torch.tensor(rng.normal(0, 1, (8, 6)), device=DEV))
    assert not w.getState()[:, 12:18].any()


def test_argument_errors():
    import nimblephysics_amd as na
    from nimblephysics_amd._lib import check
    from nimblephysics_amd.mapping import _CIKConfig
    w, m = _device("arm3_linear")
    L, h, km = w._L, w._h, m._device_map(w)
    B = 8
    t = torch.zeros((3, B), dtype=torch.float64, device=DEV)
    q = torch.full((3, B), 7.0, dtype=torch.float64, device=DEV)
    need = L.nbl_ik_workspace_bytes(h, km, B)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())
    good = _CIKConfig(1e-7, 100, 0.01, 0, 1, 0)
    huge = _CIKConfig(1e-7, 100001, 0.01, 0, 1, 0)
    lam0, steps0, neg = _CIKConfig(1e-7, 100, 0.0, 0, 1, 0), _CIKConfig(1e-7, 0, 0.01, 0, 1, 0), _CIKConfig(1e-7, 100, -0.5, 0, 1, 0)
    assert need > 0 and L.nbl_ik_workspace_bytes(None, km, B) == 0 and L.nbl_ik_workspace_bytes(h, km, 0) == 0
    for rc_want, call in ((-1, lambda: L.nbl_ik_solve(None, km, B, p(t), None, C.byref(good), p(q), None, None, p(ws), need, None)),
                          (-1, lambda: L.nbl_ik_solve(h, None, B, p(t), None, C.byref(good), p(q), None, None, p(ws), need, None)),
                          (-1, lambda: L.nbl_ik_solve(h, km, B, None, None, C.byref(good), p(q), None, None, p(ws), need, None)),
                          (-1, lambda: L.nbl_ik_solve(h, km, B, p(t), None, C.byref(good), None, None, None, p(ws), need, None)),
                          (-1, lambda: L.nbl_ik_solve(h, km, B, p(t), None, C.byref(good), p(q), None, None, None, need, None)),
                          (-1, lambda: L.nbl_ik_solve(h, km, -1, p(t), None, C.byref(good), p(q), None, None, p(ws), need, None)),
                          (-1, lambda: L.nbl_ik_solve(h, km, B, p(t), None, C.byref(steps0), p(q), None, None, p(ws), need, None)),
                          (-1, lambda: L.nbl_ik_solve(h, km, B, p(t), None, C.byref(huge), p(q), None, None, p(ws), need, None)),
                          (-1, lambda: L.nbl_ik_solve(h, km, B, p(t), None, C.byref(neg), p(q), None, None, p(ws), need, None)),
                          (-2, lambda: L.nbl_ik_solve(h, km, B, p(t), None, C.byref(lam0), p(q), None, None, p(ws), need, None)),
                          (-4, lambda: L.nbl_ik_solve(h, km, B, p(t), None, C.byref(good), p(q), None, None, p(ws), need - 1, None))):
        rc = call()
        assert rc == rc_want, (rc, rc_want)
        with pytest.raises(na.NimbleAmdError):
            check(rc, "ik")
        assert L.nbl_last_error()
    assert L.nbl_ik_solve(h, km, 0, None, None, C.byref(good), None, None, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((q == 7.0).all())                              # nothing was launched
    with pytest.raises(na.NimbleAmdError):
        na.solve_ik(w, m, torch.zeros(3), None, na.IKConfig(least_squares_damping=0.0))
    with pytest.raises(ValueError):
        na.solve_ik(w, m, torch.zeros(4))


def test_plain_c_ik_driver(tmp_path):
    """tests/c_abi_example/ik.c: nbl_ik_solve from pure C99 on the Atlas-20 model header, one linear entry on a foot."""
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/lib/libamdhip64.so"):
        pytest.skip("no gcc / ROCm runtime")
    libdir = os.path.join(ROOT, "nimblephysics_amd")
    exe = str(tmp_path / "ik")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_abi_example", "ik.c"), "-o", exe, "-L" + libdir, "-lnimble_amd",
                           "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath," + libdir])
    out = subprocess.check_output([exe, "130"]).decode()
    print(out)
    assert "ik loss worst" in out
