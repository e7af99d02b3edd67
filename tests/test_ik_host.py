"""The PRODUCT's inverse kinematics (nimblephysics_amd/csrc/ik_dev.hpp: what k_ik_solve runs per lane) compiled for the host with g++
(tests/host_shim/ik_shim.cpp) and checked against tests/ik_numpy.py, a line-by-line numpy statement of the reference's solveIK / refineIK /
clampPositionsToLimits on kin_numpy's rows and Jacobian (which forms the LARGER normal matrix, as the reference does).

Models (tests/ik_cases.py): a 3-revolute arm with a linear entry (P = n = 3), a 7-revolute arm with a spatial entry (P = 6 < n), a 2-revolute
arm with two spatial entries (P = 12 > n, mostly unreachable), a free root + ball wrist tree with a spatial and an angular entry, Atlas-20
with four spatial entries (pelvis, feet, a hand).  Targets: the rows of random configurations inside the limits.  B = 130 worlds each.

Tolerances: the dense J at 1e-10 (test_kinematics_host.py's for the same quantity).  Up to 25 steps: 1e-9 on every world - one DLS step
solves a system of condition at most (sigma_max(J)^2 + lambda) / lambda, 1e3 .. 1e4 for arms of about 1 m with lambda = 0.01, so round-off and
the switch between the two normal-matrix forms enter at about 1e-12 per step, compounded by the growth of lr, 1.1^25 = 11.  Full runs (500
steps): 1e-7, the project's parity tolerance, on the worlds whose `steps` equal the restatement's.

The restatement runs in a pool of worker processes (one world per task): it is a few milliseconds of Python per evaluation."""
import multiprocessing
import os

import numpy as np
import pytest

import ik_cases as ic
import ik_numpy as ikn
from kin_numpy import mapping_rows
from oracle import OracleWorld
from test_kinematics_host import ShimMap, shim as kin_shim  # noqa: F401  (the kinematics host build, for the loss check)

CASES = list(ic.cases().keys())
_STATE = {}


def _problem(case):
    """(md, entries, oracle, targets [B, P]) of a case, the same in every process"""
    key = ("problem", case)
    if key not in _STATE:
        md, entries = (ic.limited_arm3(), [(1, 2)]) if case == "limited_arm3" else ic.cases()[case]
        ow = OracleWorld(md)
        if case == "limited_arm3":        # targets that need 1 rad on every joint: outside the +-0.3 limits
            rng = np.random.default_rng(ic.SEED + 7)
            poses = rng.choice([-1.0, 1.0], (ic.B_TEST, 3)) * rng.uniform(0.9, 1.1, (ic.B_TEST, 3))
        else:
            poses = ic.random_poses(md, ow, entries, ic.B_TEST, ic.SEED + CASES.index(case))
        targets = np.stack([mapping_rows(ow, md, q, entries)[0] for q in poses])
        _STATE[key] = (md, entries, ow, targets, poses)
    return _STATE[key]


def _restate_world(args):
    """One world: the restatement for every max_step_count of `counts` (they share the 20-step phase)."""
    case, b, target, init, cfg, counts = args
    md, entries, ow, _, _ = _problem(case)
    prob = ikn.Problem(ow, md, entries, target)
    out, restart = [], None
    for k in counts:
        r = prob.solve(init, ikn.IKConfig(max_step_count=k, **cfg), restart)
        restart = r["restart"]
        out.append((r["pos"], r["final_loss"], r["steps"]))
    return out


def _restate(case, targets, counts, init=None, **cfg):
    """-> {count: (q [B, n], final_loss [B], steps [B])}, computed once per argument set and shared between the tests"""
    key = ("restate", case, tuple(counts), tuple(sorted(cfg.items())), None if init is None else init.tobytes(), targets.tobytes())
    if key not in _STATE:
        n = _problem(case)[0].num_dofs
        jobs = [(case, b, targets[b], np.zeros(n) if init is None else init[b], cfg, tuple(counts)) for b in range(len(targets))]
        procs = min(16, os.cpu_count() or 1, len(jobs))
        if procs > 1:
            with multiprocessing.get_context("fork").Pool(procs) as pool:
                res = pool.map(_restate_world, jobs, chunksize=max(1, len(jobs) // (4 * procs)))
        else:
            res = [_restate_world(j) for j in jobs]
        _STATE[key] = {k: (np.stack([r[i][0] for r in res]), np.array([r[i][1] for r in res]), np.array([r[i][2] for r in res]))
                       for i, k in enumerate(counts)}
    return _STATE[key]


@pytest.fixture(scope="module")
def shim():
    return ic.load_ik_shim()


def _host(shim, case):
    md, entries, _, _, _ = _problem(case)
    return ic.HostIK(shim, md, entries)


@pytest.mark.parametrize("case", CASES)
def test_the_dense_jacobian_equals_the_numpy_jacobian(shim, case):
    md, entries, ow, targets, poses = _problem(case)
    h = _host(shim, case)
    q = poses[:6] * 0.7
    diff, J, err = h.evaluate(q, targets[:6])
    for b in range(6):
        pos, Jp, _ = mapping_rows(ow, md, q[b], entries)
        assert np.abs(J[b] - Jp).max() <= 1e-10 * max(1.0, np.abs(Jp).max()), (case, b)
        assert np.abs(diff[b] - (pos - targets[b])).max() <= 1e-12 * max(1.0, np.abs(pos).max())
        assert abs(err[b] - diff[b] @ diff[b]) <= 1e-12 * max(1.0, err[b])


@pytest.mark.parametrize("case", CASES)
def test_the_first_steps_equal_the_restatement_on_every_world(shim, case):
    """max_step_count 1, 2, 3, 5 after the 20-step phase: q_out of every world of B = 130 to 1e-9."""
    _, _, _, targets, _ = _problem(case)
    h = _host(shim, case)
    ref = _restate(case, targets, (1, 2, 3, 5))
    worst = 0.0
    for k in (1, 2, 3, 5):
        q, loss, steps = h.solve(targets, max_step_count=k)
        rq, rl, rs = ref[k]
        assert np.array_equal(steps, rs), (case, k)
        worst = max(worst, float(np.abs(q - rq).max()))
    print(f"[ik host] {case}: worst |q - restatement| over max_step_count 1, 2, 3, 5 and {len(targets)} worlds: {worst:.3e}")
    assert worst <= 1e-9


def full_run_check(q, loss, steps, rq, rl, rs, what):
    """The full-run rule: worlds whose `steps` equal the reference's agree to 1e-7; a world that took another branch at a rounding-level
    errorChange is left out of that comparison, must still end with loss <= 1.01 x the reference's final loss + 1e-12, and at most 2 % of
    the worlds may be left out.  Returns (worlds left out, worst |q - ref| of the others)."""
    same = steps == rs
    out = int((~same).sum())
    worst = float(np.abs(q[same] - rq[same]).max()) if same.any() else 0.0
    print(f"[ik full run] {what}: {out} of {len(steps)} worlds left out, worst |q - reference| of the others {worst:.3e}, steps {steps.min()} .. {steps.max()}")
    assert np.isfinite(q).all() and np.isfinite(loss).all()
    assert worst <= 1e-7, what
    assert (loss[~same] <= 1.01 * rl[~same] + 1e-12).all(), what
    assert out <= 0.02 * len(steps), what
    return out, worst


@pytest.mark.parametrize("case", CASES)
def test_full_runs_equal_the_restatement(shim, case):
    """IKMapping::setPositions' configuration (500 steps, from zero), B = 130.  Observed on the development machine (g++ -O2
    -ffp-contract=off, seeds of tests/ik_cases.py): NO world of any of the five models is left out (every world takes the restatement's
    number of evaluations), worst |q - restatement| 1.6e-8 (atlas20; arm7_spatial 7e-9, the others below 1e-13); evaluations per world 11 .. 94.
    The worst per-row residual |rows(q_out) - target| the RESTATEMENT leaves on Atlas-20's 130 reachable targets is printed here and pinned
    in test_the_residual_the_reference_leaves_on_atlas20."""
    _, _, _, targets, _ = _problem(case)
    h = _host(shim, case)
    rq, rl, rs = _restate(case, targets, (500,))[500]
    q, loss, steps = h.solve(targets, max_step_count=500)
    full_run_check(q, loss, steps, rq, rl, rs, case)


def test_the_residual_the_reference_leaves_on_atlas20(shim):
    """With lambda = 0.01 and the 1e-7 convergence rule the reference's solve stops far from Atlas-20's reachable targets: the worst per-row
    residual max_b max_p |rows(q_out) - target| that tests/ik_numpy.py leaves on the 130 targets of this file is ATLAS_REFERENCE_RESIDUAL
    (measured here, used by tests/test_gpu_ik.py as the bound of IKMapping.setPositions, plus 10 %)."""
    md, entries, ow, targets, _ = _problem("atlas20")
    rq, _, _ = _restate("atlas20", targets, (500,))[500]
    resid = max(float(np.abs(mapping_rows(ow, md, rq[b], entries)[0] - targets[b]).max()) for b in range(len(targets)))
    print(f"[ik host] atlas20: worst per-row residual of the restatement over {len(targets)} targets: {resid:.6f}")
    assert abs(resid - ic.ATLAS_REFERENCE_RESIDUAL) <= 0.01 * ic.ATLAS_REFERENCE_RESIDUAL


def test_clamping_keeps_every_coordinate_inside_its_limits(shim):
    """The 3-revolute arm with limits +-0.3 rad and targets that need 1 rad: every coordinate of q_out inside its limits exactly, the
    result the restatement's to 1e-7 (full-run rule)."""
    _, _, _, targets, _ = _problem("limited_arm3")
    h = _host(shim, "limited_arm3")
    rq, rl, rs = _restate("limited_arm3", targets, (500,))[500]
    q, loss, steps = h.solve(targets, max_step_count=500)
    assert (q >= -0.3).all() and (q <= 0.3).all()
    assert (np.abs(q) == 0.3).any()                       # the limits are active
    full_run_check(q, loss, steps, rq, rl, rs, "limited_arm3")


def test_a_coordinate_started_a_turn_away_comes_back_inside_the_limits(shim):
    """q_init = q + 2 pi on one coordinate, start_clamped: clampPositionsToLimits brings it back inside [-0.3, 0.3] (its 2 pi candidates do
    not survive its own selection loop - csrc/ik_dev.hpp -: the coordinate is clamped to the upper limit, and the solve goes on from
    there), and the solve returns the restatement's positions, a turn away from where it started."""
    md, entries, ow, _, _ = _problem("limited_arm3")
    h = _host(shim, "limited_arm3")
    rng = np.random.default_rng(ic.SEED + 9)
    qt = rng.uniform(-0.25, 0.25, (16, 3))
    targets = np.stack([mapping_rows(ow, md, q, entries)[0] for q in qt])
    init = qt.copy()
    init[:, 1] += 2 * np.pi
    rq, rl, rs = _restate("limited_arm3", targets, (500,), init=init, start_clamped=True)[500]
    q, loss, steps = h.solve(targets, init=init, max_step_count=500, start_clamped=True)
    assert (q >= -0.3).all() and (q <= 0.3).all()
    assert (np.abs(q[:, 1] - init[:, 1]) > np.pi).all()
    full_run_check(q, loss, steps, rq, rl, rs, "limited_arm3 from q + 2 pi")


def test_the_clamp_equals_the_literal_routine(shim):
    """ikClamp states the net effect of clampPositionsToLimits; tests/ik_numpy.py states the routine with its loops: the same bits on
    coordinates up to several turns outside the limits, and the same rotation vectors (1e-12) after logMap(expMapRot(.))."""
    rng = np.random.default_rng(ic.SEED + 11)
    for case in ("limited_arm3", "free_ball_tree", "atlas20"):
        md = _problem(case)[0]
        dev = md.merge_welds() if md.has_welds() else md
        h = _host(shim, case)
        q = rng.normal(0, 4.0, (40, md.num_dofs))
        off = 0
        for b in dev.bodies:                                  # rotation vectors whose wrapped angle stays 0.3 rad below pi, as everywhere
            nd = {"free": 6, "ball": 3, "weld": 0}.get(b.joint_type, 1)
            if nd >= 3:
                for x in q:
                    while abs((np.linalg.norm(x[off:off + 3]) + np.pi) % (2 * np.pi) - np.pi) > np.pi - 0.3:
                        x[off:off + 3] = rng.normal(0, 4.0, 3)
            off += nd
        got = h.clamp(q)
        ref = np.stack([ikn.clamp_positions(dev, x) for x in q])
        rot = np.zeros(md.num_dofs, dtype=bool)
        off = 0
        for b in dev.bodies:
            nd = {"free": 6, "ball": 3, "weld": 0}.get(b.joint_type, 1)
            if nd >= 3:
                rot[off:off + 3] = True
            off += nd
        assert np.array_equal(got[:, ~rot], ref[:, ~rot]), case
        assert np.abs(got[:, rot] - ref[:, rot]).max(initial=0.0) <= 1e-12, case
        if rot.any():
            assert (np.linalg.norm(got[:, rot].reshape(40, -1, 3), axis=2) <= np.pi + 1e-12).all()


def test_an_unreachable_target_terminates_early(shim):
    """A point twice the arm's length away: the solve ends before its step budget (the vanishing-lr or the converged branch), finite, and
    not worse than where it started."""
    md, entries, ow, _, _ = _problem("arm3_linear")
    h = _host(shim, "arm3_linear")
    rng = np.random.default_rng(ic.SEED + 13)
    d = rng.normal(size=(ic.B_TEST, 3))
    targets = 2.0 * d / np.linalg.norm(d, axis=1, keepdims=True) + np.array([0, 0, 0.1])     # the arm (1 m) hangs on a base at z = 0.1
    q, loss, steps = h.solve(targets, max_step_count=500)
    start = np.array([np.sum((mapping_rows(ow, md, np.zeros(3), entries)[0] - t) ** 2) for t in targets])
    assert np.isfinite(q).all() and np.isfinite(loss).all()
    assert (steps < 20 + 500).all(), steps.max()
    assert (loss <= start).all()
    assert (loss > 0.5).all()                             # really unreachable: at least 1 m away


@pytest.mark.parametrize("case", CASES)
def test_the_loss_is_the_squared_error_at_the_returned_positions(shim, kin_shim, case):  # noqa: F811
    md, entries, _, targets, _ = _problem(case)
    h = _host(shim, case)
    q, loss, _ = h.solve(targets, max_step_count=500)
    rows = ShimMap(kin_shim, md, entries).run(np.concatenate([q.T, np.zeros_like(q.T)]), want=("pos",))["pos"].T
    ref = ((rows - targets) ** 2).sum(1)
    assert (np.abs(loss - ref) <= 1e-12 * np.maximum(ref, 1e-300)).all(), np.abs(loss / ref - 1).max()


def test_results_do_not_depend_on_the_batch(shim):
    """One world's solve is bit for bit the same alone and at any place of a batch."""
    _, _, _, targets, _ = _problem("atlas20")
    h = _host(shim, "atlas20")
    q, loss, steps = h.solve(targets[:9], max_step_count=500)
    for b in (0, 4, 8):
        q1, l1, s1 = h.solve(targets[b:b + 1], max_step_count=500)
        assert np.array_equal(q1[0], q[b]) and l1[0] == loss[b] and s1[0] == steps[b]
