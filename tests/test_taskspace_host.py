"""The PRODUCT's task-space code (nimblephysics_amd/csrc/taskspace_dev.hpp: what k_task_jacobian, k_task_jacobian_deriv, k_task_jacobian_vjp,
k_task_accel and k_task_accel_vjp run per lane) compiled for the host with g++ -O2 -ffp-contract=off (tests/host_shim/task_shim.cpp) and
held to tests/task_numpy.py, the numpy statement in world coordinates, on the three models of tests/task_cases.py, 130 worlds each.

  1  J, Jdot, Jdot v and J a + Jdot v against the numpy statement, every world, the outputs pre-filled with NaN; the zero columns are
     exactly zero;  J equals the velocity Jacobian of tests/kin_numpy.py (the statement behind the map_to_vel tests), Jdot v = the bias
     acceleration and J a + Jdot v = the acceleration;
  2  the reverse passes against central differences of the NUMPY statement at the step 1e-6: the bound per model is 100 x the largest
     disagreement of the reference's own differences at the steps 1e-5 and 1e-6; every world is checked;
  3  a world alone gives the bits it gives in the batch.

MEASURED (this file's inputs; printed by the tests).  Forward quantities, largest per-world deviation from the numpy statement over the
three models: J 1.2e-15, Jdot 2.4e-15, Jdot v 2.0e-15, J a + Jdot v 1.7e-15 (relative to max(1, |ref|)).  FORWARD_TOL = 100 x the
largest of them, rounded up: 2.5e-13 - the bound of the device tests too (tests/test_gpu_taskspace.py), far inside the 1e-7 parity bound.
The reference's central differences at 1e-5 and 1e-6 disagree by 7.4e-10 .. 4.4e-9 (per model and output, max over the worlds), so the
bounds of item 2 lie between 7.4e-8 and 4.4e-7; the code under test is within 4.1e-9 of the 1e-6 differences everywhere."""
import numpy as np
import pytest

import task_cases as tc
import task_numpy as tn

FORWARD_TOL = 2.5e-13
CASES = tc.cases()
IDS = list(CASES)
B = tc.B_MAX


@pytest.fixture(scope="module")
def shim():
    return tc.load_shim()


@pytest.mark.parametrize("name", IDS)
def test_forward_quantities_equal_the_numpy_statement_in_every_world(shim, name):
    md, entries = CASES[name]
    m, ne = tn.Model(md), tc.numpy_entries(entries)
    d = tc.ShimTask(shim, md, entries)
    q, v, a = tc.states(md, B)
    J, Jd = tn.jacobians(m, ne, q, v)
    ref = {"J": J, "Jdot": Jd, "Jdot v": tn.accel(m, ne, q, v), "J a + Jdot v": tn.accel(m, ne, q, v, a)}
    got = {"J": d.jacobian(q), "Jdot": d.jacobian_deriv(q, v), "Jdot v": d.accel(q, v), "J a + Jdot v": d.accel(q, v, a)}
    worst = {k: float(tc.err(got[k], ref[k]).max()) for k in ref}
    print(name, "largest per-world deviation from the numpy statement:", worst)
    for k in ref:
        e = tc.err(got[k], ref[k])
        assert np.isfinite(got[k]).all() and (e <= FORWARD_TOL).all(), (name, k, int(e.argmax()), float(e.max()))
    zero = tc.zero_mask(md, entries)
    assert zero.any() and not got["J"][:, zero].any() and not got["Jdot"][:, zero].any()
    if name == "screw_chain":                                        # the entry on the first body: nothing from the two later coordinates
        assert zero[-3:, 1:].all()
    assert (tc.err(np.einsum("brd,bd->br", got["Jdot"], v), got["Jdot v"]) <= FORWARD_TOL).all()
    assert (tc.err(np.einsum("brd,bd->br", got["J"], a) + got["Jdot v"], got["J a + Jdot v"]) <= FORWARD_TOL).all()


@pytest.mark.parametrize("name", IDS)
def test_j_times_v_is_the_velocity_of_the_existing_kinematics_code(shim, name):
    """an independent statement: J equals kin_numpy's velocity Jacobian rows (OracleWorld frames, getWorldJacobian's screws)"""
    import kin_numpy
    from oracle import OracleWorld
    md, entries = CASES[name]
    d = tc.ShimTask(shim, md, entries)
    q, v, _ = tc.states(md, 4)
    ow = OracleWorld(md)
    J = d.jacobian(q)
    for b in range(4):
        _, _, Jv = kin_numpy.mapping_rows(ow, md, q[b], entries)
        assert np.abs(J[b] - Jv).max() <= 1e-12 * max(1.0, np.abs(Jv).max()), (name, b)


@pytest.mark.parametrize("name", IDS)
def test_reverse_passes_equal_the_references_central_differences_in_every_world(shim, name):
    md, entries = CASES[name]
    m, ne = tn.Model(md), tc.numpy_entries(entries)
    d = tc.ShimTask(shim, md, entries)
    q, v, a = tc.states(md, B)
    rng = np.random.default_rng(tc.SEED + 7)
    cot, G = rng.normal(size=(B, d.R)), rng.normal(size=(B, d.R, d.n))
    fd = {}
    for eps in (1e-5, 1e-6):
        x = tn.fd_accel_vjp(m, ne, q, v, a, cot, eps)
        c = tn.fd_accel_vjp(m, ne, q, v, None, cot, eps)
        fd[eps] = {"xdd q": x[0], "xdd v": x[1], "xdd a": x[2], "bias q": c[0], "bias v": c[1], "J q": tn.fd_jacobian_vjp(m, ne, q, G, eps)}
    gx, gc = d.accel_vjp(q, v, a, cot), d.accel_vjp(q, v, None, cot)
    got = {"xdd q": gx[0], "xdd v": gx[1], "xdd a": gx[2], "bias q": gc[0], "bias v": gc[1], "J q": d.jacobian_vjp(q, G)}
    scatter = {k: float(tc.err(fd[1e-5][k], fd[1e-6][k]).max()) for k in got}
    worst = {k: float(tc.err(got[k], fd[1e-6][k]).max()) for k in got}
    print(name, "reference differences, 1e-5 against 1e-6:", scatter)
    print(name, "code under test against the 1e-6 differences:", worst)
    for k in got:
        e = tc.err(got[k], fd[1e-6][k])
        assert np.isfinite(got[k]).all() and (e <= 100.0 * scatter[k]).all(), (name, k, int(e.argmax()), float(e.max()), 100.0 * scatter[k])


def test_a_world_alone_gives_the_bits_of_the_batch(shim):
    md, entries = CASES["free_ball"]
    d = tc.ShimTask(shim, md, entries)
    q, v, a = tc.states(md, 5)
    rng = np.random.default_rng(3)
    cot, G = rng.normal(size=(5, d.R)), rng.normal(size=(5, d.R, d.n))
    full = [d.jacobian(q), d.jacobian_deriv(q, v), d.accel(q, v, a), d.jacobian_vjp(q, G), *d.accel_vjp(q, v, a, cot)]
    for b in range(5):
        s = slice(b, b + 1)
        one = [d.jacobian(q[s]), d.jacobian_deriv(q[s], v[s]), d.accel(q[s], v[s], a[s]), d.jacobian_vjp(q[s], G[s]), *d.accel_vjp(q[s], v[s], a[s], cot[s])]
        assert all(np.array_equal(x[0], y[b]) for x, y in zip(one, full))
