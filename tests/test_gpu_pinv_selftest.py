"""The device pseudo-inverses run ON THE GPU through the C ABI (nbl_selftest_pinv): coopPinv (Householder QR + complete orthogonal
decomposition, the role of Eigen's completeOrthogonalDecomposition in CGGM.cpp:280 / LCPUtils.cpp:113) and coopPinvSym (two
Cholesky factorisations with the GEMMs on the matrix cores, the route of every symmetric positive semi-definite Q) against numpy:
rank exact, Q^+ to cond(Q) eps, the two routes against each other.  (The same code on the host wave emulation: tests/test_coop_host.py.)"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _cases(rng, count, R=24):
    Q = np.zeros((count, R, R)); size = np.zeros(count, np.int32); rank = np.zeros(count, np.int32)
    for t in range(count):
        c = int(rng.integers(1, R + 1)); idx = np.sort(rng.choice(R, c, replace=False))
        kind = t % 6
        if kind == 0:                                   # a standing robot: c rows on two 6-DOF bodies
            k = min(c, 12); J = rng.normal(0, 1, (c, 12)); sub = J @ np.diag(rng.uniform(0.1, 2, 12)) @ J.T
        elif kind == 1:                                 # ... with the fallback CFM: full rank, ill conditioned
            k = c; J = rng.normal(0, 1, (c, 12)); sub = J @ np.diag(rng.uniform(0.1, 2, 12)) @ J.T + 1e-4 * np.eye(c)
        elif kind == 2:                                 # full rank, well conditioned (two contacts of a small body: the leading block only)
            c = min(c, 6); idx = np.arange(c); k = c; U = rng.normal(0, 1, (c, c + 3)); sub = U @ U.T
        else:
            k = int(rng.integers(1, c + 1)); U = rng.normal(0, 1, (c, k)); sub = U @ U.T
        Q[t][np.ix_(idx, idx)] = 0.5 * (sub + sub.T); size[t] = c; rank[t] = k
    return Q, size, rank


@pytest.mark.parametrize("R", [24, 48])      # the 24-row and the 48-row instantiation of the library (csrc/abi_variants.h)
def test_device_pseudo_inverses_equal_numpy_pinv(R):
    from nimblephysics_amd._lib import check, lib
    rng = np.random.default_rng(11 + R)
    count = 768 if R == 24 else 384
    Q, size, rank = _cases(rng, count, R)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    out = {}
    for route in (0, 1):
        P = np.zeros_like(Q); r = np.zeros(count, np.int32)
        check(lib().nbl_selftest_pinv_rows(count, R, vp(Q), vp(size), route, vp(P), vp(r), 1, None), "nbl_selftest_pinv_rows")
        out[route] = (P, r)
    worst = {0: 0.0, 1: 0.0}
    for t in range(count):
        sv = np.linalg.svd(Q[t], compute_uv=False)
        k = rank[t]; cond = sv[0] / sv[k - 1]
        ref = np.linalg.pinv(Q[t], rcond=0.5 * sv[k - 1] / sv[0])
        scale = np.abs(ref).max()
        for route in (0, 1):
            P, r = out[route]
            assert r[t] == k, (route, t, r[t], k)
            e = np.abs(P[t] - ref).max() / scale
            worst[route] = max(worst[route], e / (cond * 2.2e-16))
            assert e <= 500 * cond * 2.2e-16, (route, t, e, cond)
    print("worst error in units of cond(Q) eps: Householder route", worst[0], " Cholesky route", worst[1])


@pytest.mark.parametrize("R", [24, 48])
def test_round_off_pivots_of_exactly_singular_contact_matrices_are_rejected_like_the_references_cod(R):
    """An exactly singular Q (two contacts of one body that span five directions): the last pivot of the diagonally pivoted Cholesky
    is pure round-off but comes out ABOVE the eps * size threshold of the reference's decomposition (1.4e-15 of the first pivot against
    1.3e-15), the COD's last |R_kk| below it (3e-16): tests/golden/pinv_rank_borderline.json, a matrix the randomised soak found
    (seed 30168).  Both device routes must say rank 5 and return the rank-5 pseudo-inverse; plus 256 synthetic matrices with exactly
    repeated / linearly dependent rows."""
    import json
    import os
    from nimblephysics_amd._lib import check, lib
    f = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pinv_rank_borderline.json")))
    A = np.array([[float.fromhex(x) for x in row] for row in f["A"]])
    rng = np.random.default_rng(12)
    mats, ranks = [A], [5]
    for t in range(256):
        nc = int(rng.integers(2, R // 3 + 1)); ndof = int(rng.choice([6, 7, 12]))
        J = rng.normal(0, 1, (3 * nc, ndof))
        if t % 2 == 0:
            J[3:6] = J[0:3] + (0.0 if t % 4 == 0 else 1.0) * rng.normal(0, 1, (1, ndof))     # a repeated contact / a contact one direction away
        M = J @ np.diag(rng.uniform(0.1, 2, ndof)) @ J.T
        mats.append(0.5 * (M + M.T)); ranks.append(int(np.linalg.matrix_rank(J)))
    count = len(mats)
    Q = np.zeros((count, R, R)); size = np.zeros(count, np.int32)
    for t, M in enumerate(mats):
        Q[t, :len(M), :len(M)] = M; size[t] = len(M)
    vp = lambda a: C.c_void_p(a.ctypes.data)
    for route in (0, 1):
        P = np.zeros_like(Q); r = np.zeros(count, np.int32)
        check(lib().nbl_selftest_pinv_rows(count, R, vp(Q), vp(size), route, vp(P), vp(r), 1, None), "nbl_selftest_pinv_rows")
        assert np.array_equal(r, np.array(ranks)), (route, np.where(r != np.array(ranks))[0][:10])
        for t in (0, 1, 2, 3):
            sv = np.linalg.svd(Q[t], compute_uv=False)
            ref = np.linalg.pinv(Q[t], rcond=0.5 * sv[ranks[t] - 1] / sv[0])
            assert np.abs(P[t] - ref).max() <= 1e-9 * np.abs(ref).max(), (route, t)


# trials of the generator per build: enough for >= 200 / >= 64 accepted matrices; every third trial draws a small clamping set, so that
# Q has full rank (at most 12 independent rows exist on two 6-DOF bodies) and the full-rank completion of the route occurs too
HH_TRIALS = {24: (260, 130, (0.7, 0.2, 0.1)), 48: (72, 72, (0.82, 0.12, 0.06))}


@pytest.mark.parametrize("R", [24, 48])
def test_device_householder_route_on_contact_matrices_with_friction_rows_on_their_bound(R):
    """coopPinv ON THE DEVICE on the matrices it is there for (tests/test_coop_host.py has the same generator on the host build):
    Q = A(c, c) + A(c, u) E of a standing robot, friction rows on their bound folded into their normal's column - non-symmetric, cond <= 1e8.
    Rank exact, Q^+ within 500 cond(Q) eps of numpy's pseudo-inverse; both completions (rank = rows of the clamping set / rank below it)
    occur; and the same matrices through the host build of the same header."""
    from nimblephysics_amd._lib import check, lib
    from test_coop_host import _build_shim, _p
    from util import friction_bound_contact_matrices
    rng = np.random.default_rng(110 + R)
    dense, sparse, p_sparse = HH_TRIALS[R]
    cases = list(friction_bound_contact_matrices(rng, R, dense)) + list(friction_bound_contact_matrices(rng, R, sparse, p_cls=p_sparse))
    count = len(cases)
    assert count >= (200 if R == 24 else 64), count
    assert count <= 768
    Q = np.ascontiguousarray(np.stack([c[1] for c in cases])); size = np.array([c[2] for c in cases], np.int32)
    assert np.abs(Q - Q.transpose(0, 2, 1)).max(axis=(1, 2)).astype(bool).sum() >= count // 2       # the route's own input: not symmetric
    vp = lambda a: C.c_void_p(a.ctypes.data)
    P = np.zeros_like(Q); r = np.zeros(count, np.int32)
    check(lib().nbl_selftest_pinv_rows(count, R, vp(Q), vp(size), 0, vp(P), vp(r), 1, None), "nbl_selftest_pinv_rows")
    shim = _build_shim(R // 3)
    full = deficient = 0
    worst = worst_host = 0.0
    for t, (_, Qt, ncl, k, cond) in enumerate(cases):
        assert r[t] == k, (t, r[t], k, ncl)
        full += int(k == ncl); deficient += int(k < ncl)
        ref = np.linalg.pinv(Qt, rcond=0.5 / cond)
        scale = np.abs(ref).max()
        e = np.abs(P[t] - ref).max() / scale
        worst = max(worst, e / (cond * 2.2e-16))
        assert e <= 500 * cond * 2.2e-16, (t, e, cond, k, ncl)
        Ph = np.zeros((R, R))
        assert shim.shim_coop_pinv(_p(np.ascontiguousarray(Qt)), ncl, _p(Ph)) == k, (t, k)
        eh = np.abs(P[t] - Ph).max() / scale
        worst_host = max(worst_host, eh / (cond * 2.2e-16))
        assert eh <= 500 * cond * 2.2e-16, (t, eh, cond)          # (both are within the bound of numpy's: at most twice it from each other; held to once)
    print(f"Householder route on the device, R = {R}: {count} matrices, {full} of full rank, {deficient} rank-deficient; worst error in units of cond(Q) eps: "
          f"against numpy {worst:.3g}, against the host build {worst_host:.3g}")
    assert full >= 10 and deficient >= 10, (full, deficient)
