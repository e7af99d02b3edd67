"""Rows with FIXED finite bounds and findex -1 (joint Coulomb friction: [-f dt, f dt]) and joint-limit rows ON THE GPU, at the level of the
LCP: the three Dantzig drivers (24-row, 48-row, general) through nbl_selftest_lcp_dantzig against the reference's own dSolveLCP
(oracle/_ref) bit for bit, and the general cascade with such slots (nbl_selftest_lcp_cascade_rows: the JF = true instantiation of
gen_lcp_dev.hpp / gen_dantzig_dev.hpp) against the same source compiled for the host (tests/host_shim/gen_shim.cpp), which
tests/test_gen_host.py holds to the reference's LCPUtils, dSolveLCP and the oracle's cascade.  Reads nothing outside the tree."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


# compacted rows -> contacts + box rows: 9 and 38 run the 24- and the 48-row driver (the same interface and statement of dSolveLCP),
# 52, 66 and 140 genDantzigPar of the general instantiation
@pytest.mark.parametrize("nc,nb", [(2, 3), (8, 14), (14, 10), (20, 6), (40, 20)])
def test_device_dantzig_with_fixed_bound_rows_is_bit_identical_to_the_reference(nc, nb):
    """128 problems per size, one launch: success flag equal, x bit for bit.  A third of the problems has a rank-deficient A.  Counted on
    the reference's results, so that the test cannot pass without them: at least 10 solved problems with a box row strictly inside its
    bounds, at least 10 with one on a bound, both bounds, at least one early exit."""
    import oracle
    from nimblephysics_amd._lib import check, lib
    from util import boxed_lcp, have_ref, slots_lcp
    if not have_ref():
        pytest.skip("oracle/_ref not built")
    OL = oracle._lib()
    rng = np.random.default_rng(1000 * nc + nb)
    count, n = 128, 3 * nc + nb
    probs = []
    for k in range(count):
        ndof = nb + int(rng.choice([0, 3, 6, 10])) if k % 3 == 1 else n + int(rng.integers(0, 6))
        P = boxed_lcp(rng, nc, nb, ndof)
        if k % 4 == 1:
            P = slots_lcp(P.A, np.where(np.arange(len(P.b)) < 3 * nc, np.abs(P.b), P.b), P.mu, P.bound, P.lim)      # contacts pressed: long factor, many removals
        probs.append(P)
    A = np.ascontiguousarray(np.stack([p.A_ref for p in probs])); b = np.ascontiguousarray(np.stack([p.b_ref for p in probs]))
    lo = np.ascontiguousarray(np.stack([p.lo_ref for p in probs])); hi = np.ascontiguousarray(np.stack([p.hi_ref for p in probs]))
    fi = np.ascontiguousarray(np.stack([p.findex_ref for p in probs]).astype(np.int32))
    assert A.shape == (count, n, n)
    x = np.zeros((count, n)); rc = np.zeros(count, np.int32)
    check(lib().nbl_selftest_lcp_dantzig(count, n, _vp(A), _vp(b), _vp(lo), _vp(hi), _vp(fi), _vp(x), _vp(rc)), "nbl_selftest_lcp_dantzig")
    solved = failed = inside = on_lo = on_hi = 0
    box = np.arange(3 * nc, n)
    for i in range(count):
        xr = np.zeros(n)
        okr = OL.nbo_lcp_dantzig(n, A[i].ctypes.data_as(pd), xr.ctypes.data_as(pd), b[i].copy().ctypes.data_as(pd), lo[i].copy().ctypes.data_as(pd),
                                 hi[i].copy().ctypes.data_as(pd), fi[i].copy().ctypes.data_as(pi), 1)
        if rc[i] == -1:
            assert okr == 0 or not np.all(np.isfinite(xr)), (i, okr)
            continue
        assert okr == rc[i], (i, okr, rc[i])
        if okr == 1:
            solved += 1
            assert np.array_equal(xr, x[i]), (i, np.abs(xr - x[i]).max())
            beta = hi[i][box]
            inside += bool((np.abs(xr[box]) < beta).any()); on_lo += bool((xr[box] == -beta).any()); on_hi += bool((xr[box] == beta).any())
        else:
            failed += 1
    print(f"[device Dantzig, {nc} contacts + {nb} box rows = {n} rows] {solved} solved bit for bit, {failed} early exits; problems with a box row "
          f"strictly inside its bounds {inside}, on its lower bound {on_lo}, on its upper bound {on_hi}")
    assert inside >= 10 and on_lo + on_hi >= 10 and on_lo > 0 and on_hi > 0 and failed >= 1, (solved, failed, inside, on_lo, on_hi)


# contacts + box + limit slots (and whether a constrained-group mask is drawn); 20 + 6 + 2 is the one whose compacted problem has more than
# 64 rows (70): the Gauss-Seidel of stages 2 and 3 then leaves genPgsHeld1 for genPgsHeld<NT>
MIXES = [(0, 3, 0, False), (2, 3, 0, False), (2, 3, 2, False), (8, 14, 0, False), (20, 6, 2, False), (6, 5, 2, True)]


def _mix_problems(rng, nc, nb, nl, masked, count=4):
    from util import boxed_lcp, slots_lcp
    out = []
    for k in range(count):
        ndof = max(nb + nl, int(rng.choice([3, 6, 12, 30]))) if k % 2 else 3 * nc + nb + nl + 2
        P = boxed_lcp(rng, nc, nb, ndof, nl)
        mask = None
        if masked:
            on = rng.random(nc + nb + nl) < 0.6
            on[nc] = True                                              # (a box slot in the group at hand)
            mask = on.repeat(3).astype(np.uint8)
            P = slots_lcp(P.A * np.equal.outer(mask, mask), P.b, P.mu, P.bound, P.lim)      # block structure of two constrained groups
        out.append((P, mask))
    return out


def test_the_general_cascade_with_box_and_limit_slots_on_the_device_equals_the_same_code_on_the_host():
    """nbl_selftest_lcp_cascade_rows (any bound > 0: the JF = true kernel) against gshim_stage0_jf + gshim_cascade_jf, the same source on
    one lane: stage bits and cfm equal, row classes equal, x within 1e-8 relative (the tolerance of the neighbouring test without such
    slots, tests/test_gpu_general.py).  Six slot mixes, four problems and one launch each; every one of stages 1, 2 and 3 is reached.
    Where oracle/_ref is there, the device's standardised x must also be a solution for the reference's own isLCPSolutionValid."""
    import os
    import oracle
    from nimblephysics_amd import _lib
    from test_gen_host import CFM, REF_LCPUTILS, _build_gen_shim, _gen_stage0_then_cascade_jf
    G = _build_gen_shim(64)
    L = _lib.lib()
    R = C.CDLL(REF_LCPUTILS) if os.path.exists(REF_LCPUTILS) else None
    rng = np.random.default_rng(12)
    stages = {}
    worst = 0.0
    n_probs = n_ref_checked = 0
    for nc, nb, nl, masked in MIXES:
        probs = _mix_problems(rng, nc, nb, nl, masked)
        count, m = len(probs), 3 * (nc + nb + nl)
        A = np.ascontiguousarray(np.stack([p.A for p, _ in probs])); b = np.ascontiguousarray(np.stack([p.b for p, _ in probs]))
        mu = np.ascontiguousarray(np.stack([p.mu for p, _ in probs])); bound = np.ascontiguousarray(np.stack([p.bound for p, _ in probs]))
        lim = np.ascontiguousarray(np.stack([p.lim for p, _ in probs]).astype(np.uint8))
        on = np.ascontiguousarray(np.stack([mk for _, mk in probs])) if masked else None
        Xd = np.zeros((count, m)); cd = np.zeros((count, m), np.int32); std = np.zeros(count, np.uint32); cfmd = np.zeros(count)
        rc = L.nbl_selftest_lcp_cascade_rows(count, m, _vp(A), _vp(b), _vp(mu), _vp(bound), _vp(lim), 0, None, _vp(on), CFM, _vp(Xd), _vp(cd), _vp(std), _vp(cfmd))
        assert rc == 0, L.nbl_last_error()
        for k, (P, mask) in enumerate(probs):
            name = (nc, nb, nl, k)
            Xh, sth, cfmh, ch, _ = _gen_stage0_then_cascade_jf(G, P, mask)
            if mask is not None:
                ch = ch * mask
            n_probs += 1
            stages[int(std[k])] = stages.get(int(std[k]), 0) + 1
            assert int(std[k]) == sth, (name, hex(int(std[k])), hex(sth))
            assert cfmd[k] == cfmh, (name, cfmd[k], cfmh)
            assert np.array_equal(cd[k], ch), (name, "row classes", np.where(cd[k] != ch)[0][:10])
            err = np.abs(Xd[k] - Xh).max() / max(1.0, np.abs(Xh).max())
            worst = max(worst, err)
            assert err < 1e-8, (name, err)
            if R is not None and (int(std[k]) & 0x100):
                keep = np.array([i for i, r in enumerate(P.rows) if mask is None or mask[r]])
                rows = P.rows[keep]; n = len(rows)
                pos = {int(i): j for j, i in enumerate(keep)}
                fr = np.array([-1 if f < 0 else pos[int(f)] for f in P.findex_ref[keep]], dtype=np.int32)
                Ac = np.ascontiguousarray(P.A_ref[np.ix_(keep, keep)] + cfmd[k] * np.eye(n))
                xr = np.ascontiguousarray(P.s_ref[keep] * Xd[k][rows])
                okv = R.ref_lcp_valid(n, Ac.ctypes.data_as(pd), xr.ctypes.data_as(pd), np.ascontiguousarray(P.b_ref[keep]).ctypes.data_as(pd),
                                      np.ascontiguousarray(P.hi_ref[keep]).ctypes.data_as(pd), np.ascontiguousarray(P.lo_ref[keep]).ctypes.data_as(pd),
                                      fr.ctypes.data_as(pi), int(bool(int(std[k]) & 0x10)))
                assert okv, (name, "the device's standardised x is not a solution for the reference")
                n_ref_checked += 1
    print(f"[general cascade with box and limit slots, device vs host] {n_probs} problems, stages {{{', '.join(f'{hex(k)}: {v}' for k, v in stages.items())}}}, "
          f"worst x difference {worst:.1e}, standardised results accepted by the reference {n_ref_checked}")
    assert all(any(s & bit for s in stages) for bit in (0x4, 0x8, 0x10)), stages
