"""Stage 0 of the LCP cascade and its standardisation loop ON THE GPU, one world per wavefront, through nbl_selftest_stage0_rows
(coopClassify -> coopBuildQ -> coopPinvOfQ -> coopPinvApply -> coopValid; csrc/coop_dev.hpp), for the 24-row and the 48-row build, against
the host build of the same header (tests/host_shim/coop_shim.cpp: shim_coop_stage0_rows) and against the oracle's restatement of
LCPUtils::isLCPSolutionValid (pinned to the reference bit for bit: tests/test_oracle_ref_lcputils.py).

Device against host build: the row classes, E and the ok word are EQUAL and x is within 500 cond(Q) eps of the final clamping block (the
bound of tests/test_gpu_pinv_selftest.py: x = Q^+ b).  The two builds differ in the last bits (matrix cores and fused multiply-adds on the
device, neither on the host), so a problem whose host-build classification changes under +-1-ulp perturbations of b (16 draws, on the CPU,
cached per build) is left out of the equality; at most 3 % of the problems may be."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import oracle
from test_coop_host import _build_shim
from util import contact_lcp

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.220446049250313e-16
pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
CASES = ("friction row on its bound", "cfm 0", "cfm 1e-4", "one limit row", "two limit rows", "masked group", "warm start")
N_RANDOM, PER_CASE, N_PERTURB, MAX_UNSTABLE_SHARE = 256, 16, 16, 0.03


def _p(a):
    return a.ctypes.data_as(pd)


def _problem(R):
    return {"A": np.zeros((R, R)), "b": np.zeros(R), "mu": np.zeros(R // 3), "mask": 0, "lim": 0, "neg": 0, "cfm": 0.0, "have": 0, "xc": np.zeros(R), "tags": set()}


def fixture_problems(R):
    """the A, b, mu problems of tests/golden/lcp_fixtures.json that fit (whole frictional contacts, at most R rows), from the fixture's x and cold"""
    fix = json.load(open(os.path.join(HERE, "golden", "lcp_fixtures.json")))
    out = []
    for name in sorted(fix):
        f = fix[name]
        n = len(f["b"])
        fi, hi = np.array(f["fIndex"]), np.array(f["hi"], dtype=np.float64)
        if n % 3 or n > R or not (np.all(fi[0::3] == -1) and np.all(fi[1::3] == np.arange(0, n, 3)) and np.all(fi[2::3] == np.arange(0, n, 3))):
            continue
        for warm in (0, 1):
            p = _problem(R)
            p["A"][:n, :n] = np.array(f["A"], dtype=np.float64).reshape(n, n); p["b"][:n] = f["b"]; p["mu"][:n // 3] = hi[1::3]
            p["mask"] = (1 << n) - 1
            p["have"] = warm
            if warm:
                p["xc"][:n] = f.get("x", np.zeros(n))
            p["tags"] = {"fixture " + name}
            out.append(p)
    return out


def random_problems(R, count=N_RANDOM, seed=5):
    """Standing-robot problems from contact_lcp (tests/util.py: A = J D J^T of up to R / 3 frictional contacts on 6, 12 or 3 nc + 3 DOFs), b = A xs
    for a resting / sliding xs (+ noise), biased so that every case of CASES is drawn often: cfm 1e-4 (the loop alone on a perturbed xs, as
    after stages 2 / 3), one or two joint-limit rows (a row of their own contact slot with empty tangent rows, as the device carries them;
    the second one negated), a second constrained group that is masked out, a warm start."""
    rng = np.random.default_rng(seed + R)
    NC = R // 3
    out = []
    for t in range(count):
        p = _problem(R)
        kind = t % 8
        n_lim = {3: 1, 4: 2}.get(kind, 0)
        two_groups = kind == 5
        nc = int(rng.integers(2 if n_lim else 1, (NC // 2 if two_groups else NC) + 1)); n = 3 * nc
        A, b, lo, hi, fi = contact_lcp(rng, nc, int(rng.choice([6, 12, n + 3])))
        A = np.tril(A) + np.tril(A, -1).T
        mu = hi[1::3].copy()
        lim_rows = [3 * (nc - 1 - j) for j in range(n_lim)]
        for r in lim_rows:                                   # a joint-limit constraint: one row, no tangent rows
            A[r + 1:r + 3, :] = 0; A[:, r + 1:r + 3] = 0; mu[r // 3] = 0.0
            p["lim"] |= 1 << r
        xs = np.zeros(n)
        for c in range(nc):
            if rng.random() < 0.75:
                xs[3 * c] = rng.uniform(0.1, 2)
                xs[3 * c + 1:3 * c + 3] = rng.uniform(-0.5, 0.5, 2) * mu[c] * xs[3 * c]
                if mu[c] and rng.random() < 0.5:             # sliding: one friction row on its bound
                    xs[3 * c + 1 + int(rng.integers(0, 2))] = rng.choice([-1, 1]) * mu[c] * xs[3 * c]
        cfm = 1e-4 if kind in (1, 6) else 0.0
        bb = A @ xs + cfm * xs
        if t % 3 == 1:
            bb += rng.normal(0, 0.02, n)
        if len(lim_rows) == 2:                               # the second limit row is carried negated (an upper limit): the device's form of A, b
            r = lim_rows[1]
            p["neg"] |= 1 << r
        p["A"][:n, :n] = A; p["b"][:n] = bb; p["mu"][:nc] = mu
        p["mask"] = (1 << n) - 1
        if two_groups:                                       # a second group behind it, switched off
            nc2 = int(rng.integers(1, NC - nc + 1)); n2 = 3 * nc2
            A2, b2, _, hi2, _ = contact_lcp(rng, nc2, 6)
            p["A"][n:n + n2, n:n + n2] = np.tril(A2) + np.tril(A2, -1).T; p["b"][n:n + n2] = b2; p["mu"][nc:nc + nc2] = hi2[1::3]
            if t % 16 == 5:                                  # ... or in front of it
                p["mask"] = ((1 << n2) - 1) << n
            p["tags"].add("masked group")
        if cfm or kind == 2 or kind == 7:
            p["have"] = 1
            p["xc"][:n] = xs * (1.0 + rng.normal(0, 1e-4, n)) + (rng.normal(0, 1e-3, n) if kind == 7 else 0.0)
            p["tags"].add("warm start")
        p["cfm"] = cfm
        p["tags"].add("random")
        p["tags"].add("cfm 1e-4" if cfm else "cfm 0")
        if n_lim:
            p["tags"].add("one limit row" if n_lim == 1 else "two limit rows")
        out.append(p)
    return out


def replay_problems(R):
    """The worlds of the smoke / kinematics batches that the red runs of those checks named, as the device saw them:
    tests/golden/smoke_layers.npz holds their A, b, mu and m of the 24-row build, the warm start (have_cache = 0 and a zero x_cache: both
    checks take a cold first step) and the state inputs s, a they come from.  At most 16; the 48-row build has none.
    All of them leave stage 0 (that is why the red runs named them: a degraded oracle differs on such worlds only), so what the replay pins
    at kernel level is that stage 0 rejects them on both builds, with the same pre-solve classes and E at the rejection; their way through
    stages 1 - 3 is held by tests/test_gpu_smoke_layers.py (the solve layer of the whole batches)."""
    if R != 24:
        return []
    path = os.path.join(HERE, "golden", "smoke_layers.npz")
    assert os.path.exists(path), path
    z = np.load(path)
    assert 1 <= len(z["A"]) <= 16, len(z["A"])
    out = []
    for i in range(len(z["A"])):
        p = _problem(R)
        m = int(z["m"][i])
        p["A"][:] = z["A"][i].reshape(R, R); p["b"][:] = z["b"][i]; p["mu"][:] = z["mu"][i]; p["mask"] = (1 << m) - 1
        p["have"] = int(z["have_cache"][i]); p["xc"][:] = z["x_cache"][i]
        p["tags"] = {"replay"}
        out.append(p)
    return out


def _pack(problems, R):
    u64 = lambda k: np.array([p[k] for p in problems], dtype=np.uint64)
    return {"A": np.ascontiguousarray(np.stack([p["A"] for p in problems])), "b": np.ascontiguousarray(np.stack([p["b"] for p in problems])),
            "mu": np.ascontiguousarray(np.stack([p["mu"] for p in problems])), "mask": u64("mask"), "lim": u64("lim"), "neg": u64("neg"),
            "cfm": np.array([p["cfm"] for p in problems]), "have": np.array([p["have"] for p in problems], np.int32),
            "xc": np.ascontiguousarray(np.stack([p["xc"] for p in problems]))}


def host_stage0(shim, p, b=None):
    R = shim.R
    X = np.zeros(R); X0 = np.zeros(R); cls = np.zeros(R, np.int32); E = np.zeros(R); P = np.zeros((R, R))
    shim.shim_coop_stage0_rows.argtypes = [pd, pd, pd, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, C.c_int, pd, pd, pd, pi, pd, pd]
    ok = shim.shim_coop_stage0_rows(_p(np.ascontiguousarray(p["A"])), _p(np.ascontiguousarray(p["b"] if b is None else b)), _p(p["mu"]), p["mask"], p["lim"], p["neg"],
                                    p["cfm"], p["have"], _p(p["xc"]), _p(X), _p(X0), cls.ctypes.data_as(pi), _p(E), _p(P))
    return {"X": X, "X0": X0, "cls": cls, "E": E, "ok": ok, "P": P}


def unstable_under_one_ulp(shim, p, host, rng, draws=N_PERTURB):
    """the host build's verdict, classes or E change under +-1-ulp perturbations of b"""
    for _ in range(draws):
        h = host_stage0(shim, p, p["b"] * (1.0 + rng.integers(-1, 2, p["b"].shape) * EPS))
        if h["ok"] != host["ok"] or not np.array_equal(h["cls"], host["cls"]) or not np.array_equal(h["E"], host["E"]):
            return True
    return False


def clamping_cond(p, cls, E):
    """cond of the final clamping block Q = A(c, c) + A(c, u) E + cfm I over its numerical rank (the rank rule of friction_bound_contact_matrices)"""
    cl = np.where(cls == 1)[0]
    if len(cl) == 0:
        return 1.0
    Q = p["A"][np.ix_(cl, cl)] + p["cfm"] * np.eye(len(cl))
    for u in np.where(cls == 2)[0]:
        nrm = u - u % 3
        if cls[nrm] == 1:
            Q[:, list(cl).index(nrm)] += E[u] * p["A"][cl, u]
    sv = np.linalg.svd(Q, compute_uv=False)
    k = int((sv > 1e-12 * sv[0]).sum())
    return float(sv[0] / sv[k - 1])


def oracle_valid(p, x):
    """LCPUtils::isLCPSolutionValid (the oracle's restatement) on the rows of the constrained group at hand, A + cfm I as the solver that ended
    with that cfm sees it; a negated limit row is a plain row of the device's form of the problem"""
    rows = [r for r in range(len(x)) if (p["mask"] >> r) & 1]
    n = len(rows)
    A = np.ascontiguousarray(p["A"][np.ix_(rows, rows)] + p["cfm"] * np.eye(n)); b = np.ascontiguousarray(p["b"][rows]); xx = np.ascontiguousarray(x[rows])
    lo = np.zeros(n); hi = np.full(n, np.inf); fi = np.full(n, -1, np.int32)
    for j, r in enumerate(rows):
        if r % 3:
            lo[j], hi[j], fi[j] = -p["mu"][r // 3], p["mu"][r // 3], rows.index(r - r % 3)
    return bool(oracle._lib().nbo_lcp_valid(n, _p(A), _p(xx), _p(b), _p(lo), _p(hi), fi.ctypes.data_as(pi), 0))


_cache = {}


def host_results(R):
    """(problems, host-build results, 1-ulp-unstable flags) of one build: computed once per module"""
    if R not in _cache:
        shim = _build_shim(R // 3)
        problems = fixture_problems(R) + random_problems(R) + replay_problems(R)
        host = [host_stage0(shim, p) for p in problems]
        rng = np.random.default_rng(99)
        unstable = np.array([unstable_under_one_ulp(shim, p, h, rng) for p, h in zip(problems, host)])
        for p, h in zip(problems, host):
            if h["ok"] & 1 and (h["cls"] == 2).any():
                p["tags"].add("friction row on its bound")
        _cache[R] = (problems, host, unstable)
    return _cache[R]


@pytest.mark.parametrize("R", [24, 48])
def test_the_problem_set_covers_every_case(R):
    """(no GPU needed) >= 16 instances of every case among the random problems, fixtures present, the unstable share under the cap"""
    problems, host, unstable = host_results(R)
    counts = {c: sum(c in p["tags"] for p in problems if "random" in p["tags"]) for c in CASES}     # over the 256 random problems only
    assert sum("random" in p["tags"] for p in problems) == N_RANDOM
    assert sum("replay" in p["tags"] for p in problems) == (len(np.load(os.path.join(HERE, "golden", "smoke_layers.npz"))["A"]) if R == 24 else 0)
    print(f"[stage-0 self-test, R = {R}] {len(problems)} problems; cases:", counts, "; host build accepts", sum(h['ok'] & 1 for h in host),
          "; 1-ulp-unstable:", int(unstable.sum()))
    for c in CASES:
        assert counts[c] >= PER_CASE, (c, counts)
    assert sum(any(t.startswith("fixture") for t in p["tags"]) for p in problems) >= 2
    assert len(problems) <= 768
    assert unstable.sum() <= MAX_UNSTABLE_SHARE * len(problems), (int(unstable.sum()), len(problems))
    assert sum(h["ok"] & 1 for h in host) >= len(problems) // 4


@pytest.mark.gpu
@pytest.mark.parametrize("R", [24, 48])
def test_device_stage0_equals_the_host_build_and_its_accepted_solutions_are_valid(R):
    from nimblephysics_amd._lib import check, lib
    problems, host, unstable = host_results(R)
    count = len(problems)
    a = _pack(problems, R)
    X = np.zeros((count, R)); X0 = np.zeros((count, R)); cls = np.zeros((count, R), np.int32); E = np.zeros((count, R)); ok = np.zeros(count, np.int32)
    P = np.zeros((count, R, R))
    vp = lambda v: C.c_void_p(v.ctypes.data)
    check(lib().nbl_selftest_stage0_rows(count, R, vp(a["A"]), vp(a["b"]), vp(a["mu"]), vp(a["mask"]), vp(a["lim"]), vp(a["neg"]), vp(a["cfm"]), vp(a["have"]),
                                         vp(a["xc"]), vp(X), vp(X0), vp(cls), vp(E), vp(ok), vp(P)), "nbl_selftest_stage0_rows")
    assert unstable.sum() <= MAX_UNSTABLE_SHARE * count
    differ, wrong_x, invalid = [], [], []
    worst = 0.0
    for t, (p, h) in enumerate(zip(problems, host)):
        same = ok[t] == h["ok"] and np.array_equal(cls[t], h["cls"]) and np.array_equal(E[t], h["E"])
        if ok[t] & 1 and not oracle_valid(p, X[t]):
            invalid.append(t)
        if unstable[t]:
            continue
        if not same:
            differ.append(t)
            continue
        if ok[t] & 1:
            bound = 500 * clamping_cond(p, h["cls"], h["E"]) * EPS
            e = np.abs(X[t] - h["X"]).max() / max(np.abs(h["X"]).max(), 1e-300)
            worst = max(worst, e / bound)
            if e > bound:
                wrong_x.append((t, e, bound))
            if ok[t] & 2:
                ep = np.abs(P[t] - h["P"]).max() / max(np.abs(h["P"]).max(), 1e-300)
                if ep > bound:
                    wrong_x.append((t, ep, bound, "pinv"))
    print(f"[stage-0 self-test, R = {R}] {count} problems, device accepts {int((ok & 1).sum())}, 1-ulp-unstable (left out of the equality) {int(unstable.sum())}; "
          f"cls / E / ok differ on {differ}; x beyond the bound on {wrong_x}; accepted but invalid on {invalid}; worst x error / bound {worst:.3g}")
    assert not differ, ("cls, E or ok differ from the host build", [(t, sorted(problems[t]["tags"])) for t in differ[:8]], len(differ))
    assert not wrong_x, ("x differs from the host build beyond 500 cond(Q) eps", wrong_x[:8], len(wrong_x))
    assert not invalid, ("an accepted x fails isLCPSolutionValid", [(t, sorted(problems[t]["tags"])) for t in invalid[:8]], len(invalid))
