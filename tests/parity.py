"""Shared parity criterion of the GPU tests: every world within `tol` of the oracle, or PROOF that the reference algorithm has no
stable answer on that world (tests/test_gpu_contact.py states the reasoning).  Test infrastructure.

The error norm is PER WORLD AND PER BLOCK: the next state splits into q' and v', the state gradient into the position
and the velocity cotangent, the action gradient is one block; an entry's error is measured against the magnitude of ITS block in ITS
world of the reference (max |.| over the block), with a floor of FLOOR x the batch-wide magnitude of that block so that a block that
happens to be ~0 in one world is not held to an absolute accuracy nothing has.  (Round 3 divided by the batch-wide maximum of the
whole output: velocities of 1e-2 next to q0 = pi/2 were held to 1.6e-5 of themselves at tol 1e-7.)"""
import numpy as np

KEYS = ("next", "grad_state", "grad_action")
EPS = 2.220446049250313e-16
FLOOR = 1e-2


def _blocks(key, dim):
    """index ranges of the blocks of one output: next = [q'; v'], grad_state = [dL/dq; dL/dv], grad_action = one block"""
    if key == "grad_action" or dim % 2:
        return [(0, dim)]
    return [(0, dim // 2), (dim // 2, dim)]


def entry_scales(ref):
    """-> {key: [B, dim] array}: for every entry the magnitude it is measured against (its world's block of the reference, floored)."""
    out = {}
    for k in KEYS:
        r = np.abs(np.asarray(ref[k]))
        sc = np.empty_like(r)
        for lo, hi in _blocks(k, r.shape[1]):
            if hi <= lo:
                continue
            per_world = r[:, lo:hi].max(1)
            floor = max(FLOOR * float(per_world.max()), 1e-30)
            sc[:, lo:hi] = np.maximum(per_world, floor)[:, None]
        out[k] = sc
    return out


def block_errors(x, ref, nblocks=1):
    """The same norm for one array [B, dim] split into `nblocks` equal blocks: per world, max over its entries of |x - ref| / (the
    magnitude of the entry's block in that world of `ref`, floored at FLOOR x the batch-wide magnitude of the block)."""
    x, ref = np.asarray(x), np.asarray(ref)
    B, dim = ref.shape
    out = np.zeros(B)
    w = dim // nblocks
    for b in range(nblocks):
        lo, hi = b * w, (dim if b == nblocks - 1 else (b + 1) * w)
        pw = np.abs(ref[:, lo:hi]).max(1)
        sc = np.maximum(pw, max(FLOOR * float(pw.max()), 1e-30))
        out = np.maximum(out, np.abs(x[:, lo:hi] - ref[:, lo:hi]).max(1) / sc)
    return out


def world_errors(dev, ref):
    """Per-world error of every output: max over its entries of |dev - ref| / (the entry's block magnitude in that world, floored).
    -> ({key: [B]}, {key: [B, dim] entry scales})."""
    scales = entry_scales(ref)
    return {k: (np.abs(dev[k] - ref[k]) / scales[k]).max(1) if dev[k].shape[1] else np.zeros(len(dev[k])) for k in KEYS}, scales


def log_map_gap(md, next_state):
    """Per world: how far the NEXT rotation angle of its exponential-map joints (free, ball) is from pi (inf without such joints).  The
    reference finite-differences the position integration of those joints (central differences, eps 1e-6: FreeJoint.cpp:950-1007,
    BallJoint.cpp:351-408; the oracle restates that) and its posPos / velPos blocks lose digits like 1 / gap^2 towards the log-map
    singularity; the device differentiates exactly (tests/test_gpu_ball_joint.py pins it against 80-bit arithmetic)."""
    next_state = np.asarray(next_state)
    gap = np.full(len(next_state), np.inf)
    off = 0
    for b in md.bodies:
        nd = {"free": 6, "weld": 0, "ball": 3}.get(b.joint_type, 1)
        if b.joint_type in ("free", "ball"):
            gap = np.minimum(gap, np.abs(np.linalg.norm(next_state[:, off:off + 3], axis=1) - np.pi))
        off += nd
    return gap


FD_GAP = 0.3             # within this distance of the log-map singularity the reference's finite differences (off by 1e-9 / gap^2, at worst 4 x that) come
                         # within a factor two of the 1e-7 every world is held to
DBL_COEF, DBL_CAP = 32 * EPS, 1e-3


def gradient_tolerance(md, next_state, tol):
    """Per-world tolerance of the STATE-gradient blocks against the oracle WITH its exact-derivative instrument (see below): `tol`, except
    where the next rotation angle of a free / ball joint is within a few 1e-3 rad of pi - there ANY double-precision evaluation of the
    analytic derivative of logMap(R exp(w dt)) cancels two O(1 / gap) terms into an O(1) result and is good to ~eps / gap^3 only: the
    oracle's own instrument evaluated in doubles is off by up to 19 eps / gap^3 (median 2) from its extended-precision evaluation
    (oracle.set_exact_position_jacobians(doubles=True); 400 cfg4 worlds with gaps 3e-4 .. 5e-2), the device's reverse mode by
    1.7e-7 at gap = 2e-3 (6 eps / gap^3) from an 80-bit stencil.  Held to max(tol, 32 eps / gap^3): 1e-7 from gap = 4.1e-3 on.

    History: until round 4 this function waived 5e-9 / gap^2 within 0.15 rad of pi, on the ARGUMENT that the reference's central-difference
    Jacobians (FreeJoint.cpp:950-1007, BallJoint.cpp:351-408, restated literally in the oracle) are the inaccurate side.  Now the oracle
    carries an exact-derivative switch (oracle/dynamics.hpp::posJacobiansExact, pinned against an 80-bit stencil on the CPU:
    tests/test_oracle_exact_pos_jacobians.py) and the argument is a TEST: tests/test_gpu_contact.py::test_cfg4_box_stack_8192_worlds
    shows the cfg4 worlds that miss 1e-7 against the finite-difference oracle collapse to the tolerance above with the switch on, and
    that the reported errors (1e-3 at worst) reappear with it off."""
    gap = log_map_gap(md, next_state)
    with np.errstate(divide="ignore"):
        dbl = np.minimum(DBL_COEF / np.maximum(gap, 1e-12) ** 3, DBL_CAP)
    return np.maximum(tol, dbl)


def exact_reference_near_the_singularity(ow, md, s, a, g, ref, lcp=None, lcp_len=None):
    """ref with the gradients of the worlds within FD_GAP of the log-map singularity of a free / ball joint replaced by the oracle's
    result WITH its exact-derivative instrument (the forward pass - next state, status - does not depend on it).  Returns (ref', mask of
    those worlds, their largest state-gradient difference between the two modes: the size of the reference's finite-difference error)."""
    near = log_map_gap(md, ref["next"]) < FD_GAP
    if not near.any():
        return ref, near, 0.0
    kw = {}
    if lcp is not None:
        kw = {"lcp_in": lcp[near], "lcp_len_in": lcp_len[near]}
    ow.set_exact_position_jacobians(True)
    try:
        rex = ow.step_batch(s[near], a[near], g[near], threads=8, **kw)
    finally:
        ow.set_exact_position_jacobians(False)
    out = dict(ref)
    fd_err = 0.0
    for k in ("grad_state", "grad_action"):
        out[k] = np.array(ref[k], copy=True)
        if k == "grad_state" and out[k].shape[1]:
            sc = np.maximum(np.abs(rex[k]).max(1), 1e-300)
            fd_err = float((np.abs(rex[k] - out[k][near]).max(1) / sc).max())
        out[k][near] = rex[k]
    return out, near, fd_err


ORACLE_WITHOUT_REFERENCE_SOLVER = 0x80000000      # oracle/contact.hpp: stage 1 could not load oracle/_ref/libodelcp_ref.so


def assert_reference_solver_present(tag, ref):
    """The oracle's stage 1 IS the reference's own Dantzig solver, compiled into oracle/_ref by build().  Without that library the oracle
    treats stage 1 as failed on every world that leaves stage 0 and answers with the PGS fallback: not the reference's result, and
    stable under perturbations - so such a world reads "the reference is stable here but the device differs" (smoke() part 1: world 84
    with 0.265; the kinematics case: world 15).  The oracle flags those worlds; a flagged reference judges nothing."""
    if isinstance(ref, dict) and "status" in ref:
        flagged = np.where(np.asarray(ref["status"]).astype(np.uint32) & ORACLE_WITHOUT_REFERENCE_SOLVER)[0]
        assert len(flagged) == 0, (tag, "the oracle ran without oracle/_ref/libodelcp_ref.so (build() makes it where the reference is present): its results on "
                                   "the worlds that leave stage 0 are not the reference's", len(flagged), flagged[:8].tolist())


def assert_match_or_reference_unstable(tag, ow, s, a, g, dev, ref, tol, lcp=None, lcp_len=None, n_perturb=64, closeness=0.1, ulps=1,
                                       max_unstable=None, max_by_closeness=None, fd_model=None, only=None, verbose=True):
    """dev / ref: dicts of next, grad_state, grad_action [B, .].  Worlds above `tol` must be ones where the oracle's OWN result moves by
    more than `tol` under +-`ulps`-ulp perturbations of its inputs (state, and the LCP warm start when one is given), and the device
    result must be one of the oracle's outcomes: within `tol` of a perturbed run ("tol" branch), or - where those outcomes form a
    continuum - at least 1 / `closeness` times closer to one of them than they scatter ("closeness" branch).  The closeness branch is
    BOUNDED: at most `max_by_closeness` worlds may need it (default: 2 worlds or 0.5 % of the batch).  fd_model: the model description -
    the gradients of worlds within FD_GAP of the log-map singularity of a free / ball joint are then judged against the oracle WITH its
    exact-derivative instrument instead of the reference's finite differences (exact_reference_near_the_singularity), at `tol` - up to
    the conditioning of doubles a few 1e-3 rad from pi (gradient_tolerance); everything else against the oracle as it is, at `tol`.  only: a mask of the worlds to judge.  Prints how many
    worlds took which branch and returns (unstable worlds, worlds that needed the closeness branch)."""
    for k in KEYS:
        assert np.isfinite(dev[k]).all() and np.isfinite(ref[k]).all(), (tag, k, "non-finite values", int((~np.isfinite(dev[k])).sum()), int((~np.isfinite(ref[k])).sum()))
    assert_reference_solver_present(tag, ref)
    near = np.zeros(len(ref["next"]), dtype=bool)
    fd_err = 0.0
    if fd_model is not None:
        ref, near, fd_err = exact_reference_near_the_singularity(ow, fd_model, s, a, g, ref, lcp, lcp_len)
    errs, scales = world_errors(dev, ref)
    B = len(errs["next"])
    tolg = gradient_tolerance(fd_model, ref["next"], tol) if fd_model is not None else np.full(B, tol)
    tols = {"next": np.full(B, tol), "grad_state": tolg, "grad_action": np.full(B, tol)}   # (the positions do not depend on the action)
    excess = np.maximum.reduce([errs[k] / tols[k] for k in KEYS])           # > 1: above the tolerance of that output in that world
    worst = np.maximum.reduce([errs[k] for k in KEYS])
    if only is not None:
        excess = np.where(only, excess, 0.0)
    bad = np.where(excess > 1.0)[0]
    rng = np.random.default_rng(12345)
    by_tol = by_closeness = 0
    for wd in bad:
        s0 = s[wd]
        sp = s0[None, :] * (1.0 + rng.integers(-ulps, ulps + 1, (n_perturb, s0.size)) * EPS)
        kw = {}
        if lcp is not None:
            kw = {"lcp_in": np.repeat(lcp[wd][None], n_perturb, 0) * (1.0 + rng.integers(-ulps, ulps + 1, (n_perturb, lcp.shape[1])) * EPS),
                  "lcp_len_in": np.repeat(lcp_len[wd], n_perturb)}
        if near[wd]:
            ow.set_exact_position_jacobians(True)
        try:
            r = ow.step_batch(sp, np.repeat(a[wd][None], n_perturb, 0), np.repeat(g[wd][None], n_perturb, 0), threads=8, **kw)
        finally:
            ow.set_exact_position_jacobians(False)
        nz = [k for k in KEYS if dev[k].shape[1]]
        tw = float(tolg[wd])
        dist = np.maximum.reduce([(np.abs(r[k] - dev[k][wd][None]) / scales[k][wd][None]).max(1) for k in nz])
        spread = max(float((np.abs(r[k] - ref[k][wd][None]) / scales[k][wd][None]).max()) for k in nz)
        assert spread > tw, (tag, int(wd), "the reference is stable here but the device differs", float(worst[wd]), float(dist.min()), tw)
        assert dist.min() <= max(tw, closeness * spread), (tag, int(wd), "device result is none of the reference's own outcomes",
                                                           float(dist.min()), float(spread))
        if dist.min() <= tw:
            by_tol += 1
        else:
            by_closeness += 1
    near_pi = int((tolg > tol).sum())
    if verbose or len(bad):
        print(f"[{tag}] worlds above 1e-7 / above {tol:g} (per world and block): {(worst > 1e-7).sum()} / {(worst > tol).sum()} of {B} (max {worst.max():.2e})"
              + (f"; {int(near.sum())} worlds within {FD_GAP} rad of a log-map singularity judged against the oracle with exact position Jacobians "
                 f"(its finite differences are off by up to {fd_err:.1e} there), {near_pi} of them within the eps / gap^3 range of doubles" if near.any() else "")
              + f"; reference-unstable (oracle flips under {ulps}-ulp perturbations): {len(bad)}, device within tol of one of its outcomes: {by_tol}, "
              f"accepted by the closeness branch: {by_closeness}")
    if max_unstable is not None:
        assert len(bad) <= max_unstable, (tag, len(bad), max_unstable)
    cap = max(2, int(0.005 * B)) if max_by_closeness is None else max_by_closeness
    assert by_closeness <= cap, (tag, "too many worlds needed the closeness branch", by_closeness, cap)
    return len(bad), by_closeness
