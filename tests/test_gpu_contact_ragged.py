"""The contact step and its VJP at RAGGED batch sizes, on every build of the contact stage behind the ABI.

Every launch of the contact path takes its shape from the batch size B (csrc/nimble_amd.hip::launchForward / launchBackward): the tree grid
ceil(cnt / (wpbFwd pad)), the narrow-phase grid ceil(cnt / wlD), ceil(cnt / 2) wavefronts of k_contact_rows_coop<2> (an odd slice leaves
half a wavefront empty), coop_wave_dev.hpp::coopWorld (workgroup -> world permuted only when the grid is a multiple of 8), the cascade
kernels (cnt workgroups on the slice's compacted failList + b0 and failCount + si), the general build's scratch behind
workspaceHeadBytes(m, B), the slices of slicePer (only the last one is ragged) and the 256-thread blocks of the rollouts' row copies and of
the read-outs.  Every other contact test that looks at gradients runs at a multiple of 16.  Here: B in SIZES, odd and even, both sides of
8, 16 and 64, for every scene
  (a) next state and both gradients of ALL B worlds against the oracle (tests/parity.py, TOL = 1e-7, with the ulps / closeness / fd_model
      arguments of the existing test of that scene), `max_unstable` being the number of worlds below B whose ORACLE result moves by more
      than the tolerance under the criterion's own perturbations - counted on the CPU for the seed below, 256 perturbed runs per world
      (four times the 64 the criterion takes), nothing of the device in it - and `max_by_closeness` = 0 where that count is 0;
  (b) world b of the run at B equals world b of the run at BMAX = 130 BIT FOR BIT (next, both gradients, status, warm start): no launch
      shape of this path depends on B below 65536 worlds (pickLanes), so there is no exception to name;
  (c) the status words: the stage-0 set is what the scene is there for (below), and single worlds / an all-cascade batch of the metric
      scene equal their rows of the BMAX run bit for bit (failCount == 0, == 1 == cnt, == cnt).
NBL_ST_LCP_STAGE0 (0x2) is SET on a world that was solved at stage 0 and clear on one that was handed to the cascade.

Scenes (inputs drawn once at BMAX, prefixes s[:B]; cotangent from seed + 1; the oracle reference once per scene at BMAX).  "unstable": the
CPU count of reference-unstable worlds of the 130 for that seed; "worst": the largest per-world-and-block error against the oracle measured
on an MI355X at BMAX, next / grad_state / grad_action (box_stack: grad_state against the oracle with exact position Jacobians on the 12
worlds within 0.3 rad of the log-map singularity, as tests/parity.py judges them; 1.5e-7 against its finite differences).
  scene          model                                                       build  rowsPack  seed  unstable  worst
  atlas_resting  atlas20 on the ground, contact_inputs defaults: all stage 0    8      2      101     0      3.1e-14 / 5.7e-10 / 1.7e-12
  atlas_metric   the same, joint noise 0.02, vel 0.01, action 0.0: 67 worlds    8      2      502     0      5.1e-12 / 8.6e-10 / 5.0e-11
                 at stage 0, 63 through the cascade (16 pivoting, 2 PGS, 5 without friction, 40 failed)
                 (seeds 102, 202, 302: two unstable worlds each, 402 and 602: one - the reference flips on 1 .. 2 % of this distribution)
  box_stack      box_stack_inputs (cfg4): every world through the cascade       8      2      103     0      6.1e-11 / 6.8e-09 / 7.1e-10
  tower3         cube_tower_inputs(n_cubes=3, max_contacts=16), 12 contacts     16     1      204     0      4.5e-11 / 1.7e-09 / 2.5e-10
                 (seeds 104 and 404: a 4-ulp perturbation of some world ABORTS the reference's own Dantzig - _dLDLTAddTL,
                 "alphanew != 0" - and with it the process: not used)
  tower5         cube_tower_inputs(n_cubes=5, max_contacts=24), 20 contacts     64     -      105     0      2.4e-11 / 1.6e-09 / 2.0e-10
  tower5_cap128  the same worlds with max_contacts = 72: the general code's     128    -      105     0      the same figures (the whole
                 384-row instantiation (record and scratch are sized by the model's rows); judged by tower5's reference    test: 0.05 s)
  arm_friction   limited_arm on the ground (test_gpu_joint_friction.py's model; a cube's free root takes no friction), Coulomb friction
                 on hinge0 only: the _jf kernels of the general build (build 64, seed 106).  THE ORACLE HAS NO JOINT FRICTION ROWS, so
                 (a) does not exist for this scene: (b), and the properties test_gpu_joint_friction.py checks (impulse within
                 [-f dt, f dt], a hinge whose impulse is strictly inside has stopped: 5 of the 130 worlds stick).
rowsPack (worlds per wavefront of k_contact_rows_coop) has no query behind the ABI; _rows_pack restates nbl_model_create's rule and the
test prints it.  Both 24-row scenes get 2, so no further model is needed for the two-worlds-per-wavefront kernel.

The ragged last slice (inputs of their own, oracle on the first and the last 130 worlds; unstable: of those 260; worst: all outputs):
  atlas_metric B = 513, 2 slices   seed 111  unstable 0                      worst 2.7e-09
  tower5       B = 513, 2 slices   seed 112  unstable 0                      worst 2.7e-09
  atlas_metric B = 1027, 4 slices  seed 113  unstable 2 (74 and 142 of 260)  worst 2.4e-09 (the device is within 1e-7 of the unperturbed
                                                                             oracle on those two as well)
Rollouts against the oracle's chain (final state / grad_state0 / grad_actions): atlas_metric 1.5e-13 / 2.1e-10 / 4.7e-11,
tower3 3.7e-12 / 1.7e-09 / 1.7e-09.  Mass gradient at B = 65: 6.7e-09 of the parameter's scale.

A bug found by this file would be named in the docstring of the test that found it: none was - every check passed on the first run."""
import copy
import functools

import numpy as np
import pytest

from parity import assert_match_or_reference_unstable, world_errors

pytestmark = pytest.mark.gpu
TOL = 1e-7
BMAX = 130
SIZES = (1, 2, 3, 7, 8, 9, 17, 63, 65, 129, 130)     # (8: a grid that IS a multiple of 8 in the kernels whose grid equals B)
ULPS = 4                                              # tests/test_gpu_contacts16.py, tests/test_gpu_general.py (their default)
ST_STAGE0, ST_CASCADE = 0x2, 0x4 | 0x8 | 0x10 | 0x20
DEV = "cuda:0"

# seed: of the inputs (the cotangent: seed + 1).  unstable: the worlds of the BMAX batch whose oracle result moves by more than TOL under
# +-ulps perturbations of the state (256 runs per world, CPU only).  kw: what the existing test of the scene hands to the criterion.
SCENES = {
    "atlas_resting": dict(build=8, seed=101, unstable=(), fd=True, kw=dict()),
    "atlas_metric": dict(build=8, seed=502, unstable=(), fd=True, kw=dict()),
    "box_stack": dict(build=8, seed=103, unstable=(), fd=True, kw=dict()),
    "tower3": dict(build=16, seed=204, unstable=(), fd=False, kw=dict(ulps=ULPS)),
    "tower5": dict(build=64, seed=105, unstable=(), fd=False, kw=dict(ulps=ULPS)),
    "tower5_cap128": dict(build=128, seed=105, unstable=(), fd=False, kw=dict(ulps=ULPS)),
    "arm_friction": dict(build=64, seed=106, unstable=None, fd=False, kw=None),
}
ORACLE_SCENES = [k for k, v in SCENES.items() if v["kw"] is not None]
# the ragged last slice (inputs of their own): (scene, B, slices) -> seed, reference-unstable worlds among the first and the last 130
SLICED = {("atlas_metric", 513, 2): dict(seed=111, unstable=()), ("tower5", 513, 2): dict(seed=112, unstable=()),
          ("atlas_metric", 1027, 4): dict(seed=113, unstable=(74, 142))}


def make(scene, B, seed):
    """-> (model description, state [B, 2n], action [B, k]) - no device involved"""
    from util import box_stack_inputs, contact_inputs, cube_tower_inputs, limited_arm
    if scene == "atlas_resting":
        return contact_inputs("atlas20", B, seed)
    if scene == "atlas_metric":
        return contact_inputs("atlas20", B, seed, joint_noise=0.02, vel_noise=0.01, action_noise=0.0)
    if scene == "box_stack":
        return box_stack_inputs(B, seed)
    if scene == "tower3":
        return cube_tower_inputs(B, seed, n_cubes=3, max_contacts=16)
    if scene in ("tower5", "tower5_cap128"):
        return cube_tower_inputs(B, seed, n_cubes=5, max_contacts=24 if scene == "tower5" else 72)
    if scene == "arm_friction":
        md = limited_arm(enforce=False, ground=True, max_contacts=24)
        [b for b in md.bodies if b.joint_name == "hinge0"][0].coulomb_friction = (0.75,)
        n = md.num_dofs
        rng = np.random.default_rng(seed)
        q = np.clip(rng.normal(0, 0.2, (B, n)), -0.3, 0.3)
        q[:, 0] = rng.uniform(-0.025, 0.0, B)                      # the base box on the ground
        return md, np.concatenate([q, rng.normal(0, 0.05, (B, n))], 1), rng.normal(0, 0.3, (B, len(md.action_map)))
    raise KeyError(scene)


def cotangent(seed, shape):
    return np.random.default_rng(seed + 1).normal(0, 1, shape)


def oracle_model(scene, md):
    """tower5_cap128 is judged by tower5's reference: the same worlds, the oracle keeps every contact whatever the capacity"""
    if scene == "tower5_cap128":
        md = copy.deepcopy(md); md.max_contacts = 24
    return md


@functools.lru_cache(maxsize=None)
def inputs(scene, B=BMAX, seed=None):
    seed = SCENES[scene]["seed"] if seed is None else seed
    md, s, a = make(scene, B, seed)
    return md, s, a, cotangent(seed, s.shape)


@functools.lru_cache(maxsize=None)
def reference(scene, B=BMAX, seed=None, worlds=None):
    """(oracle world, its step_batch result) on the scene's inputs (worlds: a tuple of world indices, default all) - computed once"""
    from oracle import OracleWorld
    md, s, a, g = inputs(scene, B, seed)
    idx = np.arange(B) if worlds is None else np.asarray(worlds)
    ow = OracleWorld(oracle_model(scene, md))
    return ow, ow.step_batch(s[idx], a[idx], g[idx], threads=8)


def _rows_pack(world, build):
    """nbl_model_create's rule for the worlds per wavefront of k_contact_rows_coop (csrc/nimble_amd.hip, `m->rowsPack =`)"""
    if build != 8:
        return 1 if build == 16 else None
    nb = len(world.model.bodies); n_free = sum(b.joint_type == "free" for b in world.model.bodies)
    one = (nb * 6 * 24 + 12 * 24 + 19 * nb + 54 * n_free + 8) * 8
    return 2 if nb <= 32 and 2 * one <= 160 * 1024 else 1


def run(md, s, a, g, slices=None, world=None):
    """timestep + backward on a fresh World -> dict of device tensors (next, grad_state, grad_action, status, cache) and the World"""
    import torch
    import nimblephysics_amd as na
    from nimblephysics_amd.timestep import timestep
    world = world or na.World(md, device=DEV)
    if slices is not None:
        world.set_slices(slices)
    world.reset_lcp_cache()
    st = torch.tensor(s, device=DEV, requires_grad=True); at = torch.tensor(a, device=DEV, requires_grad=True)
    out = timestep(world, st, at)
    status, cache = world.last_status.clone(), world.lcp_cache.clone()
    out.backward(torch.tensor(g, device=DEV))
    return {"next": out.detach().clone(), "grad_state": st.grad.clone(), "grad_action": at.grad.clone(), "status": status, "cache": cache.t().contiguous()}, world


def host(r):
    return {k: r[k].cpu().numpy() for k in ("next", "grad_state", "grad_action")}


def status_of(r):
    return r["status"].cpu().numpy().astype(np.uint32)


@functools.lru_cache(maxsize=None)
def full_run(scene):
    """the BMAX run of a scene: every smaller batch is compared with its rows"""
    md, s, a, g = inputs(scene)
    r, world = run(md, s, a, g)
    build = world._L.nbl_model_max_contacts(world._h)
    assert build == SCENES[scene]["build"], (scene, build)
    print(f"[{scene}] build {build} contact slots, rowsPack {_rows_pack(world, build)}, {world.n} DOFs, seed {SCENES[scene]['seed']}")
    return r


def assert_rows_equal(tag, got, want, rows):
    """world i of `got` == world rows[i] of `want`, every output, bit for bit"""
    import torch
    idx = torch.as_tensor(np.asarray(rows), device=DEV)
    for k in ("next", "grad_state", "grad_action", "status", "cache"):
        assert torch.equal(got[k], want[k][idx]), (tag, k, "differs from the same world inside the BMAX batch",
                                                   torch.nonzero((got[k] != want[k][idx]).reshape(len(rows), -1).any(1)).flatten()[:8].tolist())


def judge(tag, scene, dev, ow, s, a, g, ref, unstable_rows, verbose=False):
    """(a): every world within TOL of the oracle; at most the CPU-counted reference-unstable ones may need the proof, none the closeness
    branch where there are none"""
    cfg = SCENES[scene]
    n_un = len(unstable_rows)
    kw = dict(cfg["kw"])
    if n_un == 0:
        kw["max_by_closeness"] = 0
    md = inputs(scene)[0]
    return assert_match_or_reference_unstable(tag, ow, s, a, g, dev, ref, TOL, max_unstable=n_un, fd_model=md if cfg["fd"] else None, verbose=verbose, **kw)


@pytest.mark.parametrize("scene", ORACLE_SCENES)
def test_every_batch_size_equals_the_oracle_and_its_rows_of_the_full_batch(scene):
    md, s, a, g = inputs(scene)
    ow, ref = reference("tower5" if scene == "tower5_cap128" else scene)
    full = full_run(scene)
    st = status_of(full)
    assert (st & 0x1).all() and not (st & 0x80).any() and not (ref["status"] & 0x80).any(), (scene, "contact everywhere, no overflow")
    assert np.array_equal(st & 0x3, ref["status"] & 0x3), (scene, "the stage-0 set is the oracle's")
    stage0 = (st & ST_STAGE0) != 0
    if scene == "atlas_resting":          # failCount == 0 at every B
        assert stage0.all() and not (st & ST_CASCADE).any()
    elif scene == "atlas_metric":         # both classes, in every prefix from 7 worlds on
        assert 0.3 < stage0.mean() < 0.7 and all(0 < stage0[:B].sum() < B for B in SIZES if B >= 7), stage0[:9]
    elif scene == "box_stack":            # cold start: nobody is solved at stage 0, failCount == cnt at every B
        assert not stage0.any()
    e, _ = world_errors(host(full), ref)
    print(f"[{scene}] B = {BMAX}: stage 0 {int(stage0.sum())}, cascade {int((~stage0).sum())}; stages {({hex(int(k)): int(c) for k, c in zip(*np.unique(st & 0x13e, return_counts=True))})}; "
          "worst error per world and block " + ", ".join(f"{k} {v.max():.2e}" for k, v in e.items()))
    unstable = SCENES[scene]["unstable"]
    for B in SIZES:
        r = full if B == BMAX else run(md, s[:B], a[:B], g[:B])[0]
        assert_rows_equal(f"{scene} B={B}", r, full, np.arange(B))                                       # (b), and (c)'s status words
        judge(f"{scene} B={B}", scene, host(r), ow, s[:B], a[:B], g[:B], {k: (v[:B] if v is not None else None) for k, v in ref.items()},
              [w for w in unstable if w < B], verbose=B == BMAX)                                         # (a)


def test_single_worlds_and_an_all_cascade_batch_of_the_metric_scene():
    """(c): one world the BMAX run handed to the cascade, alone (one workgroup, failCount == cnt == 1); one it solved at stage 0, alone
    (failCount == 0); and nine cascade worlds in one batch (gathered from the BMAX batch, repeated to fill it: failCount == cnt == 9, the
    fail list is the identity): each equals its row of the BMAX run bit for bit."""
    md, s, a, g = inputs("atlas_metric")
    full = full_run("atlas_metric")
    stage0 = (status_of(full) & ST_STAGE0) != 0
    casc, easy = np.nonzero(~stage0)[0], np.nonzero(stage0)[0]
    # (not the first of either kind: a world from the middle of a wavefront's worth of worlds, and the very last one)
    for rows in ([casc[len(casc) // 2]], [easy[len(easy) // 2]], [casc[-1]], [easy[-1]], np.resize(casc, 9)):
        rows = np.asarray(rows)
        r, _ = run(md, s[rows], a[rows], g[rows])
        assert np.array_equal((status_of(r) & ST_STAGE0) != 0, stage0[rows])
        assert_rows_equal(f"metric worlds {rows.tolist()} on their own", r, full, rows)


def test_joint_friction_rows_at_every_batch_size():
    """The _jf kernels of the general build (one friction row next to four contacts): every B against the rows of the BMAX batch bit for
    bit; at BMAX the friction impulse lies in [-f dt, f dt] and a hinge whose impulse is strictly inside has stopped
    (tests/test_gpu_joint_friction.py::test_friction_rows_share_the_lcp_with_contacts; the oracle has no friction rows to compare with)."""
    md, s, a, g = inputs("arm_friction")
    full = full_run("arm_friction")
    st, cache, nxt = status_of(full), full["cache"].cpu().numpy(), full["next"].cpu().numpy()
    n = md.num_dofs
    both = (st & 0x801) == 0x801
    assert both.mean() > 0.5 and not (st & (0x80 | 0x40 | 0x400)).any(), both.mean()
    solved = both & ((st & 0x30) == 0)
    assert solved.mean() > 0.5
    bound = 0.75 * md.dt
    hinge = 1                                                      # DOF of hinge0
    stuck = 0
    for b in np.nonzero(solved)[0]:
        nC = int(cache[b, -1]) // 3
        x = cache[b, 3 * (nC - 1)]                                 # the one friction slot comes last
        assert abs(x) <= bound * (1 + 1e-12), (b, x)
        if abs(x) < bound * (1 - 1e-7):
            stuck += 1
            assert abs(nxt[b, n + hinge]) <= 1e-5, (b, nxt[b, n + hinge])
    print(f"[arm_friction] {int(both.sum())} of {BMAX} worlds with contacts and the friction row, {stuck} sticking")
    for k in ("next", "grad_state", "grad_action"):
        assert np.isfinite(full[k].cpu().numpy()).all() and full[k].abs().max().item() > 0
    for B in SIZES[:-1]:
        r, _ = run(md, s[:B], a[:B], g[:B])
        assert_rows_equal(f"arm_friction B={B}", r, full, np.arange(B))


# ---- the ragged last slice ---------------------------------------------------------------------------------------------------------------
def _ends(B):
    return np.concatenate([np.arange(BMAX), np.arange(B - BMAX, B)])


@pytest.mark.parametrize("scene,B,slices", list(SLICED))
def test_a_ragged_last_slice(scene, B, slices):
    """slicePer rounds a slice to 16 worlds, so only the last slice of a call is ragged: [272, 513) with two slices, [816, 1027) with four
    (slicesFor keeps 256 worlds per slice: the smallest such calls).  Forward, backward, status and warm start equal the one-slice call bit
    for bit; the first and the last 130 worlds against the oracle as in (a)."""
    cfg = SLICED[(scene, B, slices)]
    md, s, a, g = inputs(scene, B, cfg["seed"])
    one, _ = run(md, s, a, g, slices=1)
    cut, world = run(md, s, a, g, slices=slices)
    assert world.slices_for(B) == slices
    per = (((B + slices - 1) // slices) + 15) & ~15
    ranges = [(i * per, min(B, (i + 1) * per)) for i in range(slices)]        # forSlices (the deferred-join test below asks the handle)
    assert per == 272 and ranges[-1][1] == B and (B - ranges[-1][0]) % 16 != 0
    assert_rows_equal(f"{scene} B={B} in {slices} slices", cut, one, np.arange(B))
    st = status_of(cut)
    if scene == "atlas_metric":
        stage0 = (st & ST_STAGE0) != 0
        assert all(0 < stage0[lo:hi].sum() < hi - lo for lo, hi in ranges)       # every slice has a fail list of its own to compact
    ends = _ends(B)
    ow, ref = reference(scene, B, cfg["seed"], tuple(ends.tolist()))
    dev = {k: v[ends] for k, v in host(cut).items()}
    assert np.array_equal(st[ends] & 0x83, ref["status"] & 0x83)
    judge(f"{scene} B={B} in {slices} slices, first and last {BMAX}", scene, dev, ow, s[ends], a[ends], g[ends], ref, cfg["unstable"], verbose=True)


@pytest.mark.parametrize("scene", ["atlas_metric", "tower5"])
def test_a_ragged_last_slice_on_a_deferred_join_handle(scene):
    """B = 513 in two slices through step_into / backward_into / join (tests/test_gpu_deferred_join.py): the joined one-slice call's bits."""
    import torch
    import nimblephysics_amd as na
    B = 513
    md, s, a, g = inputs(scene, B, SLICED[(scene, B, 2)]["seed"])
    one, _ = run(md, s, a, g, slices=1)
    dev = torch.device(DEV)
    w = na.World(md, device=dev)
    w.set_slices(2); w.set_deferred_join(True)
    assert [(lo, hi) for _, lo, hi in w.slices(B)] == [(0, 272), (272, 513)]
    st = w.to_soa(torch.tensor(s, device=dev)); at = w.to_soa(torch.tensor(a, device=dev)); gt = w.to_soa(torch.tensor(g, device=dev))
    b = dict(nxt=torch.zeros_like(st), saved=torch.empty(w.saved_bytes(B), dtype=torch.uint8, device=dev), status=torch.zeros(B, dtype=torch.int32, device=dev),
             cache=torch.zeros((w.m, B), dtype=torch.float64, device=dev), gs=torch.zeros_like(st), ga=torch.zeros_like(at))
    w.fork()
    w.step_into(st, at, b["nxt"], b["saved"], b["status"], None, b["cache"])
    w.backward_into(b["saved"], gt, b["gs"], b["ga"])
    w.join()
    torch.cuda.synchronize()
    got = {"next": w.from_soa(b["nxt"]), "grad_state": w.from_soa(b["gs"]), "grad_action": w.from_soa(b["ga"]), "status": b["status"], "cache": b["cache"].t().contiguous()}
    assert_rows_equal(f"{scene} B={B}, deferred join", got, one, np.arange(B))


# ---- rollouts ----------------------------------------------------------------------------------------------------------------------------
def _oracle_chain(scene, s0, acts, w):
    """the oracle's T chained steps with its LCP warm start carried, and the gradient of sum(w * states) by its backprop, step by step"""
    from oracle import OracleWorld
    md = inputs(scene)[0]
    ow = OracleWorld(md)
    T = acts.shape[1]
    xs, lcps = [s0], [(None, None)]
    for t in range(T):
        r = ow.step_batch(xs[-1], acts[:, t], None, threads=8, lcp_in=lcps[-1][0], lcp_len_in=lcps[-1][1], want_lcp=True)
        xs.append(r["next"]); lcps.append((r["lcp"], r["lcp_len"]))
    g = w[:, T]
    gas = []
    for t in range(T - 1, -1, -1):
        r = ow.step_batch(xs[t], acts[:, t], g, threads=8, lcp_in=lcps[t][0], lcp_len_in=lcps[t][1])
        g = r["grad_state"] + w[:, t]; gas.append(r["grad_action"])
    return np.stack(xs, 1), g, np.stack(gas[::-1], 1)


def rollout_case(scene, B, T=3):
    md, s, a, _ = inputs(scene)
    acts = np.repeat(a[:B, None, :], T, 1)
    w = np.random.default_rng(SCENES[scene]["seed"] + 2).normal(0, 1, (BMAX, T + 1, s.shape[1]))[:B]
    return md, s[:B], acts, w


@pytest.mark.parametrize("scene", ["atlas_metric", "tower3"])
@pytest.mark.parametrize("B", [7, 65])
def test_rollouts_at_ragged_batch_sizes(scene, B):
    """T = 3 warm-started steps, a loss on every state: the [m][B] warm-start cache, k_copy_rows / k_add_rows and the checkpoint blocks at a
    B their 256-thread blocks do not divide.  rollout() with and without checkpointing and three chained timestep() calls on a fresh World:
    states, status and all gradients bit for bit (a gradient that meets a loss term is ONE addition of two terms in both, whichever way
    round); against the oracle's chain at the bounds of tests/test_gpu_rollout.py::test_rollout_vs_oracle_T_steps."""
    import torch
    import nimblephysics_amd as na
    from nimblephysics_amd.timestep import rollout, timestep
    md, s0, acts, w = rollout_case(scene, B)
    T = acts.shape[1]
    wt = torch.tensor(w, device=DEV)
    res = []
    for K in (0, 2, None):
        world = na.World(md, device=DEV)
        st = torch.tensor(s0, device=DEV, requires_grad=True); at = torch.tensor(acts, device=DEV, requires_grad=True)
        if K is None:
            xs, sts = [st], []
            for t in range(T):
                xs.append(timestep(world, xs[-1], at[:, t])); sts.append(world.last_status.clone())
            ys, status = torch.stack(xs, 1), torch.stack(sts)
        else:
            ys = rollout(world, st, at, warm_start=True, checkpoint_every=K); status = world.rollout_status.clone()
        (ys * wt).sum().backward()
        res.append((ys.detach().clone(), status, st.grad.clone(), at.grad.clone()))
    for other, what in ((res[1], "checkpoint_every = 2"), (res[2], "the chain of timesteps")):
        for name, x, y in zip(("states", "status", "grad_state0", "grad_actions"), res[0], other):
            assert torch.equal(x, y), (scene, B, "rollout against " + what, name, (x - y).abs().max().item())
    stn = res[0][1].cpu().numpy().astype(np.uint32)
    assert (stn & 0x1).all() and not (stn & 0x80).any()
    xs, g0, gas = _oracle_chain(scene, s0, acts, w)
    ys, gs, ga = (res[0][i].cpu().numpy() for i in (0, 2, 3))
    e = (np.abs(ys[:, -1] - xs[:, -1]).max() / np.abs(xs[:, -1]).max(), np.abs(gs - g0).max() / np.abs(g0).max(), np.abs(ga - gas).max() / max(np.abs(gas).max(), 1e-30))
    print(f"[rollout {scene} B={B}] against the oracle's chain: final state {e[0]:.2e}, grad_state0 {e[1]:.2e}, grad_actions {e[2]:.2e}")
    assert e[0] <= 1e-7 and e[1] <= 1e-6 and e[2] <= 1e-6, e


# ---- mass gradient and read-outs -----------------------------------------------------------------------------------------------------------
def test_mass_gradient_at_65_worlds():
    """atlas_resting with the root body's mass registered: d_mass of every world (nbl_backward_inertia, before any sum) at B = 65 equals
    the BMAX batch's rows bit for bit, and the oracle's central differences at the bound of
    tests/test_gpu_mass.py::test_standing_atlas_with_contacts (2e-4 of the parameter's scale, either of two step sizes)."""
    from nimblephysics_amd.mass import WrtMassBodyNodeEntryType as T
    from test_gpu_mass import _device, _oracle_fd
    md, s, a, g = inputs("atlas_resting")
    entries = [(0, T.INERTIA_MASS)]
    full, _, _ = _device(md, entries, s, a, g)
    B = 65
    dev, _, _ = _device(md, entries, s[:B], a[:B], g[:B])
    assert dev.shape == (B, 1) and np.array_equal(dev, full[:B]) and np.abs(dev).max() > 0
    ref, ref2 = _oracle_fd(md, entries, s[:B], a[:B], g[:B]), _oracle_fd(md, entries, s[:B], a[:B], g[:B], eps_rel=1e-5)
    ref = np.where(np.abs(ref2 - dev) < np.abs(ref - dev), ref2, ref)
    scale = np.maximum(np.abs(ref).max(0), 1e-3 * np.abs(ref).max()) + 1e-9
    err = np.abs(dev - ref) / scale
    print(f"[mass gradient, atlas_resting, B = {B}] worst error over scale {err.max():.2e}")
    assert err.max() < 2e-4, (float(err.max()), int(err.argmax()))


def test_read_outs_at_65_worlds():
    """box_stack at B = 65 (one full 64-lane block and a one-lane tail): read_contacts, body_contact_wrenches and read_constraint_rows
    equal the BMAX batch's rows bit for bit; slots past a world's count are zeros, in world 64 like everywhere."""
    import torch
    import nimblephysics_amd as na
    from nimblephysics_amd import _abi
    from nimblephysics_amd.contacts import body_contact_wrenches, read_constraint_rows, read_contacts
    md, s, a, _ = inputs("box_stack")
    out = {}
    for B in (BMAX, 65):
        world = na.World(md, device=DEV)
        _, saved, _ = world.step_soa(world.to_soa(torch.tensor(s[:B], device=DEV)), world.to_soa(torch.tensor(a[:B], device=DEV)), want_saved=True)
        r = read_contacts(world, saved, B)
        n_rows, imp, mp = read_constraint_rows(world, saved, B)
        out[B] = dict({k: getattr(r, k) for k in r.FIELDS}, wrench=body_contact_wrenches(world, saved, B, [1, 2]), n_rows=n_rows, row_impulse=imp, row_map=mp)
    for k, v in out[65].items():
        assert v.shape[0] == 65 and torch.equal(v, out[BMAX][k][:65]), k
    r = {k: v.cpu().numpy() for k, v in out[65].items()}
    assert r["count"].min() > 0 and np.abs(r["wrench"][64, :, 3:]).max() > 0.5 and (r["n_rows"] == 3 * r["count"]).all()
    for b in range(65):
        cnt = int(r["count"][b])
        for f in ("point", "normal", "depth", "type", "collider_a", "collider_b", "body_a", "body_b", "impulse", "row_class", "force"):
            assert not np.asarray(r[f][b, cnt:]).any(), (b, f, "slots past the count must be zeros")
        assert not r["row_impulse"][b, 3 * cnt:].any() and (r["row_map"][b, 3 * cnt:] == _abi.CO_MAP_NONE).all(), b
