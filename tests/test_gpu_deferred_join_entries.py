"""Every entry that is NOT a deferred entry point behaves on a deferred-join World as on a joined one (World.set_deferred_join,
include/nimble_amd.h): its inputs may be produced on the current stream right before the call, its results may be consumed there right
after it.  A bit comparison after a synchronise on an idle stream cannot see a missing fork or join, so every case here makes the
ordering observable:

  * BUSY PRODUCER: the input buffers hold a DECOY (a second random draw of world states / actions / cotangents: valid and finite, like the
    blocks the caching allocator hands to the call, which are seeded the same way); a chain of large matrix products is enqueued on the
    current stream and only its last operations copy the real inputs in.  The chain is sized to 12 x the duration of the call (measured
    with events on a joined World, whose path is the one every World took before deferred join existed) and the test ASSERTS that it ran
    at least 10 x as long, so a slice that starts without waiting for the current stream reads the decoy.  No host synchronisation
    between producer and call.
  * IMMEDIATE CONSUMER: the outputs are cloned on the current stream as soon as the call returns, and only then synchronised.
  * EXPECTED: a second World of the same model with joined calls, fed the same inputs after a full synchronise; torch.equal.

Shapes: the smallest with more than one slice (256 worlds per slice at least): 1024 worlds on 4 slices, 513 on 2 (an uneven last slice).
Measured on MI355X on the commit before the rule was enforced (there every deferred case of this file fails with a numeric difference
and every joined case passes), the call on a joined World / the busy chain, ms; every test prints its pair (`-s`):
                               atlas20 B = 1024   pendulum B = 513    cubes24 B = 1024 (max_contacts = 24: the general build)
  timestep fwd + bwd             0.92 /  11.9       0.33 /  4.3         7.8 /  84.7
  step_soa + backward_soa        0.35 /   4.3       0.08 /  2.2         7.7 /  83.3
  step_soa, no record            0.17 /   2.2       0.04 /  2.1
  rollout_soa + backward, T = 4  1.04 /  12.7       0.17 /  2.1        32.0 / 336.2
  rollout_soa, forward only      0.64 /   8.3       0.08 /  2.1
  checkpointed rollout, K = 2    1.27 /  15.5       0.19 /  3.2        48.0 / 505.0
  rollout() + mass gradient      2.09 /  24.7       0.42 /  5.3
  getters after timestep()      30.2  / 322.0       0.32 /  4.3
  forwardPass(idempotent)        0.42 /   5.7       0.14 /  2.2
  step_into, then rollout_soa    0.68 /   8.4       0.11 /  2.2        34.0 / 358.1   (and the last slice's stream busy as long)
"""
import functools
import math

import numpy as np
import pytest
import torch

from util import cfg_inputs, contact_inputs, cube_tower_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T, K = 4, 2                     # rollout steps, checkpoint_every
RATIO, SIZED = 10.0, 12.0       # asserted busy / call ratio, and the one the chain is sized for
ANCHOR_SEED = 31                # contact_inputs("atlas20", 1024, 31): resting poses, joint noise 0.002 (the oracle anchor's inputs)

#          worlds, slices, inputs(B, seed)
MODELS = {"pendulum": (513, 2, lambda B, seed: cfg_inputs("pendulum", B, seed)),
          "atlas20": (1024, 4, lambda B, seed: contact_inputs("atlas20", B, seed)),
          "cubes24": (1024, 4, lambda B, seed: cube_tower_inputs(B, seed, 5, max_contacts=24))}     # 20 contacts: the general build


class Setup:
    pass


@functools.lru_cache(maxsize=None)
def setup(name):
    """Per model, once: the Worlds (deferred, joined, and the joined one the expected values come from), the real inputs, the decoys and
    the device buffers the calls read."""
    import nimblephysics_amd as na
    B, slices, inputs = MODELS[name]
    S = Setup()
    S.name, S.B = name, B
    md, s, a = inputs(B, ANCHOR_SEED)
    _, s2, a2 = inputs(B, ANCHOR_SEED + 1)                       # the decoy: another draw of the same distribution
    S.md, S.s, S.a = md, s, a
    rng = np.random.default_rng(7)

    def draws(shape):
        return rng.normal(0, 1, shape), rng.normal(0, 1, shape)
    S.g, g2 = draws(s.shape)
    acts = np.repeat(a[:, None, :], T, 1) + rng.normal(0, 0.05, (B, T, a.shape[1]))
    acts2 = np.repeat(a2[:, None, :], T, 1) + rng.normal(0, 0.05, (B, T, a.shape[1]))
    gT, gT2 = draws((B, T + 1, s.shape[1]))
    host = {"s": (s, s2), "a": (a, a2), "g": (S.g, g2), "acts": (acts, acts2), "gT": (gT, gT2)}
    soa = {"s": lambda x: x.T, "a": lambda x: x.T, "g": lambda x: x.T, "acts": lambda x: x.transpose(1, 2, 0), "gT": lambda x: x.transpose(1, 2, 0)}
    S.real, S.decoy = {}, {}
    for k, (r, d) in host.items():
        for dst, x in ((S.real, r), (S.decoy, d)):
            dst[k] = torch.tensor(np.ascontiguousarray(x), device=DEV)
            dst[k + "_soa"] = torch.tensor(np.ascontiguousarray(soa[k](x)), device=DEV)         # [d][B] / [T][d][B]
    S.X = {k: torch.empty_like(v) for k, v in S.real.items()}

    def world(deferred):
        w = na.World(md, device=DEV)
        w.set_slices(slices)
        if name == "atlas20":
            w.tuneMass(1, na.WrtMassBodyNodeEntryType.INERTIA_MASS)
        w.set_deferred_join(deferred)
        assert w.slices_for(B) == slices
        return w
    S.ref, S.handles = world(False), {"deferred": world(True), "joined": world(False)}
    # the caller-owned buffers of step_into (the interleaving case)
    w = S.ref
    S.into = dict(nxt=torch.empty((2 * w.n, B), dtype=torch.float64, device=DEV), saved=torch.empty(w.saved_bytes(B), dtype=torch.uint8, device=DEV),
                  status=torch.empty(B, dtype=torch.int32, device=DEV), cache=torch.empty((max(w.m, 1), B), dtype=torch.float64, device=DEV))
    torch.cuda.synchronize()
    return S


class Busy:
    """The producer's chain: `reps` products of two 4096 x 4096 fp32 matrices into a third (no feedback: finite whatever `reps`)."""

    def __init__(self):
        gen = torch.Generator(device=DEV).manual_seed(0)
        self.a = torch.randn((4096, 4096), device=DEV, dtype=torch.float32, generator=gen)
        self.b = torch.randn((4096, 4096), device=DEV, dtype=torch.float32, generator=gen)
        self.c = torch.empty_like(self.a)
        self.run(3)
        self.ms = self.timed(lambda: self.run(8)) / 8

    def run(self, reps):
        for _ in range(reps):
            torch.mm(self.a, self.b, out=self.c)

    @staticmethod
    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)


@functools.lru_cache(maxsize=None)
def busy():
    return Busy()


# ---- the calls under test: (World, input buffers) -> the tensors a caller gets back ----------------------------------------------------
def leaf(x):
    return x.detach().requires_grad_(True)          # (shares the buffer the producer writes)


def c_timestep(w, X, S):
    from nimblephysics_amd.timestep import timestep
    s, a = leaf(X["s"]), leaf(X["a"])
    out = timestep(w, s, a)
    nxt, status = out.detach().clone(), w.last_status.clone()           # the consumer of the forward pass
    out.backward(X["g"])
    return [nxt, status, s.grad, a.grad]


def c_step_soa(w, X, S):
    nxt, saved, status = w.step_soa(X["s_soa"], X["a_soa"], want_saved=True)
    nxt, status, cache = nxt.clone(), status.clone(), (w.lcp_cache.clone() if w.lcp_cache is not None else status)
    gs, ga = w.backward_soa(saved, X["g_soa"])
    return [nxt, status, cache, gs, ga]


def c_step_soa_no_record(w, X, S):
    nxt, saved, status = w.step_soa(X["s_soa"], X["a_soa"], want_saved=False)
    assert saved is None
    return [nxt, status]


def c_rollout_soa(w, X, S):
    states, saved, status = w.rollout_soa(X["s_soa"], X["acts_soa"], want_saved=True)
    states, status = states.clone(), status.clone()
    g0, ga = w.rollout_backward_soa(saved, X["gT_soa"])
    return [states, status, g0, ga]


def c_rollout_soa_no_record(w, X, S):
    if w.m > 0:                # (models with colliders need the records: nbl_rollout_forward refuses without)
        states, saved, status = w.rollout_soa(X["s_soa"], X["a_soa"], T=T, want_saved=True)       # one action block for every step
    else:
        states, saved, status = w.rollout_soa(X["s_soa"], X["a_soa"], T=T, want_saved=False)
        assert saved is None
    return [states, status]


def c_rollout_checkpointed(w, X, S):
    from nimblephysics_amd.world import RolloutRecord
    states, rec, status = w.rollout_soa(X["s_soa"], X["acts_soa"], want_saved=True, checkpoint_every=K)
    assert isinstance(rec, RolloutRecord) and rec.segment == K
    states_now, status = states.clone(), status.clone()
    g0, ga = w.rollout_backward_soa(rec, X["gT_soa"])
    return [states_now, status, g0, ga]


def c_rollout_autograd(w, X, S):
    from nimblephysics_amd.timestep import rollout
    s, acts = leaf(X["s"]), leaf(X["acts"])
    mass = w.getMasses().clone().requires_grad_(True) if w.getMassDims() > 0 else None        # (a CPU tensor: no device round trip)
    ys = rollout(w, s, acts, warm_start=True, mass=mass)
    out = ys.detach().clone()
    ys.backward(X["gT"])
    res = [out, s.grad, acts.grad]
    if mass is not None:                                                                    # nbl_rollout_backward_inertia
        assert mass.grad.abs().max().item() > 0
        res.append(mass.grad.to(DEV))
    return res


def c_getters(w, X, S):
    from nimblephysics_amd.timestep import timestep
    timestep(w, X["s"], X["a"])
    return [w.getStateJacobian(), w.getActionJacobian(), w.getMassMatrix(), w.getState()]


def c_forward_pass(w, X, S):
    from nimblephysics_amd.neural import forwardPass
    w.setState(X["s"]); w.setAction(X["a"])
    snap = forwardPass(w, idempotent=True)
    nxt = torch.cat([snap.getPostStepPosition(), snap.getPostStepVelocity()], 1)
    hl = snap.backpropState(w, X["g"])
    return [nxt, snap.getStatus(), w.getState(), hl.lossWrtState, hl.lossWrtAction]


def c_step_into_then_rollout(w, X, S):
    """step_into without a join, then a rollout whose state0 is the buffer that step writes: the rollout must see the step's result"""
    b = S.into
    if w._deferred:
        w.fork()                                    # the protocol of the deferred entry points: the inputs were produced on this stream
        # ... and the last slice is late: its stream is busy (a caller's per-slice work) when the step is enqueued behind it, so the
        # rollout on the current stream would copy that slice's rows of state0 before the step has written them
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(w.slices(S.B)[-1][0]):
            e0.record(); busy().run(S.reps); e1.record()
        S.side = (e0, e1)
    w.step_into(X["s_soa"], X["a_soa"], b["nxt"], b["saved"], b["status"], None, b["cache"] if w.m > 0 else None)
    states, saved, status = w.rollout_soa(b["nxt"], X["acts_soa"], want_saved=True)
    return [states, status]


CASES = {"timestep": c_timestep, "step_soa": c_step_soa, "step_soa_no_record": c_step_soa_no_record, "rollout_soa": c_rollout_soa,
         "rollout_soa_no_record": c_rollout_soa_no_record, "rollout_checkpointed": c_rollout_checkpointed,
         "rollout_autograd_mass": c_rollout_autograd, "getters": c_getters, "forward_pass_idempotent": c_forward_pass,
         "step_into_then_rollout": c_step_into_then_rollout}
# the general build (slow dense stages): the step and the rollouts; the 2n-pass getters stay with the two other models
PARAMS = [(m, c) for m in ("atlas20", "pendulum") for c in CASES] + \
         [("cubes24", c) for c in ("timestep", "step_soa", "rollout_soa", "rollout_checkpointed", "step_into_then_rollout")]


def fill(S, src):
    for k, v in S.X.items():
        v.copy_(src[k])


def seed_allocator(S):
    """What the calls allocate (torch.empty: the [d][B] copies of their inputs, their outputs) comes out of the caching allocator's free
    blocks: leave blocks of those sizes behind that hold the decoy, so that a kernel that runs early reads a valid state there too and an
    output that is consumed before it is written reads a finite value that is not the answer."""
    d = S.decoy
    blocks = []
    for _ in range(3):
        blocks += [d["s_soa"].clone(), d["a_soa"].clone(), d["g_soa"].clone(), d["s"].clone(), d["a"].clone()]
    for _ in range(2):
        blocks += [d["s_soa"].expand(T + 1, -1, -1).clone(), d["acts_soa"].clone(), d["acts"].clone(), d["gT"].clone()]
    del blocks


def prepare(S, w):
    w.reset_lcp_cache()
    for k in ("nxt", "cache"):
        S.into[k].copy_(S.decoy["s_soa"][:1].expand_as(S.into[k]) if k == "cache" else S.decoy["s_soa"])
    S.into["status"].fill_(-1)


@functools.lru_cache(maxsize=None)
def expected(name, case):
    """(the outputs of the call on the joined reference World, real inputs, everything synchronised; the call's duration there, ms)"""
    S = setup(name)
    fill(S, S.real)
    prepare(S, S.ref)
    torch.cuda.synchronize()
    want = [t.clone() for t in CASES[case](S.ref, S.X, S)]
    torch.cuda.synchronize()
    prepare(S, S.ref)
    ms = Busy.timed(lambda: CASES[case](S.ref, S.X, S))                  # (the second run: nothing is allocated or loaded for the first time)
    return want, ms


@pytest.mark.parametrize("mode", ["deferred", "joined"])
@pytest.mark.parametrize("name,case", PARAMS)
def test_entry_behind_a_busy_producer_with_an_immediate_consumer(name, case, mode):
    S, chain = setup(name), busy()
    want, call_ms = expected(name, case)
    w = S.handles[mode]
    fill(S, S.decoy)
    prepare(S, w)
    seed_allocator(S)
    reps = max(2, math.ceil(SIZED * call_ms / chain.ms))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    chain.run(reps)
    e1.record()
    fill(S, S.real)                                                       # the producer's last operations: the real inputs
    S.reps, S.side = reps, None
    got = [t.clone() for t in CASES[case](w, S.X, S)]                     # the call, and its consumer on the current stream
    torch.cuda.synchronize()
    busy_ms = e0.elapsed_time(e1)
    if S.side is not None:                                                # (the busy slice stream of the interleaving case)
        side_ms = S.side[0].elapsed_time(S.side[1])
        print(f"[{name} B={S.B} {case} {mode}] busy slice stream {side_ms:.3f} ms")
        assert side_ms >= RATIO * call_ms, (side_ms, call_ms)
    print(f"[{name} B={S.B} {case} {mode}] call {call_ms:.3f} ms (joined World), busy producer {busy_ms:.3f} ms ({reps} products), ratio {busy_ms / call_ms:.1f}")
    assert busy_ms >= RATIO * call_ms, (busy_ms, call_ms)
    assert len(got) == len(want)
    diffs = []
    for i, (g, x) in enumerate(zip(got, want)):
        assert g.shape == x.shape and g.dtype == x.dtype, (i, g.shape, x.shape)
        assert torch.isfinite(g.double()).all(), (name, case, mode, i, "non-finite output")
        if not torch.equal(g, x):
            diffs.append((i, int((g != x).sum().item()), float((g.double() - x.double()).abs().max().item())))
    assert not diffs, (name, case, mode, "outputs that differ from the joined World's: (index, entries, max |difference|)", diffs)


def test_joined_timestep_matches_the_oracle():
    """The anchor of the bit comparisons above: the joined World's timestep() forward and backward pass on the contact model, B = 1024,
    against the CPU oracle per world and block at 1e-7 - resting poses with joint noise 0.002, on which the oracle itself does not move
    under 1-ulp perturbations of its inputs (checked on the CPU over 16 perturbed batches before the seed was fixed: no world above
    1e-7), so no world may be excused as reference-unstable."""
    from oracle import OracleWorld
    from parity import assert_match_or_reference_unstable
    S = setup("atlas20")
    want, _ = expected("atlas20", "timestep")
    dev = {"next": want[0].cpu().numpy(), "grad_state": want[2].cpu().numpy(), "grad_action": want[3].cpu().numpy()}
    ow = OracleWorld(S.md)
    ref = ow.step_batch(S.s, S.a, S.g, threads=8)
    assert np.array_equal(want[1].cpu().numpy().astype(np.uint32) & 0x3, ref["status"].astype(np.uint32) & 0x3)
    assert_match_or_reference_unstable("deferred-join entries: anchor", ow, S.s, S.a, S.g, dev, ref, 1e-7, max_unstable=0)


def test_the_mode_belongs_to_the_world():
    """World._deferred: False from __init__, follows set_deferred_join, survives a re-upload of the model (setActionSpace builds a new
    handle, which starts joined: the World puts it back into its mode), and a clone() - its own handle and streams - starts joined."""
    import nimblephysics_amd as na
    md, s, a = cfg_inputs("atlas20", 1024, 3)
    w = na.World(md, device=DEV)
    assert w._deferred is False
    w.set_slices(4)
    w.set_deferred_join(True)
    assert w._deferred is True and len(w.slices(1024)) == 4
    c = w.clone()
    assert c._deferred is False
    with pytest.raises(na.NimbleAmdError):
        c.slices(1024)                                    # nbl_slice_stream: the clone's handle is not in deferred-join mode
    w.setActionSpace(w.getActionSpace()[:-1])
    assert w._deferred is True
    w.set_slices(4)
    assert len(w.slices(1024)) == 4                       # the new handle is in the mode: nbl_slice_stream answers
    w.set_deferred_join(False)
    assert w._deferred is False
    with pytest.raises(na.NimbleAmdError):
        w.slices(1024)


def test_graphed_rollout_on_a_deferred_world_replays_the_joined_result():
    """GraphedRollout captures rollout_soa + rollout_backward_soa: on a deferred-join World the captured calls fork and join like on a
    joined one, and the replay equals the eager calls of the joined World bit for bit."""
    import nimblephysics_amd as na
    S = setup("atlas20")
    want, _ = expected("atlas20", "rollout_soa")
    gr = na.GraphedRollout(S.handles["deferred"], S.B, T)
    gr.state0.copy_(S.real["s_soa"]); gr.actions.copy_(S.real["acts_soa"]); gr.grad_states.copy_(S.real["gT_soa"])
    states, g0, ga = gr.replay()
    got = [states.clone(), gr.status.clone(), g0.clone(), ga.clone()]
    torch.cuda.synchronize()
    for i, (g, x) in enumerate(zip(got, want)):
        assert torch.equal(g, x), i
