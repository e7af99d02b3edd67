"""The three routes of the stage-0 standardisation loop (coop_dev.hpp: coopStandardizeLoop) on the GPU: a world whose final classification
is the guess rows (no second factorisation), the Cholesky route (coopPinvSym) and the Householder route (coopPinv: a friction row on its
bound).  Each batch is compared with the CPU oracle at the tolerances of test_gpu_contact.py, and BYTE FOR BYTE with what the kernels
returned before coopBuildQ's reads were batched (tests/golden/solve_routes/*.npz, written by tools/record_solve_routes_golden.py): next
state, gradients, status and the record's x, cls and pinv rows.  The routes keep every sum's term order and every fused multiply-add,
so not one bit may move."""
import os

import numpy as np
import pytest

from parity import assert_match_or_reference_unstable, world_errors

pytestmark = pytest.mark.gpu
TOL = 1e-7                       # test_gpu_contact.py
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_routes")

# the metric distribution (all three routes occur), the stage-0 regime (every world resolved from the guess rows), and two chained steps
# (the second one starts from the warm-start cache of the first)
CASES = {
    "routes": dict(B=256, seed=41, joint_noise=0.02, vel_noise=0.01, action_noise=0.0),
    "guess": dict(B=64, seed=42, joint_noise=0.002, vel_noise=0.001, action_noise=0.1),
    "warm": dict(B=16, seed=43, joint_noise=0.002, vel_noise=0.001, action_noise=0.1),
}
MAX_CONTACTS, CR_SIZE, MAX_ROWS = 8, 22, 24      # the 24-row build (csrc/model_dev.hpp)


def _route_counts(status, rec):
    """Worlds per route, counted on the device from the status words and the record.  The pseudo-inverse in the record (pflag) is that of
    the final classification: the Householder route's when a friction row sits on its bound (cls +-2), whichever kernel standardised
    the world; the guess's own when stage 0 resolved the world and the clamping set is the guess set (every friction row, the normals
    with b > 0: no second factorisation); the Cholesky route's for any other clamping set."""
    import torch
    have = rec["pflag"] != 0
    st0 = (status & 0x2) != 0
    cls = rec["cls"]
    hh = (cls.abs() == 2.0).any(1)
    normal = (torch.arange(MAX_ROWS, device=cls.device) % 3) == 0
    live = torch.arange(MAX_ROWS, device=cls.device)[None, :] < (3 * rec["nc"])[:, None]
    guess = live & (~normal[None, :] | (rec["b"] > 0))
    shortcut = st0 & ~hh & ((cls == 1.0) == guess).all(1)
    return {"guess rows": int((have & shortcut).sum()), "cholesky": int((have & ~hh & ~shortcut).sum()), "householder": int((have & hh).sum()),
            "householder, stage 0": int((have & hh & st0).sum()), "handed on": int((~st0).sum())}


def device_results(name):
    """Run case `name` on the GPU -> (arrays for the byte-for-byte comparison, everything the oracle comparison needs)."""
    import torch
    import nimblephysics_amd as na
    from nimblephysics_amd.contacts import read_constraint_rows
    from nimblephysics_amd.timestep import timestep
    from util import contact_inputs, record_rows
    c = CASES[name]
    B = c["B"]
    md, s, a = contact_inputs("atlas20", B, c["seed"], joint_noise=c["joint_noise"], vel_noise=c["vel_noise"], action_noise=c["action_noise"])
    world = na.World(md, device="cuda:0")
    g = np.random.default_rng(c["seed"] + 1).normal(0, 1, s.shape)
    st = torch.tensor(s, device="cuda:0", requires_grad=True); at = torch.tensor(a, device="cuda:0", requires_grad=True)
    out = timestep(world, st, at)
    mid = None
    if name == "warm":
        assert world.lcp_cache is not None and world.lcp_cache.shape == (world.m, B)
        mid = out.detach().cpu().numpy()
        out = timestep(world, out, at)               # the second step starts from the first one's x
    status = world.last_status.clone()
    saved = world._last_saved
    rec = record_rows(world, saved, B, MAX_CONTACTS, CR_SIZE)
    # the layout read above is the record's: its x rows are the impulses the library's own readout returns
    n_rows, imp, _ = read_constraint_rows(world, saved, B)
    assert torch.equal(n_rows.to(torch.float64), 3 * rec["nc"]) and torch.equal(imp, rec["x"])
    routes = _route_counts(status, rec)
    out.backward(torch.tensor(g, device="cuda:0"))
    torch.cuda.synchronize()
    dev = {"next": out.detach().cpu().numpy(), "grad_state": st.grad.cpu().numpy(), "grad_action": at.grad.cpu().numpy()}
    arrays = dict(dev, status=status.cpu().numpy().astype(np.uint32), x=rec["x"].cpu().numpy(), cls=rec["cls"].cpu().numpy().astype(np.int8),
                  pflag=rec["pflag"].cpu().numpy().astype(np.int8), pinv=rec["pinv"].cpu().numpy())
    return arrays, {"md": md, "s": s, "a": a, "g": g, "dev": dev, "routes": routes, "mid": mid}


_cache = {}


def _results(name):
    if name not in _cache:
        _cache[name] = device_results(name)
    return _cache[name]


def golden_files(name):
    """(file, keys) pairs: the pinv rows of 256 worlds get a file of their own (every committed file stays below 1 MiB)"""
    return [(os.path.join(GOLDEN, f"{name}.npz"), ("next", "grad_state", "grad_action", "status", "x", "cls", "pflag")),
            (os.path.join(GOLDEN, f"{name}_pinv.npz"), ("pinv",))]


@pytest.mark.parametrize("name", list(CASES))
def test_results_are_byte_identical_to_the_recorded_ones(name):
    arrays, _ = _results(name)
    for path, keys in golden_files(name):
        gold = np.load(path)
        for k in keys:
            assert gold[k].dtype == arrays[k].dtype and gold[k].shape == arrays[k].shape, (name, k)
            assert gold[k].tobytes() == arrays[k].tobytes(), (name, k, int((gold[k] != arrays[k]).sum()), "entries differ")


def test_all_three_routes_occur_on_the_metric_distribution():
    _, info = _results("routes")
    print("[solve routes] B = 256, noise 0.02:", info["routes"])
    for route in ("guess rows", "cholesky", "householder", "householder, stage 0"):
        assert info["routes"][route] >= 1, info["routes"]
    assert info["routes"]["handed on"] >= 1


def test_metric_distribution_matches_the_oracle():
    """Like test_gpu_contact.py::test_full_lcp_cascade_on_noisy_poses: every world within 1e-7, or the oracle itself proven unstable there."""
    from oracle import OracleWorld
    arrays, info = _results("routes")
    B = CASES["routes"]["B"]
    ow = OracleWorld(info["md"])
    ref = ow.step_batch(info["s"], info["a"], info["g"], threads=8)
    dev = info["dev"]
    for k in dev:
        assert np.isfinite(dev[k]).all() and np.isfinite(ref[k]).all(), k
    gpu0, ora0 = (arrays["status"] & 0x2) != 0, (ref["status"] & 0x2) != 0
    assert np.array_equal(gpu0, ora0)
    assert not np.any((arrays["status"] & 0x1) == 0)
    errs, _ = world_errors(dev, ref)
    bad, _ = assert_match_or_reference_unstable("solve routes B=256", ow, info["s"], info["a"], info["g"], dev, {k: ref[k] for k in dev}, TOL, fd_model=info["md"])
    assert bad <= 0.01 * B
    assert (errs["next"][gpu0] > TOL).sum() == 0
    for k in ("grad_state", "grad_action"):
        assert errs[k][gpu0].max() < TOL


def test_guess_rows_batch_matches_the_oracle():
    from oracle import OracleWorld
    arrays, info = _results("guess")
    assert np.all(arrays["status"] & 0x1) and np.all(arrays["status"] & 0x2)
    r = info["routes"]
    assert r["guess rows"] == CASES["guess"]["B"] and r["cholesky"] == 0 and r["householder"] == 0, r
    ref = OracleWorld(info["md"]).step_batch(info["s"], info["a"], info["g"], threads=8)
    assert np.array_equal(arrays["status"] & 0x3, ref["status"] & 0x3)
    errs, _ = world_errors(info["dev"], ref)
    for k, e in errs.items():
        assert e.max() < TOL, (k, e.max())


def test_warm_started_step_matches_the_oracle():
    """Like test_gpu_contact.py::test_contact_trajectory_with_warm_start, two steps: the second starts from the first one's LCP cache."""
    from oracle import OracleWorld
    from util import rel_err
    arrays, info = _results("warm")
    assert not np.any(arrays["status"] & 0x20) and np.all(arrays["status"] & 0x2)
    s, a, g, md = info["s"], info["a"], info["g"], info["md"]
    fin = np.zeros_like(s); gs = np.zeros_like(s); ga = np.zeros_like(a)
    for b in range(s.shape[0]):
        w1, w2 = OracleWorld(md), OracleWorld(md)
        x1 = w1.step(s[b], a[b])
        w2.set_lcp_cache(w1.get_lcp_cache())
        fin[b] = w2.step(x1, a[b])
        g1, ga2 = w2.backprop(g[b])
        gs[b], ga1 = w1.backprop(g1)
        ga[b] = ga1 + ga2
    assert rel_err(info["dev"]["next"], fin) < TOL
    assert rel_err(info["dev"]["grad_state"], gs) < 1e-6
    assert rel_err(info["dev"]["grad_action"], ga) < 1e-6
