"""The reverse pass of the batched inverse kinematics on the device (csrc/ik_grad.hip: nbl_ik_solve_vjp, solve_ik(differentiable=True),
solve_ik_vjp) against tests/ik_grad_numpy.py under the tolerance rule of tests/ik_grad_cases.py (10 x the disagreement of the two NumPy
forms on the same inputs, cond(J_F) <= 1e3 asserted), on the pendulum, a chain of ten ball joints and Atlas-20 with two spatial entries at
B = 1, 63, 65 and 130; bit-identity across batch sizes, accumulate, free_count, autograd end to end, CPU tensors, deferred join, immobile
skeletons, a chunked batch and the argument errors of the C entry point."""
import ctypes as C

import numpy as np
import pytest
import torch

import ik_cases as ic
import ik_grad_cases as gc
import ik_grad_numpy as ign

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODELS = gc.device_models()
BATCHES = (1, 63, 65, 130)
CASES = [(name, cls) for name, (md, entries) in MODELS.items() for cls in gc.case_classes(md, sum(ic.ROWS[k] for k, _ in entries))]
_STATE = {}


def _host(name):
    if ("host", name) not in _STATE:
        md, entries = MODELS[name]
        _STATE["host", name] = gc.HostIKGrad(ic.load_ik_shim(), gc.load_grad_shim(), md, entries)
    return _STATE["host", name]


def _device(name):
    import nimblephysics_amd as na
    if ("device", name) not in _STATE:
        md, entries = MODELS[name]
        w = na.World(md, device=DEV)
        m = na.IKMapping(w)
        for kind, body in entries:
            (m.addSpatialBodyNode, m.addLinearBodyNode, m.addAngularBodyNode)[kind](body)
        _STATE["device", name] = (w, m)
    return _STATE["device", name]


def _problem(name, cls):
    """130 worlds of a class, their NumPy reference at both mu, made once"""
    if (name, cls) not in _STATE:
        md, entries = MODELS[name]
        h = _host(name)
        q, g = gc.problem(h, md, entries, cls, max(BATCHES), gc.SEED + 100 + CASES.index((name, cls)))
        _STATE[name, cls] = (q, g, {mu: gc.reference(h, md, q, g, mu) for mu in gc.MUS})
    return _STATE[name, cls]


def _vjp(name, q, g, mu):
    import nimblephysics_amd as na
    w, m = _device(name)
    gt, free = na.solve_ik_vjp(w, m, torch.tensor(q, device=DEV), torch.tensor(g, device=DEV), mu)
    return gt.cpu().numpy(), free.cpu().numpy()


def test_the_models_are_the_three_asked_for():
    dims = {name: (sum(ic.ROWS[k] for k, _ in entries), md.num_dofs) for name, (md, entries) in MODELS.items()}
    assert dims == {"pendulum": (6, 1), "ball_chain": (9, 30), "atlas20_two": (12, 20)}
    assert ("atlas20_two", "one_at_limit") in CASES and ("atlas20_two", "fewer_free_than_rows") in CASES


@pytest.mark.parametrize("mu", gc.MUS)
@pytest.mark.parametrize("name,cls", CASES)
def test_device_against_numpy(name, cls, mu):
    """every batch size, every world: the tolerance rule, free_count equal to NumPy's, and world b of a batch of B bit-identical to the
    same world alone and inside B = 130"""
    q, g, refs = _problem(name, cls)
    want, d, cnt, cond = refs[mu]
    full, full_cnt = _vjp(name, q, g, mu)
    err = float(np.abs(full - want).max())
    host = _host(name).vjp(q, g, mu)[0]
    print(f"[ik grad gpu] {name} / {cls} / mu = {mu:g}: |F| in [{cnt.min()}, {cnt.max()}], worst cond(J_F) {cond:.1f}, NumPy forms disagree by "
          f"{d:.3e}, device off by {err:.3e} (host build {float(np.abs(host - want).max()):.3e})")
    assert np.array_equal(full_cnt, cnt)
    if cls == "all_at_limit":
        assert not full.any() and (cnt == 0).all()
    assert np.isfinite(full).all()
    assert err <= 10.0 * d
    for B in BATCHES[:-1]:
        part, part_cnt = _vjp(name, q[:B], g[:B], mu)
        assert np.array_equal(part, full[:B]) and np.array_equal(part_cnt, cnt[:B]), B
    for b in (64, 129):
        one, _ = _vjp(name, q[b:b + 1], g[b:b + 1], mu)
        assert np.array_equal(one[0], full[b]), b


def test_accumulate_and_null_free_count():
    w, m = _device("atlas20_two")
    q, g, refs = _problem("atlas20_two", "one_at_limit")
    L, h, km = w._L, w._h, m._device_map(w)
    B, P = len(q), m.getPosDim()
    p = lambda x: C.c_void_p(x.data_ptr())
    qs, gs = w.to_soa(torch.tensor(q, device=DEV)), w.to_soa(torch.tensor(g, device=DEV))
    need = L.nbl_ik_grad_workspace_bytes(h, km, B)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    plain = torch.empty((P, B), dtype=torch.float64, device=DEV)
    free = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    assert L.nbl_ik_solve_vjp(h, km, B, p(qs), p(gs), 1e-9, p(plain), 0, p(free), p(ws), need, w._stream()) == 0
    base = torch.tensor(np.random.default_rng(4).normal(0, 1, (P, B)), device=DEV)
    acc = base.clone()
    assert L.nbl_ik_solve_vjp(h, km, B, p(qs), p(gs), 1e-9, p(acc), 1, None, p(ws), need, w._stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(acc, base + plain)
    assert np.array_equal(free.cpu().numpy(), refs[1e-9][2])
    assert np.array_equal(plain.t().cpu().numpy(), _vjp("atlas20_two", q, g, 1e-9)[0])


def test_argument_errors():
    import nimblephysics_amd as na
    from nimblephysics_amd._lib import check
    w, m = _device("pendulum")
    L, h, km = w._L, w._h, m._device_map(w)
    B = 8
    q = torch.zeros((1, B), dtype=torch.float64, device=DEV)
    out = torch.full((6, B), 7.0, dtype=torch.float64, device=DEV)
    need = L.nbl_ik_grad_workspace_bytes(h, km, B)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())
    assert need > 0 and L.nbl_ik_grad_workspace_bytes(None, km, B) == 0 and L.nbl_ik_grad_workspace_bytes(h, None, B) == 0
    assert L.nbl_ik_grad_workspace_bytes(h, km, 0) == 0
    for rc_want, call in ((-1, lambda: L.nbl_ik_solve_vjp(None, km, B, p(q), p(q), 1e-9, p(out), 0, None, p(ws), need, None)),
                          (-1, lambda: L.nbl_ik_solve_vjp(h, None, B, p(q), p(q), 1e-9, p(out), 0, None, p(ws), need, None)),
                          (-1, lambda: L.nbl_ik_solve_vjp(h, km, B, None, p(q), 1e-9, p(out), 0, None, p(ws), need, None)),
                          (-1, lambda: L.nbl_ik_solve_vjp(h, km, B, p(q), None, 1e-9, p(out), 0, None, p(ws), need, None)),
                          (-1, lambda: L.nbl_ik_solve_vjp(h, km, B, p(q), p(q), 1e-9, None, 0, None, p(ws), need, None)),
                          (-1, lambda: L.nbl_ik_solve_vjp(h, km, B, p(q), p(q), 1e-9, p(out), 0, None, None, need, None)),
                          (-1, lambda: L.nbl_ik_solve_vjp(h, km, -1, p(q), p(q), 1e-9, p(out), 0, None, p(ws), need, None)),
                          (-1, lambda: L.nbl_ik_solve_vjp(h, km, B, p(q), p(q), -1.0, p(out), 0, None, p(ws), need, None)),
                          (-2, lambda: L.nbl_ik_solve_vjp(h, km, B, p(q), p(q), 0.0, p(out), 0, None, p(ws), need, None)),
                          (-4, lambda: L.nbl_ik_solve_vjp(h, km, B, p(q), p(q), 1e-9, p(out), 0, None, p(ws), need - 1, None))):
        rc = call()
        assert rc == rc_want, (rc, rc_want)
        with pytest.raises(na.NimbleAmdError):
            check(rc, "ik grad")
        assert L.nbl_last_error()
    assert L.nbl_ik_solve_vjp(h, km, 0, None, None, 1e-9, None, 0, None, None, 0, None) == 0     # B = 0: a no-op
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                              # nothing was launched
    with pytest.raises(na.NimbleAmdError):
        na.solve_ik(w, m, torch.zeros(6, device=DEV), differentiable=True, grad_damping=0.0)


def _autograd(name, targets, init, device=DEV, **kw):
    import nimblephysics_amd as na
    w, m = _device(name)
    t = torch.tensor(targets, device=device, requires_grad=True)
    q, loss, steps = na.solve_ik(w, m, t, None if init is None else torch.tensor(init, device=device), na.IKConfig(max_step_count=200),
                                 differentiable=True, **kw)
    assert q.requires_grad and not loss.requires_grad and not steps.requires_grad
    state = torch.cat([q, torch.zeros_like(q)], -1)
    rows = na.map_to_pos(w, m, state)
    return t, q, rows


def test_autograd_end_to_end_equals_the_numpy_composition():
    """solve_ik(differentiable=True) -> map_to_pos -> a weighted sum: targets.grad = VJP(J^T w) by NumPy, under the tolerance rule"""
    name = "atlas20_two"
    md, entries = MODELS[name]
    h = _host(name)
    q0, _, _ = _problem(name, "interior")
    B = 65
    targets = h.evaluate(q0[:B], np.zeros((B, h.P)))[0]                 # reachable: the rows of poses inside the limits
    t, q, rows = _autograd(name, targets, q0[:B] + 0.05)
    wgt = torch.tensor(np.random.default_rng(6).normal(0, 1, (B, h.P)), device=DEV)
    (rows * wgt).sum().backward()
    qn = q.detach().cpu().numpy()
    J = h.evaluate(qn, targets)[1]
    gq = np.einsum("bpn,bp->bn", J, wgt.cpu().numpy())
    lo, hi = gc.limits(md)
    pr, du, cnt, cond = ign.vjp_batch(J, gq, qn, lo, hi, 1e-9)
    ok = cond <= gc.COND_MAX                                              # (the solver chose these poses; the rule speaks of the others)
    assert ok.sum() >= B // 2
    want = np.where((h.P < cnt)[:, None], du, pr)
    d = float(np.abs(pr - du)[ok].max())
    err = float(np.abs(t.grad.cpu().numpy() - want)[ok].max())
    print(f"[ik grad gpu] autograd on {name}: {int(ok.sum())} of {B} worlds with cond(J_F) <= 1e3, NumPy forms disagree by {d:.3e}, targets.grad off by {err:.3e}")
    assert err <= 10.0 * d


def test_on_a_reachable_square_case_the_gradient_is_the_upstream_gradient():
    """P = n, interior, converged: rows(q(t)) = t, so d loss / d t of sum(w * rows) is w itself (J J^+ = I) - to the tolerance rule's
    10 d plus the Tikhonov term's mu |w| / sigma_min^2, both measured here"""
    import nimblephysics_amd as na
    md, entries = ic.arm(3, (0.4, 0.3, 0.3)), [(2, 2)]
    w = na.World(md, device=DEV)
    m = na.IKMapping(w)
    m.addAngularBodyNode(2)
    h = gc.HostIKGrad(ic.load_ik_shim(), gc.load_grad_shim(), md, entries)
    B = 65
    q0 = np.random.default_rng(9).uniform(-0.6, 0.6, (B, 3))
    targets = h.evaluate(q0, np.zeros((B, 3)))[0]
    t = torch.tensor(targets, device=DEV, requires_grad=True)
    q, loss, _ = na.solve_ik(w, m, t, torch.tensor(q0 + 0.1, device=DEV), na.IKConfig(max_step_count=500, convergence_threshold=1e-12,
                                                                                      least_squares_damping=1e-10), differentiable=True)
    assert float(loss.max()) < 1e-20
    wgt = np.random.default_rng(10).normal(0, 1, (B, 3))
    rows = na.map_to_pos(w, m, torch.cat([q, torch.zeros_like(q)], -1))
    (rows * torch.tensor(wgt, device=DEV)).sum().backward()
    qn = q.detach().cpu().numpy()
    J = h.evaluate(qn, targets)[1]
    gq = np.einsum("bpn,bp->bn", J, wgt)
    lo, hi = gc.limits(md)
    pr, du, cnt, cond = ign.vjp_batch(J, gq, qn, lo, hi, 1e-9)
    smin = min(np.linalg.svd(Jb, compute_uv=False)[-1] for Jb in J)
    d = float(np.abs(pr - du).max())
    tol = 10.0 * d + 1e-9 * float(np.abs(wgt).sum(1).max()) / smin ** 2
    err = float(np.abs(t.grad.cpu().numpy() - wgt).max())
    print(f"[ik grad gpu] square reachable case: |targets.grad - upstream| {err:.3e}, allowed {tol:.3e} (forms disagree by {d:.3e}, sigma_min {smin:.3f})")
    assert (cnt == 3).all() and cond.max() <= gc.COND_MAX
    assert err <= tol


def test_cpu_tensors_in_and_out():
    import nimblephysics_amd as na
    name = "atlas20_two"
    q0, g, _ = _problem(name, "interior")
    h = _host(name)
    targets = h.evaluate(q0[:8], np.zeros((8, h.P)))[0]
    td, qd, rd = _autograd(name, targets, q0[:8] + 0.05)
    tc, qc, rc = _autograd(name, targets, q0[:8] + 0.05, device="cpu")
    assert qc.device.type == "cpu" and torch.equal(qc.detach(), qd.detach().cpu())
    qd.sum().backward(); qc.sum().backward()
    assert tc.grad.device.type == "cpu" and torch.equal(tc.grad, td.grad.cpu())
    w, m = _device(name)
    gt, free = na.solve_ik_vjp(w, m, torch.tensor(q0[:8]), torch.tensor(g[:8]))
    assert gt.device.type == "cpu" and free.device.type == "cpu"
    assert np.array_equal(gt.numpy(), _vjp(name, q0[:8], g[:8], 1e-9)[0])
    one, f1 = na.solve_ik_vjp(w, m, torch.tensor(q0[3]), torch.tensor(g[3]))          # [n] -> [P]
    assert one.shape == (h.P,) and f1.dim() == 0 and torch.equal(one, gt[3])


def test_a_chunked_batch_equals_the_whole_one(monkeypatch):
    from nimblephysics_amd import mapping as mp
    name = "atlas20_two"
    q, g, _ = _problem(name, "one_at_limit")
    whole = _vjp(name, q, g, 1e-9)
    w, m = _device(name)
    per = w._L.nbl_ik_grad_workspace_bytes(w._h, m._device_map(w), 1)
    monkeypatch.setattr(mp, "IK_WORKSPACE_BYTES", 64 * per)             # launches of 64 worlds: 64 + 64 + 2
    w._ik_ws = None
    cut = _vjp(name, q, g, 1e-9)
    assert w._ik_ws.numel() == 64 * per
    assert np.array_equal(cut[0], whole[0]) and np.array_equal(cut[1], whole[1])
    h = _host(name)
    targets = h.evaluate(q[:130], np.zeros((130, h.P)))[0]
    t, qq, _ = _autograd(name, targets, q + 0.05)
    qq.sum().backward()
    monkeypatch.undo()
    w._ik_ws = None
    t2, qq2, _ = _autograd(name, targets, q + 0.05)
    qq2.sum().backward()
    assert torch.equal(qq.detach(), qq2.detach()) and torch.equal(t.grad, t2.grad)


def test_deferred_join_world():
    import nimblephysics_amd as na
    md = na.atlas("atlas20", ground=True)
    plain, entries = MODELS["atlas20_two"]
    q, g, _ = _problem("atlas20_two", "one_at_limit")
    want = _vjp("atlas20_two", q[:64], g[:64], 1e-9)
    B = 4096
    dw = na.World(md, device=DEV)
    m = na.IKMapping(dw)
    for kind, body in entries:
        m.addSpatialBodyNode(plain.bodies[body].name)
    dw.set_deferred_join(True)
    assert dw.slices_for(B) > 1
    n = md.num_dofs
    rng = np.random.default_rng(8)
    S = np.zeros((B, 2 * n)); S[:, 0] = -np.pi / 2; S[:, 4] = 1.0; S[:, 6:n] = rng.normal(0, 0.02, (B, n - 6))
    s_soa = dw.to_soa(torch.tensor(S, device=DEV)); a_soa = dw.to_soa(torch.zeros((B, dw.k), dtype=torch.float64, device=DEV))
    buf = {"nxt": torch.empty_like(s_soa), "saved": torch.empty(dw.saved_bytes(B), dtype=torch.uint8, device=DEV),
           "status": torch.empty(B, dtype=torch.int32, device=DEV), "cache": torch.empty((dw.m, B), dtype=torch.float64, device=DEV)}
    dw.step_into(s_soa, a_soa, buf["nxt"], buf["saved"], buf["status"], None, buf["cache"])       # slices in flight
    gt, free = na.solve_ik_vjp(dw, m, torch.tensor(q[:64], device=DEV), torch.tensor(g[:64], device=DEV))
    assert np.array_equal(gt.cpu().numpy(), want[0]) and np.array_equal(free.cpu().numpy(), want[1])
    dw.join()
    torch.cuda.synchronize()


def test_immobile_skeleton_world(tmp_path):
    import nimblephysics_amd as na
    from test_ref_layout import load
    md = load(tmp_path)
    w = na.World(md, device=DEV)
    assert w.ref_layout is not None and w.n == 6
    mobile = [b.name for b in md.bodies if b.skeleton not in set(md.immobile_skeletons or ())]
    m = na.IKMapping(w)
    m.addSpatialBodyNode(mobile[-1])
    rng = np.random.default_rng(2)
    full = np.zeros((8, 24)); full[:, 6:12] = rng.normal(0, 0.3, (8, 6))
    target = na.map_to_pos(w, m, torch.tensor(full, device=DEV)).detach().requires_grad_(True)
    q, loss, steps = na.solve_ik(w, m, target, None, na.IKConfig(max_step_count=100), differentiable=True)
    assert q.shape == (8, 6)                                            # over the mobile coordinates, as solve_ik returns them
    gq = torch.tensor(rng.normal(0, 1, (8, 6)), device=DEV)
    (q * gq).sum().backward()
    gt, free = na.solve_ik_vjp(w, m, q.detach(), gq)
    assert torch.equal(target.grad, gt) and target.grad.shape == (8, 6) and bool(target.grad.abs().sum() > 0)
    wide = torch.zeros((8, 12), dtype=torch.float64, device=DEV); wide[:, 6:] = q.detach()      # the reference's layout
    wide_g = torch.zeros_like(wide); wide_g[:, 6:] = gq
    gt2, _ = na.solve_ik_vjp(w, m, wide, wide_g)
    assert torch.equal(gt2, gt)
