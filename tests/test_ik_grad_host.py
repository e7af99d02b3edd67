"""The reverse pass of the PRODUCT's inverse kinematics (nimblephysics_amd/csrc/ik_grad_dev.hpp: what k_ik_solve_vjp runs per lane)
compiled for the host with g++ (tests/host_shim/ik_grad_shim.cpp), against
  * tests/ik_grad_numpy.py, the convention of include/nimble_amd.h by numpy.linalg.solve, under the tolerance rule of
    tests/ik_grad_cases.py (10 x the disagreement of the two NumPy forms on the same inputs, every pose with cond(J_F) <= 1e3);
  * the host build of the solver itself: central differences of nbl_ik_solve's result in the target, on a converged square problem;
and the Python surface of solve_ik(differentiable=...) / solve_ik_vjp on a stand-in World (no device needed).
Measured on the cases below (B = 12 worlds each): the two NumPy forms disagree by 0 (every coordinate clamped) up to 1.4e-5 (the redundant
arm at mu = 1e-9, where the |F| x |F| form is singular but for mu); the host build is at most 1.95 of that disagreement away (the limited
seven-link arm with one coordinate clamped, P = |F| = 6: 2.4e-10 against 1.3e-10), 10 being allowed."""
import types

import numpy as np
import pytest
import torch

import ik_cases as ic
import ik_grad_cases as gc
import ik_grad_numpy as ign

B = 12
MODELS = gc.models()
CASES = [(name, cls) for name, (md, entries) in MODELS.items()
         for cls in gc.case_classes(md, sum(ic.ROWS[k] for k, _ in entries))]


@pytest.fixture(scope="module")
def hosts():
    solver, grad = ic.load_ik_shim(), gc.load_grad_shim()
    return {name: gc.HostIKGrad(solver, grad, md, entries) for name, (md, entries) in MODELS.items()}


def test_the_cases_cover_what_they_must():
    """P = n, P < n and P > n; a model without limits; every class; the smaller side changed by clamping (|F| < P <= n)"""
    dims = {name: (sum(ic.ROWS[k] for k, _ in entries), md.num_dofs) for name, (md, entries) in MODELS.items()}
    assert any(P == n for P, n in dims.values()) and any(P < n for P, n in dims.values()) and any(P > n for P, n in dims.values())
    assert any(not np.isfinite(gc.limits(md)[0]).any() and not np.isfinite(gc.limits(md)[1]).any() for md, _ in MODELS.values())
    for cls in ("interior", "one_at_limit", "all_at_limit", "fewer_free_than_rows"):
        assert any(c == cls for _, c in CASES), cls
    assert ("limited_arm3", "fewer_free_than_rows") in CASES and ("limited_arm7", "fewer_free_than_rows") in CASES


@pytest.mark.parametrize("mu", gc.MUS)
@pytest.mark.parametrize("name,cls", CASES)
def test_host_build_against_numpy(hosts, name, cls, mu):
    md, entries = MODELS[name]
    h = hosts[name]
    q, g = gc.problem(h, md, entries, cls, B, gc.SEED + CASES.index((name, cls)))
    want, d, cnt, cond = gc.reference(h, md, q, g, mu)
    got, got_cnt = h.vjp(q, g, mu)
    err = float(np.abs(got - want).max())
    print(f"[ik grad host] {name} / {cls} / mu = {mu:g}: |F| in [{cnt.min()}, {cnt.max()}], P = {h.P}, n = {h.n}, worst cond(J_F) {cond:.1f}, "
          f"NumPy forms disagree by {d:.3e}, host build off by {err:.3e}")
    assert np.array_equal(got_cnt, cnt)
    n = md.num_dofs
    if cls == "interior":
        assert (cnt == n).all()
    elif cls == "one_at_limit":
        assert (cnt == n - 1).all()
    elif cls == "all_at_limit":
        assert (cnt == 0).all() and not got.any() and d == 0.0          # exact zeros
    else:
        assert (cnt == h.P - 1).all() and h.P <= n                       # |F| < P <= n: the side is |F|, not min(P, n)
    assert np.isfinite(got).all()
    assert err <= 10.0 * d


def test_accumulate_adds_bit_for_bit(hosts):
    md, entries = MODELS["free_ball_tree"]
    h = hosts["free_ball_tree"]
    q, g = gc.problem(h, md, entries, "one_at_limit", B, gc.SEED + 77)
    plain, _ = h.vjp(q, g, 1e-9)
    base = np.random.default_rng(3).normal(0, 1, plain.shape)
    acc, _ = h.vjp(q, g, 1e-9, accumulate_into=base)
    assert np.array_equal(acc, base + plain)


def test_the_convention_is_the_derivative_of_the_solve_where_one_exists():
    """An elbow arm (yaw, shoulder, elbow; two unit links) with a LINEAR entry on its tip: P = n = 3, no limits (an interior solution),
    a reachable target, the host solver run to convergence (convergence_threshold 1e-12, 2000 steps; least_squares_damping 1e-10 and a
    start 0.05 rad away, because refineIK's ladder stops a run once its loss changes by less than the threshold, which the default
    damping 0.01 reaches well above 1e-20) and checked to have converged: loss < 1e-20.  Central differences of the solve in the target
    with h = 1e-5 against the VJP at mu = 1e-9; the differences' own noise is what h and h / 2 disagree by, and the VJP is allowed 10 x
    that.

    WHY THIS CASE.  The convention carries its own Tikhonov term: along a singular direction J (J^T J + mu I)^-1 g differs from J^-T g by
    mu g / sigma^3.  The yardstick's noise is truncation, (h^2 / 8) q''' g with q''' the third derivative of the solve in the target, and
    the differences themselves are (h^2 / 6) q''' g = 4/3 of that noise away from the derivative.  The comparison says something at
    10 x the noise only where mu / sigma^3 stays below a few times (h^2 / 8) q'''.  On a generic pose both scale as 1 / sigma^3 and the
    Tikhonov term wins (measured on the angular three-link arm of ik_cases, cond 1.3: noise 4.2e-11, VJP 1.6e-9 away, 37 x - all of it
    the Tikhonov term: with mu = 1e-12 it is 1.7e-11), so the case must be one where the solve is strongly curved.  An elbow bent by q2
    from straight has reach R - c q2^2 / 2 with c = l1 l2 / (l1 + l2) = 1/2: along the reach sigma = c q2 and q''' = 3 c^2 / sigma^5, so
    the Tikhonov term is (8 mu / 3 h^2 c^2) sigma^2 = 26.7 q2^2 times the noise.  q2 = 0.2 predicts 1.1, plus the 4/3 of the
    differences' own truncation: 2.4 of the 10 allowed, at cond(J) = 25 (sigma_min = 0.089).  Measured: noise 3.1e-7, VJP 1.0e-6 away,
    3.2 x."""
    import nimblephysics_amd as na
    axes, lengths = [(0, 0, 1), (0, 1, 0), (0, 1, 0)], [0.0, 1.0, 1.0]
    md = na.ModelDescription("elbow3", [na.BodySpec(f"link{i}", i - 1, "revolute", f"joint{i}", axis=axes[i], T_pj=np.eye(4),
                                                    T_cj=ic._tr(-lengths[i], 0, 0)) for i in range(3)], [], max_contacts=0)
    entries = [(1, 2)]
    h = gc.HostIKGrad(ic.load_ik_shim(), gc.load_grad_shim(), md, entries)
    q0 = np.array([0.4, -0.5, 0.2])
    t0 = h.evaluate(q0[None], np.zeros((1, 3)))[0][0]                    # rows(q0): reachable
    cfg = dict(convergence_threshold=1e-12, max_step_count=2000, least_squares_damping=1e-10)

    def solve(t):
        t = np.atleast_2d(t)
        q, loss, _ = h.solve(t, init=np.repeat((q0 + 0.05)[None], len(t), 0), **cfg)
        return q, loss

    qs, loss = solve(t0)
    assert loss[0] < 1e-20, loss
    s = np.linalg.svd(h.evaluate(qs, t0[None])[1][0], compute_uv=False)
    assert s[0] / s[-1] <= gc.COND_MAX
    lo, hi = gc.limits(md)
    assert ign.free_set(qs[0], lo, hi).all()

    def jac(step):                                                       # d q / d t, [n, P]
        q, l = solve(np.concatenate([t0 + step * np.eye(3), t0 - step * np.eye(3)]))
        assert (l < 1e-20).all(), l
        return ((q[:3] - q[3:]) / (2 * step)).T

    D1, D2 = jac(1e-5), jac(0.5e-5)
    g = np.random.default_rng(11).normal(0, 1, (1, 3))
    fd1, fd2 = D1.T @ g[0], D2.T @ g[0]
    noise = float(np.abs(fd1 - fd2).max())
    got, cnt = h.vjp(qs, g, 1e-9)
    err = float(np.abs(got[0] - fd1).max())
    print(f"[ik grad host] solver differences: cond(J) {s[0] / s[-1]:.1f}, h against h / 2 {noise:.3e}, VJP against the differences {err:.3e}, "
          f"|grad_t| {np.abs(got).max():.3f}")
    assert cnt[0] == 3
    assert err <= 10.0 * noise


# ---- the Python surface, on a stand-in World (what solve_ik touches of one), with the two device calls replaced ----------------------------
class _World:
    n, device, ref_layout, _deferred = 3, torch.device("cpu"), None, False

    def to_soa(self, x):
        return x.t().contiguous()

    def from_soa(self, x):
        return x.t().contiguous()

    def _prep(self, x, width, what):
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.dim() != 2 or x.shape[1] != width:
            raise ValueError(f"{what}: {tuple(x.shape)}")
        return x.detach().to(torch.float64)

    def _to_host(self, *t):
        return t[0] if len(t) == 1 else t


@pytest.fixture
def surface(monkeypatch):
    from nimblephysics_amd import mapping as mp
    md, entries = MODELS["arm3_linear"]
    world = _World()
    m = mp.IKMapping(types.SimpleNamespace(description=md))
    m.addLinearBodyNode(entries[0][1])
    calls = {"solve": 0, "vjp": []}

    def solve(w, mapping, t_soa, init_soa, config):
        calls["solve"] += 1
        Bn = t_soa.shape[1]
        return 2.0 * t_soa.clone(), torch.zeros(Bn, dtype=torch.float64), torch.ones(Bn, dtype=torch.int32)

    def vjp(w, mapping, q_soa, g_soa, mu):
        calls["vjp"].append((tuple(q_soa.shape), tuple(g_soa.shape), mu))
        return 3.0 * g_soa.clone(), torch.full((q_soa.shape[1],), 3, dtype=torch.int32)

    monkeypatch.setattr(mp, "_solve_ik_soa", solve)
    monkeypatch.setattr(mp, "_solve_ik_vjp_soa", vjp)
    return mp, world, m, calls


def test_not_differentiable_by_default(surface):
    mp, world, m, calls = surface
    t = torch.zeros((4, 3), dtype=torch.float64, requires_grad=True)
    for out in (mp.solve_ik(world, m, t), mp.solve_ik(world, m, t, differentiable=False, grad_damping=0.0)):   # (grad_damping is not read)
        assert len(out) == 3
        for x in out:
            assert x.grad_fn is None and not x.requires_grad
    assert calls["solve"] == 2 and not calls["vjp"]


def test_differentiable_carries_the_gradient_to_the_targets_only(surface):
    mp, world, m, calls = surface
    t = torch.ones((4, 3), dtype=torch.float64, requires_grad=True)
    init = torch.zeros((4, 3), dtype=torch.float64, requires_grad=True)
    q, loss, steps = mp.solve_ik(world, m, t, init, differentiable=True, grad_damping=1e-3)
    assert q.requires_grad and q.grad_fn is not None and not loss.requires_grad and not steps.requires_grad
    w = torch.arange(12, dtype=torch.float64).reshape(4, 3)
    (q * w).sum().backward()
    assert calls["vjp"] == [((3, 4), (3, 4), 1e-3)]
    assert torch.equal(t.grad, 3.0 * w) and init.grad is None            # no gradient to init
    one = torch.ones(3, dtype=torch.float64, requires_grad=True)         # a [P] target
    q1, l1, s1 = mp.solve_ik(world, m, one, differentiable=True)
    assert q1.shape == (3,) and l1.dim() == 0 and s1.dim() == 0
    q1.sum().backward()
    assert one.grad.shape == (3,) and calls["vjp"][-1] == ((3, 1), (3, 1), 1e-9)
    fixed = mp.solve_ik(world, m, torch.ones((2, 3), dtype=torch.float64), differentiable=True)[0]
    assert not fixed.requires_grad                                        # nothing to differentiate to


def test_surface_errors(surface):
    from nimblephysics_amd import NimbleAmdError
    mp, world, m, calls = surface
    t = torch.ones((4, 3), dtype=torch.float64, requires_grad=True)
    with pytest.raises(NimbleAmdError):
        mp.solve_ik(world, m, t, differentiable=True, grad_damping=0.0)
    with pytest.raises(ValueError):
        mp.solve_ik(world, m, t, differentiable=True, grad_damping=-1.0)
    with pytest.raises(ValueError):
        mp.solve_ik(world, m, t, differentiable=True, grad_damping=float("nan"))
    assert calls["solve"] == 0                                           # refused before anything is solved
    with pytest.raises(ValueError):
        mp.solve_ik(world, m, torch.ones((4, 5), dtype=torch.float64), differentiable=True)
    with pytest.raises(ValueError):
        mp.solve_ik(world, m, t, torch.zeros((3, 3), dtype=torch.float64), differentiable=True)
    q = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(NimbleAmdError):
        mp.solve_ik_vjp(world, m, q, q, grad_damping=0.0)
    with pytest.raises(ValueError):
        mp.solve_ik_vjp(world, m, q, q[:3])
    with pytest.raises(ValueError):
        mp.solve_ik_vjp(world, m, q, q[0])
    with pytest.raises(ValueError):
        mp.solve_ik_vjp(world, m, torch.zeros((4, 2), dtype=torch.float64), torch.zeros((4, 2), dtype=torch.float64))
    gt, free = mp.solve_ik_vjp(world, m, q, torch.ones_like(q))
    assert gt.shape == (4, 3) and free.shape == (4,) and free.dtype == torch.int32 and gt.grad_fn is None
    gt1, free1 = mp.solve_ik_vjp(world, m, q[0], torch.ones(3, dtype=torch.float64))
    assert gt1.shape == (3,) and free1.dim() == 0
