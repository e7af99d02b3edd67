"""Gradients of the batched dynamics calls to the registered inertia parameters on the device (k_inverse_dynamics_inertia_vjp through
nimblephysics_amd/dynamics.py: inverse_dynamics_mass_gradient / _jacobian, forward_dynamics_mass_gradient / _jacobian and the mass= keyword
of the six joint-space functions) against the exact reference of tests/dynmass_ref.py: central differences of the CPU oracle's inverse
dynamics in parameters it is linear (the centre of mass: quadratic) in, D, after D at h and at h / 2 agreed to 1e-11 max(1, |D|); for
forward dynamics the identity -M_o^-1 D(q, v, a).  Every world and every parameter is held to max|x - ref| / max(1, |ref|) <= 1e-10, the
bound of tests/test_gpu_dynamics.py and tests/test_gpu_forward_dynamics.py.

B = 130: two full wavefronts and a two-lane tail across a block boundary of DYN_BLOCK = 64.  The reference of a model is computed once
(_case) and shared."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B = 130
NAMES = ["free_below_root", "ball_arm", "cartpole", "atlas20"]


def _model(name):
    import nimblephysics_amd as na
    from nimblephysics_amd.mass import WrtMassBodyNodeEntryType as T
    from test_ball_joint import ball_model
    from test_dynamics_host import free_below_root
    if name == "free_below_root":                              # a free joint below the root, a ball joint at a leaf
        return free_below_root(), [("base", T.INERTIA_DIAGONAL), ("floater", T.INERTIA_FULL), ("wrist", T.INERTIA_COM_MU), ("slider", T.INERTIA_MASS)]
    if name == "ball_arm":
        md = ball_model(2, True)
        return md, [(0, T.INERTIA_COM), (len(md.bodies) - 1, T.INERTIA_OFF_DIAGONAL), (1, T.INERTIA_MASS)]
    if name == "cartpole":
        return na.cartpole(), [(0, T.INERTIA_MASS), (1, T.INERTIA_FULL)]
    md = na.atlas("atlas20")
    foot = next(i for i, b in enumerate(md.bodies) if "foot" in b.name and b.joint_type != "weld")
    return md, [(foot, T.INERTIA_FULL), (0, T.INERTIA_MASS)]


def _states(md, nB, seed):
    rng = np.random.default_rng(seed)
    n = md.num_dofs
    return np.concatenate([rng.normal(0, 0.5, (nB, n)), rng.normal(0, 1.0, (nB, n))], 1), rng.normal(0, 2.0, (nB, n)), rng.normal(0, 1.0, (nB, n))


def _world(md, entries):
    import nimblephysics_amd as na
    w = na.World(copy.deepcopy(md), device=DEV)              # (setMasses writes into the description: the shared case stays as it is)
    for b, t in entries:
        w.tuneMass(b, t)
    return w


@functools.lru_cache(maxsize=None)
def _case(name):
    """the model with its COM_MU bodies on their line, its entries, B states, and D at flags 0 on every world (computed once; read only)"""
    from dynmass_ref import InertiaReference, on_the_mu_line
    md, entries = _model(name)
    md = on_the_mu_line(md, entries)
    ref = InertiaReference(md, entries)
    S, A, g = _states(md, B, 71)
    n = md.num_dofs
    D = np.stack([ref.checked_D(S[b, :n], S[b, n:], A[b]) for b in range(B)])
    D.setflags(write=False)
    return dict(md=md, entries=entries, ref=ref, S=S, A=A, g=g, D=D, n=n)


def _t(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


@pytest.mark.parametrize("name", NAMES)
def test_inverse_dynamics_mass_gradient_and_jacobian_equal_the_exact_differences(name):
    import nimblephysics_amd as na
    from dynmass_ref import JOINT_FORCES, NO_GRAVITY, NO_VELOCITY, TOL, rel
    from nimblephysics_amd.dynamics import inverse_dynamics_inertia_vjp_soa
    c = _case(name)
    md, ref, S, A, g, D, n = c["md"], c["ref"], c["S"], c["A"], c["g"], c["D"], c["n"]
    w = _world(md, c["entries"])
    st, at, gt = _t(S), _t(A), _t(g)
    got = na.inverse_dynamics_mass_gradient(w, st, at, gt).cpu().numpy()
    got_jf = na.inverse_dynamics_mass_gradient(w, st, at, gt, joint_forces=True).cpu().numpy()
    J = na.inverse_dynamics_mass_jacobian(w, st, at).cpu().numpy()
    assert got.shape == (B, ref.P) and J.shape == (B, n, ref.P)
    s_soa, a_soa, g_soa = w.to_soa(st), w.to_soa(at), w.to_soa(gt)
    flagged = {fl: inverse_dynamics_inertia_vjp_soa(w, s_soa, a, g_soa, fl).t().cpu().numpy()
               for fl, a in ((NO_VELOCITY, a_soa), (NO_GRAVITY, a_soa), (JOINT_FORCES, a_soa), (0, None))}
    worst = {}
    for b in range(B):
        q, v, a = S[b, :n], S[b, n:], A[b]
        e = {"grad": rel(got[b], D[b].T @ g[b]), "grad jf": rel(got_jf[b], D[b].T @ g[b]), "jac": rel(J[b], D[b]),
             "no velocity": rel(flagged[NO_VELOCITY][b], ref.checked_D(q, v, a, NO_VELOCITY).T @ g[b]),
             "no gravity": rel(flagged[NO_GRAVITY][b], ref.checked_D(q, v, a, NO_GRAVITY).T @ g[b]),
             "joint forces": rel(flagged[JOINT_FORCES][b], D[b].T @ g[b]),
             "accel None": rel(flagged[0][b], ref.checked_D(q, v, None).T @ g[b])}
        for k, x in e.items():
            worst[k] = max(worst.get(k, 0.0), x)
        assert max(e.values()) <= TOL, (name, b, e)
    print(name, "worst over", B, "worlds:", worst)
    assert np.abs(got).max() > 0


@pytest.mark.parametrize("name", NAMES)
def test_forward_dynamics_mass_gradient_and_jacobian_equal_minus_minv_d(name):
    """a from the oracle's forward_dynamics (it carries the joint forces: joint_forces=True here); with wrenches, a from the device's own
    forward call, which tests/test_gpu_wrench.py holds to the oracle."""
    import nimblephysics_amd as na
    from dynmass_ref import TOL, rel
    c = _case(name)
    md, ref, S, n = c["md"], c["ref"], c["S"], c["n"]
    w = _world(md, c["entries"])
    ow = ref.world()
    rng = np.random.default_rng(72)
    tau, g = rng.normal(0, 2.0, (B, n)), rng.normal(0, 1.0, (B, n))
    st, tt, gt = _t(S), _t(tau), _t(g)
    got = na.forward_dynamics_mass_gradient(w, st, tt, gt, joint_forces=True).cpu().numpy()
    J = na.forward_dynamics_mass_jacobian(w, st, tt, joint_forces=True).cpu().numpy()
    bodies = [len(md.bodies) - 1, 0]
    W = rng.normal(0, 1.0, (B, 12))
    wr = {}
    for frame in (False, True):
        acc = na.forward_dynamics(w, st, tt, wrenches=_t(W), bodies=bodies, world_frame=frame).cpu().numpy()
        wr[frame] = (acc, na.forward_dynamics_mass_gradient(w, st, tt, gt, wrenches=_t(W), bodies=bodies, world_frame=frame).cpu().numpy())
    worst = {}
    for b in range(B):
        q, v = S[b, :n], S[b, n:]
        Jo = ref.fd_jacobian(q, v, ow.forward_dynamics(q, v, tau[b]))
        e = {"grad": rel(got[b], Jo.T @ g[b]), "jac": rel(J[b], Jo)}
        for frame in (False, True):
            e["wrench world" if frame else "wrench body"] = rel(wr[frame][1][b], ref.fd_jacobian(q, v, wr[frame][0][b]).T @ g[b])
        for k, x in e.items():
            worst[k] = max(worst.get(k, 0.0), x)
        assert max(e.values()) <= TOL, (name, b, e)
    print(name, "worst over", B, "worlds:", worst)


def _mass_tensor(w):
    return w.getMasses().clone().requires_grad_(True)


@pytest.mark.parametrize("name", NAMES)
def test_autograd_through_mass_sums_the_per_world_results_and_changes_no_other_bit(name):
    import nimblephysics_amd as na
    from dynmass_ref import TOL, rel
    c = _case(name)
    md, ref, S, A, g, n = c["md"], c["ref"], c["S"], c["A"], c["g"], c["n"]
    w = _world(md, c["entries"])
    rng = np.random.default_rng(73)
    G = rng.normal(0, 1.0, (B, n, n))
    X = rng.normal(0, 1.0, (B, n, 2))
    GX = rng.normal(0, 1.0, (B, n, 2))

    def run(fn, args, cot, with_mass):
        leaves = [_t(a).requires_grad_(True) for a in args]
        mass = _mass_tensor(w) if with_mass else None
        out = fn(w, *leaves, mass=mass) if with_mass else fn(w, *leaves)
        out.backward(_t(cot))
        return out.detach(), [x.grad for x in leaves], (mass.grad if with_mass else None)

    def same(fn, args, cot):
        o0, g0, _ = run(fn, args, cot, False)
        o1, g1, gm = run(fn, args, cot, True)
        assert torch.equal(o0, o1) and all(torch.equal(x, y) for x, y in zip(g0, g1)), fn.__name__
        assert gm.shape == (ref.P,) and gm.device.type == "cpu"
        return gm.numpy()

    st, at, gt = _t(S), _t(A), _t(g)
    # the vector functions: the per-world results, summed
    gm = same(na.inverse_dynamics, (S, A), g)
    per = na.inverse_dynamics_mass_gradient(w, st, at, gt).sum(0).cpu().numpy()
    assert rel(gm, per) <= 1e-13
    gm = same(na.coriolis_and_gravity, (S,), g)
    assert rel(gm, na.inverse_dynamics_mass_gradient(w, st, None, gt).sum(0).cpu().numpy()) <= 1e-13
    gm = same(na.forward_dynamics, (S, A), g)
    assert rel(gm, na.forward_dynamics_mass_gradient(w, st, at, gt).sum(0).cpu().numpy()) <= 1e-13
    # the matrices: d <G, M> / d theta by the same exact differences of the oracle's mass matrix (column j of M is ID(q, 0, e_j) without
    # gravity), d <G, M^-1> = -<M^-T G M^-T, dM>
    gM = same(na.mass_matrix, (S,), G)
    gMi = same(na.inv_mass_matrix, (S,), G)
    gY = same(na.multiply_by_inv_mass_matrix, (S, X), GX)
    want_M, want_Mi, want_Y = np.zeros(ref.P), np.zeros(ref.P), np.zeros(ref.P)
    for b in range(B):
        q = S[b, :n]
        Mi = np.linalg.inv(ref.world().mass_matrix(q))
        for p in range(ref.P):
            dM = (ref.world(True, p, ref.h[p]).mass_matrix(q) - ref.world(True, p, -ref.h[p]).mass_matrix(q)) / (2 * ref.h[p])
            want_M[p] += (G[b] * dM).sum()
            want_Mi[p] -= ((Mi.T @ G[b] @ Mi.T) * dM).sum()
            want_Y[p] -= ((Mi.T @ GX[b] @ (Mi @ X[b]).T) * dM).sum()
    e = {"M": rel(gM, want_M), "Minv": rel(gMi, want_Mi), "Minv x": rel(gY, want_Y)}
    print(name, e)
    assert max(e.values()) <= TOL, (name, e)
    # ... and device against device: the per-world gradients of their columns (world b, column r: a = y_r, the cotangent c_r, no
    # velocity, no gravity), summed.  Another order of summation than the launch over R x B worlds: 1e-12, not bits.
    from nimblephysics_amd.dynamics import ID_NO_GRAVITY, ID_NO_VELOCITY, inverse_dynamics_inertia_vjp_soa
    s_soa = w.to_soa(st)

    def columns(Y, Cot):                                          # [B, n, R] each
        tot = torch.zeros(ref.P, dtype=torch.float64, device=DEV)
        for r in range(Y.shape[2]):
            tot += inverse_dynamics_inertia_vjp_soa(w, s_soa, Y[:, :, r].t().contiguous(), Cot[:, :, r].t().contiguous(), ID_NO_VELOCITY | ID_NO_GRAVITY).sum(1)
        return tot.cpu().numpy()
    Gt, Xt, GXt = _t(G), _t(X), _t(GX)
    Minv = na.inv_mass_matrix(w, st)
    d = {"M": rel(gM, columns(torch.eye(n, dtype=torch.float64, device=DEV).expand(B, n, n), Gt)),
         "Minv": rel(gMi, columns(Minv, -(Minv @ Gt))), "Minv x": rel(gY, columns(Minv @ Xt, -(Minv @ GXt)))}
    assert max(d.values()) <= 1e-12, (name, d)
    # forward_dynamics(..., wrenches=, mass=) through autograd: the per-world results with the same wrenches, summed
    bodies = [len(md.bodies) - 1]
    Wt = _t(rng.normal(0, 1.0, (B, 6)))
    for frame in (False, True):
        mass = _mass_tensor(w)
        na.forward_dynamics(w, st, at, wrenches=Wt, bodies=bodies, world_frame=frame, mass=mass).backward(gt)
        per = na.forward_dynamics_mass_gradient(w, st, at, gt, wrenches=Wt, bodies=bodies, world_frame=frame).sum(0).cpu().numpy()
        assert rel(mass.grad.numpy(), per) <= 1e-13 and np.abs(per).max() > 0, frame


@pytest.mark.parametrize("name", ["cartpole", "ball_arm"])
def test_gradcheck_through_mass(name):
    import nimblephysics_amd as na
    c = _case(name)
    w = _world(c["md"], c["entries"])
    S, A, _ = _states(c["md"], 3, 4)        # the states the gradchecks of tests/test_gpu_dynamics.py and test_gpu_forward_dynamics.py run on
    st, at = _t(S).requires_grad_(True), _t(A).requires_grad_(True)
    m = w.getMasses().clone().to(DEV).requires_grad_(True)
    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradcheck(lambda s, a, mm: na.inverse_dynamics(w, s, a, mass=mm), (st, at, m), **kw)
    assert torch.autograd.gradcheck(lambda s, mm: na.coriolis_and_gravity(w, s, mass=mm), (st, m), **kw)
    assert torch.autograd.gradcheck(lambda s, mm: na.mass_matrix(w, s, mass=mm), (st, m), **kw)
    assert torch.autograd.gradcheck(lambda s, a, mm: na.forward_dynamics(w, s, a, mass=mm), (st, at, m), **kw)
    assert torch.autograd.gradcheck(lambda s, a, mm: na.multiply_by_inv_mass_matrix(w, s, a, mass=mm), (st, at, m), **kw)
    assert torch.autograd.gradcheck(lambda s, mm: na.inv_mass_matrix(w, s, mass=mm), (st, m), **kw)


def test_euler_identity_mass_weighted_jacobian_columns_give_tau():
    """tau is homogeneous of degree 1 in the masses (INERTIA_MASS rescales the moments): sum_p m_p J[:, :, p] = inverse_dynamics(...),
    device against device, 1e-12 relative."""
    import nimblephysics_amd as na
    from nimblephysics_amd.mass import WrtMassBodyNodeEntryType as T
    for name in ("free_below_root", "atlas20"):
        md = _case(name)["md"]
        S, A, _ = _states(md, B, 75)
        w = _world(md, [(i, T.INERTIA_MASS) for i in range(len(md.bodies))])
        J = na.inverse_dynamics_mass_jacobian(w, _t(S), _t(A))
        tau = na.inverse_dynamics(w, _t(S), _t(A))
        got = (J * w.getMasses().to(DEV)).sum(-1)
        assert float((got - tau).abs().max()) <= 1e-12 * max(1.0, float(tau.abs().max())), name


def test_a_wrench_changes_nothing_and_set_masses_moves_the_reference():
    import nimblephysics_amd as na
    from dynmass_ref import InertiaReference, TOL, rel
    c = _case("free_below_root")
    md, S, A, g, n = c["md"], c["S"], c["A"], c["g"], c["n"]
    w = _world(md, c["entries"])
    st, at, gt = _t(S), _t(A), _t(g)
    W = _t(np.random.default_rng(76).normal(0, 1.0, (B, 6)))
    grads = []
    for kw in ({}, dict(wrenches=W, bodies=["wrist"]), dict(wrenches=W, bodies=["wrist"], world_frame=True)):
        m = _mass_tensor(w)
        na.inverse_dynamics(w, st, at, mass=m, **kw).backward(gt)
        grads.append(m.grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    # new values, the centre of mass of the FULL body moved: the gradient is the oracle's at the new values
    x = w.getMasses().numpy().copy()
    x[3] *= 1.4; x[4:7] += np.array([0.03, -0.02, 0.05]); x[7:10] *= 1.2
    w.setMasses(torch.tensor(x))
    ref2 = InertiaReference(w.getWrtMass().description, c["entries"])
    assert np.allclose(ref2.x0, x)
    got = na.inverse_dynamics_mass_gradient(w, st[:8], at[:8], gt[:8]).cpu().numpy()
    for b in range(8):
        assert rel(got[b], ref2.checked_D(S[b, :n], S[b, n:], A[b]).T @ g[b]) <= TOL, b
    assert np.abs(got - (c["D"][:8].transpose(0, 2, 1) @ g[:8, :, None])[..., 0]).max() > 1e-6      # the edit matters


def test_shapes_layouts_bits_and_errors():
    import ctypes as C
    import nimblephysics_amd as na
    from nimblephysics_amd._lib import NimbleAmdError
    from nimblephysics_amd.dynamics import _fd_workspace, _workspace, inverse_dynamics_inertia_vjp_soa
    from nimblephysics_amd.mapping import _ptr
    c = _case("atlas20")
    md, S, A, g, n = c["md"], c["S"], c["A"], c["g"], c["n"]
    w = _world(md, c["entries"])
    st, at, gt = _t(S), _t(A), _t(g)
    one = na.inverse_dynamics_mass_gradient(w, st, at, gt)
    fd = na.forward_dynamics_mass_gradient(w, st, at, gt)
    assert torch.equal(one, na.inverse_dynamics_mass_gradient(w, st, at, gt)) and torch.equal(fd, na.forward_dynamics_mass_gradient(w, st, at, gt))
    # rollout-shaped input [T + 1, B, .] in one launch = the per-slice calls
    T1 = 4
    S4, A4, g4 = (np.stack([np.roll(x, t, 0) for t in range(T1)]) for x in (S, A, g))
    roll = na.inverse_dynamics_mass_gradient(w, _t(S4), _t(A4), _t(g4))
    rollfd = na.forward_dynamics_mass_gradient(w, _t(S4), _t(A4), _t(g4))
    assert roll.shape == (T1, B, w.getMassDims())
    for t in range(T1):
        assert torch.equal(roll[t], na.inverse_dynamics_mass_gradient(w, _t(S4[t]), _t(A4[t]), _t(g4[t])))
        assert torch.equal(rollfd[t], na.forward_dynamics_mass_gradient(w, _t(S4[t]), _t(A4[t]), _t(g4[t])))
    # a world alone (1-D) = the same world in the batch, at both ends of it and across the block boundary
    for b in (0, 63, 64, 129):
        assert torch.equal(na.inverse_dynamics_mass_gradient(w, st[b], at[b], gt[b]), one[b])
        assert torch.equal(na.forward_dynamics_mass_gradient(w, st[b], at[b], gt[b]), fd[b])
        assert torch.equal(na.inverse_dynamics_mass_jacobian(w, st[b], at[b]), na.inverse_dynamics_mass_jacobian(w, st, at)[b])
    # accumulate adds
    s_soa, a_soa, g_soa = w.to_soa(st), w.to_soa(at), w.to_soa(gt)
    base = torch.randn((w.getMassDims(), B), dtype=torch.float64, device=DEV)
    acc = inverse_dynamics_inertia_vjp_soa(w, s_soa, a_soa, g_soa, 0, out=base.clone())
    assert float((acc - (base + one.t())).abs().max()) <= 1e-12 * max(1.0, float(one.abs().max()))
    # CPU tensors in, CPU tensors out
    cpu = na.inverse_dynamics_mass_gradient(w, st.cpu(), at.cpu(), gt.cpu())
    assert cpu.device.type == "cpu" and torch.equal(cpu, one.cpu())
    assert na.forward_dynamics_mass_jacobian(w, st.cpu()[:3], at.cpu()[:3]).device.type == "cpu"
    # a deferred-join handle gives the joined handle's bits
    dw = _world(md, c["entries"])
    dw.set_deferred_join(True)
    assert torch.equal(na.inverse_dynamics_mass_gradient(dw, st, at, gt), one) and torch.equal(na.forward_dynamics_mass_gradient(dw, st, at, gt), fd)
    dw.join()
    # argument errors: nothing is launched
    with pytest.raises(ValueError, match="getMassDims"):
        na.inverse_dynamics(w, st, at, mass=torch.ones(3, dtype=torch.float64))
    bare = na.World(md, device=DEV)
    with pytest.raises(ValueError, match="registered"):
        na.forward_dynamics(bare, st, at, mass=torch.ones(0, dtype=torch.float64))
    with pytest.raises(ValueError, match="registered"):
        na.inverse_dynamics_mass_jacobian(bare, st, at)
    L, ws = w._L, _workspace(w, B)
    out = torch.full((w.getMassDims(), B), 7.0, dtype=torch.float64, device=DEV)
    args = lambda flags, o, nbytes: (w._h, B, _ptr(s_soa), _ptr(a_soa), flags, _ptr(g_soa), o, 0, _ptr(ws), nbytes, w._stream())
    assert L.nbl_inverse_dynamics_backward_inertia(*args(0, _ptr(out), L.nbl_dynamics_workspace_bytes(w._h, B) - 8)) == -4      # NBL_E_WORKSPACE
    assert L.nbl_inverse_dynamics_backward_inertia(*args(16, _ptr(out), ws.numel())) == -1                                   # unknown flag bits
    assert L.nbl_inverse_dynamics_backward_inertia(*args(0, None, ws.numel())) == -1                                         # null output, count > 0
    fws = _fd_workspace(w, B)
    assert L.nbl_forward_dynamics_backward_inertia(w._h, None, B, _ptr(s_soa), _ptr(a_soa), None, 0, _ptr(g_soa), _ptr(out), 0, _ptr(fws), 8,
                                                   w._stream()) == -4
    assert L.nbl_forward_dynamics_backward_inertia(w._h, None, B, _ptr(s_soa), _ptr(a_soa), None, 8, _ptr(g_soa), _ptr(out), 0, _ptr(fws), fws.numel(),
                                                   w._stream()) == -1                                                         # NBL_WRENCH_WORLD without a wrench set
    # the wrench form of the forward-dynamics entry: a short nbl_wrench_workspace_bytes, a null output, a null wrench array
    from nimblephysics_amd.dynamics import _km, _wr_workspace, wrench_set
    mapping = wrench_set(w, [len(md.bodies) - 1])               # (kept alive: it owns the device map)
    km = _km(w, mapping)
    wws = _wr_workspace(w, km, B)
    wr = torch.zeros((6, B), dtype=torch.float64, device=DEV)
    fdw = lambda wrench, o, nbytes: L.nbl_forward_dynamics_backward_inertia(w._h, km, B, _ptr(s_soa), _ptr(a_soa), wrench, 8, _ptr(g_soa), o, 0, _ptr(wws),
                                                                           nbytes, w._stream())
    assert fdw(_ptr(wr), _ptr(out), L.nbl_wrench_workspace_bytes(w._h, km, B) - 8) == -4
    assert fdw(_ptr(wr), None, wws.numel()) == -1
    assert fdw(None, _ptr(out), wws.numel()) == -1
    assert L.nbl_forward_dynamics_backward_inertia(w._h, None, B, _ptr(s_soa), _ptr(a_soa), None, 0, _ptr(g_soa), None, 0, _ptr(fws), fws.numel(),
                                                   w._stream()) == -1                                                         # null output, no wrench set
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert fdw(_ptr(wr), _ptr(out), wws.numel()) == 0                                                                         # a zero wrench: what no wrench gives
    assert float((out.t() - fd).abs().max()) <= 1e-12 * max(1.0, float(fd.abs().max()))
    # no parameter registered, or B = 0: a no-op that succeeds
    bws = _workspace(bare, B)
    assert bare._L.nbl_inverse_dynamics_backward_inertia(bare._h, B, _ptr(s_soa), _ptr(a_soa), 0, _ptr(g_soa), None, 0, _ptr(bws), bws.numel(), bare._stream()) == 0
    assert L.nbl_inverse_dynamics_backward_inertia(w._h, 0, None, None, 0, None, None, 0, None, 0, w._stream()) == 0


def test_immobile_skeletons_take_the_references_layout(tmp_path):
    import nimblephysics_amd as na
    from test_ref_layout import load
    md = load(tmp_path)
    w = na.World(md, device=DEV)
    assert w.ref_layout is not None and w.n == 6
    mobile = next(i for i, b in enumerate(md.bodies) if md.weld_targets()[0][i] >= 0)
    w.tuneMass(mobile)
    rng = np.random.default_rng(77)
    full = np.zeros((8, 24)); full[:, 6:12] = rng.normal(0, 0.3, (8, 6)); full[:, 18:] = rng.normal(0, 1, (8, 6))
    afull, gfull = rng.normal(0, 1, (8, 12)), rng.normal(0, 1, (8, 12))
    short = (np.concatenate([full[:, 6:12], full[:, 18:]], 1), afull[:, 6:], gfull[:, 6:])
    got = na.inverse_dynamics_mass_gradient(w, _t(full), _t(afull), _t(gfull))
    assert torch.equal(got, na.inverse_dynamics_mass_gradient(w, *(_t(x) for x in short)))
    gotfd = na.forward_dynamics_mass_gradient(w, _t(full), _t(afull), _t(gfull))
    assert torch.equal(gotfd, na.forward_dynamics_mass_gradient(w, *(_t(x) for x in short))) and float(gotfd.abs().max()) > 0


def test_world_getters_equal_the_functions_and_the_oracles_jacobians():
    """World.getJacobianOfC / M / ID / Minv / FD on the current state: wrt = the mass vector against the functions above, wrt = positions /
    velocities against ow.jac_C and ow.jac_Mx (1e-10, every world); any other wrt raises NotImplementedError."""
    import nimblephysics_amd as na
    from dynmass_ref import TOL, rel
    from nimblephysics_amd import neural
    from nimblephysics_amd.dynamics import ID_NO_GRAVITY, ID_NO_VELOCITY, inverse_dynamics_inertia_vjp_soa
    for name, nB in (("free_below_root", 9), ("atlas20", 3)):
        c = _case(name)
        md, ref, n = c["md"], c["ref"], c["n"]
        S, X, act = c["S"][:nB], c["A"][:nB], c["g"][:nB]
        w = _world(md, c["entries"])
        ow = ref.world()
        st, xt = _t(S), _t(X)
        w.setState(st)
        w.setAction(_t(act[:, :w.k]))
        wm = w.getWrtMass()
        # the mass vector
        assert torch.equal(w.getJacobianOfC(wm), na.inverse_dynamics_mass_jacobian(w, st, None))
        assert torch.equal(w.getJacobianOfID(xt, wm), na.inverse_dynamics_mass_jacobian(w, st, xt))
        tau = torch.zeros((nB, n), dtype=torch.float64, device=DEV)
        tau[:, md.action_map] = _t(act[:, :w.k])
        assert torch.equal(w.getJacobianOfFD(wm), na.forward_dynamics_mass_jacobian(w, st, tau, joint_forces=True))
        JM = w.getJacobianOfM(xt, wm)
        rows = torch.stack([inverse_dynamics_inertia_vjp_soa(w, w.to_soa(st), w.to_soa(xt), w.to_soa(torch.eye(n, dtype=torch.float64, device=DEV)[i].expand(nB, n).contiguous()),
                                                             ID_NO_VELOCITY | ID_NO_GRAVITY).t() for i in range(n)], 1)
        assert torch.equal(JM, rows)
        Minv = na.inv_mass_matrix(w, st)
        JMi = w.getJacobianOfMinv(xt, wm)
        y = (Minv @ xt[:, :, None])[:, :, 0]
        assert float((JMi + Minv @ w.getJacobianOfM(y, wm)).abs().max()) <= 1e-12 * max(1.0, float(JMi.abs().max()))
        # positions and velocities
        P, V = neural.WRT_POSITION, neural.WRT_VELOCITY
        got = {k: v.cpu().numpy() for k, v in {"Cq": w.getJacobianOfC(P), "Cv": w.getJacobianOfC(V), "Mq": w.getJacobianOfM(xt, P), "Mv": w.getJacobianOfM(xt, V),
                                               "IDq": w.getJacobianOfID(xt, P), "IDv": w.getJacobianOfID(xt, V), "Miq": w.getJacobianOfMinv(xt, P),
                                               "Miv": w.getJacobianOfMinv(xt, V), "FDq": w.getJacobianOfFD(P), "FDv": w.getJacobianOfFD(V)}.items()}
        fl = md.flat()
        for b in range(nB):
            q, v, x = S[b, :n], S[b, n:], X[b]
            Mo = ow.mass_matrix(q)
            Cq, Cv, Mq = ow.jac_C(q, v, 0), ow.jac_C(q, v, 1), ow.jac_Mx(q, x)
            a = ow.forward_dynamics(q, v, tau[b].cpu().numpy())
            e = {"Cq": rel(got["Cq"][b], Cq), "Cv": rel(got["Cv"][b], Cv), "Mq": rel(got["Mq"][b], Mq), "IDq": rel(got["IDq"][b], Mq + Cq),
                 "IDv": rel(got["IDv"][b], Cv), "Miq": rel(got["Miq"][b], -np.linalg.solve(Mo, ow.jac_Mx(q, np.linalg.solve(Mo, x)))),
                 "FDq": rel(got["FDq"][b], -np.linalg.solve(Mo, ow.jac_Mx(q, a) + Cq + np.diag(fl["spring"]))),
                 "FDv": rel(got["FDv"][b], -np.linalg.solve(Mo, Cv + np.diag(fl["damping"] + md.dt * fl["spring"])))}
            assert max(e.values()) <= TOL, (name, b, e)
            assert not got["Mv"][b].any() and not got["Miv"][b].any()
        # one world given as a 1-D vector
        w.setState(st[0])
        assert torch.equal(w.getJacobianOfC(wm), na.inverse_dynamics_mass_jacobian(w, st[0], None)) and w.getJacobianOfC(P).shape == (n, n)
        for bad in (neural.WRT_ACCELERATION, "force", None, na.World(md, device=DEV).getWrtMass()):
            with pytest.raises((NotImplementedError, ValueError)):
                w.getJacobianOfC(bad)
        with pytest.raises(NotImplementedError, match="acceleration"):
            w.getJacobianOfID(xt[0], neural.WRT_ACCELERATION)


def test_plain_c_dynamics_inertia_driver(tmp_path):
    """tests/c_abi_example/dynamics_inertia.c: both new entries from pure C99 on the Atlas-20 model header - the Euler identity, the forward-
    dynamics gradient from its two halves (nbl_inv_mass_apply, the inverse-dynamics entry at (q, v, a)), a wrench set, the argument errors."""
    import os
    import subprocess
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.join(ROOT, "nimblephysics_amd")
    exe = str(tmp_path / "dynamics_inertia")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_abi_example", "dynamics_inertia.c"), "-o", exe, "-L" + libdir, "-lnimble_amd",
                           "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath," + libdir])
    out = subprocess.check_output([exe, "130"]).decode()
    print(out)
    assert "max residuals" in out
