"""Wrenches on bodies in the dynamics calls and contact inverse dynamics on the device (k_inverse_dynamics_wrench, k_inverse_dynamics_wrench_vjp,
k_forward_dynamics_wrench, k_forward_dynamics_wrench_lambda, k_contact_inverse_dynamics of csrc/dynamics.hip through nimblephysics_amd/dynamics.py):
the device against the host build of the same header (tests/test_wrench_host.py holds that build to the oracle), bit identity over the batch
and against the calls without wrenches, torch.autograd.gradcheck in both frames of expression, the ID o FD round trip, CPU tensors, the
rollout shape, a deferred-join handle, the World methods, argument errors and the plain-C driver.

DEVICE AGAINST HOST BUILD: 1e-13 relative (_rel of tests/test_gpu_dynamics.py), the figure tests/test_gpu_dynamics.py and
tests/test_gpu_forward_dynamics.py hold the same pair of compilers to (hipcc contracts a * b + c into fused multiply-adds, its sincos is
not glibc's)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_dynamics import _rel, _states

gpu = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_LANES = 130                      # two full wavefronts and a two-lane tail


def _model(name):
    import nimblephysics_amd as na
    from test_dynamics_host import free_below_root
    return {"atlas20": lambda: na.atlas("atlas20"), "free_below_root": free_below_root}[name]()


def _entries(md, name):
    """[(body index of md, frame in it)]: the feet of Atlas-20 (the right one with an offset frame) / the bodies test_wrench_host picks"""
    from test_wrench_host import _contact_entries, wrench_entries
    return _contact_entries(md, ["l_foot", "r_foot"]) if name == "atlas20" else wrench_entries(md)


def _mapping(na, world, entries):
    """the IKMapping of spatial entries on the frames of `entries` (an offset frame goes into the entry as the loaders' welds do)"""
    m = na.IKMapping(world)
    for i, Tx in entries:
        m.addSpatialBodyNode(int(i))
        k, ib, mb, T = m._entries[-1]
        m._entries[-1] = (k, ib, mb, T @ Tx)
    return m


def _t(x):
    return torch.tensor(np.ascontiguousarray(x), device=DEV)


@gpu
@pytest.mark.parametrize("name", ["atlas20", "free_below_root"])
def test_the_device_kernels_equal_the_host_build_to_1e_13(name):
    import nimblephysics_amd as na
    from nimblephysics_amd.dynamics import (CID_MIN_TORQUE, CID_NEAREST, ID_JOINT_FORCES, WRENCH_WORLD, _wrench_vjp_soa, contact_inverse_dynamics_soa,
                                            forward_dynamics_wrench_soa, inverse_dynamics_wrench_soa)
    from test_wrench_host import ShimWrench, load_shim
    md = _model(name)
    entries = _entries(md, name)
    host = ShimWrench(load_shim(), md, entries)
    w = na.World(md, device=DEV)
    mp = _mapping(na, w, entries)
    B = B_LANES
    S, A, g = _states(md, B, 51)
    W = np.random.default_rng(52).normal(0, 3.0, (B, 6 * host.E))
    s, a, gg, ww = _t(S.T), _t(A.T), _t(g.T), _t(W.T)
    c = lambda x: x.cpu().numpy()
    worst = {}
    for flags in (0, WRENCH_WORLD, WRENCH_WORLD | ID_JOINT_FORCES):
        tau = inverse_dynamics_wrench_soa(w, mp, s, a, ww, flags)
        worst[("tau", flags)] = _rel(c(tau), host.wtau(S.T, A.T, W.T, flags))
        worst[("accel", flags)] = _rel(c(forward_dynamics_wrench_soa(w, mp, s, a, ww, flags)), host.waccel(S.T, A.T, W.T, flags))
        for fn, ref in (("nbl_inverse_dynamics_wrench_backward", host.wvjp(S.T, A.T, W.T, g.T, flags)),
                        ("nbl_forward_dynamics_wrench_backward", host.wfd_vjp(S.T, A.T, W.T, g.T, flags))):
            got = _wrench_vjp_soa(w, fn, mp, s, a, ww, gg, flags, True, True, True)
            for key, x, r in zip(("grad_state", "grad_x", "grad_wrench"), got, ref):
                worst[(fn[4:20], key, flags)] = _rel(c(x), r)
    if name == "atlas20":
        G = np.random.default_rng(53).normal(0, 20.0, (B, 6 * host.E))
        for mode, guess in ((CID_NEAREST, G), (CID_MIN_TORQUE, None)):
            Wd, td = contact_inverse_dynamics_soa(w, mp, s, a, None if guess is None else _t(guess.T), mode)
            Wh, th = host.cid(S.T, A.T, mode, None if guess is None else guess.T)
            assert not c(td)[:6].any()
            worst[("cid wrench", mode)], worst[("cid tau", mode)] = _rel(c(Wd), Wh), _rel(c(td), th)
    print(name, "device vs host build:", worst)
    assert max(worst.values()) <= 1e-13, worst


def _run(na, w, mp, s, a, W, g, world_frame):
    x, y, z = s.clone().requires_grad_(True), a.clone().requires_grad_(True), W.clone().requires_grad_(True)
    tau = na.inverse_dynamics(w, x, y, joint_forces=True, wrenches=z, bodies=mp, world_frame=world_frame)
    tau.backward(g)
    x2, y2, z2 = s.clone().requires_grad_(True), a.clone().requires_grad_(True), W.clone().requires_grad_(True)
    acc = na.forward_dynamics(w, x2, y2, joint_forces=True, wrenches=z2, bodies=mp, world_frame=world_frame)
    acc.backward(g)
    return tau.detach(), x.grad, y.grad, z.grad, acc.detach(), x2.grad, y2.grad, z2.grad


@gpu
def test_bit_identity_over_the_batch_the_rollout_shape_and_cpu_tensors():
    import nimblephysics_amd as na
    md = _model("atlas20")
    n, B = md.num_dofs, B_LANES
    w = na.World(md, device=DEV)
    mp = _mapping(na, w, _entries(md, "atlas20"))
    S, A, g = _states(md, B, 54)
    W = np.random.default_rng(55).normal(0, 3.0, (B, 12))
    st, at, gt, wt = _t(S), _t(A), _t(g), _t(W)
    first = _run(na, w, mp, st, at, wt, gt, True)
    for u, v in zip(first, _run(na, w, mp, st, at, wt, gt, True)):
        assert torch.equal(u, v)
    for b in (0, 63, 64, B - 1):                                          # world b of the batch = the same world alone
        for u, v in zip(_run(na, w, mp, st[b:b + 1], at[b:b + 1], wt[b:b + 1], gt[b:b + 1], True), first):
            assert torch.equal(u[0], v[b]), b
    Wc, tc = na.contact_inverse_dynamics(w, st, at, mp)
    assert Wc.shape == (B, 2, 6) and tc.shape == (B, n) and not tc[:, :6].any()
    for b in (0, B - 1):
        W1, t1 = na.contact_inverse_dynamics(w, st[b:b + 1], at[b:b + 1], mp)
        assert torch.equal(W1[0], Wc[b]) and torch.equal(t1[0], tc[b])
    # [3, 5, 2n]: one launch over 15 worlds
    sh = lambda x: x[:15].reshape(3, 5, -1)
    roll = _run(na, w, mp, sh(st), sh(at), sh(wt), sh(gt), True)
    assert roll[0].shape == (3, 5, n) and roll[1].shape == (3, 5, 2 * n) and roll[3].shape == (3, 5, 12)
    for u, v in zip(roll, first):
        assert torch.equal(u.reshape(15, -1), v[:15])
    Wr, tr = na.contact_inverse_dynamics(w, sh(st), sh(at), mp, wrench_guesses=sh(wt).reshape(3, 5, 2, 6))
    assert Wr.shape == (3, 5, 2, 6) and tr.shape == (3, 5, n)
    # CPU float64 in -> CPU out, one world as a 1-D vector
    one = na.inverse_dynamics(w, st[0].cpu(), at[0].cpu(), joint_forces=True, wrenches=wt[0].cpu(), bodies=mp, world_frame=True)
    assert one.device.type == "cpu" and one.shape == (n,) and torch.equal(one, first[0][0].cpu())
    one = na.forward_dynamics(w, st[0].cpu(), at[0].cpu(), joint_forces=True, wrenches=wt[0].cpu(), bodies=mp, world_frame=True)
    assert one.device.type == "cpu" and torch.equal(one, first[4][0].cpu())
    Wh, th = na.contact_inverse_dynamics(w, st[0].cpu(), at[0].cpu(), ["l_foot", "r_foot"])
    assert Wh.device.type == "cpu" and Wh.shape == (2, 6) and th.shape == (n,)
    with pytest.raises(ValueError):
        na.inverse_dynamics(w, st, at, wrenches=wt[:, :6], bodies=mp)
    with pytest.raises(ValueError):
        na.inverse_dynamics(w, st, at, bodies=mp)
    lin = na.IKMapping(w); lin.addLinearBodyNode("l_foot")
    with pytest.raises(ValueError):
        na.forward_dynamics(w, st, at, wrenches=wt[:, :3], bodies=lin)


@gpu
@pytest.mark.parametrize("name", ["atlas20", "free_below_root"])
def test_no_entries_and_zero_wrenches_give_the_bits_of_the_calls_without_wrenches(name):
    import nimblephysics_amd as na
    from nimblephysics_amd.dynamics import (ID_JOINT_FORCES, WRENCH_WORLD, _wrench_vjp_soa, forward_dynamics_soa, forward_dynamics_wrench_soa,
                                            inverse_dynamics_soa, inverse_dynamics_vjp_soa, inverse_dynamics_wrench_soa)
    md = _model(name)
    w = na.World(md, device=DEV)
    mp = _mapping(na, w, _entries(md, name))
    B = B_LANES
    S, A, g = _states(md, B, 56)
    s, a, gg = _t(S.T), _t(A.T), _t(g.T)
    Z = torch.zeros((6 * len(mp._entries), B), dtype=torch.float64, device=DEV)
    none = torch.empty((0, B), dtype=torch.float64, device=DEV)
    tau, acc = inverse_dynamics_soa(w, s, a, ID_JOINT_FORCES), forward_dynamics_soa(w, s, a, ID_JOINT_FORCES)
    gs, ga = inverse_dynamics_vjp_soa(w, s, a, gg, ID_JOINT_FORCES)
    for m, W, wf in ((None, none, 0), (mp, Z, 0), (mp, Z, WRENCH_WORLD)):
        fl = ID_JOINT_FORCES | wf
        assert torch.equal(inverse_dynamics_wrench_soa(w, m, s, a, W, fl), tau)
        assert torch.equal(forward_dynamics_wrench_soa(w, m, s, a, W, fl), acc)
        ws, wa, _ = _wrench_vjp_soa(w, "nbl_inverse_dynamics_wrench_backward", m, s, a, W, gg, fl, True, True, W.shape[0] > 0)
        assert torch.equal(ws, gs) and torch.equal(wa, ga)
    st, at = _t(S), _t(A)
    assert torch.equal(na.inverse_dynamics(w, st, at, wrenches=Z.t().contiguous(), bodies=mp), na.inverse_dynamics(w, st, at))
    assert torch.equal(na.forward_dynamics(w, st, at, wrenches=torch.zeros((B, 0), dtype=torch.float64, device=DEV), bodies=[]), na.forward_dynamics(w, st, at))


@gpu
@pytest.mark.parametrize("world_frame", [False, True])
@pytest.mark.parametrize("name", ["atlas20", "free_below_root"])
def test_gradcheck_with_respect_to_state_accel_and_wrenches(name, world_frame):
    import nimblephysics_amd as na
    md = _model(name)
    w = na.World(md, device=DEV)
    mp = _mapping(na, w, _entries(md, name))
    S, A, _ = _states(md, 3, 57)
    W = np.random.default_rng(58).normal(0, 3.0, (3, 6 * len(mp._entries)))
    x, y, z = (torch.tensor(v, device=DEV, requires_grad=True) for v in (S, A, W))
    f = lambda s, a, ww: na.inverse_dynamics(w, s, a, joint_forces=True, wrenches=ww, bodies=mp, world_frame=world_frame)
    assert torch.autograd.gradcheck(f, (x, y, z), eps=1e-6, atol=1e-6, rtol=1e-5)
    tau = f(x, y, z).detach().requires_grad_(True)
    h = lambda s, t, ww: na.forward_dynamics(w, s, t, joint_forces=True, wrenches=ww, bodies=mp, world_frame=world_frame)
    assert torch.autograd.gradcheck(h, (x, tau, z), eps=1e-6, atol=1e-6, rtol=1e-5)
    # the round trip: forward dynamics of that tau under the same wrenches gives the accelerations back (1e-10 of their size: M^-1 M)
    assert _rel(h(x, tau, z).detach().cpu().numpy(), A) <= 1e-10


@gpu
def test_contact_inverse_dynamics_world_methods_and_predictions():
    import nimblephysics_amd as na
    md = _model("atlas20")
    n, B = md.num_dofs, 6
    w = na.World(md, device=DEV)
    S, A, _ = _states(md, B, 59)
    st, at = _t(S), _t(A)
    feet = ["l_foot", "r_foot"]
    W, tau = na.contact_inverse_dynamics(w, st, at, feet)                 # several bodies, no guesses: min torque
    back = na.forward_dynamics(w, st, tau, joint_forces=True, wrenches=W.reshape(B, 12), bodies=feet)
    assert _rel(back.cpu().numpy(), A) <= 1e-9                            # the reference's sumError, in units of the accelerations
    G = torch.tensor(np.random.default_rng(60).normal(0, 20.0, (B, 2, 6)), device=DEV)
    Wn, taun = na.contact_inverse_dynamics(w, st, at, feet, wrench_guesses=G)
    assert float((Wn - G).norm()) < float((W - G).norm())                 # nearer to the guesses than another solution
    assert _rel(na.forward_dynamics(w, st, taun, joint_forces=True, wrenches=Wn.reshape(B, 12), bodies=feet).cpu().numpy(), A) <= 1e-9
    W1, t1 = na.contact_inverse_dynamics(w, st, at, "l_foot")             # one body: getContactInverseDynamics
    assert W1.shape == (B, 1, 6) and not t1[:, :6].any()
    # the World's current state
    w.setState(st)
    Ww, tw = w.getMultipleContactInverseDynamics(at, feet)
    assert torch.equal(Ww, W) and torch.equal(tw, tau)
    Wg, tg = w.getMultipleContactInverseDynamics(at, feet, G)
    assert torch.equal(Wg, Wn) and torch.equal(tg, taun)
    Ws, ts = w.getContactInverseDynamics(at, "l_foot")
    assert Ws.shape == (B, 6) and torch.equal(Ws, W1[:, 0]) and torch.equal(ts, t1)
    # predictions in the root frame: the local wrenches of the solve, taken to the root frame by hand, give the solve's torques outside the
    # root rows (there the solve wrote zeros and inverse dynamics gives 0 +- rounding)
    from nimblephysics_amd.dynamics import _rotvec_matrix, wrench_set
    pos = na.map_to_pos(w, wrench_set(w, feet + ["pelvis"]), st)
    Rr, pr = _rotvec_matrix(pos[:, 12:15]), pos[:, 15:18]
    rootW = []
    for e in range(2):
        Rb, pb = _rotvec_matrix(pos[:, 6 * e:6 * e + 3]), pos[:, 6 * e + 3:6 * e + 6]
        fw = (Rb @ W[:, e, 3:, None])[..., 0]
        tw0 = (Rb @ W[:, e, :3, None])[..., 0] + torch.linalg.cross(pb - pr, fw)          # world coordinates, about the root's origin
        rootW += [(Rr.transpose(1, 2) @ tw0[..., None])[..., 0], (Rr.transpose(1, 2) @ fw[..., None])[..., 0]]
    pred = na.inverse_dynamics_from_predictions(w, st, at, feet, torch.cat(rootW, -1))
    scale = max(1.0, float(tau.abs().max()))
    assert float((pred[:, 6:] - tau[:, 6:]).abs().max()) <= 1e-10 * scale and float(pred[:, :6].abs().max()) <= 1e-9 * scale
    assert torch.equal(w.getInverseDynamicsFromPredictions(at, feet, torch.cat(rootW, -1)), pred)
    res = torch.tensor(np.random.default_rng(61).normal(0, 5.0, (B, 6)), device=DEV)
    with_res = na.inverse_dynamics_from_predictions(w, st, at, feet, torch.cat(rootW, -1), res)
    want = na.inverse_dynamics(w, st, at, joint_forces=True, wrenches=torch.cat([W.reshape(B, 12), res], -1), bodies=feet + ["pelvis"])
    assert float((with_res - want).abs().max()) <= 1e-10 * scale


@gpu
def test_a_deferred_join_handle_gives_the_same_bits():
    import nimblephysics_amd as na
    md = na.atlas("atlas20", ground=True)
    n, B = md.num_dofs, 4096
    S, A, _ = _states(md, B, 62)
    S[:, 0] = -np.pi / 2; S[:, 4] += 1.0
    st, at = _t(S), _t(A)
    Wt = torch.tensor(np.random.default_rng(63).normal(0, 3.0, (B, 12)), device=DEV)
    feet = ["l_foot", "r_foot"]
    ref, dw = na.World(md, device=DEV), na.World(md, device=DEV)
    s_soa = ref.to_soa(st); a_soa = ref.to_soa(torch.zeros((B, ref.k), dtype=torch.float64, device=DEV))
    want_next, _, _ = ref.step_soa(s_soa, a_soa, want_saved=True)
    want = na.inverse_dynamics(ref, want_next.t(), at, wrenches=Wt, bodies=feet), na.contact_inverse_dynamics(ref, want_next.t(), at, feet)[0]
    dw.set_deferred_join(True)
    assert dw.slices_for(B) > 1
    buf = {"nxt": torch.empty_like(s_soa), "saved": torch.empty(dw.saved_bytes(B), dtype=torch.uint8, device=DEV),
           "status": torch.empty(B, dtype=torch.int32, device=DEV), "cache": torch.empty((dw.m, B), dtype=torch.float64, device=DEV)}
    dw.step_into(s_soa, a_soa, buf["nxt"], buf["saved"], buf["status"], None, buf["cache"])
    got = na.inverse_dynamics(dw, buf["nxt"].t(), at, wrenches=Wt, bodies=feet), na.contact_inverse_dynamics(dw, buf["nxt"].t(), at, feet)[0]
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    dw.join()
    torch.cuda.synchronize()


@gpu
def test_argument_errors_return_their_codes_and_launch_nothing():
    import ctypes as C
    import nimblephysics_amd as na
    from nimblephysics_amd.dynamics import _fd_workspace, _workspace, _wr_workspace
    from test_ball_joint import ball_model
    md = _model("atlas20")
    n = md.num_dofs
    w = na.World(md, device=DEV)
    mp = _mapping(na, w, _entries(md, "atlas20"))
    lin = na.IKMapping(w); lin.addLinearBodyNode("l_foot")
    k, klin = mp._device_map(w), lin._device_map(w)
    S, A, _ = _states(md, 8, 64)
    L, h = w._L, w._h
    s8, a8 = w.to_soa(_t(S)), w.to_soa(_t(A))
    W8 = torch.zeros((12, 8), dtype=torch.float64, device=DEV)
    SENT = -12345.0
    out = torch.full((2 * n, 8), SENT, dtype=torch.float64, device=DEV)
    ws = _wr_workspace(w, k, 8)
    need = L.nbl_wrench_workspace_bytes(h, k, 8)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert need == L.nbl_forward_dynamics_workspace_bytes(h, 8) + 8 * 8 * (3 * 15 + 12 * 2)      # + 3 per body (15 device bodies), 12 per entry
    assert L.nbl_wrench_workspace_bytes(None, k, 8) == 0 and L.nbl_wrench_workspace_bytes(h, k, 0) == 0
    assert L.nbl_wrench_workspace_bytes(h, None, 8) == need - 8 * 8 * 24
    BAD, UNS, WSP = -1, -2, -4
    idf, idb, fdf, fdb, cid = (L.nbl_inverse_dynamics_wrench_forward, L.nbl_inverse_dynamics_wrench_backward, L.nbl_forward_dynamics_wrench_forward,
                               L.nbl_forward_dynamics_wrench_backward, L.nbl_contact_inverse_dynamics)
    other = na.World(ball_model(2, False), device=DEV)                    # no free root
    om = na.IKMapping(other); om.addSpatialBodyNode("hand")
    ok_, oh = om._device_map(other), other._h
    so = other.to_soa(_t(_states(other.description, 8, 65)[0])); ao = other.to_soa(_t(_states(other.description, 8, 65)[1]))
    wo = _wr_workspace(other, ok_, 8)
    stack = na.World(na.box_stack(), device=DEV)                          # two free roots
    roots = [i for i, b in enumerate(stack.description.bodies) if b.parent < 0 and b.joint_type == "free"][:2]
    sm = na.IKMapping(stack); sm.addSpatialBodyNode(roots[0]); sm.addSpatialBodyNode(roots[1])
    sk, sh_ = sm._device_map(stack), stack._h
    ss = stack.to_soa(_t(_states(stack.description, 8, 66)[0])); sa = stack.to_soa(_t(_states(stack.description, 8, 66)[1]))
    sws = _wr_workspace(stack, sk, 8)
    dws, fws = _workspace(w, 8), _fd_workspace(w, 8)
    cases = ((BAD, lambda: idf(None, k, 8, p(s8), p(a8), p(W8), 0, p(out), p(ws), need, None)),
             (BAD, lambda: idf(h, k, -1, p(s8), p(a8), p(W8), 0, p(out), p(ws), need, None)),
             (BAD, lambda: idf(h, k, 8, None, p(a8), p(W8), 0, p(out), p(ws), need, None)),
             (BAD, lambda: idf(h, k, 8, p(s8), p(a8), None, 0, p(out), p(ws), need, None)),              # entries without wrenches
             (BAD, lambda: idf(h, k, 8, p(s8), p(a8), p(W8), 0, None, p(ws), need, None)),
             (BAD, lambda: idf(h, k, 8, p(s8), p(a8), p(W8), 0, p(out), None, need, None)),
             (BAD, lambda: idf(h, k, 8, p(s8), p(a8), p(W8), 16, p(out), p(ws), need, None)),
             (BAD, lambda: idf(h, klin, 8, p(s8), p(a8), p(W8), 0, p(out), p(ws), need, None)),          # a non-spatial entry
             (BAD, lambda: idf(h, ok_, 8, p(s8), p(a8), p(W8), 0, p(out), p(ws), need, None)),           # a map of another model
             (WSP, lambda: idf(h, k, 8, p(s8), p(a8), p(W8), 0, p(out), p(ws), need - 1, None)),
             (BAD, lambda: idb(h, k, 8, p(s8), p(a8), p(W8), 0, None, p(out), p(out), p(out), 0, p(ws), need, None)),
             (BAD, lambda: idb(h, klin, 8, p(s8), p(a8), p(W8), 8, p(a8), p(out), p(out), p(out), 0, p(ws), need, None)),
             (WSP, lambda: idb(h, k, 8, p(s8), p(a8), p(W8), 8, p(a8), p(out), p(out), p(out), 0, p(ws), 8, None)),
             (BAD, lambda: fdf(h, k, 8, p(s8), p(a8), p(W8), 32, p(out), p(ws), need, None)),
             (BAD, lambda: fdf(h, klin, 8, p(s8), p(a8), p(W8), 0, p(out), p(ws), need, None)),
             (WSP, lambda: fdf(h, k, 8, p(s8), p(a8), p(W8), 0, p(out), p(ws), need // 2, None)),
             (BAD, lambda: fdb(h, k, 8, p(s8), p(a8), p(W8), 0, None, p(out), p(out), p(out), 0, p(ws), need, None)),
             (WSP, lambda: fdb(h, k, 8, p(s8), p(a8), p(W8), 0, p(a8), p(out), p(out), p(out), 0, p(ws), 0, None)),
             # the calls without wrenches keep rejecting bit 8
             (BAD, lambda: L.nbl_inverse_dynamics_forward(h, 8, p(s8), p(a8), 8, p(out), p(dws), dws.numel(), None)),
             (BAD, lambda: L.nbl_inverse_dynamics_backward(h, 8, p(s8), p(a8), 8, p(a8), p(out), p(out), 0, p(dws), dws.numel(), None)),
             (BAD, lambda: L.nbl_forward_dynamics_forward(h, 8, p(s8), p(a8), 8, p(out), p(fws), fws.numel(), None)),
             (BAD, lambda: L.nbl_forward_dynamics_backward(h, 8, p(s8), p(a8), 8, p(a8), p(out), p(out), 0, p(fws), fws.numel(), None)),
             # contact inverse dynamics
             (BAD, lambda: cid(h, None, 8, p(s8), p(a8), None, 2, 0, p(out), p(out), p(ws), need, None)),
             (BAD, lambda: cid(h, k, 8, p(s8), p(a8), None, 2, 8, p(out), p(out), p(ws), need, None)),   # NBL_WRENCH_WORLD: the reference's result is local
             (BAD, lambda: cid(h, k, 8, p(s8), p(a8), None, 0, 0, p(out), p(out), p(ws), need, None)),   # NBL_CID_SINGLE with two bodies
             (BAD, lambda: cid(h, k, 8, p(s8), p(a8), None, 1, 0, p(out), p(out), p(ws), need, None)),   # NBL_CID_NEAREST without guesses
             (BAD, lambda: cid(h, k, 8, p(s8), p(a8), None, 7, 0, p(out), p(out), p(ws), need, None)),
             (BAD, lambda: cid(h, klin, 8, p(s8), p(a8), None, 0, 0, p(out), p(out), p(ws), need, None)),
             (BAD, lambda: cid(h, k, 8, p(s8), None, None, 2, 0, p(out), p(out), p(ws), need, None)),
             (WSP, lambda: cid(h, k, 8, p(s8), p(a8), None, 2, 0, p(out), p(out), p(ws), need - 1, None)),
             (UNS, lambda: cid(oh, ok_, 8, p(so), p(ao), None, 0, 0, p(out), p(out), p(wo), wo.numel(), None)),      # no free root
             (UNS, lambda: cid(sh_, sk, 8, p(ss), p(sa), None, 2, 0, p(out), p(out), p(sws), sws.numel(), None)))    # entries under different roots
    for i, (rc_want, call) in enumerate(cases):
        rc = call()
        assert rc == rc_want, (i, rc, rc_want)
        assert L.nbl_last_error()
    assert bool((out == SENT).all())                                      # no kernel ran
    for call in (lambda: idf(h, k, 0, None, None, None, 0, None, None, 0, None), lambda: fdf(h, None, 0, None, None, None, 0, None, None, 0, None),
                 lambda: idb(h, k, 0, None, None, None, 0, None, None, None, None, 0, None, 0, None),
                 lambda: fdb(h, k, 0, None, None, None, 0, None, None, None, None, 0, None, 0, None),
                 lambda: cid(h, k, 0, None, None, None, 2, 0, None, None, None, 0, None)):                           # B = 0: a no-op
        assert call() == 0
    with pytest.raises(na.NimbleAmdError, match="free joint"):
        na.contact_inverse_dynamics(other, _t(_states(other.description, 2, 1)[0]), _t(_states(other.description, 2, 1)[1]), "hand")


@gpu
def test_plain_c_contact_inverse_dynamics_driver(tmp_path):
    """tests/c_abi_example/contact_inverse_dynamics.c: the wrench calls and the contact solve from pure C99 on the Atlas-20 model header."""
    if shutil.which("gcc") is None or not os.path.exists("/opt/rocm/lib/libamdhip64.so"):
        pytest.skip("no gcc / ROCm runtime")
    libdir = os.path.join(ROOT, "nimblephysics_amd")
    exe = str(tmp_path / "contact_inverse_dynamics")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_abi_example", "contact_inverse_dynamics.c"), "-o", exe, "-L" + libdir, "-lnimble_amd",
                           "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath," + libdir])
    out = subprocess.check_output([exe, "130"]).decode()
    print(out)
    assert "max residuals" in out and "root rows not zero 0" in out and "differ 0" in out
