"""Task-space Jacobians, their time derivative and task-space accelerations of an `IKMapping`'s rows, for batches of states, with exact
gradients: the second-order side of `map_to_pos` / `map_to_vel` (the reference's BodyNode::getJacobian, getJacobianClassicDeriv,
getLinearJacobianDeriv and getAngularJacobianDeriv, batched over worlds and over the mapping's entries).

With R = mapping.getVelDim() rows (the rows of `map_to_vel`, in its order and frames: world coordinates) and n coordinates:

    J  = task_jacobian(world, map, state)                  [..., 2n] -> [..., R, n]    map_to_vel = J v; gradient to the positions
    c  = task_jacobian_dot_times_v(world, map, state)      [..., 2n] -> [..., R]       the bias acceleration Jdot v; gradients to q and v
    xa = map_to_acc(world, map, state, accel)              [..., 2n], [..., n] -> [..., R]   J accel + Jdot v; gradients to q, v and accel
    Jd = task_jacobian_deriv(world, map, state)            [..., 2n] -> [..., R, n]    d/dt J along the motion; DETACHED (no gradient)

A linear row of `map_to_acc` is the classical acceleration of the body frame's origin, an angular row the angular acceleration: each is
the time derivative of the `map_to_vel` row.  Gravity is not part of it.  Ball and free joints carry their Sdot v term.

Each call is one launch of csrc/taskspace.hip over all the leading dimensions ([2n] one world, [B, 2n] a batch, [T+1, B, 2n] a rollout)
and one more for its backward pass.  The gradients are exact: unlike `map_to_vel`, whose gradient leaves d(J v)/dq out as the reference's
layer does, nothing is left out here.  J is computed in one pass down every entry's ancestor chain (not one reverse-mode world per row,
as IKMapping.getRealVelToMappedVelJac does).

Rules shared with sensors.py / centroidal.py: CPU float64 tensors come back as CPU tensors, device tensors stay on the device; the
World's state is untouched; a World in deferred-join mode is joined first; on a world with immobile skeletons `state` and `accel` may
come in the reference's layout (the frozen coordinates get zero gradient and zero Jacobian columns)."""
from __future__ import annotations

import torch

from ._lib import NimbleAmdError, check
from .dynamics import _expand, _give, _restrict
from .mapping import IKMapping, _join_if_deferred, _ptr


def _workspace(world, B: int):
    need = world._L.nbl_task_workspace_bytes(world._h, B)
    ws = getattr(world, "_task_ws", None)
    if ws is None or ws.numel() < need or ws.device != world.device:
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=world.device)
        world._task_ws = ws
    return ws


# ---- raw SoA calls: state [2n][B], accel [n][B]; vectors [R][B], matrices [R n][B] ----
def task_jacobian_soa(world, mapping: IKMapping, s_soa: torch.Tensor, deriv: bool = False) -> torch.Tensor:
    R, n, B = mapping.getVelDim(), world.n, s_soa.shape[1]
    J = torch.empty((R * n, B), dtype=torch.float64, device=world.device)
    if R > 0 and B > 0:
        fn = world._L.nbl_task_jacobian_deriv if deriv else world._L.nbl_task_jacobian
        with torch.cuda.device(world.device):
            check(fn(world._h, mapping._device_map(world), B, R, n, _ptr(s_soa), _ptr(J), world._stream()),
                  "nbl_task_jacobian_deriv" if deriv else "nbl_task_jacobian")
    return J


def task_jacobian_vjp_soa(world, mapping: IKMapping, s_soa: torch.Tensor, G_soa: torch.Tensor) -> torch.Tensor:
    R, n, B = mapping.getVelDim(), world.n, s_soa.shape[1]
    gq = torch.empty((n, B), dtype=torch.float64, device=world.device) if R > 0 else torch.zeros((n, B), dtype=torch.float64, device=world.device)
    if R > 0 and B > 0:
        with torch.cuda.device(world.device):
            check(world._L.nbl_task_jacobian_vjp(world._h, mapping._device_map(world), B, R, n, _ptr(s_soa), _ptr(G_soa), _ptr(gq), 0,
                                                 world._stream()), "nbl_task_jacobian_vjp")
    return gq


def task_accel_soa(world, mapping: IKMapping, s_soa: torch.Tensor, a_soa) -> torch.Tensor:
    """J accel + Jdot v [R][B]; a_soa None: the bias acceleration Jdot v"""
    R, n, B = mapping.getVelDim(), world.n, s_soa.shape[1]
    out = torch.empty((R, B), dtype=torch.float64, device=world.device)
    if R > 0 and B > 0:
        with torch.cuda.device(world.device):
            check(world._L.nbl_task_accel(world._h, mapping._device_map(world), B, R, n, _ptr(s_soa), _ptr(a_soa),
                                          _ptr(out) if a_soa is None else None, None if a_soa is None else _ptr(out), world._stream()),
                  "nbl_task_accel")
    return out


def task_accel_vjp_soa(world, mapping: IKMapping, s_soa: torch.Tensor, a_soa, g_soa: torch.Tensor, want_accel: bool):
    """-> (grad_state [2n][B], grad_accel [n][B] or None)"""
    R, n, B = mapping.getVelDim(), world.n, s_soa.shape[1]
    make = torch.empty if R > 0 else torch.zeros
    gs = make((2 * n, B), dtype=torch.float64, device=world.device)
    ga = make((n, B), dtype=torch.float64, device=world.device) if want_accel and a_soa is not None else None
    if R > 0 and B > 0:
        ws = _workspace(world, B)
        with torch.cuda.device(world.device):
            check(world._L.nbl_task_accel_vjp(world._h, mapping._device_map(world), B, R, n, _ptr(s_soa), _ptr(a_soa), _ptr(g_soa), _ptr(gs),
                                              _ptr(ga), 0, _ptr(ws), ws.numel(), world._stream()), "nbl_task_accel_vjp")
    return gs, ga


def _inputs(world, what, state, accel):
    """(state [2n][B], accel [n][B] or None on the device, the leading shape, (ref, width) of state and of accel)"""
    n = world.n
    x, ref_s, width_s = _restrict(world, state.detach(), what, "state")
    lead = tuple(x.shape[:-1])
    s_soa = world.to_soa(world._prep(x.reshape(-1, 2 * n), 2 * n, "dyn_state"))
    a_soa, ref_a, width_a = None, False, n
    if accel is not None:
        a, ref_a, width_a = _restrict(world, accel.detach(), what, "accel")
        if tuple(a.shape[:-1]) != lead:
            raise ValueError(f"{what}: accel has leading shape {tuple(a.shape[:-1])}, state {lead}")
        a_soa = world.to_soa(world._prep(a.reshape(-1, n), n, "dyn_accel"))
    return s_soa, a_soa, lead, (ref_s, width_s), (ref_a, width_a)


def _matrix_out(world, J_soa, R, lead, lay_s, like_device):
    """[R n][B] -> lead + (R, n) (the reference's columns when the state came in its layout), given back like the input"""
    n = world.n
    J = world.from_soa(J_soa).reshape(lead + (R, n))
    if lay_s[0]:                                              # columns of the frozen coordinates: zero
        lay = world.ref_layout
        J = torch.zeros(lead + (R, lay.n_ref), dtype=torch.float64, device=world.device).index_copy(-1, lay._idx(world.device, "mobile"), J)
    return _give(world, J, like_device)


class TaskJacobianLayer(torch.autograd.Function):
    """(world, mapping, state) -> J [..., R, n]; backward: d<G, J>/dq in the position block, zero in the velocity block"""

    @staticmethod
    def forward(ctx, world, mapping, state):
        _join_if_deferred(world)                                  # before anything reads `state`: it may come out of the slices
        s_soa, _, lead, ctx.lay_s, _ = _inputs(world, "task_jacobian", state, None)
        R = mapping.getVelDim()
        out = _matrix_out(world, task_jacobian_soa(world, mapping, s_soa), R, lead, ctx.lay_s, state.device)
        ctx.world, ctx.mapping, ctx.s_soa, ctx.lead, ctx.device = world, mapping, s_soa, lead, state.device
        return out

    @staticmethod
    def backward(ctx, grad):
        world, mapping, lead, n = ctx.world, ctx.mapping, ctx.lead, ctx.world.n
        R = mapping.getVelDim()
        G = grad.detach().to(device=world.device, dtype=torch.float64)
        if ctx.lay_s[0]:
            G = G.index_select(-1, world.ref_layout._idx(world.device, "mobile"))
        G_soa = world.to_soa(G.reshape(-1, R * n)) if R > 0 else None
        gq = task_jacobian_vjp_soa(world, mapping, ctx.s_soa, G_soa)
        ds = torch.cat([world.from_soa(gq), torch.zeros((gq.shape[1], n), dtype=torch.float64, device=world.device)], 1).reshape(lead + (2 * n,))
        if ctx.lay_s[0]:
            ds = _expand(world, ds, lead, ctx.lay_s[1], "state")
        return None, None, _give(world, ds, ctx.device)


class TaskAccelLayer(torch.autograd.Function):
    """(world, mapping, state, accel or None) -> J accel + Jdot v (accel None: Jdot v) [..., R]; backward: the exact gradients"""

    @staticmethod
    def forward(ctx, world, mapping, state, accel):
        _join_if_deferred(world)
        what = "map_to_acc" if accel is not None else "task_jacobian_dot_times_v"
        s_soa, a_soa, lead, ctx.lay_s, ctx.lay_a = _inputs(world, what, state, accel)
        R = mapping.getVelDim()
        out = world.from_soa(task_accel_soa(world, mapping, s_soa, a_soa)).reshape(lead + (R,))
        ctx.world, ctx.mapping, ctx.soa, ctx.lead = world, mapping, (s_soa, a_soa), lead
        ctx.devices = (state.device, accel.device if accel is not None else None)
        return _give(world, out, state.device)

    @staticmethod
    def backward(ctx, grad):
        world, mapping, lead, n = ctx.world, ctx.mapping, ctx.lead, ctx.world.n
        R = mapping.getVelDim()
        s_soa, a_soa = ctx.soa
        g_soa = world.to_soa(grad.detach().to(device=world.device, dtype=torch.float64).reshape(-1, R)) if R > 0 else None
        want_a = a_soa is not None and ctx.needs_input_grad[3]
        gs, ga = task_accel_vjp_soa(world, mapping, s_soa, a_soa, g_soa, want_a)
        ds = world.from_soa(gs).reshape(lead + (2 * n,))
        if ctx.lay_s[0]:
            ds = _expand(world, ds, lead, ctx.lay_s[1], "state")
        da = None
        if want_a:
            da = world.from_soa(ga).reshape(lead + (n,))
            if ctx.lay_a[0]:
                da = _expand(world, da, lead, ctx.lay_a[1], "accel")
            da = _give(world, da, ctx.devices[1])
        return None, None, _give(world, ds, ctx.devices[0]), da


def task_jacobian(world, map: IKMapping, state: torch.Tensor) -> torch.Tensor:
    """The dense task Jacobian J(q) of the mapping's rows, [..., 2n] -> [..., R, n]: `map_to_vel(world, map, state) = J v`.  A column of a
    coordinate that is no ancestor of an entry's body is zero.  Differentiable with respect to the positions of `state` (exactly); the
    velocity block gets zero."""
    return TaskJacobianLayer.apply(world, map, state)


def task_jacobian_dot_times_v(world, map: IKMapping, state: torch.Tensor) -> torch.Tensor:
    """The bias acceleration Jdot(q, v) v of the mapping's rows, [..., 2n] -> [..., R]: the task-space acceleration at zero joint
    acceleration.  Differentiable with respect to positions and velocities, exactly."""
    return TaskAccelLayer.apply(world, map, state, None)


def map_to_acc(world, map: IKMapping, state: torch.Tensor, accel: torch.Tensor) -> torch.Tensor:
    """The task-space acceleration J(q) accel + Jdot(q, v) v of the mapping's rows at the joint accelerations `accel` [..., n]: the time
    derivative of `map_to_vel` along the motion, [..., R].  No gravity.  Differentiable with respect to positions, velocities and
    `accel`, exactly (d(J a + Jdot v)/dq included)."""
    if accel is None:
        raise NimbleAmdError("map_to_acc needs the accelerations (task_jacobian_dot_times_v gives the bias acceleration alone)")
    return TaskAccelLayer.apply(world, map, state, accel)


def task_jacobian_deriv(world, map: IKMapping, state: torch.Tensor) -> torch.Tensor:
    """d/dt J along the motion (q moving with v), [..., 2n] -> [..., R, n], so that `task_jacobian_deriv @ v` is
    task_jacobian_dot_times_v.  DETACHED: the forward pass only, no gradient flows through it (like the contact read-out)."""
    _join_if_deferred(world)
    s_soa, _, lead, lay_s, _ = _inputs(world, "task_jacobian_deriv", state, None)
    return _matrix_out(world, task_jacobian_soa(world, map, s_soa, deriv=True), map.getVelDim(), lead, lay_s, state.device)


# ---- the IKMapping getters on the World's current state (detached) ----
def _current_state(world) -> torch.Tensor:
    _join_if_deferred(world)
    if getattr(world, "_state", None) is None:
        raise NimbleAmdError("IKMapping: call world.setState() first")
    return world.from_soa(world._state)


def _one(world, t: torch.Tensor) -> torch.Tensor:
    return t[0] if getattr(world, "_one_d", False) else t


def _ref_columns(world, J: torch.Tensor) -> torch.Tensor:
    lay = world.ref_layout
    if lay is not None and J.shape[-1] != lay.n_ref:              # the reference's columns; the frozen ones are zero
        J = torch.zeros(J.shape[:-1] + (lay.n_ref,), dtype=torch.float64, device=world.device).index_copy(-1, lay._idx(world.device, "mobile"), J)
    return J


def current_jacobian(world, mapping: IKMapping, deriv: bool) -> torch.Tensor:
    s = _current_state(world)
    J = (task_jacobian_deriv if deriv else task_jacobian)(world, mapping, s).detach()
    return _one(world, _ref_columns(world, J))


def current_accelerations(world, mapping: IKMapping, accelerations: torch.Tensor) -> torch.Tensor:
    s = _current_state(world)
    a = accelerations.detach()
    if a.dim() == 1:
        a = a.unsqueeze(0)
    if a.shape[0] != s.shape[0]:
        raise ValueError(f"IKMapping.getAccelerations: {a.shape[0]} acceleration vectors for {s.shape[0]} worlds")
    return _one(world, map_to_acc(world, mapping, s, a.to(world.device)))
