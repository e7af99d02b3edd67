"""Joint-space dynamics quantities for batches of states: `inverse_dynamics`, `coriolis_and_gravity`, `mass_matrix`
(Skeleton::getInverseDynamics, dart/dynamics/Skeleton.cpp:9658-9666; World::getCoriolisAndGravityForces and World::getMassMatrix,
dart/simulation/World.cpp:1943-1986), and their counterparts `forward_dynamics`, `multiply_by_inv_mass_matrix`, `inv_mass_matrix`
(Skeleton::computeForwardDynamics, Skeleton.cpp:13296-13314; World::getInvMassMatrix), with exact gradients.

    tau = inverse_dynamics(world, state, accel)        [..., 2n], [..., n] -> [..., n]      tau = M(q) a + C(q, v)
    C   = coriolis_and_gravity(world, state)           [..., 2n] -> [..., n]                 inverse_dynamics with a = 0
    M   = mass_matrix(world, state)                    [..., 2n] -> [..., n, n]
    a   = forward_dynamics(world, state, tau)          [..., 2n], [..., n] -> [..., n]      a = M(q)^-1 (tau - C(q, v))
    y   = multiply_by_inv_mass_matrix(world, state, x) [..., 2n], [..., n] or [..., n, R] -> the shape of x:  y = M(q)^-1 x
    Mi  = inv_mass_matrix(world, state)                [..., 2n] -> [..., n, n]

The last three run the articulated-body recursion (O(n) per right-hand side; M is never formed) and are the inverse functions of the
first three: forward_dynamics(s, inverse_dynamics(s, a)) = a under the same `joint_forces`.  Their backward passes need no new theory:
lambda = M^-1 (cotangent) by the same recursion, the cotangent of tau / x is lambda, and the state receives -(d ID / d state)^T lambda
(-(d (M y) / dq)^T lambda for the M^-1 products) through the reverse kernel of inverse dynamics.  On a world with immobile skeletons a
`state` in the reference's layout gives THESE three outputs in the reference's layout too: the frozen coordinates have zero acceleration,
zero rows and columns in M^-1 (they cannot move, whatever acts on them) and zero gradient.

Each is one launch of csrc/dynamics.hip over all the leading dimensions (`[2n]` is one world, `[B, 2n]` a batch, `[B, T+1, 2n]` - what
`rollout()` returns - a whole trajectory), differentiable with respect to `state` and `accel`: recursive Newton-Euler with its exact
reverse pass (positions AND velocities; free and ball coordinates analytically through expMapJac), the composite-rigid-body algorithm for
M, whose backward pass is one reverse launch over n x B worlds (world (j, b): a = e_j, cotangent G[b, :, j], no velocity, no gravity;
above MASS_BACKWARD_WORLDS = 262144 launched worlds it is cut into launches of whole columns, which bounds the workspace).
The kernels read the World's current body inertias (World.setMasses).  With `joint_forces=True`, tau also carries
damping v + spring (q - rest + dt v) per coordinate - the terms the step puts on the right-hand side - so that tau applied as the joint
torques of `timestep()` reproduces `accel`.

Rules shared with mapping.py: CPU float64 tensors come back as CPU tensors, device tensors stay on the device; the World's state is left
untouched; a World in deferred-join mode is joined first.  On a world with immobile skeletons a `state` (and `accel`) in the reference's
layout is restricted to the mobile coordinates as map_to_pos does; the outputs are over the MOBILE coordinates and the gradients of the
frozen entries are zero.  The reference's own mass matrix has blocks for the immobile skeletons (their bodies keep their masses there),
which this model - it welded them to the world - cannot give.

Wrenches on bodies: `inverse_dynamics` and `forward_dynamics` take `wrenches` ([..., 6 E]: [torque; force] per entry) on `bodies` (an
IKMapping of spatial entries, or a list of body names / indices), expressed in each entry's frame and acting at its origin
(BodyNode::setExtWrench) or, with `world_frame=True`, in world coordinates at that origin: tau = M a + C - sum_e J_e^T W_e and
a = M^-1 (tau + sum_e J_e^T W_e - C), with exact gradients to the state, accel / tau AND the wrenches.  Built on them:
`contact_inverse_dynamics` (Skeleton::getContactInverseDynamics / getMultipleContactInverseDynamics, Skeleton.cpp:9705-9949; no autograd,
like the reference) and `inverse_dynamics_from_predictions` (Skeleton::getInverseDynamicsFromPredictions, Skeleton.cpp:9671-9697).
Out of scope: the ...NearCoP and ...OverTime variants of the contact solve, and gradients through it.

Inertia parameters: the six functions at the top take `mass=` (a 1-D tensor of world.getMassDims() entries, the contract of
timestep(..., mass=): world.setMasses(mass), and `mass` receives its gradient summed over all worlds), in closed form - inverse dynamics
is linear in every body's spatial inertia, forward dynamics is its inverse function.  Per world and without autograd:
`inverse_dynamics_mass_gradient`, `forward_dynamics_mass_gradient` ([..., massDims]) and `inverse_dynamics_mass_jacobian`,
`forward_dynamics_mass_jacobian` ([..., n, massDims]; Skeleton::getJacobianOfID / getJacobianOfFD with the mass vector as WithRespectTo,
Skeleton.hpp:650-718).
"""
from __future__ import annotations


import torch

from ._lib import check
from .mapping import _join_if_deferred, _ptr

ID_NO_VELOCITY, ID_NO_GRAVITY, ID_JOINT_FORCES = 1, 2, 4      # NBL_ID_* of include/nimble_amd.h
WRENCH_WORLD = 8                                               # NBL_WRENCH_WORLD: the wrench calls only
CID_SINGLE, CID_NEAREST, CID_MIN_TORQUE = 0, 1, 2              # NBL_CID_*
# mass_matrix's backward pass launches the reverse kernel over (columns x B) worlds, and the workspace is 48 doubles per body and launched
# world (Atlas-33, 34 bodies: 13 kB per world - 1.8 GB for all 33 columns of 4096 worlds).  Up to this many worlds go into ONE launch
# (3.4 GB of workspace on Atlas-33); a larger batch - 32768 worlds, or a [B, T+1] rollout - is cut into launches of whole columns.
MASS_BACKWARD_WORLDS = 1 << 18


def _workspace(world, B: int):
    """The dynamics scratch of the World: one buffer, grown to the largest B seen (like World._workspace)."""
    need = world._L.nbl_dynamics_workspace_bytes(world._h, B)
    ws = getattr(world, "_dyn_ws", None)
    if ws is None or ws.numel() < need or ws.device != world.device:
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=world.device)
        world._dyn_ws = ws
    return ws


# ---- raw SoA calls: state [2n][B], accel / tau [n][B], M [n * n][B] on the World's device ----
def inverse_dynamics_soa(world, s_soa: torch.Tensor, a_soa, flags: int = 0) -> torch.Tensor:
    B = s_soa.shape[1]
    tau = torch.empty((world.n, B), dtype=torch.float64, device=world.device)
    if B > 0:
        ws = _workspace(world, B)
        check(world._L.nbl_inverse_dynamics_forward(world._h, B, _ptr(s_soa), _ptr(a_soa), flags, _ptr(tau), _ptr(ws), ws.numel(), world._stream()),
              "nbl_inverse_dynamics_forward")
    return tau


def inverse_dynamics_vjp_soa(world, s_soa: torch.Tensor, a_soa, g_soa: torch.Tensor, flags: int = 0, want_accel: bool = True):
    B = s_soa.shape[1]
    gs = torch.empty((2 * world.n, B), dtype=torch.float64, device=world.device)
    ga = torch.empty((world.n, B), dtype=torch.float64, device=world.device) if want_accel else None
    if B > 0:
        ws = _workspace(world, B)
        check(world._L.nbl_inverse_dynamics_backward(world._h, B, _ptr(s_soa), _ptr(a_soa), flags, _ptr(g_soa), _ptr(gs), _ptr(ga), 0, _ptr(ws),
                                                     ws.numel(), world._stream()), "nbl_inverse_dynamics_backward")
    return gs, ga


def mass_matrix_soa(world, s_soa: torch.Tensor) -> torch.Tensor:
    B = s_soa.shape[1]
    M = torch.empty((world.n * world.n, B), dtype=torch.float64, device=world.device)
    if B > 0:
        ws = _workspace(world, B)
        check(world._L.nbl_mass_matrix(world._h, B, _ptr(s_soa), _ptr(M), _ptr(ws), ws.numel(), world._stream()), "nbl_mass_matrix")
    return M


def _fd_workspace(world, B: int):
    """The scratch of the forward-dynamics / M^-1 calls (84 doubles per body and world), kept like _workspace."""
    need = world._L.nbl_forward_dynamics_workspace_bytes(world._h, B)
    ws = getattr(world, "_fdyn_ws", None)
    if ws is None or ws.numel() < need or ws.device != world.device:
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=world.device)
        world._fdyn_ws = ws
    return ws


# ---- raw SoA calls: state [2n][B], tau / accel [n][B], X / Y [R][n][B], Minv [n * n][B] ----
def forward_dynamics_soa(world, s_soa: torch.Tensor, t_soa, flags: int = 0) -> torch.Tensor:
    B = s_soa.shape[1]
    acc = torch.empty((world.n, B), dtype=torch.float64, device=world.device)
    if B > 0:
        ws = _fd_workspace(world, B)
        check(world._L.nbl_forward_dynamics_forward(world._h, B, _ptr(s_soa), _ptr(t_soa), flags, _ptr(acc), _ptr(ws), ws.numel(), world._stream()),
              "nbl_forward_dynamics_forward")
    return acc


def forward_dynamics_vjp_soa(world, s_soa: torch.Tensor, t_soa, g_soa: torch.Tensor, flags: int = 0, want_state: bool = True, want_tau: bool = True):
    B = s_soa.shape[1]
    gs = torch.empty((2 * world.n, B), dtype=torch.float64, device=world.device) if want_state else None
    gt = torch.empty((world.n, B), dtype=torch.float64, device=world.device) if want_tau else None
    if B > 0:
        ws = _fd_workspace(world, B)
        check(world._L.nbl_forward_dynamics_backward(world._h, B, _ptr(s_soa), _ptr(t_soa), flags, _ptr(g_soa), _ptr(gs), _ptr(gt), 0, _ptr(ws),
                                                     ws.numel(), world._stream()), "nbl_forward_dynamics_backward")
    return gs, gt


def inv_mass_apply_soa(world, s_soa: torch.Tensor, X: torch.Tensor) -> torch.Tensor:
    """X [R, n, B] -> M^-1 X [R, n, B]"""
    R, _, B = X.shape
    Y = torch.empty_like(X)
    if B > 0:
        ws = _fd_workspace(world, B)
        check(world._L.nbl_inv_mass_apply(world._h, B, R, _ptr(s_soa), _ptr(X), _ptr(Y), _ptr(ws), ws.numel(), world._stream()), "nbl_inv_mass_apply")
    return Y


def inv_mass_matrix_soa(world, s_soa: torch.Tensor) -> torch.Tensor:
    B = s_soa.shape[1]
    Mi = torch.empty((world.n * world.n, B), dtype=torch.float64, device=world.device)
    if B > 0:
        ws = _fd_workspace(world, B)
        check(world._L.nbl_inv_mass_matrix(world._h, B, _ptr(s_soa), _ptr(Mi), _ptr(ws), ws.numel(), world._stream()), "nbl_inv_mass_matrix")
    return Mi


def _minv_grad_q(world, s_soa: torch.Tensor, Y: torch.Tensor, Lam: torch.Tensor) -> torch.Tensor:
    """-sum_r (d (M y_r) / dq)^T lambda_r, [n, B], of Y, Lam [R, n, B]: the reverse kernel of inverse dynamics over R x B worlds (world
    (r, b): a = y_r, cotangent -lambda_r, no velocity, no gravity), cut into launches of whole right-hand sides above
    MASS_BACKWARD_WORLDS like MassMatrixLayer.backward."""
    R, n, B = Y.shape
    per = max(1, min(R, MASS_BACKWARD_WORLDS // max(B, 1)))
    gq = torch.zeros((n, B), dtype=torch.float64, device=world.device)
    for r0 in range(0, R, per):
        r1 = min(R, r0 + per)
        rep = s_soa.repeat(1, r1 - r0)
        acc = Y[r0:r1].permute(1, 0, 2).reshape(n, (r1 - r0) * B).contiguous()
        cot = (-Lam[r0:r1]).permute(1, 0, 2).reshape(n, (r1 - r0) * B).contiguous()
        gs, _ = inverse_dynamics_vjp_soa(world, rep, acc, cot, ID_NO_VELOCITY | ID_NO_GRAVITY, want_accel=False)
        part = gs[:n].reshape(n, r1 - r0, B)
        for r in range(r1 - r0):                                  # summed one by one: the bits do not depend on the chunking
            gq += part[:, r]
    return gq


def _restrict(world, x: torch.Tensor, what: str, block: str):
    """(the tensor over the device's coordinates, whether it came in the reference's layout, its width)"""
    lay = world.ref_layout
    per = 2 if block == "state" else 1
    width = x.shape[-1] if x.dim() > 0 else -1
    ref = lay is not None and width == per * lay.n_ref
    if ref:
        x = lay.restrict_state(x, what, check_frozen=False) if block == "state" else x.index_select(-1, lay._idx(x.device, "mobile"))
    if x.dim() == 0 or x.shape[-1] != per * world.n:
        want = f"{per * world.n}" + (f" (or {per * lay.n_ref} in the reference's layout)" if lay is not None else "")
        raise ValueError(f"{what}: {block} has {width} entries per world; expected {want}")
    return x, ref, width


def _expand(world, d: torch.Tensor, lead, width: int, block: str) -> torch.Tensor:
    lay = world.ref_layout
    return torch.zeros(lead + (width,), dtype=torch.float64, device=world.device).index_copy(-1, lay._idx(world.device, "state" if block == "state" else "mobile"), d)


def _give(world, t: torch.Tensor, like_device):
    return world._to_host(t) if like_device.type == "cpu" else t.to(like_device)


class InverseDynamicsLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, world, state, accel, flags):
        _join_if_deferred(world)                                  # before anything reads `state`: it may come out of the slices
        n = world.n
        x, ctx.ref_s, ctx.width_s = _restrict(world, state.detach(), "inverse_dynamics", "state")
        lead = tuple(x.shape[:-1])
        s_soa = world.to_soa(world._prep(x.reshape(-1, 2 * n), 2 * n, "dyn_state"))
        a_soa = None
        if accel is not None:
            a, ctx.ref_a, ctx.width_a = _restrict(world, accel.detach(), "inverse_dynamics", "accel")
            if tuple(a.shape[:-1]) != lead:
                raise ValueError(f"inverse_dynamics: accel has leading shape {tuple(a.shape[:-1])}, state {lead}")
            a_soa = world.to_soa(world._prep(a.reshape(-1, n), n, "dyn_accel"))
            ctx.accel_device = accel.device
        tau = inverse_dynamics_soa(world, s_soa, a_soa, flags)
        out = world.from_soa(tau).reshape(lead + (n,))
        ctx.world, ctx.s_soa, ctx.a_soa, ctx.flags, ctx.lead, ctx.state_device = world, s_soa, a_soa, flags, lead, state.device
        return _give(world, out, state.device)

    @staticmethod
    def backward(ctx, grad_tau):
        world, n, lead = ctx.world, ctx.world.n, ctx.lead
        g = grad_tau.detach().to(device=world.device, dtype=torch.float64).reshape(-1, n)
        want_a = ctx.a_soa is not None and ctx.needs_input_grad[2]
        gs, ga = inverse_dynamics_vjp_soa(world, ctx.s_soa, ctx.a_soa, world.to_soa(g), ctx.flags, want_a)
        ds = world.from_soa(gs).reshape(lead + (2 * n,))
        if ctx.ref_s:                                             # zero for the frozen coordinates
            ds = _expand(world, ds, lead, ctx.width_s, "state")
        da = None
        if want_a:
            da = world.from_soa(ga).reshape(lead + (n,))
            if ctx.ref_a:
                da = _expand(world, da, lead, ctx.width_a, "accel")
        ds = _give(world, ds, ctx.state_device)
        if want_a:
            da = _give(world, da, ctx.accel_device)
        return None, ds, da, None


class MassMatrixLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, world, state):
        _join_if_deferred(world)
        n = world.n
        x, ctx.ref_s, ctx.width_s = _restrict(world, state.detach(), "mass_matrix", "state")
        lead = tuple(x.shape[:-1])
        s_soa = world.to_soa(world._prep(x.reshape(-1, 2 * n), 2 * n, "dyn_state"))
        M = mass_matrix_soa(world, s_soa)
        out = world.from_soa(M).reshape(lead + (n, n))
        ctx.world, ctx.s_soa, ctx.lead, ctx.state_device = world, s_soa, lead, state.device
        return _give(world, out, state.device)

    @staticmethod
    def backward(ctx, grad_M):
        """A reverse launch over n x B worlds (cut into whole columns above MASS_BACKWARD_WORLDS): world j * B + b has a = e_j and the cotangent G[b, :, j] (tau = M e_j is column j)."""
        world, n, lead = ctx.world, ctx.world.n, ctx.lead
        G = grad_M.detach().to(device=world.device, dtype=torch.float64).reshape(-1, n, n)
        B = G.shape[0]
        # columns j0 .. j1 per launch: all n at once while n x B stays within MASS_BACKWARD_WORLDS (the workspace is per launched world)
        per = max(1, min(n, MASS_BACKWARD_WORLDS // max(B, 1)))
        eye_n = torch.eye(n, dtype=torch.float64, device=world.device)
        Gt = G.permute(1, 2, 0)                                   # [i, j, b]
        gq = torch.zeros((n, B), dtype=torch.float64, device=world.device)
        for j0 in range(0, n, per):
            j1 = min(n, j0 + per)
            rep = ctx.s_soa.repeat(1, j1 - j0)
            eye = eye_n[:, j0:j1].repeat_interleave(B, dim=1)
            gt = Gt[:, j0:j1].reshape(n, (j1 - j0) * B).contiguous()
            gs, _ = inverse_dynamics_vjp_soa(world, rep, eye, gt, ID_NO_VELOCITY | ID_NO_GRAVITY, want_accel=False)
            part = gs[:n].reshape(n, j1 - j0, B)
            for j in range(j1 - j0):                              # summed column by column: the bits do not depend on the chunking
                gq += part[:, j]
        ds = world.from_soa(torch.cat([gq, torch.zeros_like(gq)], 0)).reshape(lead + (2 * n,))
        if ctx.ref_s:
            ds = _expand(world, ds, lead, ctx.width_s, "state")
        return None, _give(world, ds, ctx.state_device)


class ForwardDynamicsLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, world, state, tau, flags):
        _join_if_deferred(world)
        n = world.n
        x, ctx.ref_s, ctx.width_s = _restrict(world, state.detach(), "forward_dynamics", "state")
        lead = tuple(x.shape[:-1])
        s_soa = world.to_soa(world._prep(x.reshape(-1, 2 * n), 2 * n, "dyn_state"))
        t_soa = None
        if tau is not None:
            t, ctx.ref_t, ctx.width_t = _restrict(world, tau.detach(), "forward_dynamics", "tau")
            if tuple(t.shape[:-1]) != lead:
                raise ValueError(f"forward_dynamics: tau has leading shape {tuple(t.shape[:-1])}, state {lead}")
            t_soa = world.to_soa(world._prep(t.reshape(-1, n), n, "dyn_accel"))
            ctx.tau_device = tau.device
        acc = forward_dynamics_soa(world, s_soa, t_soa, flags)
        out = world.from_soa(acc).reshape(lead + (n,))
        if ctx.ref_s:                                             # zero acceleration of the frozen coordinates
            out = _expand(world, out, lead, ctx.width_s // 2, "accel")
        ctx.world, ctx.s_soa, ctx.t_soa, ctx.flags, ctx.lead, ctx.state_device = world, s_soa, t_soa, flags, lead, state.device
        return _give(world, out, state.device)

    @staticmethod
    def backward(ctx, grad_accel):
        world, n, lead = ctx.world, ctx.world.n, ctx.lead
        g = grad_accel.detach().to(device=world.device, dtype=torch.float64)
        if ctx.ref_s:
            g = g.index_select(-1, world.ref_layout._idx(world.device, "mobile"))
        want_s = ctx.needs_input_grad[1]
        want_t = ctx.t_soa is not None and ctx.needs_input_grad[2]
        gs, gt = forward_dynamics_vjp_soa(world, ctx.s_soa, ctx.t_soa, world.to_soa(g.reshape(-1, n)), ctx.flags, want_s, want_t)
        ds = dt = None
        if want_s:
            ds = world.from_soa(gs).reshape(lead + (2 * n,))
            if ctx.ref_s:
                ds = _expand(world, ds, lead, ctx.width_s, "state")
            ds = _give(world, ds, ctx.state_device)
        if want_t:
            dt = world.from_soa(gt).reshape(lead + (n,))
            if ctx.ref_t:
                dt = _expand(world, dt, lead, ctx.width_t, "tau")
            dt = _give(world, dt, ctx.tau_device)
        return None, ds, dt, None


def _state_grad_q(world, gq: torch.Tensor, ctx):
    """[n, B] position cotangent -> the cotangent of `state` (the velocity block receives nothing)"""
    n, lead = world.n, ctx.lead
    ds = world.from_soa(torch.cat([gq, torch.zeros_like(gq)], 0)).reshape(lead + (2 * n,))
    if ctx.ref_s:
        ds = _expand(world, ds, lead, ctx.width_s, "state")
    return _give(world, ds, ctx.state_device)


class InvMassApplyLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, world, state, x):
        _join_if_deferred(world)
        n = world.n
        s, ctx.ref_s, ctx.width_s = _restrict(world, state.detach(), "multiply_by_inv_mass_matrix", "state")
        lead = tuple(s.shape[:-1])
        ctx.matrix = x.dim() == state.dim() + 1                   # [..., n, R]; else [..., n]
        xr = x.detach().transpose(-1, -2) if ctx.matrix else x.detach().unsqueeze(-2)      # [..., R, n]
        xr, ctx.ref_x, ctx.width_x = _restrict(world, xr, "multiply_by_inv_mass_matrix", "x")
        if tuple(xr.shape[:-2]) != lead:
            raise ValueError(f"multiply_by_inv_mass_matrix: x has leading shape {tuple(xr.shape[:-2])}, state {lead}")
        R = xr.shape[-2]
        if R < 1:
            raise ValueError("multiply_by_inv_mass_matrix: x has no right-hand side")
        s_soa = world.to_soa(world._prep(s.reshape(-1, 2 * n), 2 * n, "dyn_state"))
        B = s_soa.shape[1]
        X = world._prep(xr.reshape(-1, n), n, "dyn_rhs").reshape(B, R, n).permute(1, 2, 0).contiguous()    # [R, n, B]
        Y = inv_mass_apply_soa(world, s_soa, X)
        ctx.world, ctx.s_soa, ctx.Y, ctx.lead, ctx.R, ctx.state_device, ctx.x_device = world, s_soa, Y, lead, R, state.device, x.device
        return _give(world, InvMassApplyLayer._shape(ctx, Y, ctx.ref_s), state.device)

    @staticmethod
    def _shape(ctx, Y, ref):
        """[R, n, B] -> [..., n, R] or [..., n], in the reference's layout if asked"""
        world, n, lead, R = ctx.world, ctx.world.n, ctx.lead, ctx.R
        out = Y.permute(2, 0, 1).reshape(lead + (R, n))
        if ref:
            out = _expand(world, out, lead + (R,), world.ref_layout.n_ref, "x")
        return out.transpose(-1, -2).contiguous() if ctx.matrix else out.squeeze(-2)

    @staticmethod
    def backward(ctx, grad_y):
        world, n, R = ctx.world, ctx.world.n, ctx.R
        g = grad_y.detach().to(device=world.device, dtype=torch.float64)
        g = g.transpose(-1, -2) if ctx.matrix else g.unsqueeze(-2)                         # [..., R, n(_ref)]
        if ctx.ref_s:
            g = g.index_select(-1, world.ref_layout._idx(world.device, "mobile"))
        B = ctx.s_soa.shape[1]
        Lam = inv_mass_apply_soa(world, ctx.s_soa, g.reshape(B, R, n).permute(1, 2, 0).contiguous())
        ds = _state_grad_q(world, _minv_grad_q(world, ctx.s_soa, ctx.Y, Lam), ctx) if ctx.needs_input_grad[1] else None
        dx = _give(world, InvMassApplyLayer._shape(ctx, Lam, ctx.ref_x), ctx.x_device) if ctx.needs_input_grad[2] else None
        return None, ds, dx


class InvMassMatrixLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, world, state):
        _join_if_deferred(world)
        n = world.n
        x, ctx.ref_s, ctx.width_s = _restrict(world, state.detach(), "inv_mass_matrix", "state")
        lead = tuple(x.shape[:-1])
        s_soa = world.to_soa(world._prep(x.reshape(-1, 2 * n), 2 * n, "dyn_state"))
        Mi = inv_mass_matrix_soa(world, s_soa)
        out = world.from_soa(Mi).reshape(lead + (n, n))
        if ctx.ref_s:                                             # zero rows and columns of the frozen coordinates
            out = _expand_square(world, out, lead)
        ctx.world, ctx.s_soa, ctx.Mi, ctx.lead, ctx.state_device = world, s_soa, Mi, lead, state.device
        return _give(world, out, state.device)

    @staticmethod
    def backward(ctx, grad_Mi):
        """Lambda = M^-1 G; grad_q = -sum_j (d (M y_j) / dq)^T lambda_j, y_j / lambda_j = column j of M^-1 / of Lambda."""
        world, n = ctx.world, ctx.world.n
        G = grad_Mi.detach().to(device=world.device, dtype=torch.float64)
        if ctx.ref_s:
            ix = world.ref_layout._idx(world.device, "mobile")
            G = G.index_select(-1, ix).index_select(-2, ix)
        B = ctx.s_soa.shape[1]
        Lam = inv_mass_apply_soa(world, ctx.s_soa, G.reshape(B, n, n).permute(2, 1, 0).contiguous())    # [j, i, b]
        Y = ctx.Mi.reshape(n, n, B)                                # [j][i][b] = Minv[i][j]: the matrix is symmetric bit for bit
        return None, _state_grad_q(world, _minv_grad_q(world, ctx.s_soa, Y, Lam), ctx)


def _expand_square(world, M: torch.Tensor, lead) -> torch.Tensor:
    """[..., n, n] over the mobile coordinates -> [..., n_ref, n_ref] with zero rows and columns for the frozen ones"""
    lay = world.ref_layout
    ix = lay._idx(world.device, "mobile")
    rows = torch.zeros(lead + (world.n, lay.n_ref), dtype=torch.float64, device=world.device).index_copy(-1, ix, M)
    return torch.zeros(lead + (lay.n_ref, lay.n_ref), dtype=torch.float64, device=world.device).index_copy(-2, ix, rows)


# ---- wrenches on bodies -------------------------------------------------------------------------------------------------------------------
def wrench_set(world, bodies):
    """`bodies` -> the IKMapping of spatial entries the wrench calls take: an IKMapping is checked and passed on, a list of body names /
    indices (of world.description.bodies) becomes one spatial entry each, in that order."""
    from .mapping import KIN_SPATIAL, IKMapping
    if isinstance(bodies, IKMapping):
        if any(k != KIN_SPATIAL for k, _, _, _ in bodies._entries):
            raise ValueError("wrenches need spatial entries (IKMapping.addSpatialBodyNode): a wrench acts on a whole frame")
        return bodies
    if bodies is None:
        raise ValueError("wrenches need `bodies`: an IKMapping of spatial entries, or a list of body names / indices")
    if isinstance(bodies, (str, int)):
        bodies = [bodies]
    m = IKMapping(world)
    for b in bodies:
        m.addSpatialBodyNode(b)
    return m


def _wr_workspace(world, km, B: int):
    """The scratch of the wrench calls and of the contact solve, kept like _workspace."""
    need = world._L.nbl_wrench_workspace_bytes(world._h, km, B)
    ws = getattr(world, "_wrench_ws", None)
    if ws is None or ws.numel() < need or ws.device != world.device:
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=world.device)
        world._wrench_ws = ws
    return ws


def _km(world, mapping):
    """the device map of `mapping`, None (a set without entries) when it has none"""
    return mapping._device_map(world) if mapping is not None and mapping._entries else None


# raw SoA calls: state [2n][B], accel / tau [n][B], wrench [6 E][B]
def inverse_dynamics_wrench_soa(world, mapping, s_soa, a_soa, w_soa, flags: int = 0) -> torch.Tensor:
    B = s_soa.shape[1]
    tau = torch.empty((world.n, B), dtype=torch.float64, device=world.device)
    if B > 0:
        km = _km(world, mapping)
        ws = _wr_workspace(world, km, B)
        check(world._L.nbl_inverse_dynamics_wrench_forward(world._h, km, B, _ptr(s_soa), _ptr(a_soa), _ptr(w_soa), flags, _ptr(tau), _ptr(ws),
                                                           ws.numel(), world._stream()), "nbl_inverse_dynamics_wrench_forward")
    return tau


def forward_dynamics_wrench_soa(world, mapping, s_soa, t_soa, w_soa, flags: int = 0) -> torch.Tensor:
    B = s_soa.shape[1]
    acc = torch.empty((world.n, B), dtype=torch.float64, device=world.device)
    if B > 0:
        km = _km(world, mapping)
        ws = _wr_workspace(world, km, B)
        check(world._L.nbl_forward_dynamics_wrench_forward(world._h, km, B, _ptr(s_soa), _ptr(t_soa), _ptr(w_soa), flags, _ptr(acc), _ptr(ws),
                                                           ws.numel(), world._stream()), "nbl_forward_dynamics_wrench_forward")
    return acc


def _wrench_vjp_soa(world, fn: str, mapping, s_soa, x_soa, w_soa, g_soa, flags, want_state, want_x, want_w):
    """(grad_state [2n][B], grad of accel / tau [n][B], grad_wrench [6 E][B]) of one of the two reverse calls; None where not wanted"""
    B, E6 = s_soa.shape[1], w_soa.shape[0]
    dev = world.device
    gs = torch.empty((2 * world.n, B), dtype=torch.float64, device=dev) if want_state else None
    gx = torch.empty((world.n, B), dtype=torch.float64, device=dev) if want_x else None
    gw = torch.empty((E6, B), dtype=torch.float64, device=dev) if want_w else None
    if B > 0:
        km = _km(world, mapping)
        ws = _wr_workspace(world, km, B)
        check(getattr(world._L, fn)(world._h, km, B, _ptr(s_soa), _ptr(x_soa), _ptr(w_soa), flags, _ptr(g_soa), _ptr(gs), _ptr(gx),
                                    _ptr(gw) if E6 else None, 0, _ptr(ws), ws.numel(), world._stream()), fn)
    return gs, gx, gw


def contact_inverse_dynamics_soa(world, mapping, s_soa, a_soa, g_soa, mode: int, flags: int = ID_JOINT_FORCES):
    """(wrenches [6 E][B], tau [n][B])"""
    B, E6 = s_soa.shape[1], 6 * len(mapping._entries)
    W = torch.empty((E6, B), dtype=torch.float64, device=world.device)
    tau = torch.empty((world.n, B), dtype=torch.float64, device=world.device)
    km = _km(world, mapping)
    ws = _wr_workspace(world, km, max(B, 1))
    check(world._L.nbl_contact_inverse_dynamics(world._h, km, B, _ptr(s_soa), _ptr(a_soa), _ptr(g_soa), mode, flags, _ptr(W), _ptr(tau), _ptr(ws),
                                                ws.numel(), world._stream()), "nbl_contact_inverse_dynamics")
    return W, tau


def _wrench_inputs(world, what, mapping, wrenches, lead):
    E6 = 6 * len(mapping._entries)
    if wrenches.dim() == 0 or wrenches.shape[-1] != E6 or tuple(wrenches.shape[:-1]) != lead:
        raise ValueError(f"{what}: wrenches have shape {tuple(wrenches.shape)}; expected {lead + (E6,)} ([torque; force] per entry)")
    if E6 == 0:                                                   # a set without entries: nothing to upload
        worlds = 1
        for d in lead:
            worlds *= d
        return torch.empty((0, worlds), dtype=torch.float64, device=world.device)
    return world.to_soa(world._prep(wrenches.detach().reshape(-1, E6), E6, "dyn_wrench"))


class _WrenchLayer(torch.autograd.Function):
    """inverse (FD = False) or forward (FD = True) dynamics with wrenches; x = accel or tau"""

    @staticmethod
    def forward(ctx, world, state, x, wrenches, mapping, flags, fd):
        _join_if_deferred(world)
        n = world.n
        what = "forward_dynamics" if fd else "inverse_dynamics"
        s, ctx.ref_s, ctx.width_s = _restrict(world, state.detach(), what, "state")
        lead = tuple(s.shape[:-1])
        s_soa = world.to_soa(world._prep(s.reshape(-1, 2 * n), 2 * n, "dyn_state"))
        x_soa = None
        if x is not None:
            xr, ctx.ref_x, ctx.width_x = _restrict(world, x.detach(), what, "tau" if fd else "accel")
            if tuple(xr.shape[:-1]) != lead:
                raise ValueError(f"{what}: {'tau' if fd else 'accel'} has leading shape {tuple(xr.shape[:-1])}, state {lead}")
            x_soa = world.to_soa(world._prep(xr.reshape(-1, n), n, "dyn_accel"))
            ctx.x_device = x.device
        w_soa = _wrench_inputs(world, what, mapping, wrenches, lead)
        out = (forward_dynamics_wrench_soa if fd else inverse_dynamics_wrench_soa)(world, mapping, s_soa, x_soa, w_soa, flags)
        out = world.from_soa(out).reshape(lead + (n,))
        if fd and ctx.ref_s:                                      # zero acceleration of the frozen coordinates
            out = _expand(world, out, lead, ctx.width_s // 2, "accel")
        ctx.world, ctx.mapping, ctx.s_soa, ctx.x_soa, ctx.w_soa, ctx.flags, ctx.fd, ctx.lead = world, mapping, s_soa, x_soa, w_soa, flags, fd, lead
        ctx.state_device, ctx.w_device = state.device, wrenches.device
        return _give(world, out, state.device)

    @staticmethod
    def backward(ctx, grad_out):
        world, n, lead, fd = ctx.world, ctx.world.n, ctx.lead, ctx.fd
        g = grad_out.detach().to(device=world.device, dtype=torch.float64)
        if fd and ctx.ref_s:
            g = g.index_select(-1, world.ref_layout._idx(world.device, "mobile"))
        want_s = ctx.needs_input_grad[1]
        want_x = ctx.x_soa is not None and ctx.needs_input_grad[2]
        want_w = ctx.needs_input_grad[3] and ctx.w_soa.shape[0] > 0
        fn = "nbl_forward_dynamics_wrench_backward" if fd else "nbl_inverse_dynamics_wrench_backward"
        gs, gx, gw = _wrench_vjp_soa(world, fn, ctx.mapping, ctx.s_soa, ctx.x_soa, ctx.w_soa, world.to_soa(g.reshape(-1, n)), ctx.flags,
                                     want_s, want_x, want_w)
        ds = dx = dw = None
        if want_s:
            ds = world.from_soa(gs).reshape(lead + (2 * n,))
            if ctx.ref_s:
                ds = _expand(world, ds, lead, ctx.width_s, "state")
            ds = _give(world, ds, ctx.state_device)
        if want_x:
            dx = world.from_soa(gx).reshape(lead + (n,))
            if ctx.ref_x:
                dx = _expand(world, dx, lead, ctx.width_x, "accel")
            dx = _give(world, dx, ctx.x_device)
        if want_w:
            dw = _give(world, world.from_soa(gw).reshape(lead + (gw.shape[0],)), ctx.w_device)
        elif ctx.needs_input_grad[3]:
            dw = torch.zeros(lead + (0,), dtype=torch.float64, device=ctx.w_device)
        return None, ds, dx, dw, None, None, None


def _wrench_flags(joint_forces: bool, world_frame: bool) -> int:
    return (ID_JOINT_FORCES if joint_forces else 0) | (WRENCH_WORLD if world_frame else 0)


# ---- gradients to the registered inertia ("mass") parameters (World.tuneMass / setMasses) ----------------------------------------------------
# Inverse dynamics is linear in every body's spatial inertia: d(g^T tau) / d theta_p = Fb_i . (dG_p A_i) - ad(V_i, Fb_i) . (dG_p V_i), one
# root -> leaf sweep and one contraction per parameter (k_inverse_dynamics_inertia_vjp); forward dynamics is its inverse function,
# d a / d theta = -M^-1 d ID / d theta at (q, v, a).  Skeleton::getJacobianOfID / C / M / Minv / FD with the mass vector as WithRespectTo
# (Skeleton.hpp:650-718), which the reference finite-differences.
def _mass_dims(world, what: str) -> int:
    d = world.getMassDims()
    if d == 0:
        raise ValueError(f"{what}: no mass parameters are registered on this world (World.tuneMass)")
    return d


def _set_mass(world, mass, what: str):
    """the contract of timestep(..., mass=): world.setMasses(mass)"""
    if not torch.is_tensor(mass) or mass.dim() != 1 or mass.shape[0] != world.getMassDims():
        raise ValueError(f"mass must be a 1-D tensor of world.getMassDims() = {world.getMassDims()} entries")
    _mass_dims(world, what)
    world.setMasses(mass)


def inverse_dynamics_inertia_vjp_soa(world, s_soa: torch.Tensor, a_soa, g_soa: torch.Tensor, flags: int = 0, out=None) -> torch.Tensor:
    """[massDims][B] = (out given: +=) (d tau / d theta)^T g per world, raw SoA like inverse_dynamics_vjp_soa"""
    B, P = s_soa.shape[1], _mass_dims(world, "inverse_dynamics_inertia_vjp_soa")
    gm = out if out is not None else torch.empty((P, B), dtype=torch.float64, device=world.device)
    if B > 0:
        ws = _workspace(world, B)
        check(world._L.nbl_inverse_dynamics_backward_inertia(world._h, B, _ptr(s_soa), _ptr(a_soa), flags, _ptr(g_soa), _ptr(gm),
                                                             1 if out is not None else 0, _ptr(ws), ws.numel(), world._stream()),
              "nbl_inverse_dynamics_backward_inertia")
    return gm


def forward_dynamics_inertia_vjp_soa(world, mapping, s_soa: torch.Tensor, t_soa, w_soa, g_soa: torch.Tensor, flags: int = 0, out=None) -> torch.Tensor:
    """[massDims][B] = (out given: +=) (d a / d theta)^T g per world; mapping / w_soa None: no wrenches"""
    B, P = s_soa.shape[1], _mass_dims(world, "forward_dynamics_inertia_vjp_soa")
    gm = out if out is not None else torch.empty((P, B), dtype=torch.float64, device=world.device)
    if B > 0:
        km = _km(world, mapping)
        ws = _wr_workspace(world, km, B) if km is not None else _fd_workspace(world, B)
        if km is None:
            flags &= ~WRENCH_WORLD                                # a frame for wrenches that are not there
        check(world._L.nbl_forward_dynamics_backward_inertia(world._h, km, B, _ptr(s_soa), _ptr(t_soa), _ptr(w_soa) if km is not None else None, flags,
                                                             _ptr(g_soa), _ptr(gm), 1 if out is not None else 0, _ptr(ws), ws.numel(), world._stream()),
              "nbl_forward_dynamics_backward_inertia")
    return gm


def _dyn_inputs(world, what: str, state, x=None, xname: str = "accel"):
    """(state [2n][B], x [n][B] or None, the leading shape) of `state` [..., 2n] and x [..., n] (the reference's layout allowed)"""
    _join_if_deferred(world)
    n = world.n
    s, _, _ = _restrict(world, state.detach(), what, "state")
    lead = tuple(s.shape[:-1])
    s_soa = world.to_soa(world._prep(s.reshape(-1, 2 * n), 2 * n, "dyn_state"))
    return s_soa, (None if x is None else _vec_soa(world, what, x, xname, lead, "dyn_accel")), lead


def _vec_soa(world, what: str, x, xname: str, lead, role: str):
    n = world.n
    xr, _, _ = _restrict(world, x.detach(), what, xname)
    if tuple(xr.shape[:-1]) != lead:
        raise ValueError(f"{what}: {xname} has leading shape {tuple(xr.shape[:-1])}, state {lead}")
    return world.to_soa(world._prep(xr.reshape(-1, n), n, role))


def _per_world(world, gm: torch.Tensor, lead, like_device):
    """[massDims][B] -> [..., massDims] where the state came from"""
    return _give(world, world.from_soa(gm).reshape(lead + (gm.shape[0],)), like_device)


def inverse_dynamics_mass_gradient(world, state: torch.Tensor, accel, grad_tau: torch.Tensor, joint_forces: bool = False) -> torch.Tensor:
    """(d tau / d mass)^T grad_tau of inverse_dynamics(world, state, accel) PER WORLD: [..., massDims], at the World's current masses; no
    autograd.  accel None: of coriolis_and_gravity.  Wrenches on bodies and the joint forces do not depend on the inertias: the result
    serves inverse_dynamics(..., wrenches=) unchanged."""
    what = "inverse_dynamics_mass_gradient"
    _mass_dims(world, what)
    s_soa, a_soa, lead = _dyn_inputs(world, what, state, accel)
    g_soa = _vec_soa(world, what, grad_tau, "grad_tau", lead, "dyn_cot")
    return _per_world(world, inverse_dynamics_inertia_vjp_soa(world, s_soa, a_soa, g_soa, ID_JOINT_FORCES if joint_forces else 0), lead, state.device)


def forward_dynamics_mass_gradient(world, state: torch.Tensor, tau, grad_accel: torch.Tensor, joint_forces: bool = False, wrenches=None,
                                   bodies=None, world_frame: bool = False) -> torch.Tensor:
    """(d a / d mass)^T grad_accel of forward_dynamics(world, state, tau[, wrenches ...]) PER WORLD: [..., massDims]; no autograd."""
    what = "forward_dynamics_mass_gradient"
    _mass_dims(world, what)
    s_soa, t_soa, lead = _dyn_inputs(world, what, state, tau, "tau")
    g_soa = _vec_soa(world, what, grad_accel, "grad_accel", lead, "dyn_cot")
    mapping = w_soa = None
    if wrenches is not None:
        mapping = wrench_set(world, bodies)
        w_soa = _wrench_inputs(world, what, mapping, wrenches, lead)
    gm = forward_dynamics_inertia_vjp_soa(world, mapping, s_soa, t_soa, w_soa, g_soa, _wrench_flags(joint_forces, world_frame and wrenches is not None))
    return _per_world(world, gm, lead, state.device)


def _mass_jacobian(world, call, s_soa: torch.Tensor, x_soa, lead, like_device) -> torch.Tensor:
    """[..., n, massDims]: call(states, x, cotangents) over n x B worlds with the unit cotangents e_i (world i * B + b), cut into launches of
    whole rows above MASS_BACKWARD_WORLDS"""
    n, B, P = world.n, s_soa.shape[1], world.getMassDims()
    per = max(1, min(n, MASS_BACKWARD_WORLDS // max(B, 1)))
    eye_n = torch.eye(n, dtype=torch.float64, device=world.device)
    J = torch.empty((P, n, B), dtype=torch.float64, device=world.device)
    for i0 in range(0, n, per):
        i1 = min(n, i0 + per)
        k = i1 - i0
        J[:, i0:i1] = call(s_soa.repeat(1, k), None if x_soa is None else x_soa.repeat(1, k), eye_n[:, i0:i1].repeat_interleave(B, dim=1).contiguous()).reshape(P, k, B)
    return _give(world, J.permute(2, 1, 0).reshape(lead + (n, P)).contiguous(), like_device)


def inverse_dynamics_mass_jacobian(world, state: torch.Tensor, accel, joint_forces: bool = False) -> torch.Tensor:
    """d tau / d mass of inverse_dynamics(world, state, accel): [..., n, massDims] - the dynamics regressor restricted to the registered
    parameters (Skeleton::getJacobianOfID wrt the mass vector; accel None: getJacobianOfC).  One launch over n x B worlds.
    joint_forces is taken for symmetry with inverse_dynamics and changes nothing: those forces do not depend on the inertias."""
    what = "inverse_dynamics_mass_jacobian"
    _mass_dims(world, what)
    s_soa, a_soa, lead = _dyn_inputs(world, what, state, accel)
    fl = ID_JOINT_FORCES if joint_forces else 0
    return _mass_jacobian(world, lambda s, a, g: inverse_dynamics_inertia_vjp_soa(world, s, a, g, fl), s_soa, a_soa, lead, state.device)


def forward_dynamics_mass_jacobian(world, state: torch.Tensor, tau, joint_forces: bool = False) -> torch.Tensor:
    """d a / d mass of forward_dynamics(world, state, tau): [..., n, massDims] (Skeleton::getJacobianOfFD wrt the mass vector).
    joint_forces: of forward_dynamics(..., joint_forces=True) - the damping and spring forces change a, and with it the Jacobian."""
    what = "forward_dynamics_mass_jacobian"
    _mass_dims(world, what)
    s_soa, t_soa, lead = _dyn_inputs(world, what, state, tau, "tau")
    fl = ID_JOINT_FORCES if joint_forces else 0
    return _mass_jacobian(world, lambda s, t, g: forward_dynamics_inertia_vjp_soa(world, None, s, t, None, g, fl), s_soa, t_soa, lead, state.device)


class _MassTap(torch.autograd.Function):
    """Hands `out` on unchanged and gives `mass` its gradient: the layers above stay the functions they are - with and without mass=
    their outputs and their other gradients are the same bits.  pull(grad_out) -> [massDims], summed over the worlds.
    The backward passes read the World's CURRENT masses (World.setMasses): this node puts the forward pass's masses back if they were
    changed in between (an unchanged vector costs nothing), so the gradients of one call are those of one mass vector whatever happened
    to the World after the forward pass.  It runs before the backward nodes of the layer it wraps because autograd reaches them only
    through it (its input is their output).  Documented on the public functions (`mass:`)."""

    @staticmethod
    def forward(ctx, out, mass, pull, world):
        ctx.pull, ctx.mass_device, ctx.world, ctx.mass_value = pull, mass.device, world, mass.detach().clone()
        return out.view_as(out)

    @staticmethod
    def backward(ctx, grad_out):
        ctx.world.setMasses(ctx.mass_value)
        d_mass = ctx.pull(grad_out.detach()).to(ctx.mass_device) if ctx.needs_input_grad[1] else None
        return grad_out, d_mass, None, None


def _columns_mass_grad(world, s_soa: torch.Tensor, Y: torch.Tensor, Cot: torch.Tensor) -> torch.Tensor:
    """sum_r (d (M y_r) / d theta)^T cot_r, [massDims, B], of Y, Cot [R, n, B]: the inertia kernel over R x B worlds (world (r, b): a = y_r,
    no velocity, no gravity), cut into launches of whole right-hand sides like _minv_grad_q"""
    R, n, B = Y.shape
    per = max(1, min(R, MASS_BACKWARD_WORLDS // max(B, 1)))
    gm = torch.zeros((world.getMassDims(), B), dtype=torch.float64, device=world.device)
    for r0 in range(0, R, per):
        r1 = min(R, r0 + per)
        acc = Y[r0:r1].permute(1, 0, 2).reshape(n, (r1 - r0) * B).contiguous()
        cot = Cot[r0:r1].permute(1, 0, 2).reshape(n, (r1 - r0) * B).contiguous()
        part = inverse_dynamics_inertia_vjp_soa(world, s_soa.repeat(1, r1 - r0), acc, cot, ID_NO_VELOCITY | ID_NO_GRAVITY).reshape(-1, r1 - r0, B)
        for r in range(r1 - r0):                                  # summed one by one: the bits do not depend on the chunking
            gm += part[:, r]
    return gm


def _square_soa(world, G: torch.Tensor, ref: bool, B: int) -> torch.Tensor:
    """a cotangent [..., n, n] (the reference's layout: its mobile rows and columns) -> [B, n, n] on the World's device"""
    G = G.to(device=world.device, dtype=torch.float64)
    if ref:
        ix = world.ref_layout._idx(world.device, "mobile")
        G = G.index_select(-1, ix).index_select(-2, ix)
    return G.reshape(B, world.n, world.n)


def inverse_dynamics(world, state: torch.Tensor, accel: torch.Tensor, joint_forces: bool = False, wrenches=None, bodies=None,
                     world_frame: bool = False, mass=None) -> torch.Tensor:
    """tau = M(q) a + C(q, v) of `state` = [q; v] ([..., 2n]) and `accel` ([..., n]) -> [..., n]; differentiable in both (exactly).
    joint_forces: + damping v + spring (q - rest + dt v), so that tau applied in timestep() reproduces accel.
    wrenches ([..., 6 E], [torque; force] per entry of `bodies`: an IKMapping of spatial entries, or body names / indices): tau also carries
    - sum_e J_e^T W_e, the wrenches expressed in their entry's frame and acting at its origin (BodyNode::setExtWrench), or with
    world_frame in world coordinates at that origin; differentiable in the wrenches too.  Without `wrenches` the call is what it was.
    mass (a 1-D tensor of world.getMassDims() entries, the contract of timestep(..., mass=)): world.setMasses(mass) first, and `mass`
    receives its gradient summed over all worlds; without it the call is what it was.  The backward pass of a call with mass= begins by
    calling world.setMasses with the forward pass's vector again: if the World's masses were changed in between, backward() resets them
    (all gradients of the call are then those of one mass vector; an unchanged vector costs nothing)."""
    if mass is not None:
        _set_mass(world, mass, "inverse_dynamics")
    if wrenches is None:
        if bodies is not None or world_frame:
            raise ValueError("inverse_dynamics: `bodies` / `world_frame` describe `wrenches`, which were not given")
        out = InverseDynamicsLayer.apply(world, state, accel, ID_JOINT_FORCES if joint_forces else 0)
    else:
        out = _WrenchLayer.apply(world, state, accel, wrenches, wrench_set(world, bodies), _wrench_flags(joint_forces, world_frame), False)
    if mass is None:
        return out
    return _MassTap.apply(out, mass, lambda g: inverse_dynamics_mass_gradient(world, state, accel, g, joint_forces).reshape(-1, mass.shape[0]).sum(0), world)


def coriolis_and_gravity(world, state: torch.Tensor, mass=None) -> torch.Tensor:
    """C(q, v): Coriolis, centrifugal and gravity forces of `state` ([..., 2n] -> [..., n]) = inverse_dynamics with a = 0.  mass: as there."""
    if mass is None:
        return InverseDynamicsLayer.apply(world, state, None, 0)
    _set_mass(world, mass, "coriolis_and_gravity")
    out = InverseDynamicsLayer.apply(world, state, None, 0)
    return _MassTap.apply(out, mass, lambda g: inverse_dynamics_mass_gradient(world, state, None, g).reshape(-1, mass.shape[0]).sum(0), world)


def mass_matrix(world, state: torch.Tensor, mass=None) -> torch.Tensor:
    """M(q) of `state` ([..., 2n] -> [..., n, n]; only the positions are read), exactly symmetric; differentiable in the positions.
    mass: as in inverse_dynamics; its gradient is one launch of the inertia kernel over n x B worlds (world (j, b): a = e_j, cotangent
    G[b, :, j], no velocity, no gravity), the way the position gradient is obtained."""
    if mass is None:
        return MassMatrixLayer.apply(world, state)
    _set_mass(world, mass, "mass_matrix")
    out = MassMatrixLayer.apply(world, state)

    def pull(G):
        s_soa, _, _ = _dyn_inputs(world, "mass_matrix", state)
        n, B = world.n, s_soa.shape[1]
        Gt = G.to(device=world.device, dtype=torch.float64).reshape(B, n, n).permute(2, 1, 0)              # [j, i, b]: the cotangent of column j
        eye = torch.eye(n, dtype=torch.float64, device=world.device)[:, :, None].expand(n, n, B)            # [j, i, b]: a = e_j
        return _columns_mass_grad(world, s_soa, eye, Gt).sum(1)
    return _MassTap.apply(out, mass, pull, world)


def forward_dynamics(world, state: torch.Tensor, tau: torch.Tensor, joint_forces: bool = False, wrenches=None, bodies=None,
                     world_frame: bool = False, mass=None) -> torch.Tensor:
    """a = M(q)^-1 (tau - C(q, v)) of `state` = [q; v] ([..., 2n]) and `tau` ([..., n]; None: 0) -> [..., n], by the articulated-body
    algorithm; differentiable in both (exactly).  joint_forces: the right-hand side also carries - damping v - spring (q - rest + dt v) as
    the step has it, so that a = (v' - v) / dt of a contact-free timestep() and forward_dynamics inverts inverse_dynamics under the same
    switch.  With a `state` in the reference's layout (immobile skeletons) the result is in that layout too: zero acceleration and zero
    gradient for the frozen coordinates.
    wrenches / bodies / world_frame as in inverse_dynamics: a = M^-1 (tau + sum_e J_e^T W_e - C), its inverse function under equal
    switches and wrenches; differentiable in the wrenches too.  Without `wrenches` the call is what it was.
    mass: as in inverse_dynamics (nbl_forward_dynamics_backward_inertia: d a / d mass = -M^-1 d ID / d mass at (q, v, a))."""
    if mass is not None:
        _set_mass(world, mass, "forward_dynamics")
    if wrenches is None:
        if bodies is not None or world_frame:
            raise ValueError("forward_dynamics: `bodies` / `world_frame` describe `wrenches`, which were not given")
        mapping = None
        out = ForwardDynamicsLayer.apply(world, state, tau, ID_JOINT_FORCES if joint_forces else 0)
    else:
        mapping = wrench_set(world, bodies)
        out = _WrenchLayer.apply(world, state, tau, wrenches, mapping, _wrench_flags(joint_forces, world_frame), True)
    if mass is None:
        return out
    return _MassTap.apply(out, mass, lambda g: forward_dynamics_mass_gradient(world, state, tau, g, joint_forces, None if wrenches is None else wrenches.detach(),
                                                                              mapping, world_frame).reshape(-1, mass.shape[0]).sum(0), world)


def contact_inverse_dynamics(world, state: torch.Tensor, accel: torch.Tensor, bodies, wrench_guesses=None, min_torque: bool = False):
    """Skeleton::getContactInverseDynamics / getMultipleContactInverseDynamics (Skeleton.cpp:9705-9949) for batches: the wrenches on the
    contact `bodies` (local coordinates, [..., E, 6]) under which `accel` needs no torque on the six coordinates of the free root joint,
    and the joint torques ([..., n], root rows 0) that go with them - with the damping and spring forces, like the reference.
    One body and no guesses: getContactInverseDynamics.  Several bodies: with `wrench_guesses` ([..., E, 6] or [..., 6 E]) the solution
    nearest to them; with none (or an empty list, or min_torque) the reference's min-torque solution.  Every body must hang below one
    free root joint.  No autograd (the reference has none); a world whose 6 x 6 system is singular gets NaN."""
    _join_if_deferred(world)
    n = world.n
    mapping = wrench_set(world, bodies)
    E = len(mapping._entries)
    if E < 1:
        raise ValueError("contact_inverse_dynamics: no contact body")
    s, _, _ = _restrict(world, state.detach(), "contact_inverse_dynamics", "state")
    lead = tuple(s.shape[:-1])
    a, _, _ = _restrict(world, accel.detach(), "contact_inverse_dynamics", "accel")
    if tuple(a.shape[:-1]) != lead:
        raise ValueError(f"contact_inverse_dynamics: accel has leading shape {tuple(a.shape[:-1])}, state {lead}")
    s_soa = world.to_soa(world._prep(s.reshape(-1, 2 * n), 2 * n, "dyn_state"))
    a_soa = world.to_soa(world._prep(a.reshape(-1, n), n, "dyn_accel"))
    g_soa = None
    have = wrench_guesses is not None and not (isinstance(wrench_guesses, (list, tuple)) and len(wrench_guesses) == 0)
    if have and not min_torque:
        g = wrench_guesses if torch.is_tensor(wrench_guesses) else torch.stack([torch.as_tensor(x, dtype=torch.float64) for x in wrench_guesses], -2)
        g = g.detach().reshape(tuple(g.shape[:-2]) + (6 * E,)) if g.shape[-1] == 6 and g.dim() == len(lead) + 2 else g.detach()
        if tuple(g.shape) != lead + (6 * E,):
            raise ValueError(f"contact_inverse_dynamics: wrench_guesses have shape {tuple(g.shape)}; expected {lead + (E, 6)}")
        g_soa = world.to_soa(world._prep(g.reshape(-1, 6 * E), 6 * E, "dyn_wrench"))
        mode = CID_NEAREST
    else:
        mode = CID_SINGLE if (E == 1 and not min_torque) else CID_MIN_TORQUE
    W, tau = contact_inverse_dynamics_soa(world, mapping, s_soa, a_soa, g_soa, mode)
    W = world.from_soa(W).reshape(lead + (E, 6))
    tau = world.from_soa(tau).reshape(lead + (n,))
    if state.device.type == "cpu":
        return world._to_host(W, tau)
    return W.to(state.device), tau.to(state.device)


def _rotvec_matrix(r: torch.Tensor) -> torch.Tensor:
    """exp([r]x) of rotation vectors [..., 3] -> [..., 3, 3] (Rodrigues), differentiable"""
    th2 = (r * r).sum(-1, keepdim=True)
    th = torch.sqrt(th2.clamp_min(1e-30))
    small = th2 < 1e-12
    A = torch.where(small, 1.0 - th2 / 6.0, torch.sin(th) / th)[..., None]
    Bc = torch.where(small, 0.5 - th2 / 24.0, (1.0 - torch.cos(th)) / th2.clamp_min(1e-30))[..., None]
    z = torch.zeros_like(r[..., 0])
    K = torch.stack([torch.stack([z, -r[..., 2], r[..., 1]], -1), torch.stack([r[..., 2], z, -r[..., 0]], -1),
                     torch.stack([-r[..., 1], r[..., 0], z], -1)], -2)
    return torch.eye(3, dtype=r.dtype, device=r.device) + A * K + Bc * (K @ K)


def inverse_dynamics_from_predictions(world, state: torch.Tensor, accel: torch.Tensor, bodies, root_frame_wrenches: torch.Tensor,
                                      root_residuals=None) -> torch.Tensor:
    """Skeleton::getInverseDynamicsFromPredictions (Skeleton.cpp:9671-9697): the joint torques ([..., n]) for `accel` given predicted
    wrenches on the contact `bodies` expressed in the ROOT body's frame ([..., E, 6] or [..., 6 E]) and, optionally, a residual wrench on
    the root body in its own frame ([..., 6]).  The reference's dAdInvT(T_wb^-1, dAdInvT(T_wr, W)) is the wrench in world coordinates
    taken to each body's origin - [R_wr t + (p_wr - p_wb) x R_wr f; R_wr f] - which inverse_dynamics takes as it is (world_frame); the
    residual is one more wrench on the root body, local there.  The root is the body of `bodies[0]`'s tree root.  With the damping and
    spring forces, like the reference; differentiable like inverse_dynamics."""
    from .mapping import map_to_pos
    contact = wrench_set(world, bodies)
    E = len(contact._entries)
    md = world.description
    if E < 1:
        raise ValueError("inverse_dynamics_from_predictions: no contact body")
    r = contact._entries[0][1]
    while md.bodies[r].parent >= 0:
        r = md.bodies[r].parent
    allm = wrench_set(world, [i for _, i, _, _ in contact._entries] + [r])         # the contact bodies, then the root
    W = root_frame_wrenches.reshape(tuple(root_frame_wrenches.shape[:-2]) + (6 * E,)) if root_frame_wrenches.shape[-1] == 6 and \
        root_frame_wrenches.dim() == state.dim() + 1 else root_frame_wrenches
    pos = map_to_pos(world, allm, state).to(W.device)                      # [..., 6 (E + 1)]: logMap(R), p per entry
    Rr = _rotvec_matrix(pos[..., 6 * E:6 * E + 3])
    pr = pos[..., 6 * E + 3:6 * E + 6]
    parts = []
    for e in range(E):
        t = (Rr @ W[..., 6 * e:6 * e + 3, None])[..., 0]
        f = (Rr @ W[..., 6 * e + 3:6 * e + 6, None])[..., 0]
        parts += [t + torch.linalg.cross(pr - pos[..., 6 * e + 3:6 * e + 6], f), f]
    if root_residuals is not None:                                                  # local on the root = world coordinates turned by R_wr
        parts += [(Rr @ root_residuals[..., 0:3, None])[..., 0], (Rr @ root_residuals[..., 3:6, None])[..., 0]]
        return inverse_dynamics(world, state, accel, True, torch.cat(parts, -1), allm, True)
    return inverse_dynamics(world, state, accel, True, torch.cat(parts, -1), contact, True)


def multiply_by_inv_mass_matrix(world, state: torch.Tensor, x: torch.Tensor, mass=None) -> torch.Tensor:
    """M(q)^-1 x of `state` ([..., 2n]; only the positions are read) and x = [..., n] or [..., n, R] (R right-hand sides per world: the
    articulated inertias are built once) -> the shape of x.  M is never formed.  Differentiable in x and in the positions (the velocity
    block receives nothing).  In the reference's layout the frozen coordinates get zeros in the result and in the gradients.
    mass: as in inverse_dynamics; its gradient is -sum_r (d (M y_r) / d mass)^T lambda_r, lambda_r = M^-1 (cotangent of y_r): the inertia
    kernel over R x B worlds."""
    if mass is None:
        return InvMassApplyLayer.apply(world, state, x)
    _set_mass(world, mass, "multiply_by_inv_mass_matrix")
    out = InvMassApplyLayer.apply(world, state, x)
    matrix = x.dim() == state.dim() + 1

    def rhs(t, lead):                                             # [..., n, R] / [..., n] -> [R, n, B]
        tr = t.detach().transpose(-1, -2) if matrix else t.detach().unsqueeze(-2)
        tr, _, _ = _restrict(world, tr, "multiply_by_inv_mass_matrix", "x")
        R = tr.shape[-2]
        return world._prep(tr.reshape(-1, world.n), world.n, "dyn_rhs").reshape(-1, R, world.n).permute(1, 2, 0).contiguous()

    def pull(g):
        s_soa, _, lead = _dyn_inputs(world, "multiply_by_inv_mass_matrix", state)
        Y = inv_mass_apply_soa(world, s_soa, rhs(x, lead))
        Lam = inv_mass_apply_soa(world, s_soa, rhs(g, lead))
        return _columns_mass_grad(world, s_soa, Y, -Lam).sum(1)
    return _MassTap.apply(out, mass, pull, world)


def inv_mass_matrix(world, state: torch.Tensor, mass=None) -> torch.Tensor:
    """M(q)^-1 of `state` ([..., 2n] -> [..., n, n]), exactly symmetric; differentiable in the positions.  In the reference's layout the
    frozen coordinates have zero rows and columns (the reference's own matrix has the inverse of their blocks there, which a model that
    welded them to the world cannot give).  mass: as in multiply_by_inv_mass_matrix, with the columns of M^-1 as right-hand sides."""
    if mass is None:
        return InvMassMatrixLayer.apply(world, state)
    _set_mass(world, mass, "inv_mass_matrix")
    out = InvMassMatrixLayer.apply(world, state)

    def pull(G):
        s_soa, _, _ = _dyn_inputs(world, "inv_mass_matrix", state)
        n, B = world.n, s_soa.shape[1]
        ref = world.ref_layout is not None and G.shape[-1] == world.ref_layout.n_ref and G.shape[-1] != n
        Y = inv_mass_matrix_soa(world, s_soa).reshape(n, n, B)     # [j][i][b] = Minv[i][j]: the matrix is symmetric bit for bit
        Lam = inv_mass_apply_soa(world, s_soa, _square_soa(world, G, ref, B).permute(2, 1, 0).contiguous())    # [j, i, b]
        return _columns_mass_grad(world, s_soa, Y, -Lam).sum(1)
    return _MassTap.apply(out, mass, pull, world)


def _current(world):
    from ._lib import NimbleAmdError
    if getattr(world, "_state", None) is None:
        raise NimbleAmdError("call world.setState() first")
    _join_if_deferred(world)
    return world._state


def world_mass_matrix(world) -> torch.Tensor:
    s = _current(world)
    M = world.from_soa(mass_matrix_soa(world, s)).reshape(s.shape[1], world.n, world.n)
    return M[0] if getattr(world, "_one_d", False) else M


def world_coriolis_and_gravity(world) -> torch.Tensor:
    s = _current(world)
    c = world.from_soa(inverse_dynamics_soa(world, s, None, 0))
    return c[0] if getattr(world, "_one_d", False) else c


def _world_vec(world, x, what):
    """a per-world vector given like the state was ([n] for a 1-D state, else [B, n]; the reference's layout allowed) -> [n][B]"""
    x = torch.as_tensor(x, dtype=torch.float64)
    x, _, _ = _restrict(world, x, what, "accel")
    return world.to_soa(world._prep(x.reshape(-1, world.n), world.n, "dyn_accel"))


def _world_torques(world, tau_soa):
    """[n][B] -> [B, n] ([n] for a 1-D state); in the reference's layout the frozen coordinates get zeros"""
    t = world.from_soa(tau_soa)
    if world.ref_layout is not None:
        t = _expand(world, t, (t.shape[0],), world.ref_layout.n_ref, "accel")
    return t[0] if getattr(world, "_one_d", False) else t


def world_contact_inverse_dynamics(world, accel, bodies, wrench_guesses=None, multiple=False):
    s = _current(world)
    mapping = wrench_set(world, bodies)
    E, B = len(mapping._entries), s.shape[1]
    a_soa = _world_vec(world, accel, "getContactInverseDynamics")
    g_soa, mode = None, CID_SINGLE if not multiple else CID_MIN_TORQUE
    if multiple and wrench_guesses is not None and len(wrench_guesses) > 0:
        g = wrench_guesses if torch.is_tensor(wrench_guesses) else torch.stack([torch.as_tensor(x, dtype=torch.float64) for x in wrench_guesses], -2)
        g_soa = world.to_soa(world._prep(g.reshape(-1, 6 * E), 6 * E, "dyn_wrench"))
        mode = CID_NEAREST
    W, tau = contact_inverse_dynamics_soa(world, mapping, s, a_soa, g_soa, mode)
    W = world.from_soa(W).reshape(B, E, 6)
    return (W[0] if getattr(world, "_one_d", False) else W), _world_torques(world, tau)


def world_inverse_dynamics_from_predictions(world, accel, bodies, root_frame_wrenches, root_residuals=None):
    s = _current(world)
    state = world.from_soa(s)
    one = getattr(world, "_one_d", False)
    a = world.from_soa(_world_vec(world, accel, "getInverseDynamicsFromPredictions"))
    W = torch.as_tensor(root_frame_wrenches, dtype=torch.float64).to(world.device).reshape(state.shape[0], -1)
    res = None if root_residuals is None else torch.as_tensor(root_residuals, dtype=torch.float64).to(world.device).reshape(state.shape[0], 6)
    tau = inverse_dynamics_from_predictions(world, state, a, bodies, W, res)
    if world.ref_layout is not None:
        tau = _expand(world, tau, (tau.shape[0],), world.ref_layout.n_ref, "accel")
    return tau[0] if one else tau


def world_inv_mass_matrix(world) -> torch.Tensor:
    s = _current(world)
    Mi = world.from_soa(inv_mass_matrix_soa(world, s)).reshape(s.shape[1], world.n, world.n)
    return Mi[0] if getattr(world, "_one_d", False) else Mi


# ---- Skeleton::getJacobianOfC / M / ID / Minv / FD on the World's current state (Skeleton.hpp:650-718) ---------------------------------------
def _wrt_kind(world, wrt) -> str:
    from .mass import WithRespectToMass
    from .sensors import WRT_POSITION, WRT_VELOCITY
    if isinstance(wrt, WithRespectToMass):
        if wrt is not world.getWrtMass():
            raise ValueError("the WithRespectToMass of another World")
        _mass_dims(world, "getJacobianOf...")
        return "mass"
    if isinstance(wrt, str) and wrt in (WRT_POSITION, WRT_VELOCITY):
        return wrt
    raise NotImplementedError(f"getJacobianOf...: wrt = {wrt!r} is not offered (world.getWrtMass(), neural.WRT_POSITION, neural.WRT_VELOCITY)")


def _id_dense(world, s_soa: torch.Tensor, a_soa, flags: int, kind: str) -> torch.Tensor:
    """[B, n, dim]: d ID(q, v, a) / d wrt under `flags`, rows by unit cotangents: the reverse kernel (positions, velocities) or the inertia
    kernel (masses) over n x B worlds, cut into launches of whole rows above MASS_BACKWARD_WORLDS"""
    n, B = world.n, s_soa.shape[1]
    if kind == "mass":
        J = _mass_jacobian(world, lambda s, a, g: inverse_dynamics_inertia_vjp_soa(world, s, a, g, flags), s_soa, a_soa, (B,), world.device)
        return J
    from .sensors import WRT_POSITION
    per = max(1, min(n, MASS_BACKWARD_WORLDS // max(B, 1)))
    eye_n = torch.eye(n, dtype=torch.float64, device=world.device)
    J = torch.empty((n, n, B), dtype=torch.float64, device=world.device)                 # [column, row i, b]
    for i0 in range(0, n, per):
        i1 = min(n, i0 + per)
        k = i1 - i0
        gs, _ = inverse_dynamics_vjp_soa(world, s_soa.repeat(1, k), None if a_soa is None else a_soa.repeat(1, k),
                                         eye_n[:, i0:i1].repeat_interleave(B, dim=1).contiguous(), flags, want_accel=False)
        J[:, i0:i1] = (gs[:n] if kind == WRT_POSITION else gs[n:]).reshape(n, k, B)
    return J.permute(2, 1, 0).contiguous()


def _fd_dense(world, s_soa: torch.Tensor, t_soa: torch.Tensor, flags: int, kind: str) -> torch.Tensor:
    """[B, n, dim]: d FD(q, v, tau) / d wrt, rows by unit cotangents through nbl_forward_dynamics_backward[_inertia]"""
    n, B = world.n, s_soa.shape[1]
    if kind == "mass":
        return _mass_jacobian(world, lambda s, t, g: forward_dynamics_inertia_vjp_soa(world, None, s, t, None, g, flags), s_soa, t_soa, (B,), world.device)
    from .sensors import WRT_POSITION
    per = max(1, min(n, MASS_BACKWARD_WORLDS // max(B, 1)))
    eye_n = torch.eye(n, dtype=torch.float64, device=world.device)
    J = torch.empty((n, n, B), dtype=torch.float64, device=world.device)
    for i0 in range(0, n, per):
        i1 = min(n, i0 + per)
        k = i1 - i0
        gs, _ = forward_dynamics_vjp_soa(world, s_soa.repeat(1, k), t_soa.repeat(1, k), eye_n[:, i0:i1].repeat_interleave(B, dim=1).contiguous(), flags,
                                         want_state=True, want_tau=False)
        J[:, i0:i1] = (gs[:n] if kind == WRT_POSITION else gs[n:]).reshape(n, k, B)
    return J.permute(2, 1, 0).contiguous()


def world_jacobian_of(world, what: str, x, wrt) -> torch.Tensor:
    """Skeleton::getJacobianOfC / M / ID / Minv / FD (`what` = "C", "M", "ID", "Minv", "FD") on the current state: [B, n, dim(wrt)] on the
    World's device ([n, dim] for a 1-D state), over the device's (mobile) coordinates, detached."""
    kind = _wrt_kind(world, wrt)
    s = _current(world)
    no_vg = ID_NO_VELOCITY | ID_NO_GRAVITY
    if what == "C":
        J = _id_dense(world, s, None, 0, kind)
    elif what == "M":                                             # d (M x) / d wrt
        J = _id_dense(world, s, _world_vec(world, x, "getJacobianOfM"), no_vg, kind)
    elif what == "ID":                                            # d (M x + C) / d wrt
        J = _id_dense(world, s, _world_vec(world, x, "getJacobianOfID"), 0, kind)
    elif what == "Minv":                                          # d (M^-1 f) / d wrt = -M^-1 d (M y) / d wrt at y = M^-1 f
        f = _world_vec(world, x, "getJacobianOfMinv")
        y = inv_mass_apply_soa(world, s, f.unsqueeze(0))[0]
        JM = _id_dense(world, s, y, no_vg, kind)                   # [B, n, dim]
        J = -inv_mass_apply_soa(world, s, JM.permute(2, 1, 0).contiguous()).permute(2, 1, 0).contiguous()
    else:                                                         # the forward dynamics of the step: the current action's torques, joint forces
        tau = torch.zeros((world.n, s.shape[1]), dtype=torch.float64, device=world.device)
        act = getattr(world, "_action", None)
        if act is not None and act.shape[1] == s.shape[1] and act.shape[0] > 0:
            tau.index_copy_(0, torch.tensor(world.model.action_map, dtype=torch.long, device=world.device), act)
        J = _fd_dense(world, s, tau, ID_JOINT_FORCES, kind)
    return J[0] if getattr(world, "_one_d", False) else J
