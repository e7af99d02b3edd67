"""World-space body kinematics: `neural.IKMapping`, `map_to_pos`, `map_to_vel` (python/nimblephysics/mapping.py:8-101,
dart/neural/IKMapping.{hpp,cpp}).

An `IKMapping` is a list of body entries; the mapped vector is their rows in the order they were added (IKMapping.cpp:146-232):
    addSpatialBodyNode   6 rows   positions: logMap(R), then p      velocities: [w; v], world coordinates (getSpatialVelocity(World, World))
    addLinearBodyNode    3 rows   positions: p                      velocities: v, the velocity of the body's origin
    addAngularBodyNode   3 rows   positions: logMap(R)              velocities: w
`map_to_pos(world, mapping, state)` / `map_to_vel(world, mapping, state)` compute them for B (or T+1 x B) worlds in one launch of
csrc/kinematics.hip, with their vector-Jacobian products as the backward pass.

Differences from the reference, all forced by batching or by this library's model:
  * a body is named by its name (as the loaders record it) or by its index in `world.description.bodies`, not by a BodyNode;
  * `state` is `[..., 2n]` (`[2n]` gives `[P]`, exactly the reference; `[B, 2n]` gives `[B, P]`; `[B, T+1, 2n]` - what `rollout()`
    returns - gives `[B, T+1, P]`); CPU float64 tensors come back as CPU tensors, device tensors stay on the device;
  * neither function changes the World's state (the reference's layers call world.setState).
The setters (IKMapping.cpp:86-135): `setPositions` runs the batched inverse-kinematics solve of csrc/ik.hip (`solve_ik`: the reference's
math::solveIK with one restart, one world per lane; no autograd, as in the reference, unless `differentiable=True` asks for the gradient
to the targets of csrc/ik_grad.hip), `setVelocities` applies the pseudo-inverse of the velocity Jacobian, `setControlForces` its
transpose.
What stays out: COM entries (no public constructor in the reference), IdentityMapping, MappedBackpropSnapshot and world.addMapping.
"""
from __future__ import annotations

import ctypes as C
import re
from dataclasses import dataclass
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from ._lib import NimbleAmdError, check, lib
from .model import ModelDescription

KIN_SPATIAL, KIN_LINEAR, KIN_ANGULAR = 0, 1, 2          # NBL_KIN_* of include/nimble_amd.h
KIN_ROWS = {KIN_SPATIAL: 6, KIN_LINEAR: 3, KIN_ANGULAR: 3}
MAX_ENTRIES = 64                                         # the library's cap (P <= 384 rows)
_VIRTUAL = re.compile(r"#v\d+$")                         # massless links of an expanded compound joint (model.expand_compound_joints)


def resolve_body(md: ModelDescription, body: Union[str, int]) -> Tuple[int, np.ndarray]:
    """Where the reference BodyNode `body` (its name, or its index in md.bodies) lives on the device model: (index of the body of
    md.merge_welds() that carries it - the index of the library's model description -, or -1 for a body welded to the world; the
    body's frame in that body, 4 x 4).  Raises on an unknown or ambiguous name, on the massless links of a compound joint (not
    BodyNodes of the reference) and on the bodies of immobile skeletons (the reference's Jacobian has columns for their frozen
    coordinates; this model welded them)."""
    bodies = md.bodies
    if isinstance(body, str):
        hits = [i for i, b in enumerate(bodies) if b.name == body]
        if not hits:
            raise ValueError(f"IKMapping: no body named {body!r} in model {md.name!r}")
        if len(hits) > 1:
            raise ValueError(f"IKMapping: {len(hits)} bodies are named {body!r} (indices {hits}): pass the index of the one you mean")
        i = hits[0]
    elif isinstance(body, (int, np.integer)) and not isinstance(body, bool):
        i = int(body)
        if not 0 <= i < len(bodies):
            raise ValueError(f"IKMapping: body index {i} out of range [0, {len(bodies)})")
    else:
        raise TypeError(f"IKMapping: a body is named by its name or its index in world.description.bodies, not {type(body).__name__}")
    if _VIRTUAL.search(bodies[i].name):
        raise ValueError(f"IKMapping: {bodies[i].name!r} is a massless link of an expanded compound joint, not a BodyNode of the reference")
    immobile = set(getattr(md, "immobile_skeletons", None) or ())
    if immobile and bodies[i].skeleton in immobile:
        raise ValueError(f"IKMapping: {bodies[i].name!r} belongs to an immobile skeleton: the reference's Jacobian has columns for its frozen "
                         "coordinates, which this model welded")
    targets, T_in = md.weld_targets()
    return int(targets[i]), np.array(T_in[i], dtype=np.float64)


class IKMapping:
    """nimble.neural.IKMapping (dart/neural/IKMapping.hpp): body entries whose world poses / velocities form the mapped vector."""

    def __init__(self, world):
        self._world = world
        self._entries: List[Tuple[int, int, int, np.ndarray]] = []   # (kind, index in description.bodies, model body, frame in it)
        self._km = None                                              # (World, handle object, nbl_kin_map*) the device map was made for

    # ---- entries (IKMapping.cpp:43-58) ----
    def _add(self, kind: int, node):
        if len(self._entries) >= MAX_ENTRIES:
            raise ValueError(f"IKMapping: at most {MAX_ENTRIES} entries ({6 * MAX_ENTRIES} rows)")
        md = self._world.description
        mb, T = resolve_body(md, node)
        i = node if not isinstance(node, str) else [k for k, b in enumerate(md.bodies) if b.name == node][0]
        self._entries.append((kind, int(i), mb, T))
        self._release()

    def addSpatialBodyNode(self, node):
        self._add(KIN_SPATIAL, node)

    def addLinearBodyNode(self, node):
        self._add(KIN_LINEAR, node)

    def addAngularBodyNode(self, node):
        self._add(KIN_ANGULAR, node)

    def getPosDim(self) -> int:
        return sum(KIN_ROWS[k] for k, _, _, _ in self._entries)

    def getVelDim(self) -> int:
        return self.getPosDim()

    # ---- the device map: made on first use, made again when the World's handle changes (World._create_handle) ----
    def _release(self):
        if self._km is not None:
            lib().nbl_kin_map_destroy(self._km[2])
            self._km = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def _device_map(self, world):
        h = world._h
        if self._km is not None and self._km[0] is world and self._km[1] is h:
            return self._km[2]
        self._release()
        L = lib()
        cnt = len(self._entries)
        kind = np.array([k for k, _, _, _ in self._entries], dtype=np.int32)
        body = np.array([mb for _, _, mb, _ in self._entries], dtype=np.int32)
        T = np.ascontiguousarray(np.stack([np.concatenate([t[:3, :3].reshape(9), t[:3, 3]]) for _, _, _, t in self._entries]), dtype=np.float64)
        if world is not self._world:                 # another World (a clone): the same bodies, resolved against its own description
            md = world.description
            targets, T_in = md.weld_targets()
            body = np.array([targets[i] for _, i, _, _ in self._entries], dtype=np.int32)
            T = np.ascontiguousarray(np.stack([np.concatenate([T_in[i][:3, :3].reshape(9), T_in[i][:3, 3]]) for _, i, _, _ in self._entries]))
        km = C.c_void_p()
        check(L.nbl_kin_map_create(h, cnt, kind.ctypes.data_as(C.c_void_p), body.ctypes.data_as(C.c_void_p),
                                   T.ctypes.data_as(C.c_void_p), C.byref(km)), "nbl_kin_map_create")
        self._km = (world, h, km)
        return km

    # ---- batched evaluation on [2n][B] device states ----
    def _forward_soa(self, world, s_soa: torch.Tensor, want_pos: bool, want_vel: bool):
        P, B = self.getPosDim(), s_soa.shape[1]
        pos = torch.empty((P, B), dtype=torch.float64, device=world.device) if want_pos else None
        vel = torch.empty((P, B), dtype=torch.float64, device=world.device) if want_vel else None
        if P > 0 and B > 0:
            _join_if_deferred(world)
            km = self._device_map(world)
            check(world._L.nbl_kinematics_forward(world._h, km, B, _ptr(s_soa), _ptr(pos), _ptr(vel), world._stream()), "nbl_kinematics_forward")
        return pos, vel

    def _backward_soa(self, world, s_soa: torch.Tensor, g_pos, g_vel) -> torch.Tensor:
        B = s_soa.shape[1]
        gs = torch.zeros((2 * world.n, B), dtype=torch.float64, device=world.device) if self.getPosDim() == 0 else \
            torch.empty((2 * world.n, B), dtype=torch.float64, device=world.device)
        if self.getPosDim() > 0 and B > 0:
            _join_if_deferred(world)
            km = self._device_map(world)
            check(world._L.nbl_kinematics_backward(world._h, km, B, _ptr(s_soa), _ptr(g_pos), _ptr(g_vel), _ptr(gs), 0, world._stream()),
                  "nbl_kinematics_backward")
        return gs

    def _current(self, world) -> torch.Tensor:
        if getattr(world, "_state", None) is None:
            raise NimbleAmdError("IKMapping: call world.setState() first")
        return world._state

    def _out(self, world, t: torch.Tensor) -> torch.Tensor:
        return t[0] if getattr(world, "_one_d", False) else t

    # ---- the reference's getters on the World's current state ----
    def getPositions(self, world) -> torch.Tensor:
        """IKMapping::getPositions: [B, P] on the World's device ([P] when the state was set as one 1-D vector)."""
        pos, _ = self._forward_soa(world, self._current(world), True, False)
        return self._out(world, pos.t().contiguous())

    def getVelocities(self, world) -> torch.Tensor:
        """IKMapping::getVelocities: [B, P]; see getPositions."""
        _, vel = self._forward_soa(world, self._current(world), False, True)
        return self._out(world, vel.t().contiguous())

    def _dense(self, world, block: int) -> torch.Tensor:
        """[B, P, n]: row p is the vector-Jacobian product with the unit cotangent e_p (one launch over P x B worlds)."""
        s = self._current(world)
        P, B, n = self.getPosDim(), s.shape[1], world.n
        rep = s.repeat(1, P)                                          # world p * B + b = (row p, world b)
        eye = torch.eye(P, dtype=torch.float64, device=world.device).repeat_interleave(B, dim=1)
        gs = self._backward_soa(world, rep, eye if block == 0 else None, eye if block == 1 else None)
        J = gs[block * n:(block + 1) * n].reshape(n, P, B).permute(2, 1, 0).contiguous()
        lay = world.ref_layout
        if lay is not None:                                           # columns of the frozen coordinates: zero
            full = torch.zeros((B, P, lay.n_ref), dtype=torch.float64, device=world.device)
            J = full.index_copy(2, lay._idx(world.device, "mobile"), J)
        return self._out(world, J)

    def getRealPosToMappedPosJac(self, world) -> torch.Tensor:
        """IKMapping::getRealPosToMappedPosJac = getPosJacobian (IKMapping.cpp:371-416): [B, P, n], dense."""
        return self._dense(world, 0)

    def getRealVelToMappedVelJac(self, world) -> torch.Tensor:
        """IKMapping::getRealVelToMappedVelJac = getVelJacobian (IKMapping.cpp:429-473): [B, P, n], dense."""
        return self._dense(world, 1)

    # ---- second order, on the World's current state (taskspace.py; one pass of csrc/taskspace.hip, detached) ----
    def getJacobian(self, world) -> torch.Tensor:
        """[B, P, n]: the velocity Jacobian, getVelocities = J v.  Agrees with getRealVelToMappedVelJac, without its P reverse-mode worlds."""
        from .taskspace import current_jacobian
        return current_jacobian(world, self, False)

    def getJacobianDeriv(self, world) -> torch.Tensor:
        """[B, P, n]: d/dt of getJacobian along the motion of the World's state."""
        from .taskspace import current_jacobian
        return current_jacobian(world, self, True)

    def getAccelerations(self, world, accelerations: torch.Tensor) -> torch.Tensor:
        """[B, P]: the time derivative of getVelocities at the joint accelerations [B, n] ([n] for a state set as one 1-D vector):
        J accelerations + Jdot v, no gravity."""
        from .taskspace import current_accelerations
        return current_accelerations(world, self, accelerations)

    # ---- the reference's setters on the World's current state (IKMapping.cpp:86-135) ----
    def setPositions(self, world, positions: torch.Tensor):
        """IKMapping::setPositions: solve for joint positions whose mapped positions are `positions` ([B, P], or [P] for a state set as
        one 1-D vector) - from ZERO with 500 steps, like the reference - and write them into the position block of the World's state.
        The velocities are kept; the coordinates of immobile skeletons stay zero."""
        s = self._current(world)
        q_soa, _, _ = _solve_ik_soa(world, self, _targets_soa(world, self, positions, s.shape[1], "IKMapping.setPositions"), None, None)
        s[:world.n].copy_(q_soa)      # in place: world._state is the World's own tensor (to_soa allocates it fresh in setState / step)

    def _dense_device(self, world, block: int) -> torch.Tensor:
        """_dense over the device's coordinates, always [B, P, n]"""
        J = self._dense(world, block)
        if getattr(world, "_one_d", False):
            J = J.unsqueeze(0)
        lay = world.ref_layout
        return J if lay is None else J.index_select(2, lay._idx(world.device, "mobile"))

    def setVelocities(self, world, velocities: torch.Tensor):
        """IKMapping::setVelocities: v = pinv(Jvel) velocities (getVelJacobianInverse, IKMapping.cpp:122-127) into the velocity block of
        the World's state; the positions are kept."""
        s = self._current(world)
        w_soa = _targets_soa(world, self, velocities, s.shape[1], "IKMapping.setVelocities")          # [P][B]
        v = torch.linalg.pinv(self._dense_device(world, 1)) @ w_soa.t().unsqueeze(-1)               # [B, n, 1]
        s[world.n:].copy_(v.squeeze(-1).t())

    def setControlForces(self, world, forces: torch.Tensor):
        """IKMapping::setControlForces: tau = Jvel^T forces (IKMapping.cpp:130-135) through the kinematics VJP, restricted to the World's
        action space (World.setAction's vector)."""
        s = self._current(world)
        f_soa = _targets_soa(world, self, forces, s.shape[1], "IKMapping.setControlForces")
        gs = self._backward_soa(world, s, None, f_soa)
        cols = torch.tensor(list(world.model.action_map), dtype=torch.long, device=world.device)
        world._action = gs[world.n:].index_select(0, cols).contiguous()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- batched inverse kinematics (csrc/ik.hip) ------------------------------------------------------------------------------------------
@dataclass
class IKConfig:
    """math::IKConfig (dart/math/IKSolver.hpp:15-42) without the restart and logging fields: one restart, as IKMapping::setPositions runs
    it.  The defaults are the reference's; setPositions itself uses max_step_count = 500."""
    convergence_threshold: float = 1e-7
    max_step_count: int = 100
    least_squares_damping: float = 0.01
    start_clamped: bool = False
    line_search: bool = True
    dont_exit_transpose: bool = False

    def setConvergenceThreshold(self, v):
        self.convergence_threshold = float(v); return self

    def setMaxStepCount(self, v):
        self.max_step_count = int(v); return self

    def setLeastSquaresDamping(self, v):
        self.least_squares_damping = float(v); return self

    def setStartClamped(self, v):
        self.start_clamped = bool(v); return self

    def setLineSearch(self, v):
        self.line_search = bool(v); return self

    def setDontExitTranspose(self, v):
        self.dont_exit_transpose = bool(v); return self


class _CIKConfig(C.Structure):       # nbl_ik_config
    _fields_ = [("convergence_threshold", C.c_double), ("max_step_count", C.c_int32), ("least_squares_damping", C.c_double),
                ("start_clamped", C.c_int32), ("line_search", C.c_int32), ("dont_exit_transpose", C.c_int32)]


# The solver's scratch is 3 n + P + min(P, n) + P n + min(P, n)^2 doubles per world (IkLayout, csrc/ik_dev.hpp: 7.9 kB on Atlas-20 with four spatial entries, 230 kB at the
# caps P = 384, n = 64): a batch whose scratch would pass this many bytes is cut into launches of whole wavefronts (the results do not
# depend on the cut: a world's solve does not depend on the batch).
IK_WORKSPACE_BYTES = 1 << 30


def _targets_soa(world, mapping: "IKMapping", t: torch.Tensor, B_expected: Optional[int], what: str) -> torch.Tensor:
    P = mapping.getPosDim()
    x = t.detach()
    if x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dim() != 2 or x.shape[1] != P:
        raise ValueError(f"{what}: expected [B, {P}] (or [{P}]) mapped values; got {tuple(t.shape)}")
    if B_expected is not None and x.shape[0] != B_expected:
        raise ValueError(f"{what}: {x.shape[0]} worlds given, the World's state holds {B_expected}")
    if P == 0:
        return torch.zeros((0, x.shape[0]), dtype=torch.float64, device=world.device)
    return world.to_soa(world._prep(x, P, "ik_target"))


def _solve_ik_soa(world, mapping: "IKMapping", t_soa: torch.Tensor, init_soa, config: Optional[IKConfig]):
    """target [P][B], init [n][B] or None -> (q [n][B], loss [B], steps [B] int32) on the World's device"""
    _join_if_deferred(world)
    P, B, n = mapping.getPosDim(), t_soa.shape[1], world.n
    q = torch.empty((n, B), dtype=torch.float64, device=world.device)
    loss = torch.empty((B,), dtype=torch.float64, device=world.device)
    steps = torch.empty((B,), dtype=torch.int32, device=world.device)
    if P == 0:
        raise ValueError("solve_ik: the mapping has no entries")
    cfg = None
    if config is not None:
        cfg = _CIKConfig(config.convergence_threshold, config.max_step_count, config.least_squares_damping, int(config.start_clamped),
                         int(config.line_search), int(config.dont_exit_transpose))
    if B == 0:
        return q, loss, steps
    km = mapping._device_map(world)
    L = world._L
    per = L.nbl_ik_workspace_bytes(world._h, km, 1)
    chunk = max(64, (IK_WORKSPACE_BYTES // max(per, 1)) // 64 * 64)
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        whole = b0 == 0 and b1 == B
        tc = t_soa if whole else t_soa[:, b0:b1].contiguous()
        ic = init_soa if (whole or init_soa is None) else init_soa[:, b0:b1].contiguous()
        qc = q if whole else torch.empty((n, b1 - b0), dtype=torch.float64, device=world.device)
        need = L.nbl_ik_workspace_bytes(world._h, km, b1 - b0)
        ws = getattr(world, "_ik_ws", None)
        if ws is None or ws.numel() < need or ws.device != world.device:
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=world.device)
            world._ik_ws = ws
        check(L.nbl_ik_solve(world._h, km, b1 - b0, _ptr(tc), _ptr(ic), C.byref(cfg) if cfg is not None else None, _ptr(qc),
                             _ptr(loss[b0:b1]), _ptr(steps[b0:b1]), _ptr(ws), ws.numel(), world._stream()), "nbl_ik_solve")
        if not whole:
            q[:, b0:b1] = qc
    return q, loss, steps


def _check_grad_damping(grad_damping, what: str) -> float:
    mu = float(grad_damping)
    if not mu >= 0.0:
        raise ValueError(f"{what}: grad_damping must not be negative (got {grad_damping})")
    if mu == 0.0:                                      # NBL_E_UNSUPPORTED of nbl_ik_solve_vjp, said before anything is solved
        raise NimbleAmdError(f"{what}: grad_damping = 0 (a pseudo-inverse of a possibly singular Jacobian) is outside the device path")
    return mu


def _solve_ik_vjp_soa(world, mapping: "IKMapping", q_soa: torch.Tensor, g_soa: torch.Tensor, grad_damping: float):
    """q, grad_q [n][B] -> (grad_target [P][B], free_count [B] int32) on the World's device; cut into launches like _solve_ik_soa (a
    world's result does not depend on the cut)"""
    _join_if_deferred(world)
    P, B, n = mapping.getPosDim(), q_soa.shape[1], world.n
    if P == 0:
        raise ValueError("solve_ik_vjp: the mapping has no entries")
    gt = torch.empty((P, B), dtype=torch.float64, device=world.device)
    free = torch.empty((B,), dtype=torch.int32, device=world.device)
    if B == 0:
        return gt, free
    km = mapping._device_map(world)
    L = world._L
    per = L.nbl_ik_grad_workspace_bytes(world._h, km, 1)
    chunk = max(64, (IK_WORKSPACE_BYTES // max(per, 1)) // 64 * 64)
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        whole = b0 == 0 and b1 == B
        qc = q_soa if whole else q_soa[:, b0:b1].contiguous()
        gc = g_soa if whole else g_soa[:, b0:b1].contiguous()
        oc = gt if whole else torch.empty((P, b1 - b0), dtype=torch.float64, device=world.device)
        need = L.nbl_ik_grad_workspace_bytes(world._h, km, b1 - b0)
        ws = getattr(world, "_ik_ws", None)
        if ws is None or ws.numel() < need or ws.device != world.device:
            ws = torch.empty(max(need, 1), dtype=torch.uint8, device=world.device)
            world._ik_ws = ws
        check(L.nbl_ik_solve_vjp(world._h, km, b1 - b0, _ptr(qc), _ptr(gc), grad_damping, _ptr(oc), 0, _ptr(free[b0:b1]), _ptr(ws),
                                 ws.numel(), world._stream()), "nbl_ik_solve_vjp")
        if not whole:
            gt[:, b0:b1] = oc
    return gt, free


def _coords_soa(world, x: torch.Tensor, B: Optional[int], what: str, name: str) -> torch.Tensor:
    """[B, n] / [n] joint coordinates (or the reference's layout on a World with immobile skeletons) -> [n][B] on the World's device"""
    given = tuple(x.shape)
    x = x.detach()
    if x.dim() == 1:
        x = x.unsqueeze(0)
    lay = world.ref_layout
    if lay is not None and x.shape[-1] == lay.n_ref:
        x = x.index_select(-1, lay._idx(x.device, "mobile"))
    if x.dim() != 2 or x.shape[1] != world.n or (B is not None and x.shape[0] != B):
        raise ValueError(f"{what}: {name} has shape {given}; expected [{'B' if B is None else B}, {world.n}]")
    return world.to_soa(world._prep(x, world.n, "ik_" + name))


def _solve_ik_detached(world, map: "IKMapping", targets: torch.Tensor, init, config):
    """solve_ik without autograd -> (q, loss, steps as solve_ik returns them, q [n][B] on the World's device)"""
    _join_if_deferred(world)
    one = targets.dim() == 1
    t_soa = _targets_soa(world, map, targets, None, "solve_ik")
    B = t_soa.shape[1]
    init_soa = None
    if init is not None:
        x = init.detach()
        if x.dim() == 1:
            x = x.unsqueeze(0)
        lay = world.ref_layout
        if lay is not None and x.shape[-1] == lay.n_ref:
            x = x.index_select(-1, lay._idx(x.device, "mobile"))
        if x.dim() != 2 or x.shape != (B, world.n):
            raise ValueError(f"solve_ik: init has shape {tuple(init.shape)}; expected [{B}, {world.n}]")
        init_soa = world.to_soa(world._prep(x, world.n, "ik_init"))
    q_soa, loss, steps = _solve_ik_soa(world, map, t_soa, init_soa, config if config is not None else IKConfig())
    q = world.from_soa(q_soa)
    if targets.device.type == "cpu":
        q, loss = world._to_host(q, loss)
        steps = steps.cpu()
    else:
        q, loss, steps = q.to(targets.device), loss.to(targets.device), steps.to(targets.device)
    return ((q[0], loss[0], steps[0]) if one else (q, loss, steps)) + (q_soa,)


class SolveIKLayer(torch.autograd.Function):
    """solve_ik(..., differentiable=True): forward = the solve; backward = nbl_ik_solve_vjp at the returned positions (the Gauss-Newton
    sensitivity on the free coordinates, csrc/ik_grad.hip) into `targets`.  `init` gets None; loss and steps carry no gradient."""

    @staticmethod
    def forward(ctx, world, mapping, targets, init, config, grad_damping):
        q, loss, steps, q_soa = _solve_ik_detached(world, mapping, targets, init, config)
        ctx.world, ctx.mapping, ctx.q_soa, ctx.mu = world, mapping, q_soa, grad_damping
        ctx.one, ctx.in_device = targets.dim() == 1, targets.device
        ctx.mark_non_differentiable(loss, steps)
        return q, loss, steps

    @staticmethod
    def backward(ctx, grad_q, _grad_loss, _grad_steps):
        world = ctx.world
        g = grad_q.detach().to(device=world.device, dtype=torch.float64).reshape(-1, world.n)
        gt_soa, _ = _solve_ik_vjp_soa(world, ctx.mapping, ctx.q_soa, world.to_soa(g), ctx.mu)
        gt = world.from_soa(gt_soa)
        gt = world._to_host(gt) if ctx.in_device.type == "cpu" else gt.to(ctx.in_device)
        return None, None, (gt[0] if ctx.one else gt), None, None, None


def solve_ik(world, map: "IKMapping", targets: torch.Tensor, init: Optional[torch.Tensor] = None, config: Optional[IKConfig] = None,
             differentiable: bool = False, grad_damping: float = 1e-9):
    """Batched inverse kinematics: joint positions whose mapped positions (`map_to_pos`) meet `targets`, by the reference's
    math::solveIK with one restart (20 steps of refineIK, then config.max_step_count steps; IKSolver.cpp:195-493), one world per lane of
    csrc/ik.hip.  targets [B, P] or [P]; init [B, n] / [n] (None: zeros, as IKMapping::setPositions starts); config None: IKConfig()
    (the reference's defaults, 100 steps).  Returns (q [B, n], loss [B] = |rows(q) - target|^2 at q, steps [B] int32 = evaluations
    used); [P] gives q [n] and 0-d loss / steps.  CPU tensors come back as CPU tensors.  The World's state is left untouched; a World in
    deferred-join mode is joined first.  On a World with immobile skeletons q is over the mobile coordinates (init may come in either
    layout).

    differentiable=False (the default): no autograd, whatever `targets` requires - the reference has none either.
    differentiable=True: q carries the gradient to `targets` that csrc/ik_grad.hip computes (`solve_ik_vjp`): with J the position
    Jacobian at q and F the coordinates NOT left exactly on a finite limit, grad_targets = J_F (J_F^T J_F + mu I)^-1 (grad_q)_F with
    mu = grad_damping > 0 (a Tikhonov term of the gradient alone, not config.least_squares_damping; 0 raises).  Two limits: the
    second-order term sum_k (rows(q) - target)_k grad^2 rows_k is left out, so this is the derivative of the solve where the target is met
    and its Gauss-Newton approximation elsewhere; and `init` gets no gradient (None).  loss and steps stay detached."""
    if not differentiable:
        return _solve_ik_detached(world, map, targets, init, config)[:3]
    return SolveIKLayer.apply(world, map, targets, init, config, _check_grad_damping(grad_damping, "solve_ik"))


def solve_ik_vjp(world, map: "IKMapping", q: torch.Tensor, grad_q: torch.Tensor, grad_damping: float = 1e-9):
    """The backward pass of solve_ik(differentiable=True) as a function, without autograd: q [B, n] / [n] as solve_ik returned it, grad_q
    alike -> (grad_targets [B, P] / [P], free_count [B] int32 / 0-d: the coordinates of each world not left exactly on a finite limit).
    CPU tensors come back as CPU tensors; a World in deferred-join mode is joined first."""
    mu = _check_grad_damping(grad_damping, "solve_ik_vjp")
    _join_if_deferred(world)
    one = q.dim() == 1
    if grad_q.dim() != q.dim():
        raise ValueError(f"solve_ik_vjp: q has shape {tuple(q.shape)} and grad_q {tuple(grad_q.shape)}")
    q_soa = _coords_soa(world, q, None, "solve_ik_vjp", "q")
    g_soa = _coords_soa(world, grad_q, q_soa.shape[1], "solve_ik_vjp", "grad_q")
    gt_soa, free = _solve_ik_vjp_soa(world, map, q_soa, g_soa, mu)
    gt = world.from_soa(gt_soa)
    if q.device.type == "cpu":
        gt, free = world._to_host(gt), free.cpu()
    else:
        gt, free = gt.to(q.device), free.to(q.device)
    return (gt[0], free[0]) if one else (gt, free)


def _join_if_deferred(world):
    """A World in deferred-join mode (World.set_deferred_join) may still have slices in flight: the current stream waits for them."""
    if getattr(world, "_deferred", False):
        world.join()


class _MapLayer(torch.autograd.Function):
    BLOCK = 0    # 0: positions (MapToPosLayer), 1: velocities (MapToVelLayer)

    @classmethod
    def _run(cls, ctx, world, mapping: IKMapping, state: torch.Tensor):
        _join_if_deferred(world)                                  # before anything reads `state`: it may come out of the slices
        lay = world.ref_layout
        width = state.shape[-1] if state.dim() > 0 else -1
        ctx.ref = lay is not None and width == 2 * lay.n_ref
        x = state.detach()
        if ctx.ref:                                               # the reference's layout (ref_layout.py): drop the frozen coordinates
            x = lay.restrict_state(x, "map_to_pos" if cls.BLOCK == 0 else "map_to_vel", check_frozen=False)
        if x.shape[-1] != 2 * world.n:
            want = f"{2 * world.n}" + (f" (or {2 * lay.n_ref} in the reference's layout)" if lay is not None else "")
            raise ValueError(f"map_to_{'pos' if cls.BLOCK == 0 else 'vel'}: state has {x.shape[-1]} entries per world; expected {want}")
        lead = tuple(x.shape[:-1])
        flat = x.reshape(-1, 2 * world.n)
        s_soa = world.to_soa(world._prep(flat, 2 * world.n, "map_state"))
        pos, vel = mapping._forward_soa(world, s_soa, cls.BLOCK == 0, cls.BLOCK == 1)
        out = world.from_soa(pos if cls.BLOCK == 0 else vel).reshape(lead + (mapping.getPosDim(),))
        ctx.world, ctx.mapping, ctx.s_soa, ctx.lead = world, mapping, s_soa, lead
        ctx.in_device, ctx.in_width = state.device, width
        if state.device.type == "cpu":
            return world._to_host(out)
        return out.to(state.device)

    @classmethod
    def _grad(cls, ctx, grad):
        world, mapping = ctx.world, ctx.mapping
        P = mapping.getPosDim()
        g = grad.detach().to(device=world.device, dtype=torch.float64).reshape(-1, P)
        g_soa = world.to_soa(g) if P > 0 else torch.zeros((0, g.shape[0]), dtype=torch.float64, device=world.device)
        gs = mapping._backward_soa(world, ctx.s_soa, g_soa if cls.BLOCK == 0 else None, g_soa if cls.BLOCK == 1 else None)
        d = world.from_soa(gs).reshape(ctx.lead + (2 * world.n,))
        if ctx.ref:                                               # zero for the frozen coordinates
            lay = world.ref_layout
            d = torch.zeros(ctx.lead + (ctx.in_width,), dtype=torch.float64, device=world.device).index_copy(-1, lay._idx(world.device, "state"), d)
        if ctx.in_device.type == "cpu":
            return None, None, world._to_host(d)
        return None, None, d.to(ctx.in_device)


class MapToPosLayer(_MapLayer):
    """python/nimblephysics/mapping.py:8-44: forward = the mapped positions; backward = Jpos^T g in the position block, zeros in the
    velocity block."""
    BLOCK = 0

    @staticmethod
    def forward(ctx, world, mapping, state):
        return MapToPosLayer._run(ctx, world, mapping, state)

    @staticmethod
    def backward(ctx, grad_pos):
        return MapToPosLayer._grad(ctx, grad_pos)


class MapToVelLayer(_MapLayer):
    """python/nimblephysics/mapping.py:55-92: forward = the mapped velocities; backward = Jvel^T g in the velocity block, zeros in the
    position block."""
    BLOCK = 1

    @staticmethod
    def forward(ctx, world, mapping, state):
        return MapToVelLayer._run(ctx, world, mapping, state)

    @staticmethod
    def backward(ctx, grad_vel):
        return MapToVelLayer._grad(ctx, grad_vel)


def map_to_pos(world, map: IKMapping, state: torch.Tensor) -> torch.Tensor:
    """nimble.map_to_pos (mapping.py:47-52): the mapped positions of `state` ([..., 2n] -> [..., P]), differentiable with respect to
    `state`: the gradient is Jpos^T g in the position block (the exact derivative, logMap's included) and zero in the velocity block.
    The World's state is left as it was.  The angular rows follow logMap's regular branch up to theta = pi - 1e-6 (the reference's
    dLogMap has a special branch there)."""
    return MapToPosLayer.apply(world, map, state)


def map_to_vel(world, map: IKMapping, state: torch.Tensor) -> torch.Tensor:
    """nimble.map_to_vel (mapping.py:94-99): the mapped velocities J(q) v of `state` ([..., 2n] -> [..., P]).  Like the reference's
    MapToVelLayer, the gradient is Jvel^T g in the velocity block and ZERO in the position block: the dependence of J(q) v on the
    positions, d(J v)/dq, is deliberately left out.  The World's state is left as it was."""
    return MapToVelLayer.apply(world, map, state)
