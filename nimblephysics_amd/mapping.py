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
What stays out: COM entries (no public constructor in the reference), the IK setters (setPositions runs an IK solve), IdentityMapping,
MappedBackpropSnapshot and world.addMapping.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import List, Tuple, Union

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


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


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
