"""What a step's contacts were: points, normals, depths, colliders and bodies, LCP impulses and row classes, contact forces, and the
contact wrench on a body - read out of the step's saved record by the kernels of csrc/contact_readout.hip.

Reference API mirrored: `World::getLastCollisionResult()` -> `Contact{point, normal, penetrationDepth, type, collisionObject1/2, force,
lcpResult, lcpResultTangent1/2}` (dart/collision/Contact.hpp:90-147; `force` as ContactConstraint::applyImpulse fills it,
ContactConstraint.cpp:630-684) and BackpropSnapshot's getContactConstraintImpulses / getContactConstraintMappings
(BackpropSnapshot.cpp:1601-1705).  Batched: every quantity carries a leading world dimension, padded to C = the model's max_contacts slots
with `count` saying how many are in use.

All read-outs are DETACHED: no gradient flows through them (the reference has none there either).  They only read the record; the step
and its results are untouched.  A World in deferred-join mode is joined first.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Union

import numpy as np
import torch

from . import _abi
from ._lib import NimbleAmdError, check
from .mapping import _join_if_deferred, resolve_body


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class ContactReadout:
    """The contacts of B worlds (leading shape [B], or [T, B] for a rollout), tensors on the World's device; C = the model's max_contacts:
        count [B] int32                  collider contacts of every world; slots at or above it are zeros in every field
        point, normal, force [B, C, 3]   world coordinates; force = (n l0 + t1 l1 + t2 l2) / dt (Contact::force)
        depth, type [B, C]               penetration depth; the narrow phase's contact type code
        collider_a, collider_b [B, C]    int64, indices into world.description.boxes
        body_a, body_b [B, C]            int64, indices into world.description.bodies (a welded body is reported itself, not the body
                                         it was merged into); -1 = fixed to the world
        impulse [B, C, 3]                LCP impulses: normal, tangent 1, tangent 2 (lcpResult, lcpResultTangent1 / 2)
        row_class [B, C, 3]              0 not clamping, 1 clamping, +2 / -2 a friction row on its upper / lower bound; the two tangent
                                         slots of a frictionless contact: impulse 0, class -1 (`_abi.CO_CLASS_EMPTY`)
        n_limit_rows, n_friction_rows [B] int32: the joint-limit / joint Coulomb friction rows of the same LCP (not contacts)."""

    FIELDS = ("count", "point", "normal", "depth", "type", "collider_a", "collider_b", "body_a", "body_b", "impulse", "row_class", "force",
              "n_limit_rows", "n_friction_rows")

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, kw[k])

    @staticmethod
    def stack(items: Sequence["ContactReadout"]) -> "ContactReadout":
        return ContactReadout(**{k: torch.stack([getattr(it, k) for it in items]) for k in ContactReadout.FIELDS})


def _slots(world) -> int:
    return max(int(world.model.max_contacts), 0)


def _record(world, saved, B: int, what: str):
    if not isinstance(saved, torch.Tensor):
        raise NimbleAmdError(f"{what}: `saved` must be the record tensor of a step (a checkpointed rollout keeps a RolloutRecord: see rollout_contacts)")
    need = world.saved_bytes(B) if B > 0 else 0
    if saved.numel() * saved.element_size() < need:
        raise NimbleAmdError(f"{what}: the record holds {saved.numel() * saved.element_size()} bytes, a step of {B} worlds writes {need}")
    if saved.device != world.device:
        raise NimbleAmdError(f"{what}: the record lives on {saved.device}, the World on {world.device}")
    return saved


def _node_table(world):
    """collider index -> body of world.description that carries it (BoxSpec.node after merge_welds), or None when the model's own body
    indices are the description's"""
    if world.model is world.description:
        return None
    return torch.tensor([(bx.node if bx.node >= 0 else bx.body) for bx in world.model.boxes] or [0], dtype=torch.int64, device=world.device)


def read_contacts(world, saved: torch.Tensor, B: int) -> ContactReadout:
    """The contacts of the step that wrote `saved` (one record of world.saved_bytes(B) bytes: what step_soa / forwardPass / timestep keep)
    for its B worlds -> ContactReadout.  One launch of k_contact_readout, one world per lane; detached."""
    B = int(B)
    _record(world, saved, B, "read_contacts")
    _join_if_deferred(world)
    Cn, dev = _slots(world), world.device
    count = torch.empty(B, dtype=torch.int32, device=dev)
    nlim, nfr = torch.empty_like(count), torch.empty_like(count)
    table = torch.empty((_abi.CO_FIELDS, Cn, B), dtype=torch.float64, device=dev)
    if B > 0:
        with torch.cuda.device(dev):
            check(world._L.nbl_contact_readout(world._h, B, _ptr(saved), _ptr(count), _ptr(nlim), _ptr(nfr), _ptr(table) if Cn > 0 else None,
                                               world._stream()), "nbl_contact_readout")
    t = table.permute(2, 1, 0)                                  # [B, C, field]
    out = {}
    off = 0
    for name, width in _abi.CO_FIELD_LIST:
        out[name] = t[:, :, off:off + width].contiguous() if width > 1 else t[:, :, off].contiguous()
        off += width
    for k in ("collider_a", "collider_b", "body_a", "body_b"):
        out[k] = out[k].to(torch.int64)
    nodes = _node_table(world)
    if nodes is not None:                                        # welded bodies: the collider's own BodyNode, not the body it merged into
        used = torch.arange(Cn, device=dev)[None, :] < count[:, None]
        for side in ("a", "b"):
            out["body_" + side] = torch.where(used, nodes[out["collider_" + side].clamp(0, nodes.shape[0] - 1)], torch.zeros_like(out["body_" + side]))
    return ContactReadout(count=count, n_limit_rows=nlim, n_friction_rows=nfr, **out)


def _model_bodies(world, bodies) -> List[int]:
    if isinstance(bodies, (str, int, np.integer)):
        bodies = [bodies]
    out = []
    for b in bodies:
        mb, T = resolve_body(world.description, b)
        if mb < 0:
            raise NimbleAmdError(f"body_contact_wrenches: {b!r} is welded to the world: it has no body of the device model to read a wrench for")
        if not np.allclose(T, np.eye(4), atol=0.0):
            raise NimbleAmdError(f"body_contact_wrenches: {b!r} is welded into another body and shares its contacts: name the body that carries it")
        out.append(int(mb))
    if len(out) > _abi.CO_MAX_BODIES:
        raise ValueError(f"body_contact_wrenches: at most {_abi.CO_MAX_BODIES} bodies; got {len(out)}")
    return out


def body_contact_wrenches(world, saved: torch.Tensor, B: int, bodies: Sequence[Union[str, int]]) -> torch.Tensor:
    """The contact wrench on each of `bodies` (names or indices into world.description.bodies, resolved by mapping.resolve_body) in the step
    that wrote `saved` -> [B, E, 6]: [torque(3); force(3)] in world coordinates, acting at the origin of the body's frame: the sum over the
    world's contacts of + force on the body of collider A and - force on the body of collider B with their moments about that origin.  The
    result plugs into forward_dynamics / inverse_dynamics(wrenches=W.reshape(B, 6 E), bodies=bodies, world_frame=True) unchanged.
    Joint-limit and joint-friction rows are generalized forces and contribute nothing.  A body named twice raises.  Detached."""
    B = int(B)
    _record(world, saved, B, "body_contact_wrenches")
    idx = _model_bodies(world, bodies)
    _join_if_deferred(world)
    E = len(idx)
    W = torch.empty((6 * E, B), dtype=torch.float64, device=world.device)
    arr = np.asarray(idx, dtype=np.int32)
    with torch.cuda.device(world.device):
        check(world._L.nbl_contact_body_wrenches(world._h, B, _ptr(saved) if B > 0 else None, E, arr.ctypes.data_as(C.c_void_p) if E else None,
                                                 _ptr(W) if E and B else None, world._stream()), "nbl_contact_body_wrenches")
    return W.reshape(E, 6, B).permute(2, 0, 1).contiguous()


def read_constraint_rows(world, saved: torch.Tensor, B: int):
    """The live LCP rows of the step in the reference's order (constraint by constraint: three rows for a contact with friction, one for a
    frictionless contact, a joint-limit row and a joint-friction row) -> (n_rows [B] int32, impulse [B, 3 C], mapping [B, 3 C] int32),
    PADDED: rows at or above n_rows[b] read impulse 0 and mapping `_abi.CO_MAP_NONE`.  mapping: -1 clamping, -2 not clamping, >= 0 a
    friction row on its bound (the row index of its contact's normal), as neural::ConstraintMapping.  Detached."""
    B = int(B)
    _record(world, saved, B, "read_constraint_rows")
    _join_if_deferred(world)
    R, dev = 3 * _slots(world), world.device
    n_rows = torch.empty(B, dtype=torch.int32, device=dev)
    imp = torch.empty((R, B), dtype=torch.float64, device=dev)
    mp = torch.empty((R, B), dtype=torch.int32, device=dev)
    if B > 0:
        with torch.cuda.device(dev):
            check(world._L.nbl_contact_readout_rows(world._h, B, _ptr(saved), _ptr(n_rows), _ptr(imp) if R else None, _ptr(mp) if R else None,
                                                    world._stream()), "nbl_contact_readout_rows")
    return n_rows, imp.t().contiguous(), mp.t().contiguous()


def _rollout_records(world, what: str):
    """(record tensor, T, B, stride in bytes) of world.rollout_record, or the documented error when only part of it is resident"""
    rec = getattr(world, "rollout_record", None)
    status = getattr(world, "rollout_status", None)
    if rec is None or status is None:
        raise NimbleAmdError(f"{what}: no rollout() with a saved record has been taken on this World")
    if not isinstance(rec, torch.Tensor):
        raise NimbleAmdError(f"{what}: the rollout ran with checkpoint_every = {rec.segment}: only the records of its last segment are resident, "
                             "not those of every step - run rollout() with checkpoint_every = 0 to read its contacts")
    T, B = int(status.shape[0]), int(status.shape[1])
    return rec, T, B, world.saved_bytes(B)


def rollout_contacts(world) -> ContactReadout:
    """The contacts of every step of the last rollout() on `world` (world.rollout_record) -> ContactReadout with leading shape [T, B]: one
    read-out per step at the record stride (the rows of a record are interleaved over its own B worlds).  A rollout with
    checkpoint_every > 0 keeps only its last segment's records: NimbleAmdError, no partial data."""
    rec, T, B, stride = _rollout_records(world, "rollout_contacts")
    return ContactReadout.stack([read_contacts(world, rec[t * stride:(t + 1) * stride], B) for t in range(T)])


def rollout_body_contact_wrenches(world, bodies) -> torch.Tensor:
    """body_contact_wrenches for every step of the last rollout() -> [T, B, E, 6]; see rollout_contacts."""
    rec, T, B, stride = _rollout_records(world, "rollout_body_contact_wrenches")
    return torch.stack([body_contact_wrenches(world, rec[t * stride:(t + 1) * stride], B, bodies) for t in range(T)])
