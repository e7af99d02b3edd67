"""Centre of mass, momentum and energy of a set of bodies for batches of states, with exact gradients: the whole-body quantities of the
reference's Skeleton (getMass, getCOM, getCOMLinearVelocity, getCOMLinearAcceleration, getCOMLinearJacobian, computeKineticEnergy,
computePotentialEnergy: dart/dynamics/Skeleton.cpp:11310, 13598-13790; python/_nimblephysics/dynamics/Skeleton.cpp:1873-2035) and the sum
over the set of BodyNode::getAngularMomentum / getLinearMomentum (BodyNode.cpp:2378-2391; the sum is this project's extension).

    c   = center_of_mass(world, state)                       [..., 2n] -> [..., 3]
    cd  = com_velocity(world, state)                         [..., 2n] -> [..., 3]       world coordinates
    cdd = com_acceleration(world, state, accel)              [..., 2n], [..., n] -> [..., 3]   classical, WITHOUT gravity
    h   = centroidal_momentum(world, state)                  [..., 2n] -> [..., 6]       [angular about the COM; linear], world coordinates
    T   = kinetic_energy(world, state)                       [..., 2n] -> [...]
    U   = potential_energy(world, state)                     [..., 2n] -> [...]          gravity at the bodies' centres of mass + joint springs
    J   = com_jacobian(world, state)                         [..., 2n] -> [..., 3, n]    detached; com_velocity = J v
    out = centroidal(world, state, accel=None)               all of the above but J, as a named tuple, from ONE launch (and one backward launch)

Each call is one launch of csrc/centroidal.hip over all the leading dimensions ([2n] one world, [B, 2n] a batch, [T+1, B, 2n] a rollout),
differentiable with respect to `state` (positions AND velocities: the velocity- and acceleration-level outputs carry their full dependence
on q; free and ball coordinates go through expMapJac) and `accel`.  `bodies` (names or indices into world.description.bodies) or
`skeleton` (an id of world.description.body_skeletons()) restrict the set; the default is every body that is not fixed to the world.  A set
must name a weld-merged group of bodies as a whole and no body welded to the world: the device model has merged them.

The kernels read the World's current body inertias (World.setMasses).  Rules shared with dynamics.py: CPU float64 tensors come back as CPU
tensors, device tensors stay on the device; the World's state is untouched; a World in deferred-join mode is joined first; on a world with
immobile skeletons a `state` in the reference's layout is restricted to the mobile coordinates (their bodies are fixed to the world and
belong to no set; the frozen coordinates get zero gradient and zero Jacobian columns).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from ._abi import CEN_NO_SPRINGS, CEN_PE_BODY_ORIGIN      # NBL_CEN_* of include/nimble_amd.h
from ._lib import NimbleAmdError, check
from .dynamics import _expand, _give, _restrict
from .mapping import _join_if_deferred, _ptr, resolve_body

Centroidal = namedtuple("Centroidal", ["com", "com_vel", "com_acc", "momentum", "ke", "pe"])
_ROWS = (3, 3, 3, 6, 1, 1)                                  # rows of the outputs, in the order of Centroidal


def resolve_body_set(md, bodies: Optional[Sequence[Union[str, int]]] = None, skeleton: Optional[int] = None) -> Optional[List[int]]:
    """The bodies of md.merge_welds() - the library's model description - that carry the set, sorted; None: the default set (every body
    of the model).  Raises NimbleAmdError on a body welded to the world and on a set that names part of a weld-merged group."""
    if bodies is not None and skeleton is not None:
        raise ValueError("a body set is chosen by `bodies` or by `skeleton`, not both")
    if bodies is None and skeleton is None:
        return None
    targets, _ = md.weld_targets()
    if skeleton is not None:
        skel = md.body_skeletons()
        named = [i for i, s in enumerate(skel) if s == int(skeleton) and targets[i] >= 0]
        if not named:
            raise NimbleAmdError(f"no body of model {md.name!r} that can move belongs to skeleton {skeleton!r} (ids: {sorted(set(skel))})")
    else:
        if isinstance(bodies, (str, int, np.integer)):
            bodies = [bodies]
        named = []
        for b in bodies:
            try:
                mb, _ = resolve_body(md, b)
            except (ValueError, TypeError) as e:                  # resolve_body speaks for the mapping it was written for
                raise type(e)(str(e).replace("IKMapping:", "body set:", 1)) from None
            i = b if not isinstance(b, str) else [k for k, x in enumerate(md.bodies) if x.name == b][0]
            if mb < 0:
                raise NimbleAmdError(f"body set: {b!r} is welded to the world: it has no body of the device model and moves nothing")
            if int(i) in named:
                raise NimbleAmdError(f"body set: {b!r} is named twice")
            named.append(int(i))
        if not named:
            raise NimbleAmdError("body set: no body named")
    out = sorted({int(targets[i]) for i in named})
    for t in out:
        group = [i for i, x in enumerate(targets) if x == t]
        missing = [md.bodies[i].name for i in group if i not in named]
        if missing:
            raise NimbleAmdError(f"body set: {md.bodies[[i for i in group if i in named][0]].name!r} is welded into one body with {missing}: "
                                 "the device model has merged their inertias - name the whole group")
    return out


def origin_moments(md) -> Optional[np.ndarray]:
    """Per body of md.merge_welds(): sum_k m_k o_k over the bodies welded into it, o_k the origin of body k's frame in the merged body's
    frame ([bodies][3]); None for a model without welds.  What NBL_CEN_PE_BODY_ORIGIN needs to give the reference's number on merged bodies."""
    if not md.has_welds():
        return None
    targets, T_in = md.weld_targets()
    out = np.zeros((max(targets) + 1, 3))
    for i, t in enumerate(targets):
        if t >= 0:
            out[t] += float(md.bodies[i].mass) * np.asarray(T_in[i], dtype=np.float64)[:3, 3]
    return out


class _SetHandle:
    def __init__(self, L, ptr):
        self.L, self.ptr = L, ptr
        self.mass_version = None                                  # World._mass_version the origin moments were uploaded at

    def __del__(self):
        try:
            self.L.nbl_body_set_destroy(self.ptr)
        except Exception:
            pass


def _body_set(world, bodies=None, skeleton=None):
    """(the nbl_body_set* of the set on this World's handle, made on first use and again when the handle changes).  What a call costs
    after the first one for its set: a dictionary look-up - the set is resolved once per (bodies, skeleton), and the origin moments of
    weld-merged bodies are computed again only after World.setMasses has changed the masses (World._mass_version)."""
    cache = getattr(world, "_cen_sets", None)
    if cache is None or cache[0] is not world._h:
        cache = (world._h, {}, {})                                # handle, user key -> set handle, resolved bodies -> set handle
        world._cen_sets = cache
    ukey = (tuple(bodies) if isinstance(bodies, (list, tuple)) else bodies, skeleton)
    got = cache[1].get(ukey)
    if got is None:
        idx = resolve_body_set(world.description, bodies, skeleton)
        key = None if idx is None else tuple(idx)
        got = cache[2].get(key)
        if got is None:
            ptr = C.c_void_p()
            arr = np.asarray(idx if idx is not None else [], dtype=np.int32)
            check(world._L.nbl_body_set_create(world._h, int(arr.size), arr.ctypes.data_as(C.c_void_p) if arr.size else None, C.byref(ptr)),
                  "nbl_body_set_create")
            got = _SetHandle(world._L, ptr)
            cache[2][key] = got
        cache[1][ukey] = got
    version = getattr(world, "_mass_version", 0)
    if got.mass_version != version:                               # first use, or the masses of welded bodies may have changed
        mo = origin_moments(world.description)
        if mo is not None:
            mo = np.ascontiguousarray(mo)
            ids = np.arange(mo.shape[0], dtype=np.int32)
            check(world._L.nbl_body_set_origin_moments(world._h, got.ptr, int(ids.size), ids.ctypes.data_as(C.c_void_p),
                                                       mo.ctypes.data_as(C.c_void_p)), "nbl_body_set_origin_moments")
        got.mass_version = version
    return got


def _workspace(world, B: int):
    need = world._L.nbl_centroidal_workspace_bytes(world._h, B)
    ws = getattr(world, "_cen_ws", None)
    if ws is None or ws.numel() < need or ws.device != world.device:
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=world.device)
        world._cen_ws = ws
    return ws


# ---- raw SoA calls: state [2n][B], accel [n][B]; outputs [3][B], [3][B], [3][B], [6][B], [B], [B], Jcom [3 n][B] ----
def centroidal_soa(world, bset, s_soa: torch.Tensor, a_soa, flags: int = 0, want=(True,) * 6, want_jac: bool = False, ws=None):
    B = s_soa.shape[1]
    outs = [torch.empty((r, B) if r > 1 else (B,), dtype=torch.float64, device=world.device) if w else None for r, w in zip(_ROWS, want)]
    J = torch.empty((3 * world.n, B), dtype=torch.float64, device=world.device) if want_jac else None
    if B > 0:
        ws = _workspace(world, B) if ws is None else ws
        with torch.cuda.device(world.device):
            check(world._L.nbl_centroidal_forward(world._h, bset.ptr, B, _ptr(s_soa), _ptr(a_soa), flags, *[_ptr(o) for o in outs], _ptr(J), _ptr(ws),
                                                  ws.numel(), world._stream()), "nbl_centroidal_forward")
    return outs, J


def centroidal_vjp_soa(world, bset, s_soa: torch.Tensor, a_soa, cots, flags: int = 0, want_accel: bool = True, ws=None):
    B = s_soa.shape[1]
    gs = torch.empty((2 * world.n, B), dtype=torch.float64, device=world.device)
    ga = torch.empty((world.n, B), dtype=torch.float64, device=world.device) if want_accel else None
    if B > 0:
        ws = _workspace(world, B) if ws is None else ws
        with torch.cuda.device(world.device):
            check(world._L.nbl_centroidal_backward(world._h, bset.ptr, B, _ptr(s_soa), _ptr(a_soa), flags, *[_ptr(c) for c in cots], _ptr(gs), _ptr(ga),
                                                   0, _ptr(ws), ws.numel(), world._stream()), "nbl_centroidal_backward")
    return gs, ga


class CentroidalLayer(torch.autograd.Function):
    """(world, state, accel, body set, flags, which outputs) -> the requested outputs, in the order of Centroidal"""

    @staticmethod
    def forward(ctx, world, state, accel, bset, flags, want):
        _join_if_deferred(world)                                  # before anything reads `state`: it may come out of the slices
        n = world.n
        x, ctx.ref_s, ctx.width_s = _restrict(world, state.detach(), "centroidal", "state")
        lead = tuple(x.shape[:-1])
        s_soa = world.to_soa(world._prep(x.reshape(-1, 2 * n), 2 * n, "dyn_state"))
        a_soa = None
        if accel is not None:
            a, ctx.ref_a, ctx.width_a = _restrict(world, accel.detach(), "centroidal", "accel")
            if tuple(a.shape[:-1]) != lead:
                raise ValueError(f"centroidal: accel has leading shape {tuple(a.shape[:-1])}, state {lead}")
            a_soa = world.to_soa(world._prep(a.reshape(-1, n), n, "dyn_accel"))
            ctx.accel_device = accel.device
        elif want[2]:
            raise NimbleAmdError("com_acceleration needs the accelerations")
        outs, _ = centroidal_soa(world, bset, s_soa, a_soa, flags, want)
        res = []
        for o, r in zip(outs, _ROWS):
            if o is None:
                continue
            o = world.from_soa(o).reshape(lead + (r,)) if r > 1 else o.reshape(lead)
            res.append(_give(world, o, state.device))
        ctx.world, ctx.bset, ctx.s_soa, ctx.a_soa, ctx.flags, ctx.want, ctx.lead, ctx.state_device = world, bset, s_soa, a_soa, flags, want, lead, state.device
        ctx.set_materialize_grads(False)
        return tuple(res)

    @staticmethod
    def backward(ctx, *grads):
        world, n, lead = ctx.world, ctx.world.n, ctx.lead
        cots, it = [], iter(grads)
        for w, r in zip(ctx.want, _ROWS):
            g = next(it) if w else None
            if g is None:
                cots.append(None)
                continue
            g = g.detach().to(device=world.device, dtype=torch.float64)
            cots.append(world.to_soa(g.reshape(-1, r)) if r > 1 else g.reshape(-1).contiguous())
        want_a = ctx.a_soa is not None and ctx.needs_input_grad[2]
        gs, ga = centroidal_vjp_soa(world, ctx.bset, ctx.s_soa, ctx.a_soa, cots, ctx.flags, want_a)
        ds = world.from_soa(gs).reshape(lead + (2 * n,))
        if ctx.ref_s:                                             # zero for the frozen coordinates
            ds = _expand(world, ds, lead, ctx.width_s, "state")
        ds = _give(world, ds, ctx.state_device)
        da = None
        if want_a:
            da = world.from_soa(ga).reshape(lead + (n,))
            if ctx.ref_a:
                da = _expand(world, da, lead, ctx.width_a, "accel")
            da = _give(world, da, ctx.accel_device)
        return None, ds, da, None, None, None


def _one(world, state, accel, bodies, skeleton, flags, k):
    want = tuple(i == k for i in range(6))
    return CentroidalLayer.apply(world, state, accel, _body_set(world, bodies, skeleton), flags, want)[0]


def center_of_mass(world, state: torch.Tensor, bodies=None, skeleton=None) -> torch.Tensor:
    """Skeleton::getCOM in world coordinates: [..., 2n] -> [..., 3]."""
    return _one(world, state, None, bodies, skeleton, 0, 0)


def com_velocity(world, state: torch.Tensor, bodies=None, skeleton=None) -> torch.Tensor:
    """Skeleton::getCOMLinearVelocity(World, World): [..., 2n] -> [..., 3].  Its gradient to the positions is complete."""
    return _one(world, state, None, bodies, skeleton, 0, 1)


def com_acceleration(world, state: torch.Tensor, accel: torch.Tensor, bodies=None, skeleton=None) -> torch.Tensor:
    """Skeleton::getCOMLinearAcceleration at the joint accelerations `accel` [..., n]: the mass-weighted classical acceleration of the
    bodies' centres of mass, [..., 3].  Gravity is not part of it: with accel = forward_dynamics(...) it IS the gravity vector plus the
    external forces over the mass."""
    return _one(world, state, accel, bodies, skeleton, 0, 2)


def centroidal_momentum(world, state: torch.Tensor, bodies=None, skeleton=None) -> torch.Tensor:
    """[angular momentum about the set's centre of mass; linear momentum] in world coordinates, [..., 6]: the sum over the set of
    BodyNode::getAngularMomentum(com) / getLinearMomentum (the reference has them per body only)."""
    return _one(world, state, None, bodies, skeleton, 0, 3)


def kinetic_energy(world, state: torch.Tensor, bodies=None, skeleton=None) -> torch.Tensor:
    """Skeleton::computeKineticEnergy: [..., 2n] -> [...]."""
    return _one(world, state, None, bodies, skeleton, 0, 4)


def _pe_flags(at_com: bool, springs: bool) -> int:
    return (0 if at_com else CEN_PE_BODY_ORIGIN) | (0 if springs else CEN_NO_SPRINGS)


def potential_energy(world, state: torch.Tensor, bodies=None, skeleton=None, at_com: bool = True, springs: bool = True) -> torch.Tensor:
    """Gravitational potential energy -sum m g . x of the set plus the spring energy of its joints, [...].  at_com=True takes x at every
    body's centre of mass; at_com=False at the origin of its frame, which is what the reference's BodyNode::computePotentialEnergy
    returns (BodyNode.cpp:2372-2375).  springs=False leaves the joint springs out."""
    return _one(world, state, None, bodies, skeleton, _pe_flags(at_com, springs), 5)


def centroidal(world, state: torch.Tensor, accel: Optional[torch.Tensor] = None, bodies=None, skeleton=None, at_com: bool = True,
               springs: bool = True) -> Centroidal:
    """All of the above from one launch (and one backward launch): Centroidal(com, com_vel, com_acc, momentum, ke, pe); com_acc is None
    without `accel`."""
    want = (True, True, accel is not None, True, True, True)
    res = list(CentroidalLayer.apply(world, state, accel, _body_set(world, bodies, skeleton), _pe_flags(at_com, springs), want))
    if accel is None:
        res.insert(2, None)
    return Centroidal(*res)


def com_jacobian(world, state: torch.Tensor, bodies=None, skeleton=None) -> torch.Tensor:
    """Skeleton::getCOMLinearJacobian in world coordinates, [..., 3, n]: com_velocity = J v.  Detached, like the dense getters."""
    _join_if_deferred(world)
    n = world.n
    x, ref, width = _restrict(world, state.detach(), "com_jacobian", "state")
    lead = tuple(x.shape[:-1])
    s_soa = world.to_soa(world._prep(x.reshape(-1, 2 * n), 2 * n, "dyn_state"))
    _, J = centroidal_soa(world, _body_set(world, bodies, skeleton), s_soa, None, 0, (False,) * 6, True)
    out = world.from_soa(J).reshape(lead + (3, n))
    if ref:                                                       # zero columns for the frozen coordinates
        lay = world.ref_layout
        out = torch.zeros(lead + (3, width // 2), dtype=torch.float64, device=world.device).index_copy(-1, lay._idx(world.device, "mobile"), out)
    return _give(world, out, state.device)


def total_mass(world, bodies=None, skeleton=None) -> float:
    """Skeleton::getMass of the set at the World's current inertias."""
    return float(world._L.nbl_body_set_mass(world._h, _body_set(world, bodies, skeleton).ptr))


# ---- the World's getters on its current state (detached, like getMassMatrix) ----
def _current(world):
    if getattr(world, "_state", None) is None:
        raise NimbleAmdError("call world.setState() first")
    return world._state


def world_centroidal(world, k: int, skeleton=None, accelerations=None, flags: int = 0) -> torch.Tensor:
    _join_if_deferred(world)
    s = _current(world)
    a_soa = None
    if accelerations is not None:
        a, _, _ = _restrict(world, accelerations.detach(), "getCOMLinearAcceleration", "accel")
        a_soa = world.to_soa(world._prep(a.reshape(-1, world.n), world.n, "dyn_accel"))
        if a_soa.shape[1] != s.shape[1]:
            raise ValueError(f"getCOMLinearAcceleration: {a_soa.shape[1]} acceleration vectors for {s.shape[1]} worlds")
    bset = _body_set(world, None, skeleton)
    one = getattr(world, "_one_d", False)
    if k == 6:
        _, J = centroidal_soa(world, bset, s, None, 0, (False,) * 6, True)
        out = world.from_soa(J).reshape(-1, 3, world.n)
    else:
        outs, _ = centroidal_soa(world, bset, s, a_soa, flags, tuple(i == k for i in range(6)))
        out = world.from_soa(outs[k]) if _ROWS[k] > 1 else outs[k]
    return out[0] if one else out


# `nimblephysics_amd.centroidal` names this module AND - re-exported by the package - the function above; once the module has been imported
# the package attribute is the module, so the module itself answers a call like the function.
import sys as _sys
import types as _types


class _CallableModule(_types.ModuleType):
    def __call__(self, *args, **kwargs):
        return centroidal(*args, **kwargs)


_sys.modules[__name__].__class__ = _CallableModule
