"""Gyroscope, accelerometer and magnetometer readings of sensors fixed in bodies, for batches of states, with exact gradients: the
reference's Skeleton::getGyroReadings, getAccelerometerReadings, getMagnetometerReadings and their ...JacobianWrt getters
(dart/dynamics/Skeleton.cpp:8082-8460; www/docs/accs-and-gyros.rst).

A sensor list is a sequence of (body, T) pairs - the reference's List[Tuple[BodyNode, Isometry3]]: `body` a name or an index into
world.description.bodies (-1: the world), `T` the sensor's frame in that body, 4 x 4 (None: identity).  With the body's spatial velocity
[w; v] and spatial acceleration [al; a] in body coordinates, its world rotation R, the model's gravity g and a world-frame field m:

    gyro = R_bs^T w        acc = R_bs^T (a + al x p_bs + w x (v + w x p_bs) - R^T g)        mag = R_bs^T R^T m

    w = gyro_readings(world, sensors, state)                        [..., 2n] -> [..., 3 S]     sensor-major, xyz
    a = accelerometer_readings(world, sensors, state, accel)        [..., 2n], [..., n] -> [..., 3 S]
    m = magnetometer_readings(world, sensors, state, field)         [..., 2n], [3] or [..., 3] -> [..., 3 S]
    r = imu_readings(world, sensors, state, accel, field=None)      IMUReadings(gyro, acc, mag) from ONE launch; mag is None without field
    J = gyro_jacobian(world, sensors, state, wrt)                   [B, 2n] -> [B, 3 S, n]      wrt: "position", "velocity", "acceleration"
    J = accelerometer_jacobian(world, sensors, state, accel, wrt)
    J = magnetometer_jacobian(world, sensors, state, field, wrt)    wrt may also be "field": [B, 3 S, 3]

Each reading call is one launch of csrc/sensors.hip over all the leading dimensions ([2n] one world, [B, 2n] a batch, [T+1, B, 2n] a
rollout) and one more for its backward pass, which gives the exact gradients to `state` (positions AND velocities), `accel` and `field`.
A Jacobian is one launch of the reverse kernel over 3 S x B worlds with unit cotangents; the blocks that are identically zero
(d gyro / d accel, d mag / d velocity, d mag / d accel) come back as zeros without a launch.

Rules shared with centroidal.py: CPU float64 tensors come back as CPU tensors, device tensors stay on the device; the World's state is
untouched; a World in deferred-join mode is joined first; on a world with immobile skeletons `state` and `accel` may come in the
reference's layout (the frozen coordinates get zero gradient and zero Jacobian columns).  Body scales do not exist in this library (they
are 1), so there is no GROUP_SCALES `wrt`; markers are IKMapping.addLinearBodyNode + map_to_pos.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from ._lib import NimbleAmdError, check
from .dynamics import _expand, _give, _restrict
from .mapping import KIN_SPATIAL, MAX_ENTRIES, _join_if_deferred, _ptr, resolve_body

IMUReadings = namedtuple("IMUReadings", ["gyro", "acc", "mag"])
WRT_POSITION, WRT_VELOCITY, WRT_ACCELERATION, WRT_FIELD = "position", "velocity", "acceleration", "field"


def resolve_sensors(md, sensors):
    """[(body of md.merge_welds() that carries the sensor or -1 for the world, the sensor's frame in it, 4 x 4)] of a sensor list."""
    if isinstance(sensors, tuple) and len(sensors) == 2 and isinstance(sensors[0], (str, int, np.integer)):
        sensors = [sensors]
    out = []
    for k, item in enumerate(sensors):
        try:
            body, T = item
        except (TypeError, ValueError):
            raise ValueError(f"sensors: entry {k} is not a (body, transform) pair") from None
        T = np.eye(4) if T is None else np.array(T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else T, dtype=np.float64)
        if T.shape != (4, 4) or not np.isfinite(T).all():
            raise ValueError(f"sensors: entry {k}: the transform must be a finite 4 x 4 array, got shape {T.shape}")
        if isinstance(body, (int, np.integer)) and not isinstance(body, bool) and int(body) == -1:
            out.append((-1, T))
            continue
        try:
            mb, T_in = resolve_body(md, body)
        except (ValueError, TypeError) as e:                      # resolve_body speaks for the mapping it was written for
            raise type(e)(str(e).replace("IKMapping:", "sensors:", 1)) from None
        out.append((mb, T_in @ T))
    if not out:
        raise ValueError("sensors: the list is empty")
    if len(out) > MAX_ENTRIES:
        raise ValueError(f"sensors: at most {MAX_ENTRIES} sensors in one list; got {len(out)}")
    return out


class _SetHandle:
    def __init__(self, L, ptr, count):
        self.L, self.ptr, self.count = L, ptr, count

    def __del__(self):
        try:
            self.L.nbl_kin_map_destroy(self.ptr)
        except Exception:
            pass


def _sensor_set(world, sensors) -> _SetHandle:
    """The device map of the sensor list on this World's handle: made on first use, kept on the World, made again when its handle changes."""
    cache = getattr(world, "_sens_sets", None)
    if cache is None or cache[0] is not world._h:
        cache = (world._h, {})
        world._sens_sets = cache
    res = resolve_sensors(world.description, sensors)
    key = tuple((mb, T.tobytes()) for mb, T in res)
    got = cache[1].get(key)
    if got is None:
        cnt = len(res)
        kind = np.full(cnt, KIN_SPATIAL, dtype=np.int32)
        body = np.array([mb for mb, _ in res], dtype=np.int32)
        T = np.ascontiguousarray(np.stack([np.concatenate([t[:3, :3].reshape(9), t[:3, 3]]) for _, t in res]), dtype=np.float64)
        ptr = C.c_void_p()
        check(world._L.nbl_kin_map_create(world._h, cnt, kind.ctypes.data_as(C.c_void_p), body.ctypes.data_as(C.c_void_p),
                                          T.ctypes.data_as(C.c_void_p), C.byref(ptr)), "nbl_kin_map_create")
        got = _SetHandle(world._L, ptr, cnt)
        cache[1][key] = got
    return got


def _workspace(world, B: int):
    need = world._L.nbl_sensors_workspace_bytes(world._h, B)
    ws = getattr(world, "_sens_ws", None)
    if ws is None or ws.numel() < need or ws.device != world.device:
        ws = torch.empty(max(need, 1), dtype=torch.uint8, device=world.device)
        world._sens_ws = ws
    return ws


# ---- raw SoA calls: state [2n][B], accel [n][B], field [3][B]; outputs and cotangents [3 S][B] ----
def sensors_soa(world, sset, s_soa: torch.Tensor, a_soa, f_soa, want=(True, True, True)):
    B = s_soa.shape[1]
    outs = [torch.empty((3 * sset.count, B), dtype=torch.float64, device=world.device) if w else None for w in want]
    if B > 0:
        ws = _workspace(world, B)
        with torch.cuda.device(world.device):
            check(world._L.nbl_sensors_forward(world._h, sset.ptr, B, _ptr(s_soa), _ptr(a_soa), _ptr(f_soa), *[_ptr(o) for o in outs], _ptr(ws),
                                               ws.numel(), world._stream()), "nbl_sensors_forward")
    return outs


def sensors_vjp_soa(world, sset, s_soa: torch.Tensor, a_soa, f_soa, cots, want=(True, True, True)):
    """-> (grad_state [2n][B], grad_accel [n][B], grad_field [3][B]), None where `want` is False"""
    B, n = s_soa.shape[1], world.n
    grads = [torch.empty((r, B), dtype=torch.float64, device=world.device) if w else None for r, w in zip((2 * n, n, 3), want)]
    if B > 0:
        ws = _workspace(world, B)
        with torch.cuda.device(world.device):
            check(world._L.nbl_sensors_backward(world._h, sset.ptr, B, _ptr(s_soa), _ptr(a_soa), _ptr(f_soa), *[_ptr(c) for c in cots],
                                                *[_ptr(g) for g in grads], 0, _ptr(ws), ws.numel(), world._stream()), "nbl_sensors_backward")
    return grads


def _inputs(world, what, state, accel, field):
    """(state [2n][B], accel [n][B] or None, field [3][B] or None on the device, the leading shape, (ref, width) of state and of accel)"""
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
    f_soa = None
    if field is not None:
        f = field.detach()
        if f.dim() == 0 or f.shape[-1] != 3:
            raise ValueError(f"{what}: field has shape {tuple(field.shape)}; expected [3] or [..., 3]")
        try:
            f = f.expand(lead + (3,))
        except RuntimeError:
            raise ValueError(f"{what}: field has shape {tuple(field.shape)}, which does not broadcast to {lead + (3,)}") from None
        f_soa = world.to_soa(world._prep(f.reshape(-1, 3), 3, "sens_field"))
    return s_soa, a_soa, f_soa, lead, (ref_s, width_s), (ref_a, width_a)


class SensorLayer(torch.autograd.Function):
    """(world, state, accel, field [lead + (3,)], sensor set, which outputs) -> the requested outputs, in the order of IMUReadings"""

    @staticmethod
    def forward(ctx, world, state, accel, field, sset, want):
        _join_if_deferred(world)                                  # before anything reads `state`: it may come out of the slices
        if want[1] and accel is None:
            raise NimbleAmdError("accelerometer readings need the accelerations")
        if want[2] and field is None:
            raise NimbleAmdError("magnetometer readings need the magnetic field")
        s_soa, a_soa, f_soa, lead, ctx.lay_s, ctx.lay_a = _inputs(world, "sensor readings", state, accel if want[1] else None,
                                                                  field if want[2] else None)
        outs = sensors_soa(world, sset, s_soa, a_soa, f_soa, want)
        res = tuple(_give(world, world.from_soa(o).reshape(lead + (3 * sset.count,)), state.device) for o in outs if o is not None)
        ctx.world, ctx.sset, ctx.soa, ctx.want, ctx.lead = world, sset, (s_soa, a_soa, f_soa), want, lead
        ctx.devices = (state.device, accel.device if accel is not None else None, field.device if field is not None else None)
        ctx.set_materialize_grads(False)
        return res

    @staticmethod
    def backward(ctx, *grads):
        world, n, lead, rows = ctx.world, ctx.world.n, ctx.lead, 3 * ctx.sset.count
        s_soa, a_soa, f_soa = ctx.soa
        cots, it = [], iter(grads)
        for w in ctx.want:
            g = next(it) if w else None
            cots.append(None if g is None else world.to_soa(g.detach().to(device=world.device, dtype=torch.float64).reshape(-1, rows)))
        want_a = a_soa is not None and ctx.needs_input_grad[2]
        want_f = f_soa is not None and ctx.needs_input_grad[3]
        gs, ga, gf = sensors_vjp_soa(world, ctx.sset, s_soa, a_soa, f_soa, cots, (True, want_a, want_f))
        ds = world.from_soa(gs).reshape(lead + (2 * n,))
        if ctx.lay_s[0]:                                          # zero for the frozen coordinates
            ds = _expand(world, ds, lead, ctx.lay_s[1], "state")
        ds = _give(world, ds, ctx.devices[0])
        da = df = None
        if want_a:
            da = world.from_soa(ga).reshape(lead + (n,))
            if ctx.lay_a[0]:
                da = _expand(world, da, lead, ctx.lay_a[1], "accel")
            da = _give(world, da, ctx.devices[1])
        if want_f:
            df = _give(world, world.from_soa(gf).reshape(lead + (3,)), ctx.devices[2])
        return None, ds, da, df, None, None


def _spread(field, state):
    """`field` [3] or [..., 3] over the leading dimensions of `state`, by torch's own broadcasting (so its gradient is summed back)"""
    if field is None:
        return None
    if not isinstance(field, torch.Tensor):
        field = torch.as_tensor(np.asarray(field, dtype=np.float64), device=state.device)
    if field.dim() == 0 or field.shape[-1] != 3:
        raise ValueError(f"magnetometer readings: field has shape {tuple(field.shape)}; expected [3] or [..., 3]")
    try:
        return field.expand(tuple(state.shape[:-1]) + (3,))
    except RuntimeError:
        raise ValueError(f"magnetometer readings: field has shape {tuple(field.shape)}, which does not broadcast to "
                         f"{tuple(state.shape[:-1]) + (3,)}") from None


def gyro_readings(world, sensors, state: torch.Tensor) -> torch.Tensor:
    """Skeleton::getGyroReadings: the bodies' angular velocities in the sensors' frames, [..., 2n] -> [..., 3 S]."""
    return SensorLayer.apply(world, state, None, None, _sensor_set(world, sensors), (True, False, False))[0]


def accelerometer_readings(world, sensors, state: torch.Tensor, accel: torch.Tensor) -> torch.Tensor:
    """Skeleton::getAccelerometerReadings at the joint accelerations `accel` [..., n]: the proper acceleration of every sensor's origin
    in its own frame (a body at rest reads -g; one in free fall reads 0), [..., 3 S]."""
    return SensorLayer.apply(world, state, accel, None, _sensor_set(world, sensors), (False, True, False))[0]


def magnetometer_readings(world, sensors, state: torch.Tensor, field) -> torch.Tensor:
    """Skeleton::getMagnetometerReadings: the world-frame field `field` ([3] or [..., 3]) in the sensors' frames, [..., 3 S]."""
    return SensorLayer.apply(world, state, None, _spread(field, state), _sensor_set(world, sensors), (False, False, True))[0]


def imu_readings(world, sensors, state: torch.Tensor, accel: torch.Tensor, field=None) -> IMUReadings:
    """Gyroscope, accelerometer and - with `field` - magnetometer readings from one launch (and one backward launch)."""
    want = (True, True, field is not None)
    res = list(SensorLayer.apply(world, state, accel, _spread(field, state), _sensor_set(world, sensors), want))
    if field is None:
        res.append(None)
    return IMUReadings(*res)


# ---- dense Jacobians: one launch of the reverse kernel over 3 S x B worlds ----
_BLOCKS = {WRT_POSITION: 0, WRT_VELOCITY: 1, WRT_ACCELERATION: 2, WRT_FIELD: 3}
_ZERO = {(0, 2), (2, 1), (2, 2)}                                  # (output, block): identically zero


def _jacobian(world, sensors, which: int, state, accel, field, wrt, what: str) -> torch.Tensor:
    _join_if_deferred(world)
    if wrt not in _BLOCKS or (wrt == WRT_FIELD and which != 2):
        allowed = [k for k in _BLOCKS if k != WRT_FIELD or which == 2]
        raise ValueError(f"{what}: wrt must be one of {allowed}; got {wrt!r} (body scales do not exist in this library)")
    block = _BLOCKS[wrt]
    one = state.dim() == 1
    if state.dim() > 2:
        raise ValueError(f"{what}: state must be [B, 2n] or [2n]; got {tuple(state.shape)}")
    sset = _sensor_set(world, sensors)
    s_soa, a_soa, f_soa, lead, (ref_s, width_s), (ref_a, width_a) = _inputs(
        world, what, state, accel if which == 1 else None, _spread(field, state) if which == 2 else None)
    P, B, n = 3 * sset.count, s_soa.shape[1], world.n
    cols = 3 if block == 3 else n
    if (which, block) in _ZERO or B == 0:
        J = torch.zeros((B, P, cols), dtype=torch.float64, device=world.device)
    else:
        rep = lambda t: None if t is None else t.repeat(1, P)       # world p * B + b = (row p, world b)
        eye = torch.eye(P, dtype=torch.float64, device=world.device).repeat_interleave(B, dim=1)
        cots = [eye if k == which else None for k in range(3)]
        g = sensors_vjp_soa(world, sset, rep(s_soa), rep(a_soa), rep(f_soa), cots, (block < 2, block == 2, block == 3))
        G = g[0][block * n:(block + 1) * n] if block < 2 else g[block - 1]
        J = G.reshape(cols, P, B).permute(2, 1, 0).contiguous()
    lay = world.ref_layout
    if block < 3 and lay is not None and (ref_s or ref_a):         # columns of the frozen coordinates: zero
        J = torch.zeros((B, P, lay.n_ref), dtype=torch.float64, device=world.device).index_copy(2, lay._idx(world.device, "mobile"), J)
    J = _give(world, J, state.device)
    return J[0] if one else J


def gyro_jacobian(world, sensors, state: torch.Tensor, wrt: str) -> torch.Tensor:
    """Skeleton::getGyroReadingsJacobianWrt: d gyro / d positions, velocities or accelerations (zeros), [B, 3 S, n].  Detached."""
    return _jacobian(world, sensors, 0, state, None, None, wrt, "gyro_jacobian")


def accelerometer_jacobian(world, sensors, state: torch.Tensor, accel: torch.Tensor, wrt: str) -> torch.Tensor:
    """Skeleton::getAccelerometerReadingsJacobianWrt: [B, 3 S, n].  Detached."""
    return _jacobian(world, sensors, 1, state, accel, None, wrt, "accelerometer_jacobian")


def magnetometer_jacobian(world, sensors, state: torch.Tensor, field, wrt: str) -> torch.Tensor:
    """Skeleton::getMagnetometerReadingsJacobianWrt ([B, 3 S, n]; zeros for velocities and accelerations) and, with wrt = "field",
    getMagnetometerReadingsJacobianWrtMagneticField ([B, 3 S, 3]).  Detached."""
    return _jacobian(world, sensors, 2, state, None, field, wrt, "magnetometer_jacobian")


# ---- the World's getters on its current state (detached, like getCOM) ----
def _current_state(world) -> torch.Tensor:
    """the World's state as [B, 2n] over the device's coordinates, on the device"""
    _join_if_deferred(world)
    if getattr(world, "_state", None) is None:
        raise NimbleAmdError("call world.setState() first")
    return world.from_soa(world._state)


def world_readings(world, which: int, sensors, accelerations=None, field=None) -> torch.Tensor:
    s = _current_state(world)
    if accelerations is not None and accelerations.dim() == 1:
        accelerations = accelerations.unsqueeze(0)
    if accelerations is not None and accelerations.shape[0] != s.shape[0]:
        raise ValueError(f"getAccelerometerReadings: {accelerations.shape[0]} acceleration vectors for {s.shape[0]} worlds")
    want = tuple(k == which for k in range(3))
    out = SensorLayer.apply(world, s, accelerations, _spread(field, s), _sensor_set(world, sensors), want)[0]
    return out[0] if getattr(world, "_one_d", False) else out


def world_jacobian(world, which: int, sensors, wrt, accelerations=None, field=None) -> torch.Tensor:
    s = _current_state(world)
    if accelerations is not None and accelerations.dim() == 1:
        accelerations = accelerations.unsqueeze(0)
    if accelerations is not None:
        accelerations = accelerations.to(world.device)
    J = _jacobian(world, sensors, which, s, accelerations, field, wrt, ("getGyro", "getAccelerometer", "getMagnetometer")[which] + "ReadingsJacobianWrt")
    lay = world.ref_layout
    if lay is not None and wrt != WRT_FIELD and J.shape[-1] != lay.n_ref:     # the reference's columns; the frozen ones are zero
        J = torch.zeros(J.shape[:-1] + (lay.n_ref,), dtype=torch.float64, device=world.device).index_copy(2, lay._idx(world.device, "mobile"), J)
    return J[0] if getattr(world, "_one_d", False) else J
