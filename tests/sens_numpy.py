"""A numpy statement of the inertial-sensor readings (Skeleton::getGyroReadings, getAccelerometerReadings, getMagnetometerReadings) for the
tests of csrc/sensors_dev.hpp (not product code).

Built on three things only: OracleWorld.body_world_transform for the body frames, kin_numpy.joint_screws for the world screws of every
coordinate (through cen_numpy.Kin, which collects both along the ancestor chains), and the world-frame spatial acceleration as
cen_numpy.Kin.com_acc writes it out.  Everything is written in WORLD coordinates about the world origin - the device code works in body
frames - and on the description as it stands: a welded body is its own body here.

A sensor is (body index of md, or -1 for the world; T 4 x 4 in that body).  With the body's frame (R, p), R_s = R R_bs, the sensor's origin
x = p + R p_bs, the body's world twist (w, vo) and world spatial acceleration (al, ao) about the world origin, gravity g and field m:
  gyro = R_s^T w        acc = R_s^T (ao + al x x + w x (vo + w x x) - g)        mag = R_s^T m
(ao + al x x + w x (vo + w x x) is the classical acceleration of the body-fixed point x.)
Closed-form Jacobians: d gyro / dv = R_s^T Jang, d acc / da = R_s^T (Jlin - [x]x Jang), d mag / dm = R_s^T; everything else by central
differences of these functions (fd_vjp)."""
import numpy as np

import cen_numpy
from kin_numpy import skew

ORDER = ("gyro", "acc", "mag")


def _kin(ow, md, q, sensors):
    return cen_numpy.Kin(ow, md, q, sorted({i for i, _ in sensors if i >= 0}))


def _twists(k, v, a, i):
    """(w, vo, al, ao) of body i: A = sum_d s_d a_d + ad(V_body(d), s_d) v_d, a screw moving with the child body of its joint"""
    Vw, Vv, Aw, Av = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)
    for c in reversed(k.path(i)):
        for d, _, (sw, sv) in k.screws[c]:
            Vw, Vv = Vw + sw * v[d], Vv + sv * v[d]
        for d, _, (sw, sv) in k.screws[c]:
            Aw = Aw + sw * a[d] + np.cross(Vw, sw) * v[d]
            Av = Av + sv * a[d] + (np.cross(Vw, sv) + np.cross(Vv, sw)) * v[d]
    return Vw, Vv, Aw, Av


def _frame(k, i, T):
    W = k.W[i] if i >= 0 else np.eye(4)
    return W[:3, :3] @ T[:3, :3], W[:3, 3] + W[:3, :3] @ T[:3, 3]


def readings(ow, md, sensors, q, v, a, m, kin=None):
    """{gyro, acc, mag: [3 S]} for one world"""
    k = kin if kin is not None else _kin(ow, md, q, sensors)
    g = np.asarray(md.gravity, dtype=np.float64)
    out = {nm: [] for nm in ORDER}
    for i, T in sensors:
        Rs, x = _frame(k, i, T)
        w, vo, al, ao = _twists(k, v, a, i) if i >= 0 else (np.zeros(3),) * 4
        out["gyro"].append(Rs.T @ w)
        out["acc"].append(Rs.T @ (ao + np.cross(al, x) + np.cross(w, vo + np.cross(w, x)) - g))
        out["mag"].append(Rs.T @ m)
    return {nm: np.concatenate(x) for nm, x in out.items()}


def closed_form_jacobians(ow, md, sensors, q):
    """{gyro_v [3 S][n], acc_a [3 S][n], mag_m [3 S][3]}"""
    k = _kin(ow, md, q, sensors)
    n = md.num_dofs
    gv, aa, mm = [], [], []
    for i, T in sensors:
        Rs, x = _frame(k, i, T)
        Ja, Jl = k.jac(i) if i >= 0 else (np.zeros((3, n)), np.zeros((3, n)))
        gv.append(Rs.T @ Ja)
        aa.append(Rs.T @ (Jl - skew(x) @ Ja))
        mm.append(Rs.T)
    return {"gyro_v": np.concatenate(gv), "acc_a": np.concatenate(aa), "mag_m": np.concatenate(mm)}


def fd_vjp(ow, md, sensors, q, v, a, m, cot, h):
    """{output: gradient [3 n + 3] of <cot[output], output> to (q, v, a, m)} by central differences of `readings` with the step h"""
    n = md.num_dofs
    x0 = np.concatenate([q, v, a, m])
    out = {nm: np.zeros(3 * n + 3) for nm in ORDER}
    base = _kin(ow, md, q, sensors)                                 # a step in v, a or m leaves the frames and screws where they are
    for j in range(3 * n + 3):
        xp, xm = x0.copy(), x0.copy()
        xp[j] += h
        xm[j] -= h
        kin = base if j >= n else None
        fp = readings(ow, md, sensors, xp[:n], xp[n:2 * n], xp[2 * n:3 * n], xp[3 * n:], kin)
        fm = readings(ow, md, sensors, xm[:n], xm[n:2 * n], xm[2 * n:3 * n], xm[3 * n:], kin)
        for nm in ORDER:
            out[nm][j] = cot[nm] @ (fp[nm] - fm[nm]) / (2 * h)
    return out
