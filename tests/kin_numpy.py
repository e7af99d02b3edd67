"""A numpy statement of the reference's world-space body Jacobians, for the IKMapping tests (not product code).

  positions   Skeleton::getWorldPositionJacobian (Skeleton.cpp:11010-11060): for every DOF on the body's ancestor path the joint's
              world position screw [w; v] (Joint::getWorldAxisScrewForPosition; BallJoint / FreeJoint::getWorldAxisScrewAt build it on
              expMapJac in the parent's joint frame), then linear rows v + w x p_body, angular rows dLogMap(R, [w] R);
  velocities  Skeleton::getWorldJacobian: the world velocity screw AdT(W_child, S) of every DOF, linear rows v + w x p_body.
Body world transforms come from the CPU oracle (OracleWorld.body_world_transform); logMap and its derivative are written out from
their formulas (regular branch, theta < pi - 1e-6)."""
import numpy as np

ROWS = {0: 6, 1: 3, 2: 3}


def skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def logmap(R):
    c = np.clip(0.5 * (np.trace(R) - 1.0), -1.0, 1.0)
    th = np.arccos(c)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    alpha = 0.5 * th / np.sin(th) if th > 1e-6 else 0.5 + th * th / 12.0
    return alpha * w


def dlogmap(R, dR):
    """d/dt logMap(R(t)) for R' = dR: r = alpha(theta) w(R), theta = acos((tr R - 1) / 2)."""
    c = np.clip(0.5 * (np.trace(R) - 1.0), -1.0, 1.0)
    th = np.arccos(c)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    dw = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    if th > 1e-6:
        s = np.sin(th)
        alpha = 0.5 * th / s
        dth = -0.5 * np.trace(dR) / s
        dalpha = 0.5 * (s - th * np.cos(th)) / (s * s) * dth
    else:
        alpha, dalpha = 0.5 + th * th / 12.0, -np.trace(dR) / 12.0      # d(theta^2) = -tr(dR) near theta = 0
    return dalpha * w + alpha * dw


def expmapjac(r):
    th = np.linalg.norm(r)
    S = skew(r)
    if th < 1e-3:
        A, B = 0.5, 1.0 / 6.0
    else:
        A, B = (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return np.eye(3) + A * S + B * S @ S


def _ndof(b):
    return {"free": 6, "ball": 3, "weld": 0}.get(b.joint_type, 1)


def dof_offsets(md):
    off, out = 0, []
    for b in md.bodies:
        out.append(off)
        off += _ndof(b)
    return out


def _adt(T, w, v):
    """AdT(T, [w; v]) for a 4 x 4 transform"""
    R, p = T[:3, :3], T[:3, 3]
    Rw = R @ w
    return Rw, R @ v + np.cross(p, Rw)


def joint_screws(ow, md, q, c):
    """[(dof, position screw (w, v), velocity screw (w, v))] of the joint of body c (world coordinates, at the world origin)"""
    b = md.bodies[c]
    nd = _ndof(b)
    if nd == 0:
        return []
    o = dof_offsets(md)[c]
    Wc = ow.body_world_transform(q, c)
    Wp = ow.body_world_transform(q, b.parent) if b.parent >= 0 else np.eye(4)
    Tpj, Tcj = np.asarray(b.T_pj, dtype=np.float64), np.asarray(b.T_cj, dtype=np.float64)
    WJ = Wc @ Tcj                        # the joint frame on the child's side
    out = []
    if b.joint_type in ("revolute", "prismatic", "screw"):
        a = np.asarray(b.axis, dtype=np.float64)
        a = a / np.linalg.norm(a)                                         # (RevoluteJoint::setAxis normalizes; so does ModelDescription.flat)
        w = WJ[:3, :3] @ a
        if b.joint_type == "prismatic":
            s = (np.zeros(3), w)
        else:
            v = np.cross(WJ[:3, 3], w) + (b.pitch / (2 * np.pi) * w if b.joint_type == "screw" else 0.0)
            s = (w, v)
        return [(o, s, s)]
    F0 = Wp @ Tpj                        # the joint frame on the parent's side
    E = np.eye(3)
    if b.joint_type == "ball":
        J = expmapjac(q[o:o + 3])
        for k in range(3):
            out.append((o + k, _adt(F0, J[:, k], np.zeros(3)), _adt(WJ, E[k], np.zeros(3))))
        return out
    r, t = q[o:o + 3], q[o + 3:o + 6]                                     # free joint
    J = expmapjac(r)
    Tt = np.eye(4); Tt[:3, 3] = t
    for k in range(6):
        if k < 3:
            ps = _adt(F0, *_adt(Tt, J[:, k], np.zeros(3)))
            vs = _adt(WJ, E[k], np.zeros(3))
        else:
            ps = _adt(F0, np.zeros(3), E[k - 3])
            vs = _adt(WJ, np.zeros(3), E[k - 3])
        out.append((o + k, ps, vs))
    return out


def body_jacobians(ow, md, q, e):
    """(W_e, Jpos [6][n], Jvel [6][n]) of body e of md (rows [angular; linear])"""
    n = md.num_dofs
    W = ow.body_world_transform(q, e)
    R, p = W[:3, :3], W[:3, 3]
    Jp, Jv = np.zeros((6, n)), np.zeros((6, n))
    c = e
    while c >= 0:
        for d, (pw, pv), (vw, vv) in joint_screws(ow, md, q, c):
            Jp[:3, d] = dlogmap(R, skew(pw) @ R)
            Jp[3:, d] = pv + np.cross(pw, p)
            Jv[:3, d] = vw
            Jv[3:, d] = vv + np.cross(vw, p)
        c = md.bodies[c].parent
    return W, Jp, Jv


def mapping_rows(ow, md, q, entries):
    """entries [(kind, body index of md)] -> (positions [P], Jpos [P][n], Jvel [P][n]) like IKMapping (rows in entry order)"""
    pos, Jp, Jv = [], [], []
    for kind, e in entries:
        W, P6, V6 = body_jacobians(ow, md, q, e)
        rows = {0: slice(0, 6), 1: slice(3, 6), 2: slice(0, 3)}[kind]
        full = np.concatenate([logmap(W[:3, :3]), W[:3, 3]])
        pos.append(full[rows]); Jp.append(P6[rows]); Jv.append(V6[rows])
    return np.concatenate(pos), np.concatenate(Jp), np.concatenate(Jv)
