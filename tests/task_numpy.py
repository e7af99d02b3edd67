"""A numpy statement of the task-space Jacobian J of an IKMapping's rows, of its time derivative Jdot and of the task-space acceleration
xdd = J a + Jdot v, for the tests of csrc/taskspace_dev.hpp (not product code; the instrument of those tests).

Built on the flat model arrays only (ModelDescription.flat(): parent, joint_type, dof_offset, T_pj, T_cj, axis, pitch) and written in
WORLD coordinates about the world origin, vectorised over a leading batch dimension N - the device code works in body frames, one world
per lane, on a model whose welds are merged and whose ball joints are chains; here a weld is a joint without coordinates and a ball joint
is one joint.

  forward kinematics   W_i = W_parent T_pj Q(q) T_cj^-1, Q by joint type (revolute / screw: rotation about the axis, the screw with
                       pitch / 2 pi of translation per radian; prismatic; ball: exp(q); free: [exp(q[0:3]), q[3:6]])
  screws               coordinate d of body i has the world screw X_d = Ad(W_i T_cj) s_d, s_d constant in the joint frame on the child's
                       side: [axis; 0], [0; axis], [axis; h axis], [e_k; 0] / [0; e_k].  It moves with body i.
  J                    column d of an entry on body e with frame F = W_e T_off at p: angular X_d.w, linear X_d.v + X_d.w x p for the
                       coordinates of e and its ancestors, zero for the others
  Jdot                 dX_d/dt = ad(V_i, X_d) with V_i = sum of X_d v_d over i and its ancestors (the closed-form time derivative of the
                       column: the screw is fixed in body i);  angular Xdot.w, linear Xdot.v + Xdot.w x p + X.w x pdot, pdot = J_lin v
  xdd                  J a + Jdot v
Gradients only by central differences of these functions (fd_*)."""
import numpy as np

REVOLUTE, PRISMATIC, FREE, WELD, BALL, SCREW = 0, 1, 2, 3, 4, 5      # NBL_JOINT_*
NDOF = {REVOLUTE: 1, PRISMATIC: 1, FREE: 6, WELD: 0, BALL: 3, SCREW: 1}
KIN_SPATIAL, KIN_LINEAR, KIN_ANGULAR = 0, 1, 2
ROWS = {KIN_SPATIAL: 6, KIN_LINEAR: 3, KIN_ANGULAR: 3}


def _t44(t12):
    T = np.eye(4)
    T[:3, :3] = np.asarray(t12[:9]).reshape(3, 3)
    T[:3, 3] = t12[9:]
    return T


def _skew(r):
    K = np.zeros(r.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -r[..., 2], r[..., 1], r[..., 2], -r[..., 0], -r[..., 1], r[..., 0]
    return K


def _exp(r):
    """Rodrigues' formula on rotation vectors r [N, 3]"""
    th = np.linalg.norm(r, axis=-1)[..., None, None]
    K = _skew(r)
    with np.errstate(invalid="ignore", divide="ignore"):
        a = np.where(th > 1e-9, np.sin(th) / th, 1.0)
        b = np.where(th > 1e-9, (1 - np.cos(th)) / th ** 2, 0.5)
    return np.eye(3) + a * K + b * K @ K


class Model:
    """the flat arrays of a ModelDescription (as it stands: welds are bodies of their own)"""

    def __init__(self, md):
        fl = md.flat()
        self.n, self.nb = md.num_dofs, len(md.bodies)
        self.parent, self.jt, self.off = fl["parent"], fl["joint_type"], fl["dof_offset"]
        self.Tpj = [_t44(t) for t in fl["T_pj"]]
        self.Tcj = [_t44(t) for t in fl["T_cj"]]
        self.TcjInv = [np.linalg.inv(T) for T in self.Tcj]
        self.axis, self.h = fl["axis"], fl["pitch"] / (2 * np.pi)
        assert all(self.parent[i] < i for i in range(self.nb))

    def ancestors(self, e):
        out = []
        while e >= 0:
            out.append(int(e))
            e = self.parent[e]
        return out


def kinematics(m, q):
    """q [N, n] -> (W [nb][N, 4, 4], X [n] of (w [N, 3], v [N, 3]): the world screws, body [n]: the body each coordinate moves)"""
    N = q.shape[0]
    W, X, body = [], [None] * m.n, [0] * m.n
    for i in range(m.nb):
        jt, o, ax = m.jt[i], m.off[i], m.axis[i]
        Q = np.tile(np.eye(4), (N, 1, 1))
        if jt in (REVOLUTE, SCREW):
            Q[:, :3, :3] = _exp(q[:, o, None] * ax)
            if jt == SCREW:
                Q[:, :3, 3] = m.h[i] * q[:, o, None] * ax
        elif jt == PRISMATIC:
            Q[:, :3, 3] = q[:, o, None] * ax
        elif jt == BALL:
            Q[:, :3, :3] = _exp(q[:, o:o + 3])
        elif jt == FREE:
            Q[:, :3, :3] = _exp(q[:, o:o + 3])
            Q[:, :3, 3] = q[:, o + 3:o + 6]
        Wi = m.Tpj[i] @ Q @ m.TcjInv[i]
        if m.parent[i] >= 0:
            Wi = W[m.parent[i]] @ Wi
        W.append(Wi)
        WJ = Wi @ m.Tcj[i]                                   # the joint frame on the child's side
        R, p = WJ[:, :3, :3], WJ[:, :3, 3]
        E = np.eye(3)
        local = {REVOLUTE: [(ax, 0 * ax)], PRISMATIC: [(0 * ax, ax)], SCREW: [(ax, m.h[i] * ax)], WELD: [],
                 BALL: [(E[k], 0 * E[k]) for k in range(3)], FREE: [(E[k], 0 * E[k]) for k in range(3)] + [(0 * E[k], E[k]) for k in range(3)]}[jt]
        for k, (sw, sv) in enumerate(local):
            w = R @ sw
            X[o + k] = (w, R @ sv + np.cross(p, w))
            body[o + k] = i
    return W, X, body


def jacobians(m, entries, q, v=None):
    """entries [(kind, body index, T_off 4 x 4 or None)]; q [N, n], v [N, n] or None -> (J [N, R, n], Jdot [N, R, n] or None)"""
    N = q.shape[0]
    W, X, body = kinematics(m, q)
    R = sum(ROWS[k] for k, _, _ in entries)
    J = np.zeros((N, R, m.n))
    Jd = np.zeros((N, R, m.n)) if v is not None else None
    if v is not None:                                        # world twists of the bodies
        V = []
        for i in range(m.nb):
            Vw, Vv = (V[m.parent[i]][0].copy(), V[m.parent[i]][1].copy()) if m.parent[i] >= 0 else (np.zeros((N, 3)), np.zeros((N, 3)))
            for d in range(m.off[i], m.off[i] + NDOF[m.jt[i]]):
                Vw, Vv = Vw + X[d][0] * v[:, d, None], Vv + X[d][1] * v[:, d, None]
            V.append((Vw, Vv))
    r = 0
    for kind, e, T in entries:
        nr = ROWS[kind]
        ra = r if kind != KIN_LINEAR else None
        rl = r + 3 if kind == KIN_SPATIAL else (r if kind == KIN_LINEAR else None)
        r += nr
        if e < 0:
            continue                                         # fixed in the world
        F = W[e] @ (np.eye(4) if T is None else np.asarray(T, dtype=np.float64))
        p = F[:, :3, 3]
        dofs = [d for i in m.ancestors(e) for d in range(m.off[i], m.off[i] + NDOF[m.jt[i]])]
        Jl = np.zeros((N, 3, m.n))
        for d in dofs:
            Jl[:, :, d] = X[d][1] + np.cross(X[d][0], p)
            if ra is not None:
                J[:, ra:ra + 3, d] = X[d][0]
        if rl is not None:
            J[:, rl:rl + 3] = Jl
        if v is None:
            continue
        pd = np.einsum("nrd,nd->nr", Jl, v)
        for d in dofs:
            Vw, Vv = V[body[d]]
            Xw, Xv = X[d]
            Xdw, Xdv = np.cross(Vw, Xw), np.cross(Vw, Xv) + np.cross(Vv, Xw)
            if ra is not None:
                Jd[:, ra:ra + 3, d] = Xdw
            if rl is not None:
                Jd[:, rl:rl + 3, d] = Xdv + np.cross(Xdw, p) + np.cross(Xw, pd)
    return J, Jd


def accel(m, entries, q, v, a=None):
    """xdd [N, R] = J a + Jdot v (a None: the bias acceleration Jdot v)"""
    J, Jd = jacobians(m, entries, q, v)
    out = np.einsum("nrd,nd->nr", Jd, v)
    if a is not None:
        out = out + np.einsum("nrd,nd->nr", J, a)
    return out


def _fd(f, xs, k, eps):
    """central differences of the scalar function f(*xs) -> [N] with respect to xs[k] [N, d]: [N, d], all steps in one batched call"""
    N, d = xs[k].shape
    rep = [np.repeat(x, 2 * d, axis=0) for x in xs]                     # world b, step j: row b * 2 d + j
    step = np.concatenate([np.eye(d), -np.eye(d)]) * eps
    rep[k] = rep[k] + np.tile(step, (N, 1))
    y = f(*rep).reshape(N, 2, d)
    return (y[:, 0] - y[:, 1]) / (2 * eps)


def fd_accel_vjp(m, entries, q, v, a, cot, eps):
    """(g_q, g_v, g_a) [N, n] each of <cot, xdd> (a None: of <cot, Jdot v>, g_a None) by central differences with the step eps"""
    if a is None:
        f = lambda q_, v_: np.einsum("nr,nr->n", np.repeat(cot, q_.shape[0] // cot.shape[0], axis=0), accel(m, entries, q_, v_))
        return _fd(f, [q, v], 0, eps), _fd(f, [q, v], 1, eps), None
    f = lambda q_, v_, a_: np.einsum("nr,nr->n", np.repeat(cot, q_.shape[0] // cot.shape[0], axis=0), accel(m, entries, q_, v_, a_))
    return tuple(_fd(f, [q, v, a], k, eps) for k in range(3))


def fd_jacobian_vjp(m, entries, q, G, eps):
    """g_q [N, n] of <G, J(q)>, G [N, R, n], by central differences with the step eps"""
    f = lambda q_: np.einsum("nrd,nrd->n", np.repeat(G, q_.shape[0] // G.shape[0], axis=0), jacobians(m, entries, q_)[0])
    return _fd(f, [q], 0, eps)
