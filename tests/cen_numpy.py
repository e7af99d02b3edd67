"""A numpy statement of the centre-of-mass family (Skeleton::getCOM, getCOMLinearVelocity, getCOMLinearAcceleration, getCOMLinearJacobian,
computeKineticEnergy, computePotentialEnergy; BodyNode::getLinearMomentum / getAngularMomentum summed over a set of bodies) for the tests
of csrc/centroidal_dev.hpp (not product code).

Built on three things only: OracleWorld.body_world_transform for the body frames, kin_numpy.joint_screws for the world screws of every
coordinate (the columns of kin_numpy.body_jacobians), and the description's masses, local centres of mass and inertias.  Everything is
written in WORLD coordinates about the world origin - the device code works in body frames - and on the description as it stands: a
welded body is its own body here, with its own mass (the device model merged it into its parent).

  com      = sum m (p + R c) / M                      Jcom = sum m (Jlin - [R c]x Jang) / M            com_vel = Jcom v
  momentum = [sum R I R^T w + m (x - com) x xdot;  sum m xdot]        (x = p + R c, w = Jang v, xdot = Jx v)
  ke       = v^T M v / 2 (OracleWorld.mass_matrix; the whole model)  and  sum m |xdot|^2 / 2 + w^T R I R^T w / 2 (any set): the two routes
             whose disagreement is the measured floor of ke
  pe       = -sum m g . x  (body origin rule: -sum m g . p)  + sum_d k_d (q_d - rest_d)^2 / 2 over the coordinates of the set's joints
  com_acc  = sum m xddot / M with the spatial acceleration of every body in world coordinates,
             A = sum_d s_d a_d + ad(V_body(d), s_d) v_d  (a screw moves with the child body of its joint), and
             xddot = A.lin + A.ang x x + w x (V.lin + w x x): the classical acceleration of the body-fixed point x.  No gravity.
Closed-form gradients: d com / dq from the position screws (d x / dq_d = pv + pw x x), d ke / dv = M v, d ke / dq = jac_Mx(q, v)^T v / 2;
everything else by central differences of these functions (fd_vjp)."""
import numpy as np

from kin_numpy import _ndof, dof_offsets, joint_screws, skew


def _inertia(b):
    xx, yy, zz, xy, xz, yz = (float(x) for x in b.inertia)
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def default_set(md):
    """every body that is not welded (through other welds) to the world"""
    out = []
    for i, b in enumerate(md.bodies):
        c = i
        while c >= 0 and md.bodies[c].joint_type == "weld":
            c = md.bodies[c].parent
        if c >= 0:
            out.append(i)
    return out


def set_dofs(md, sel):
    off = dof_offsets(md)
    return [off[i] + k for i in sel for k in range(_ndof(md.bodies[i]))]


class Kin:
    """frames and screws of every body of `sel` and of its ancestors at the positions q"""

    def __init__(self, ow, md, q, sel):
        self.md, self.sel, self.n = md, list(sel), md.num_dofs
        self.q = np.asarray(q, dtype=np.float64)
        self._jac = {}
        need = set()
        for i in self.sel:
            c = i
            while c >= 0 and c not in need:
                need.add(c)
                c = md.bodies[c].parent
        self.W = {i: ow.body_world_transform(self.q, i) for i in need}
        self.screws = {i: joint_screws(ow, md, self.q, i) for i in need}
        self.m = {i: float(md.bodies[i].mass) for i in self.sel}
        self.M = sum(self.m.values())
        self.x = {i: self.W[i][:3, 3] + self.W[i][:3, :3] @ np.asarray(md.bodies[i].com, dtype=np.float64) for i in self.sel}
        self.Iw = {i: self.W[i][:3, :3] @ _inertia(md.bodies[i]) @ self.W[i][:3, :3].T for i in self.sel}

    def path(self, i):
        out = []
        while i >= 0:
            out.append(i)
            i = self.md.bodies[i].parent
        return out

    def jac(self, i, position=False):
        """(Jang [3][n], Jlin at the world origin [3][n]) of body i from the velocity (position) screws"""
        if (i, position) in self._jac:
            return self._jac[(i, position)]
        Ja, Jl = np.zeros((3, self.n)), np.zeros((3, self.n))
        for c in self.path(i):
            for d, ps, vs in self.screws[c]:
                w, v = ps if position else vs
                Ja[:, d], Jl[:, d] = w, v
        self._jac[(i, position)] = (Ja, Jl)
        return Ja, Jl

    def jx(self, i, position=False):
        """Jacobian of the body's centre of mass x_i"""
        Ja, Jl = self.jac(i, position)
        return Jl - skew(self.x[i]) @ Ja

    def com(self):
        return sum(self.m[i] * self.x[i] for i in self.sel) / self.M

    def jcom(self, position=False):
        return sum(self.m[i] * self.jx(i, position) for i in self.sel) / self.M

    def momentum(self, v):
        c = self.com()
        L, P = np.zeros(3), np.zeros(3)
        for i in self.sel:
            Ja, _ = self.jac(i)
            w, xd = Ja @ v, self.jx(i) @ v
            L += self.Iw[i] @ w + self.m[i] * np.cross(self.x[i] - c, xd)
            P += self.m[i] * xd
        return np.concatenate([L, P])

    def ke_bodies(self, v):
        e = 0.0
        for i in self.sel:
            Ja, _ = self.jac(i)
            w, xd = Ja @ v, self.jx(i) @ v
            e += 0.5 * self.m[i] * xd @ xd + 0.5 * w @ self.Iw[i] @ w
        return e

    def pe(self, gravity, at_com=True, springs=True):
        g = np.asarray(gravity, dtype=np.float64)
        e = -sum(self.m[i] * g @ (self.x[i] if at_com else self.W[i][:3, 3]) for i in self.sel)
        if springs:
            fl = self.md.flat()
            for d in set_dofs(self.md, self.sel):
                e += 0.5 * fl["spring"][d] * (self.q[d] - fl["rest"][d]) ** 2
        return e

    def com_acc(self, v, a):
        V, A = {}, {}

        def twist(i):
            if i in V:
                return
            p = self.md.bodies[i].parent
            if p >= 0:
                twist(p)
                Vw, Vv, Aw, Av = V[p][0].copy(), V[p][1].copy(), A[p][0].copy(), A[p][1].copy()
            else:
                Vw, Vv, Aw, Av = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3)
            for d, _, (sw, sv) in self.screws[i]:
                Vw, Vv = Vw + sw * v[d], Vv + sv * v[d]
            for d, _, (sw, sv) in self.screws[i]:                       # the screws move with THIS body: sdot = ad(V_i, s)
                Aw = Aw + sw * a[d] + np.cross(Vw, sw) * v[d]
                Av = Av + sv * a[d] + (np.cross(Vw, sv) + np.cross(Vv, sw)) * v[d]
            V[i], A[i] = (Vw, Vv), (Aw, Av)

        out = np.zeros(3)
        for i in self.sel:
            twist(i)
            (w, vo), (al, ao), x = V[i], A[i], self.x[i]
            out += self.m[i] * (ao + np.cross(al, x) + np.cross(w, vo + np.cross(w, x)))
        return out / self.M


def outputs(ow, md, sel, q, v, a, at_com=True, springs=True, kin=None):
    """every output of the device code for one world, as a dict (kin: the Kin of these positions, if the caller has it)"""
    k = kin if kin is not None else Kin(ow, md, q, sel)
    J = k.jcom()
    return {"com": k.com(), "com_vel": J @ v, "com_acc": k.com_acc(v, a), "momentum": k.momentum(v), "ke": np.array([k.ke_bodies(v)]),
            "pe": np.array([k.pe(md.gravity, at_com, springs)]), "Jcom": J, "mass": k.M}


ORDER = ("com", "com_vel", "com_acc", "momentum", "ke", "pe")


def fd_vjp(ow, md, sel, q, v, a, cot, eps, at_com=True, springs=True):
    """{output: gradient [3n] of <cot[output], output> to (q, v, a)} by central differences of `outputs` with the step eps"""
    n = md.num_dofs
    x0 = np.concatenate([q, v, a])
    out = {k: np.zeros(3 * n) for k in ORDER}
    base = Kin(ow, md, q, sel)                                     # a step in v or a leaves the frames and screws where they are
    for j in range(3 * n):
        xp, xm = x0.copy(), x0.copy()
        xp[j] += eps
        xm[j] -= eps
        kin = base if j >= n else None
        fp = outputs(ow, md, sel, xp[:n], xp[n:2 * n], xp[2 * n:], at_com, springs, kin)
        fm = outputs(ow, md, sel, xm[:n], xm[n:2 * n], xm[2 * n:], at_com, springs, kin)
        for k in ORDER:
            out[k][j] = cot[k] @ (fp[k] - fm[k]) / (2 * eps)
    return out


def closed_form_vjp(ow, md, sel, q, v, cot, whole_model):
    """the gradients the oracle and the position screws give in closed form: com -> q, com_vel -> v, com_acc -> a, pe -> q (at the centres
    of mass, with springs) and - for the whole model - ke -> q, v"""
    n = md.num_dofs
    k = Kin(ow, md, q, sel)
    Jp, Jv = k.jcom(position=True), k.jcom()
    fl = md.flat()
    gpe = -k.M * Jp.T @ np.asarray(md.gravity, dtype=np.float64)
    for d in set_dofs(md, sel):
        gpe[d] += fl["spring"][d] * (q[d] - fl["rest"][d])
    out = {"com_q": Jp.T @ cot["com"], "com_vel_v": Jv.T @ cot["com_vel"], "com_acc_a": Jv.T @ cot["com_acc"], "pe_q": cot["pe"][0] * gpe}
    if whole_model:
        out["ke_v"] = cot["ke"][0] * (ow.mass_matrix(q) @ v)
        out["ke_q"] = cot["ke"][0] * 0.5 * (ow.jac_Mx(q, v).T @ v)
    return out
