"""The reference of the inertia-parameter gradients of the dynamics calls (tests/test_dynamics_mass_host.py, tests/test_gpu_dynamics_mass.py).

Inverse dynamics is linear in every body's spatial inertia G, and G is linear in the mass (INERTIA_MASS rescales the moments with it) and
in the moment entries and quadratic in the centre of mass: central differences of the CPU oracle's
    ID_o(q, v, a; theta) = ow.mass_matrix(q) @ a + ow.coriolis_gravity(q, v)
are exact up to rounding at ANY step size,
    D_p(q, v, a) = [ID_o(theta + h_p e_p) - ID_o(theta - h_p e_p)] / (2 h_p),
with the steps h_p of STEPS below.  A perturbed moment need not stay positive definite: ID_o factors nothing.  The joint-force terms of
NBL_ID_JOINT_FORCES do not depend on the inertias, so D is the same with and without them.  For forward dynamics the reference is the
identity  d a / d theta = -M_o^-1 D(q, v, a)  at a = the forward dynamics' own result: no differencing of a nonlinear function."""
import copy

import numpy as np

from nimblephysics_amd.mass import WithRespectToMass, WrtMassBodyNodeEntryType as T
from oracle import OracleWorld

NO_VELOCITY, NO_GRAVITY, JOINT_FORCES = 1, 2, 4          # NBL_ID_* of include/nimble_amd.h
TOL = 1e-10                                               # max|x - ref| / max(1, |ref|): tests/test_dynamics_host.py, tests/test_fdyn_host.py
H_AGREE = 1e-11                                           # D at h and at h / 2 agree to this times max(1, |D|)
STEP_COM, STEP_DIAG, STEP_OFF, STEP_MASS_REL = 0.02, 0.01, 0.005, 0.25
ALL_TYPES = (T.INERTIA_MASS, T.INERTIA_COM, T.INERTIA_COM_MU, T.INERTIA_DIAGONAL, T.INERTIA_OFF_DIAGONAL, T.INERTIA_FULL)


def _steps(md, entries):
    out = []
    for body, t in entries:
        m = float(md.bodies[body].mass)
        out += {T.INERTIA_MASS: [STEP_MASS_REL * m], T.INERTIA_COM: [STEP_COM] * 3, T.INERTIA_COM_MU: [STEP_COM], T.INERTIA_DIAGONAL: [STEP_DIAG] * 3,
                T.INERTIA_OFF_DIAGONAL: [STEP_OFF] * 3, T.INERTIA_FULL: [STEP_MASS_REL * m] + [STEP_COM] * 3 + [STEP_DIAG] * 3 + [STEP_OFF] * 3}[T(t)]
    return np.asarray(out)


def _index(md, body):
    return [b.name for b in md.bodies].index(body) if isinstance(body, str) else int(body)


def rel(x, ref):
    return float(np.abs(np.asarray(x) - np.asarray(ref)).max() / max(1.0, np.abs(ref).max())) if np.size(ref) else 0.0


class InertiaReference:
    """D, and the oracle at theta itself, for the model `md` with `entries` = [(body, entry type), ...] registered in that order at the
    model's CURRENT values.  The perturbed oracle worlds are built once and kept."""

    def __init__(self, md, entries):
        self.md = copy.deepcopy(md)
        self.entries = [(_index(md, b), T(t)) for b, t in entries]
        self.x0 = self._wrt(self.md).get()
        self.h = _steps(self.md, self.entries)
        self.P = self.x0.shape[0]
        self._worlds = {}

    def _wrt(self, md):
        w = WithRespectToMass(md)
        for b, t in self.entries:
            w.registerNode(b, t)
        return w

    def world(self, nograv=False, p=None, step=0.0):
        """the oracle at theta + step e_p (p None: at theta), with or without gravity"""
        key = (bool(nograv), p, float(step))
        if key not in self._worlds:
            md = copy.deepcopy(self.md)
            if nograv:
                md.gravity = (0.0, 0.0, 0.0)
            if p is not None:
                x = self.x0.copy()
                x[p] += step
                self._wrt(md).set(x)
            self._worlds[key] = OracleWorld(md)
        return self._worlds[key]

    @staticmethod
    def _id(ow, q, v, a):
        tau = ow.coriolis_gravity(q, v)
        return tau if a is None else tau + ow.mass_matrix(q) @ a

    def D(self, q, v, a, flags=0, scale=1.0):
        """[n, P]: d ID / d theta at (q, v, a) under the NBL_ID_* flags; a None: the Coriolis-and-gravity vector's"""
        v = np.zeros_like(q) if flags & NO_VELOCITY else v
        ng = bool(flags & NO_GRAVITY)
        cols = []
        for p in range(self.P):
            h = scale * self.h[p]
            cols.append((self._id(self.world(ng, p, +h), q, v, a) - self._id(self.world(ng, p, -h), q, v, a)) / (2 * h))
        return np.stack(cols, 1) if cols else np.zeros((q.shape[0], 0))

    def checked_D(self, q, v, a, flags=0):
        """D after the condition on the reference alone: the quotients at h and at h / 2 agree to H_AGREE max(1, |D|)"""
        D, D2 = self.D(q, v, a, flags), self.D(q, v, a, flags, 0.5)
        gap = np.abs(D - D2).max() if D.size else 0.0
        assert gap <= H_AGREE * max(1.0, np.abs(D).max() if D.size else 0.0), ("the reference disagrees with itself", gap, np.abs(D).max())
        return D

    def fd_jacobian(self, q, v, a, flags=0):
        """[n, P]: d a / d theta = -M_o^-1 D(q, v, a), a = the forward dynamics' result"""
        return -np.linalg.solve(self.world().mass_matrix(q), self.checked_D(q, v, a, flags))


def pick_entries(md, k):
    """Up to three bodies of `md` - the root-most, a leaf, one in a ball or free chain where the model has one - with one entry type each;
    model number k takes the types 3 k, 3 k + 1, 3 k + 2 (mod 6), so two consecutive models cover all six."""
    targets, _ = md.weld_targets()
    live = [i for i in range(len(md.bodies)) if targets[i] >= 0]
    parents = {b.parent for b in md.bodies}
    root = live[0]
    leaf = [i for i in live if i not in parents][-1]
    chain = [i for i in live if md.bodies[i].joint_type == "ball" or (md.bodies[i].joint_type == "free" and md.bodies[i].parent >= 0)]
    bodies = [root]
    for i in [leaf] + chain[:1]:
        if i not in bodies:
            bodies.append(i)
    return [(b, ALL_TYPES[(3 * k + j) % 6]) for j, b in enumerate(bodies)]


def on_the_mu_line(md, entries):
    """A copy of `md` in which every INERTIA_COM_MU body has its centre of mass ON the line beta mu the entry moves it along (COM = beta mu,
    WithRespectToMass.cpp:76-92): elsewhere set(get()) already moves the body, and the entry has no derivative AT the model's values
    (tests/test_gpu_mass.py prepares its COM_MU body the same way)."""
    md = copy.deepcopy(md)
    for body, t in entries:
        if T(t) == T.INERTIA_COM_MU:
            b = md.bodies[_index(md, body)]
            k = 0 if b.beta[0] != 0 else (1 if b.beta[1] != 0 else 2)
            mu = float(b.com[k]) / float(b.beta[k])
            b.com = tuple(float(be) * mu for be in b.beta)
    return md
