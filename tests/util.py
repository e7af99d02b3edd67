"""Seeded synthetic inputs for the BASELINE.md configs (numpy default_rng(seed))."""
import numpy as np

import nimblephysics_amd as na


def rel_err(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-30))


def cfg_inputs(name, B, seed):
    """Returns (model_description, state[B,2n], action[B,k])."""
    rng = np.random.default_rng(seed)
    if name == "pendulum":  # cfg1
        md = na.single_pendulum()
        q = rng.uniform(-np.pi, np.pi, (B, 1)); v = rng.uniform(-1, 1, (B, 1)); a = rng.uniform(-1, 1, (B, 1))
    elif name == "cartpole":  # cfg2
        md = na.cartpole()
        q = np.stack([rng.uniform(-1, 1, B), rng.uniform(-np.pi / 2, np.pi / 2, B)], 1)
        v = rng.normal(0, 1, (B, 2))
        a = np.stack([rng.uniform(-10, 10, B), np.zeros(B)], 1)
    elif name in ("atlas33", "atlas20"):  # cfg3 (free fall, no ground)
        md = na.atlas(name)
        fl = md.merge_welds().flat()
        n = md.num_dofs
        q = np.zeros((B, n))
        q[:, 0:3] = rng.normal(0, 0.3, (B, 3)); q[:, 0] += -np.pi / 2
        lo, hi = fl["pos_lo"][6:], fl["pos_hi"][6:]
        q[:, 6:] = rng.uniform(0.2 * lo, 0.2 * hi, (B, n - 6))
        v = rng.normal(0, 0.1, (B, n))
        a = rng.normal(0, 1, (B, n))
    else:
        raise KeyError(name)
    return md, np.concatenate([q, v], 1), a


def contact_inputs(name, B, seed, joint_noise=0.002, vel_noise=0.001, action_noise=0.1):
    """Standing Atlas on the ground box (cfg5 / metric config pose: q[0] = -pi/2, q[4] = -0.01,
    unittests/unit/test_AtlasGradients.cpp:235-236) with small joint noise: both feet flat, 8 foot-corner
    contacts, contact stays in the sticking regime where the LCP warm start / guess is already valid."""
    rng = np.random.default_rng(seed)
    md = na.atlas(name, ground=True)
    n = md.num_dofs
    q = np.zeros((B, n)); q[:, 0] = -np.pi / 2; q[:, 4] = -0.01
    q[:, 6:] = rng.normal(0, joint_noise, (B, n - 6))
    v = rng.normal(0, vel_noise, (B, n))
    a = rng.normal(0, action_noise, (B, n))
    return md, np.concatenate([q, v], 1), a


def box_stack_inputs(B, seed, overhang=False):
    """cfg4: welded ground box + two FreeJoint cubes (0.2^3, mu = 1).  Default: box 2 stacked on box 1 with the same
    yaw and a small lateral offset -> 4 + 4 = 8 contacts (FACE_VERTEX below, EDGE_EDGE / FACE_VERTEX / VERTEX_FACE
    between the cubes), penetration 1e-4..1e-3.  overhang=True: one cube hanging over the rim of the ground box
    (EDGE_EDGE contacts against the world-fixed box, stage-0 regime), the other cube parked far above."""
    rng = np.random.default_rng(seed)
    md = na.box_stack()
    # geometry of the loaded model: top face of the ground box and the zero-configuration centres of the two cubes
    gb = md.boxes[0]
    top = (md.bodies[0].T_pj @ gb.T)[1, 3] + 0.5 * gb.size[1]
    c1, c2 = md.bodies[1].T_pj[:3, 3], md.bodies[2].T_pj[:3, 3]
    q = np.zeros((B, 12)); v = np.zeros((B, 12))
    pen1, pen2 = rng.uniform(1e-4, 1e-3, B), rng.uniform(1e-4, 1e-3, B)
    yaw = rng.uniform(-np.pi, np.pi, B)
    if overhang:
        q[:, 1] = yaw; q[:, 3] = rng.uniform(0.9, 0.99, B) * rng.choice([-1, 1], B) - c1[0]; q[:, 4] = top + 0.1 - pen1 - c1[1]; q[:, 5] = rng.uniform(-0.5, 0.5, B) - c1[2]
        q[:, 10] = 5.0
        v[:, 0:6] = rng.normal(0, 0.001, (B, 6))
    else:
        x1, z1 = rng.uniform(-0.3, 0.3, B), rng.uniform(-0.3, 0.3, B)
        q[:, 1] = yaw; q[:, 4] = top + 0.1 - pen1 - c1[1]; q[:, 3] = x1 - c1[0]; q[:, 5] = z1 - c1[2]
        off = rng.uniform(0.005, 0.03, (B, 2)) * rng.choice([-1, 1], (B, 2))
        c, s_ = np.cos(yaw), np.sin(yaw)
        q[:, 7] = yaw
        q[:, 9] = x1 + c * off[:, 0] + s_ * off[:, 1] - c2[0]; q[:, 11] = z1 - s_ * off[:, 0] + c * off[:, 1] - c2[2]
        q[:, 10] = top + 0.3 - pen1 - pen2 - c2[1]
        v[:, [3, 5, 9, 11]] = rng.normal(0, 0.05, (B, 4))
    a = np.zeros((B, 12))
    return md, np.concatenate([q, v], 1), a


# ---- sphere colliders (tests/test_oracle_spheres.py, tests/test_gpu_spheres.py) ----
def ball_world(order="box_first", n_balls=1, radius=0.1, arm=False):
    """Free-joint balls over a welded ground box (top face at y = 0)."""
    bodies, cols = [], []
    ground = na.BoxSpec(-1, na.make_transform((0, -0.5, 0)), (4.0, 1.0, 4.0), 1.0)
    for i in range(n_balls):
        I = 0.4 * 1.0 * radius * radius
        bodies.append(na.BodySpec(f"ball{i}", -1, "free", f"ball{i}_joint", mass=1.0, inertia=(I, I, I, 0, 0, 0)))
        cols.append(na.SphereSpec(i, np.eye(4), radius, 0.8))
    if arm:   # a revolute link carrying a second sphere, hinged on ball 0
        bodies.append(na.BodySpec("arm", 0, "revolute", "arm_joint", axis=(0, 0, 1), T_pj=na.make_transform((0.15, 0, 0)),
                                  T_cj=na.make_transform((-0.15, 0, 0)), mass=0.5, inertia=(0.002, 0.002, 0.002, 0, 0, 0)))
        cols.append(na.SphereSpec(len(bodies) - 1, np.eye(4), radius, 0.8))
    boxes = [ground] + cols if order == "box_first" else cols + [ground]
    return na.ModelDescription("balls", bodies, boxes, max_contacts=8)


# ---- self-collision (tests/test_oracle_self_collision.py, tests/test_gpu_self_collision.py) ----
def folding_arm(self_collision=True, tip="sphere", adjacent=False):
    """A planar three-link arm (revolute joints about z, links of 0.3 m along their x axes, a box on each of the first two links) whose last
    link folds back onto the FIRST one (q1 ~ 2.1, q2 ~ 1.9): a contact between two non-adjacent bodies of one skeleton, with joint 0 above
    both of them.  tip: the collider of the last link, "sphere" or "box"."""
    I = (0.002, 0.002, 0.002, 0, 0, 0)
    kw = dict(self_collision=self_collision, adjacent_body_check=adjacent)
    bodies = [na.BodySpec("l0", -1, "revolute", "j0", axis=(0, 0, 1), T_cj=na.make_transform((-0.15, 0, 0)), mass=1.0, inertia=I, **kw),
              na.BodySpec("l1", 0, "revolute", "j1", axis=(0, 0, 1), T_pj=na.make_transform((0.15, 0, 0)), T_cj=na.make_transform((-0.15, 0, 0)), mass=0.8, inertia=I, **kw),
              na.BodySpec("l2", 1, "revolute", "j2", axis=(0, 0, 1), T_pj=na.make_transform((0.15, 0, 0)), T_cj=na.make_transform((-0.15, 0, 0)), mass=0.6, inertia=I, **kw)]
    cols = [na.BoxSpec(0, np.eye(4), (0.3, 0.06, 0.06), 0.8), na.BoxSpec(1, np.eye(4), (0.3, 0.06, 0.06), 0.8),
            na.SphereSpec(2, na.make_transform((0.12, 0, 0)), 0.04, 0.8) if tip == "sphere" else na.BoxSpec(2, na.make_transform((0.1, 0, 0), rpy=(0.5, 0.3, 0.2)), (0.1, 0.06, 0.06), 0.8)]   # (tilted: no parallel edges)
    return na.ModelDescription("folding_arm", bodies, cols, gravity=(0, -9.81, 0), max_contacts=8)


# ---- joint-limit rows (tests/test_oracle_joint_limits.py, tests/test_gpu_joint_limits.py) ----
def limited_arm(enforce=True, ground=False, n_links=4, max_contacts=None):
    """A prismatic base (vertical slide) carrying a chain of revolute links with position limits [-0.5, 0.4]; every joint enforces its
    limits when `enforce`.  With `ground`: a ground box under it and a box collider on the base, which touches the ground for slide positions
    in (-0.03, 0] (contacts and limit rows in one LCP)."""
    bodies = [na.BodySpec("base", -1, "prismatic", "slide", axis=(0, 1, 0), mass=1.0, inertia=(0.01, 0.01, 0.01, 0, 0, 0), pos_lo=(-0.2,), pos_hi=(0.6,),
                          limit_enforced=enforce)]
    for k in range(n_links):
        bodies.append(na.BodySpec(f"link{k}", k, "revolute", f"hinge{k}", axis=(0, 0, 1) if k % 2 == 0 else (1, 0, 0),
                                  T_pj=na.make_transform((0.2 if k else 0.0, 0, 0)), T_cj=na.make_transform((-0.1, 0, 0)), mass=0.5,
                                  inertia=(0.002, 0.003, 0.004, 0, 0, 0), damping=(0.05,), pos_lo=(-0.5,), pos_hi=(0.4,), limit_enforced=enforce))
    boxes = []
    if ground:
        boxes = [na.BoxSpec(-1, na.make_transform((0, -0.55, 0)), (6.0, 1.0, 6.0), 1.0),
                 na.BoxSpec(0, np.eye(4), (0.2, 0.1, 0.2), 0.8)]
    # (with the ground: four corner contacts + up to five limit rows - more than 8 constraint slots: the 48-row build)
    return na.ModelDescription("limited_arm", bodies, boxes, max_contacts=max_contacts or (16 if ground else 8))


# ---- capsule colliders (tests/test_oracle_capsules.py, tests/test_gpu_capsules.py) ----
def capsule_world(order="fixed_first", kinds=("capsule",), radius=0.1, height=0.4):
    """Free-joint capsules (axis = their z, radius 0.1, cylinder height 0.4) / spheres (radius 0.1) over a world-fixed capsule of radius
    0.25 whose axis is the world's z axis through the origin (a capsule cannot meet a box: that pair is libccd's in the reference)."""
    bodies, cols = [], []
    ground = na.CapsuleSpec(-1, np.eye(4), 0.25, 3.0, 1.0)
    for i, kind in enumerate(kinds):
        I = 0.4 * radius * radius
        bodies.append(na.BodySpec(f"{kind}{i}", -1, "free", f"{kind}{i}_joint", mass=1.0, inertia=(I, I, 0.5 * I, 0, 0, 0)))
        cols.append(na.CapsuleSpec(i, np.eye(4), radius, height, 0.8) if kind == "capsule" else na.SphereSpec(i, np.eye(4), radius, 0.8))
    boxes = [ground] + cols if order == "fixed_first" else cols + [ground]
    return na.ModelDescription("capsules", bodies, boxes, max_contacts=8)


def ball_state(md, centres, seed, pen=2e-3, radius=0.1):
    rng = np.random.default_rng(seed)
    n = md.num_dofs
    q = np.zeros(n); v = rng.normal(0, 0.02, n)
    for i, (x, z) in enumerate(centres):
        q[6 * i + 0:6 * i + 3] = rng.normal(0, 0.3, 3)
        q[6 * i + 3] = x; q[6 * i + 4] = radius - pen; q[6 * i + 5] = z
    return np.concatenate([q, v]), rng.normal(0, 0.1, n)




# ---- random frictional-contact LCPs for the solver tests (host emulation and GPU self-test) ----
def contact_lcp(rng, nc, ndof, cfm=0.0):
    """A = J D J^T (+ cfm I) of nc frictional contacts on an ndof-DOF system (rank-deficient when ndof < 3 nc), random b,
    bounds as DantzigBoxedLcpSolver::solve receives them (friction rows: lo = -mu, hi = mu, findex = their normal row)."""
    n = 3 * nc
    J = rng.normal(0, 1, (n, ndof))
    A = J @ np.diag(rng.uniform(0.1, 2, ndof)) @ J.T + cfm * np.eye(n)
    b = rng.normal(0, 1, n) * rng.choice([1, 0.01])
    mu = rng.choice([0.5, 1.0], nc)
    lo = np.zeros(n); hi = np.full(n, np.inf); fi = np.full(n, -1, np.int32)
    for c in range(nc):
        for k in (1, 2):
            lo[3 * c + k] = -mu[c]; hi[3 * c + k] = mu[c]; fi[3 * c + k] = 3 * c
    return np.ascontiguousarray(A, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64), lo, hi, fi


class BoxedLcp(tuple):
    """What boxed_lcp returns: unpacks as (A, b, lo, hi, findex) - the problem in the DEVICE's slot layout - and carries the rest by name."""
    def __new__(cls, **kw):
        self = super().__new__(cls, (kw["A"], kw["b"], kw["lo"], kw["hi"], kw["findex"]))
        self.__dict__.update(kw)
        return self


def boxed_lcp(rng, n_contacts, n_box, ndof, n_limit=0, dofs=None, betas=None):
    """A boxed LCP with the three kinds of slot the general kernels carry, in the DEVICE's slot layout (three rows per slot): first the
    contacts [normal, t1, t2] (bounds as in contact_lcp), then n_box joint-friction slots - the fixed bounds [-beta, beta] and findex -1 on
    the first row, two EMPTY tangent rows -, then n_limit joint-limit slots - [0, inf) on the first row, two empty tangent rows; every
    second one is of the negated kind, (-inf, 0] in the reference's problem, which the device carries as the negated row.
    Physical: A = J M^-1 J^T with a random symmetric positive definite M (ndof x ndof), contact rows of J random, box and limit rows unit
    vectors e_d on DISTINCT DOFs (dofs: the DOF of every box / limit slot instead - repeats allowed, for the merge tests); b random with
    the scale mix of contact_lcp; a box row has b = -qdot_d, and beta = |b_d / A_dd| times 0.4 or 2.5 (betas: given instead), so that
    about half of them slide (alone such a row ends on a bound) and half stick (strictly inside).  Needs n_box + n_limit <= ndof.

    Returns a BoxedLcp: (A, b, lo, hi, findex) of the 3 * slots device rows (empty tangent rows: zero rows and columns of A, lo = hi = 0),
    and by name
      mu [slot], bound [slot] (beta, 0 on the other slots), lim [slot] (0, 1, 2 = negated): what the shims and the self-test take,
      lim_rows, neg_rows [row] (bytes): the same per row, as gen_shim.cpp's fillRows takes them,
      rows: the device rows that are rows of the reference's problem, in order (everything but the empty tangent rows) - and
      A_ref, b_ref, lo_ref, hi_ref, findex_ref: that compacted problem as the reference's functions get it (what genLoadProblem builds,
      up to the sign map),
      S [row] = -1 on the negated limit rows, +1 elsewhere: A = S A_ref' S, b = S b_ref', x_ref' = S x (' = scattered to the device rows);
      s_ref = S[rows]."""
    slots = n_contacts + n_box + n_limit
    m = 3 * slots
    n_pseudo = n_box + n_limit
    if dofs is None:
        assert n_pseudo <= ndof
        dofs = rng.choice(ndof, n_pseudo, replace=False)
    J = np.zeros((m, ndof))
    J[:3 * n_contacts] = rng.normal(0, 1, (3 * n_contacts, ndof))
    for k, d in enumerate(dofs):
        J[3 * (n_contacts + k), d] = 1.0
    G = rng.normal(0, 1, (ndof, ndof))
    M = G @ np.diag(rng.uniform(0.5, 5.0, ndof)) @ G.T / ndof + np.diag(rng.uniform(0.5, 2.0, ndof))
    A = J @ np.linalg.solve(M, J.T)
    A = 0.5 * (A + A.T)
    b = rng.normal(0, 1, m) * rng.choice([1, 0.01])
    mu = np.zeros(slots); bound = np.zeros(slots); lim = np.zeros(slots, np.uint8)
    mu[:n_contacts] = rng.choice([0.5, 1.0], n_contacts)
    for s in range(n_contacts, slots):
        r = 3 * s
        if s < n_contacts + n_box:
            k = s - n_contacts
            bound[s] = betas[k] if betas is not None else abs(b[r] / A[r, r]) * rng.choice([0.4, 2.5])
        else:
            lim[s] = 2 if (s - n_contacts - n_box) % 2 else 1
    return slots_lcp(A, b, mu, bound, lim)


def slots_lcp(A, b, mu, bound, lim):
    """The BoxedLcp (boxed_lcp) of 3 * slots device rows A, b and the per-slot description mu / bound / lim: bounds, findex, the rows of
    the reference's problem and that problem.  A slot with bound > 0 is a joint-friction slot, one with lim > 0 a joint-limit slot, every
    other one a contact (mu <= 1e-3: frictionless, its tangent rows empty like a pseudo-contact's)."""
    mu = np.where(np.asarray(mu, float) > 1e-3, mu, 0.0); bound = np.asarray(bound, float); lim = np.asarray(lim, np.uint8)
    slots = len(mu); m = 3 * slots
    A = np.array(A, dtype=np.float64); b = np.array(b, dtype=np.float64)
    pseudo = (bound > 0) | (lim > 0)
    mu = np.where(pseudo, 0.0, mu)
    lo = np.zeros(m); hi = np.zeros(m); fi = np.full(m, -1, np.int32)
    S = np.ones(m)
    keep = np.zeros(m, bool)
    for s in range(slots):
        r = 3 * s
        fi[r + 1] = fi[r + 2] = r
        keep[r] = True
        if mu[s] > 0:
            keep[r + 1] = keep[r + 2] = True
            lo[r + 1] = lo[r + 2] = -mu[s]; hi[r + 1] = hi[r + 2] = mu[s]
        else:                                          # empty tangent rows: not rows of the problem
            A[r + 1:r + 3, :] = 0.0; A[:, r + 1:r + 3] = 0.0; b[r + 1:r + 3] = 0.0
        if bound[s] > 0:
            lo[r] = -bound[s]; hi[r] = bound[s]
        else:
            hi[r] = np.inf
            if lim[s] == 2:
                S[r] = -1.0
    rows = np.where(keep)[0]
    lim_rows = np.zeros(m, np.uint8); neg_rows = np.zeros(m, np.uint8)
    lim_rows[0::3] = pseudo; neg_rows[0::3] = lim == 2
    # the reference's problem: the compacted rows, the negated limit rows in the reference's own sign ((-inf, 0])
    sr = S[rows]
    A_ref = np.ascontiguousarray(sr[:, None] * A[np.ix_(rows, rows)] * sr[None, :])
    b_ref = sr * b[rows]
    lo_ref = np.where(sr < 0, -hi[rows], lo[rows]) + 0.0
    hi_ref = np.where(sr < 0, -lo[rows], hi[rows]) + 0.0
    pos = {int(r): i for i, r in enumerate(rows)}
    fi_ref = np.array([-1 if fi[r] < 0 else pos[int(fi[r])] for r in rows], dtype=np.int32)
    return BoxedLcp(A=np.ascontiguousarray(A), b=np.ascontiguousarray(b), lo=lo, hi=hi, findex=fi, mu=np.ascontiguousarray(mu), bound=np.ascontiguousarray(bound),
                    lim=np.ascontiguousarray(lim), lim_rows=lim_rows, neg_rows=neg_rows, rows=rows, S=S, s_ref=sr, A_ref=A_ref, b_ref=np.ascontiguousarray(b_ref),
                    lo_ref=np.ascontiguousarray(lo_ref), hi_ref=np.ascontiguousarray(hi_ref), findex_ref=fi_ref)


def have_ref():
    """oracle/_ref (the reference's own Dantzig solver compiled from its vendored sources) is present."""
    import os
    import oracle
    return os.path.exists(os.path.join(os.path.dirname(oracle.__file__), "_ref", "libodelcp_ref.so"))


def duplicate_filter_scene(deep=4):
    """One free body carrying `deep` + 1 small boxes in a row above a ground plate: the first `deep` sit 0.05 deep in the ground (their
    four bottom corners are narrow-phase points that the depth filter drops - 0.03 is the clipping depth), the last one 0.01 deep (four
    contacts).  With deep = 4 the kept contacts arrive as distinct points 17..20 of the world: past the 16 the device's duplicate
    filter remembers (NBL_ST_CONTACT_OVERFLOW); with deep = 3 as points 13..16: no flag.  -> (model, state [1, 12], action [1, 6])."""
    import nimblephysics_amd as na
    I = (0.02, 0.02, 0.02, 0.0, 0.0, 0.0)
    bodies = [na.BodySpec("carrier", -1, "free", "root", mass=1.0, inertia=I)]
    boxes = [na.BoxSpec(-1, na.make_transform((0.0, -0.5, 0.0)), (10.0, 1.0, 10.0), 1.0)]
    for k in range(deep + 1):
        down = 0.05 if k < deep else 0.01
        boxes.append(na.BoxSpec(0, na.make_transform((0.3 * k, 0.05 - down, 0.0)), (0.1, 0.1, 0.1), 1.0))
    md = na.ModelDescription("duplicate_filter", bodies, boxes, gravity=(0.0, -9.81, 0.0), dt=1e-3, max_contacts=8)
    s = np.zeros((1, 12)); s[0, 1] = 0.01                        # a little yaw: no two corners share a coordinate
    return md, s, np.zeros((1, 6))


# ---- more than 8 contacts per world: the 48-row instantiation of the library (tests/test_gpu_contacts16.py) ----
def cube_world(n_cubes=3, max_contacts=16, side=0.2, mass=0.1, mu=1.0):
    """A welded ground plate (top face y = 0) and `n_cubes` FreeJoint cubes (zero configuration: centre at the origin)."""
    I = mass * side * side / 6.0
    bodies = [na.BodySpec(f"cube{i}", -1, "free", f"cube{i}_joint", mass=mass, inertia=(I, I, I, 0, 0, 0)) for i in range(n_cubes)]
    boxes = [na.BoxSpec(-1, na.make_transform((0, -0.5, 0)), (6.0, 1.0, 6.0), mu)]
    boxes += [na.BoxSpec(i, np.eye(4), (side, side, side), mu) for i in range(n_cubes)]
    return na.ModelDescription("cubes", bodies, boxes, gravity=(0.0, -9.81, 0.0), dt=1e-3, max_contacts=max_contacts)


def cube_tower_inputs(B, seed, n_cubes=3, side=0.2, **kw):
    """A tower of cubes on the ground plate: 4 contacts per interface (FACE_VERTEX / VERTEX_FACE / EDGE_EDGE between cubes of one yaw and a
    small lateral offset), 12 contacts with three cubes, 16 with four."""
    rng = np.random.default_rng(seed)
    md = cube_world(n_cubes, side=side, **kw)
    n = 6 * n_cubes
    q = np.zeros((B, n)); v = np.zeros((B, n))
    yaw = rng.uniform(-1.0, 1.0, B)
    x, z = rng.uniform(-0.3, 0.3, B), rng.uniform(-0.3, 0.3, B)
    c, s_ = np.cos(yaw), np.sin(yaw)
    y = np.zeros(B)
    for k in range(n_cubes):
        y = y + (0.5 * side if k == 0 else side) - rng.uniform(1e-4, 1e-3, B)
        off = (rng.uniform(0.005, 0.03, (B, 2)) * rng.choice([-1, 1], (B, 2))) if k else np.zeros((B, 2))
        x = x + c * off[:, 0] + s_ * off[:, 1]; z = z - s_ * off[:, 0] + c * off[:, 1]
        q[:, 6 * k + 1] = yaw; q[:, 6 * k + 3] = x; q[:, 6 * k + 4] = y; q[:, 6 * k + 5] = z
        v[:, [6 * k + 3, 6 * k + 5]] = rng.normal(0, 0.05, (B, 2))
    return md, np.concatenate([q, v], 1), np.zeros((B, n))


def table_inputs(B, seed, feet=4, max_contacts=16):
    """One free body standing on `feet` small boxes (4 contacts each: 16 with four feet), randomly pushed: 48 LCP rows of rank 6."""
    rng = np.random.default_rng(seed)
    I = (0.05, 0.08, 0.05, 0.0, 0.0, 0.0)
    bodies = [na.BodySpec("table", -1, "free", "root", mass=2.0, inertia=I)]
    boxes = [na.BoxSpec(-1, na.make_transform((0.0, -0.5, 0.0)), (10.0, 1.0, 10.0), 1.0)]
    corners = [(-0.3, -0.2), (0.3, -0.2), (-0.3, 0.2), (0.3, 0.2), (0.0, 0.0)][:feet]
    for (cx, cz) in corners:
        boxes.append(na.BoxSpec(0, na.make_transform((cx, 0.05, cz)), (0.1, 0.1, 0.1), 1.0))
    md = na.ModelDescription("table", bodies, boxes, gravity=(0.0, -9.81, 0.0), dt=1e-3, max_contacts=max_contacts)
    s = np.zeros((B, 12))
    s[:, 1] = rng.uniform(-1.0, 1.0, B)                                   # yaw
    s[:, 3] = rng.uniform(-1, 1, B); s[:, 5] = rng.uniform(-1, 1, B)
    s[:, 4] = -rng.uniform(1e-4, 2e-3, B)                                 # feet 0.1 .. 2 mm in the ground
    s[:, 6:] = rng.normal(0, 0.05, (B, 6)) * np.where(rng.random((B, 1)) < 0.7, 1.0, 0.02)   # most pushed / spun, some nearly at rest
    return md, s, rng.normal(0, 0.2, (B, 6))


# ---- the matrices the Householder route is there for (tests/test_coop_host.py, tests/test_gpu_pinv_selftest.py) ----
def friction_bound_contact_matrices(rng, R, trials, p_cls=(0.15, 0.6, 0.25)):
    """Q = A(c, c) + A(c, u) E of a robot standing on one or two flat feet (6-DOF bodies, inertias spread over 1e2), some friction rows on
    their bound folded into their normal's column: non-symmetric, R x R with the rows / columns outside the clamping set zero.  p_cls: the
    shares of not clamping / clamping / upper-bound rows.  Yields (trial, Q, rows in the clamping set, rank, cond) for the matrices
    with cond <= 1e8 (beyond it there is no clear gap between the singular values that count and round-off)."""
    NC = R // 3
    for trial in range(trials):
        nb = int(rng.integers(1, 3))                                   # one or two 6-DOF bodies
        J = np.zeros((R, 6 * nb))
        for cidx in range(NC):                                          # contact -> body, point on its sole
            bdy = int(rng.integers(0, nb)); pt = np.array([rng.uniform(-0.1, 0.1), 0.0, rng.uniform(-0.05, 0.05)])
            for ax in range(3):
                d = np.eye(3)[[1, 0, 2][ax]]
                J[3 * cidx + ax, 6 * bdy:6 * bdy + 3] = np.cross(pt, d); J[3 * cidx + ax, 6 * bdy + 3:6 * bdy + 6] = d
        Lam = np.zeros((6 * nb, 6 * nb))
        for bdy in range(nb):
            M = rng.normal(0, 1, (6, 6)); Lam[6 * bdy:6 * bdy + 6, 6 * bdy:6 * bdy + 6] = M @ np.diag(10 ** rng.uniform(-1, 1, 6)) @ M.T
        A = J @ Lam @ J.T
        cls = rng.choice([0, 1, 2], size=R, p=list(p_cls))             # not clamping / clamping / upper bound (friction rows only)
        cls[0::3] = np.where(cls[0::3] == 2, 1, cls[0::3])
        Q = np.zeros((R, R))
        cl = np.where(cls == 1)[0]
        if len(cl) == 0:
            continue
        Q[np.ix_(cl, cl)] = A[np.ix_(cl, cl)]
        for u in np.where(cls == 2)[0]:
            nrm = u - u % 3
            if cls[nrm] == 1:
                Q[cl, nrm] += rng.choice([-1.0, 1.0]) * rng.uniform(0.3, 1.0) * A[cl, u]
        sub = Q[np.ix_(cl, cl)]
        sv = np.linalg.svd(sub, compute_uv=False)
        k = int((sv > 1e-12 * sv[0]).sum())
        cond = sv[0] / sv[k - 1]
        if cond > 1e8:
            continue
        yield trial, Q, len(cl), k, cond


# ---- the saved record of a step (SavedLayout, csrc/model_dev.hpp / nimble_amd.hip) ----
def record_rows(world, saved, B, max_contacts=8, cr_size=22):
    """x, b, cls, cfm, pflag rows, the Delassus matrix A and the pinv block of the saved record of the 24- / 48-row builds, on the device."""
    import torch
    n = world.n
    max_rows = 3 * max_contacts
    rec = saved.view(torch.float64)
    x0 = 5 * n + 1 + max_contacts * cr_size
    b0, cls0, cfm0 = x0 + max_rows, x0 + 2 * max_rows, x0 + 3 * max_rows
    pflag0 = x0 + 4 * max_rows
    total = pflag0 + 1 + max_contacts
    pinv_off = max_rows * max_rows + 2 * n * max_rows
    dense = pinv_off + max_rows * max_rows
    rows = rec[: total * B].view(total, B)
    blocks = rec[total * B: total * B + B * dense].view(B, dense)
    pflag = rows[pflag0]
    pinv = torch.where((pflag != 0)[:, None], blocks[:, pinv_off:pinv_off + max_rows * max_rows], torch.zeros((), dtype=torch.float64, device=rec.device))
    return {"nc": rows[5 * n], "x": rows[x0:x0 + max_rows].t(), "b": rows[b0:b0 + max_rows].t(), "cls": rows[cls0:cls0 + max_rows].t(),
            "cfm": rows[cfm0:cfm0 + max_rows].t(), "contacts": rows[5 * n + 1:x0].t(), "A": blocks[:, :max_rows * max_rows],
            "pflag": pflag, "pinv": pinv}       # (pinv of a world without the flag is whatever the buffer held: zeroed)
