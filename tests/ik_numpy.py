"""A numpy statement of the reference's inverse kinematics, for the IK tests (not product code):

  refine_ik / solve_ik   math::refineIK / math::solveIK (dart/math/IKSolver.cpp:291-493, 195-289), line by line, including the reference's
                         choice of the LARGER normal matrix (J J^T + lambda I when n < P, J^T J + lambda I otherwise), factored with
                         numpy.linalg.cholesky;
  clamp_positions        Skeleton::clampPositionsToLimits (dart/dynamics/Skeleton.cpp:3642-3740), line by line, with its 2 pi candidate
                         loops and its selection loop as they lie (Euler, universal and planar-rotation coordinates are revolute joints
                         of this model);
  Problem                IKMapping::setPositions' callbacks (dart/neural/IKMapping.cpp:99-112) on kin_numpy.mapping_rows.
"""
import numpy as np

from kin_numpy import dof_offsets, mapping_rows


class IKConfig:
    def __init__(self, convergence_threshold=1e-7, max_step_count=100, least_squares_damping=0.01, start_clamped=False,
                 line_search=True, dont_exit_transpose=False):
        self.convergence_threshold, self.max_step_count, self.least_squares_damping = convergence_threshold, max_step_count, least_squares_damping
        self.start_clamped, self.line_search, self.dont_exit_transpose = start_clamped, line_search, dont_exit_transpose

    def with_steps(self, k):
        return IKConfig(self.convergence_threshold, k, self.least_squares_damping, self.start_clamped, self.line_search, self.dont_exit_transpose)


def logmap_full(R):
    """math::logMap (Geometry.cpp:720-) with its branch near pi (kin_numpy.logmap states the regular branch only)"""
    c = min(max(0.5 * (np.trace(R) - 1.0), -1.0), 1.0)
    th = np.arccos(c)
    if th > np.pi - 1e-6:
        delta = 0.5 + 0.125 * (np.pi - th) ** 2
        a, b, d = (th * np.sqrt(1.0 + (R[k, k] - 1.0) * delta) for k in range(3))
        return np.array([a if R[2, 1] > R[1, 2] else -a, b if R[0, 2] > R[2, 0] else -b, d if R[1, 0] > R[0, 1] else -d])
    alpha = 0.5 * th / np.sin(th) if th > 1e-6 else 0.5 + th * th / 12.0
    return alpha * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])


def expmaprot(q):
    th = np.linalg.norm(q)
    S = np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]])
    A, B = (1.0, 0.5) if th < 1e-3 else (np.sin(th) / th, (1 - np.cos(th)) / th ** 2)
    return np.eye(3) + A * S + B * S @ S


def clamp_positions(md, q):
    """Skeleton::clampPositionsToLimits on the coordinates q of md (a ModelDescription without welds)"""
    q = np.array(q, dtype=np.float64)
    flat = md.flat()
    lo_all, hi_all = flat["pos_lo"], flat["pos_hi"]
    offs = dof_offsets(md)
    for i, b in enumerate(md.bodies):
        nd = {"free": 6, "ball": 3, "weld": 0}.get(b.joint_type, 1)
        for k in range(nd):
            d = offs[i] + k
            lo, hi = lo_all[d], hi_all[d]
            if b.joint_type == "revolute":                       # wrapByTwoPi
                poses = []
                clamped = q[d]
                poses.append(clamped)
                while clamped > hi:
                    clamped -= 2 * np.pi
                    poses.append(clamped)
                while clamped < lo:
                    clamped += 2 * np.pi
                    poses.append(clamped)
                lowest = np.inf
                for pos in poses:
                    if lo <= clamped <= hi:                      # (the reference tests clampedPos, the LAST candidate, here ...
                        q[d] = pos
                        break
                    elif clamped > hi:                           # ... and here)
                        violation = clamped - hi
                        if violation < lowest:
                            q[d] = pos
                            lowest = violation
                    elif clamped < lo:
                        violation = lo - pos
                        if violation < lowest:
                            q[d] = pos
                            lowest = violation
            if q[d] > hi:
                q[d] = hi
            if q[d] < lo:
                q[d] = lo
    for i, b in enumerate(md.bodies):
        if b.joint_type in ("free", "ball"):
            o = offs[i]
            q[o:o + 3] = logmap_full(expmaprot(q[o:o + 3]))
    return q


def refine_ik(initial, set_pos_and_clamp, evaluate, cfg):
    """math::refineIK -> dict(pos, loss, clamped, evals)"""
    pos = np.array(initial, dtype=np.float64)
    last_error = np.inf
    lr = 1.0
    use_transpose = False
    clamp = bool(cfg.start_clamped)
    pos = set_pos_and_clamp(pos, clamp)
    last_pos = pos.copy()
    evals = 0
    for i in range(cfg.max_step_count):
        if i > cfg.max_step_count - 5:
            clamp = True
        diff, J = evaluate(pos)
        evals += 1
        current = float(diff @ diff)
        if i > 0:
            change = current - last_error
            if current < 1e-21:
                last_error = current
                break
            if change > 0:
                lr *= 0.5
                if lr < 1e-4:
                    use_transpose = True
                elif not cfg.dont_exit_transpose:
                    use_transpose = False
                if cfg.line_search:
                    pos = set_pos_and_clamp(last_pos, clamp)
                if lr < 1e-10:
                    last_error = current
                    break
            elif change > -cfg.convergence_threshold:
                if not use_transpose:
                    if lr > 5e-5:
                        lr = 5e-5
                    use_transpose = True
                elif not clamp:
                    clamp = True
                else:
                    break
            else:
                lr *= 1.1
                last_error = current
        if use_transpose:
            delta = J.T @ diff
        else:
            lam = cfg.least_squares_damping
            assert lam != 0
            if J.shape[1] < J.shape[0]:
                L = np.linalg.cholesky(J @ J.T + lam * np.eye(J.shape[0]))
                delta = J.T @ np.linalg.solve(L.T, np.linalg.solve(L, diff))
            else:
                L = np.linalg.cholesky(J.T @ J + lam * np.eye(J.shape[1]))
                delta = np.linalg.solve(L.T, np.linalg.solve(L, J.T @ diff))
        last_pos = pos.copy()
        pos = set_pos_and_clamp(pos - (lr * delta), clamp)
    return {"pos": pos, "loss": last_error, "clamped": clamp, "evals": evals}


def solve_ik(initial, set_pos_and_clamp, evaluate, cfg, restart=None):
    """math::solveIK with maxRestarts = 1 -> dict(pos: refineIK's final positions, loss: what solveIK returns (the restart phase's),
    final_loss: the squared error at pos, steps: eval calls of both phases).  restart: a cached result of the 20-step phase."""
    initial = np.array(initial, dtype=np.float64)
    best_error, best = np.inf, initial
    pos = set_pos_and_clamp(initial, bool(cfg.start_clamped))
    r1 = restart if restart is not None else refine_ik(pos, set_pos_and_clamp, evaluate, cfg.with_steps(20))
    if r1["loss"] < best_error and (r1["clamped"] or not np.isfinite(best_error)):
        best_error, best = r1["loss"], r1["pos"]
    set_pos_and_clamp(best, True)
    r2 = refine_ik(best, set_pos_and_clamp, evaluate, cfg)
    d, _ = evaluate(r2["pos"])
    return {"pos": r2["pos"], "loss": best_error, "final_loss": float(d @ d), "steps": r1["evals"] + r2["evals"], "restart": r1}


class _CachedTransforms:
    """kin_numpy asks the oracle for a body's world transform several times per evaluation: keep them per q"""

    def __init__(self, ow):
        self._ow, self._key, self._T = ow, None, {}

    def body_world_transform(self, q, body):
        key = np.asarray(q).tobytes()
        if key != self._key:
            self._key, self._T = key, {}
        if body not in self._T:
            self._T[body] = self._ow.body_world_transform(q, body)
        return self._T[body]


class Problem:
    """setPositions' callbacks for the entries [(kind, body index of md)] of the model md (no welds) and one target [P]"""

    def __init__(self, ow, md, entries, target):
        self.ow, self.md, self.entries, self.target = _CachedTransforms(ow), md, entries, np.asarray(target, dtype=np.float64)

    def rows(self, q):
        return mapping_rows(self.ow, self.md, np.asarray(q, dtype=np.float64), self.entries)[0]

    def evaluate(self, q):
        pos, Jp, _ = mapping_rows(self.ow, self.md, np.asarray(q, dtype=np.float64), self.entries)
        return pos - self.target, Jp

    def set_pos_and_clamp(self, q, clamp):
        return clamp_positions(self.md, q) if clamp else np.array(q, dtype=np.float64)

    def solve(self, init, cfg, restart=None):
        return solve_ik(init, self.set_pos_and_clamp, self.evaluate, cfg, restart)
