"""NumPy restatement of the gradient convention of nbl_ik_solve_vjp (include/nimble_amd.h; not product code): for one world, with J the
dense position Jacobian [P, n] at q and F the coordinates NOT left bit for bit on a finite limit,
    grad_t = J_F (J_F^T J_F + mu I)^-1 g_F  =  (J_F J_F^T + mu I)^-1 J_F g_F
by numpy.linalg.solve on BOTH forms.  The two agree in exact arithmetic; how far they disagree in floating point on given inputs is the
yardstick the tests hold the product to (it factors the smaller one with its own summation order)."""
import numpy as np


def free_set(q, lo, hi):
    """boolean [n]: True where the coordinate is free"""
    q, lo, hi = np.asarray(q), np.asarray(lo), np.asarray(hi)
    clamped = ((q == lo) & np.isfinite(lo)) | ((q == hi) & np.isfinite(hi))
    return ~clamped


def vjp_primal(J, g, free, mu):
    """J_F (J_F^T J_F + mu I)^-1 g_F: the |F| x |F| form"""
    JF, gF = J[:, free], g[free]
    if JF.shape[1] == 0:
        return np.zeros(J.shape[0])
    return JF @ np.linalg.solve(JF.T @ JF + mu * np.eye(JF.shape[1]), gF)


def vjp_dual(J, g, free, mu):
    """(J_F J_F^T + mu I)^-1 J_F g_F: the P x P form"""
    JF, gF = J[:, free], g[free]
    if JF.shape[1] == 0:
        return np.zeros(J.shape[0])
    return np.linalg.solve(JF @ JF.T + mu * np.eye(J.shape[0]), JF @ gF)


def vjp_batch(J, g, q, lo, hi, mu):
    """J [B, P, n], g, q [B, n] -> (primal [B, P], dual [B, P], free_count [B], cond(J_F) [B] (0 where |F| = 0))"""
    B = J.shape[0]
    pr, du = np.zeros((B, J.shape[1])), np.zeros((B, J.shape[1]))
    cnt, cond = np.zeros(B, dtype=np.int32), np.zeros(B)
    for b in range(B):
        f = free_set(q[b], lo, hi)
        cnt[b] = int(f.sum())
        pr[b], du[b] = vjp_primal(J[b], g[b], f, mu), vjp_dual(J[b], g[b], f, mu)
        if cnt[b]:
            s = np.linalg.svd(J[b][:, f], compute_uv=False)
            cond[b] = s[0] / s[-1] if s[-1] > 0 else np.inf
    return pr, du, cnt, cond
