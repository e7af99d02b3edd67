"""A literal numpy restatement of Skeleton::getContactInverseDynamics and Skeleton::getMultipleContactInverseDynamics
(dart/dynamics/Skeleton.cpp:9705-9949), for tests/test_wrench_host.py.  Test harness only.

Inputs are what the reference computes first: `jacs` [6 E, n], the stacked LOCAL Jacobians getJacobian(body) of the contact bodies,
`tau_plain` [n] = massTorques + coriolisAndGravity (with the damping and spring forces), and `root`, the six columns of the free root joint
(the reference's head<6>()).  The 6 x 6 solve and the nearest mode go through numpy.linalg.lstsq (the reference: Eigen's complete orthogonal
decomposition, the minimum-norm least-squares solution as well), the min-torque mode through a QR solve of the full KKT matrix
(the reference: householderQr().solve).  `*_normal` are the normal-equations closed forms of the same answers, the second numpy route the
tests measure the first against."""
import numpy as np

EPS = 0.01                                   # the weight of the forces in the min-torque QP (Skeleton.cpp:9899)


def _finish(jacs, tau_plain, root, W):
    tau = tau_plain - jacs.T @ W             # contactTorques = jacs^T correctedForces
    tau[root] = 0.0                          # jointTorques.head<6>().setZero()
    return W, tau


def contact_inverse_dynamics(jac, tau_plain, root):
    """getContactInverseDynamics: one body, jac [6, n] -> (wrench [6], joint torques [n])"""
    jacBlock = jac[:, root].T
    rootTorque = tau_plain[root]
    W = np.linalg.lstsq(jacBlock, rootTorque, rcond=None)[0]
    return _finish(jac, tau_plain, root, W)


def weights(E):
    B = np.eye(6 * E)
    for i in range(E):
        B[6 * i + 3, 6 * i + 3] = B[6 * i + 4, 6 * i + 4] = B[6 * i + 5, 6 * i + 5] = EPS
    return B


def multiple_contact_inverse_dynamics(jacs, tau_plain, root, guesses=None):
    """getMultipleContactInverseDynamics: jacs [6 E, n]; guesses [6 E] or None / empty (the min-torque QP) -> (wrenches [6 E], torques [n])"""
    jacBlock = jacs[:, root].T                                           # 6 x 6 E
    rootTorque = tau_plain[root]
    n, m = jacs.shape[0], 6
    if guesses is None or len(guesses) == 0:
        KKT = np.zeros((n + m, n + m))
        KKT[:n, :n] = weights(n // 6)
        KKT[n:, :n] = jacBlock
        KKT[:n, n:] = jacBlock.T
        eq = np.zeros(n + m)
        eq[n:] = rootTorque
        Q, R = np.linalg.qr(KKT)
        corrected = np.linalg.solve(R, Q.T @ eq)[:n]
    else:
        forces = np.asarray(guesses, dtype=np.float64)
        corrected = np.linalg.lstsq(jacBlock, rootTorque - jacBlock @ forces, rcond=None)[0] + forces
    return _finish(jacs, tau_plain, root, corrected)


def multiple_contact_inverse_dynamics_normal(jacs, tau_plain, root, guesses=None, min_torque=False):
    """the same answers by the normal equations: W = W0 + D A^T (A D A^T)^-1 (r - A W0), D = B^-1 (min torque) or I"""
    A = jacs[:, root].T
    r = tau_plain[root]
    D = np.linalg.inv(weights(jacs.shape[0] // 6)) if min_torque else np.eye(jacs.shape[0])
    W0 = np.zeros(jacs.shape[0]) if guesses is None or len(guesses) == 0 else np.asarray(guesses, dtype=np.float64)
    W = W0 + D @ A.T @ np.linalg.solve(A @ D @ A.T, r - A @ W0)
    return _finish(jacs, tau_plain, root, W)
