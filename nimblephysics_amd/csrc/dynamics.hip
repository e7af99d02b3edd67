// dynamics.hip — joint-space dynamics quantities for B worlds (nbl_inverse_dynamics_forward / _backward, nbl_mass_matrix,
// nbl_forward_dynamics_forward / _backward, nbl_inv_mass_apply, nbl_inv_mass_matrix, the nbl_*_wrench_* calls and
// nbl_contact_inverse_dynamics): the device side of Skeleton::getInverseDynamics,
// World::getCoriolisAndGravityForces, World::getMassMatrix, Skeleton::computeForwardDynamics and World::getInvMassMatrix and of their
// vector-Jacobian products (nimblephysics_amd/dynamics.py).  The math is in dynamics_dev.hpp.
//
// ONE WORLD PER LANE, like k_step_forward's Ctx path and the kinematics kernels: the body constants are wave-uniform (scalar loads), and
// the per-body T / V / A / F and their adjoints, which must survive between the two tree sweeps, live in the caller's workspace laid out
// [body][slot][B], so every access of a wavefront is one coalesced line and a lane holds one body's quantities in registers at a time.
// B may be (T + 1) x worlds, or n x worlds (the mass matrix's backward pass): 64-bit world indices throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dynamics_dev.hpp"

namespace NBL_NS {

constexpr int DYN_BLOCK = 64;

__global__ __launch_bounds__(DYN_BLOCK) void k_inverse_dynamics(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs, DevModel mdl,
                                                                int flags, int64_t B, const double* __restrict__ state,
                                                                const double* __restrict__ accel, double* __restrict__ tau, double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
  if (b >= B) return;
  idForwardWorld(bodies, dofs, mdl.nb, mdl.n, mdl.gravity, mdl.dt, flags, B, b, state, accel, tau, ws);
}

__global__ __launch_bounds__(DYN_BLOCK) void k_inverse_dynamics_vjp(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs, DevModel mdl,
                                                                    int flags, int64_t B, const double* __restrict__ state,
                                                                    const double* __restrict__ accel, const double* __restrict__ gtau,
                                                                    double* __restrict__ gstate, double* __restrict__ gaccel, int accumulate,
                                                                    double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
  if (b >= B) return;
  idVjpWorld(bodies, dofs, mdl.nb, mdl.n, mdl.gravity, mdl.dt, flags, B, b, state, accel, gtau, gstate, gaccel, accumulate, ws);
}

// grad_params [count][B] (= or +=) (d tau / d theta)^T grad_tau for the registered inertia parameters: sweep 1 of the kernel above, then
// one contraction per parameter.  The table is wave-uniform (scalar loads), V / A / Fb of the parameter's body come back as [slot][B]
// lines, and so does the output.
__global__ __launch_bounds__(DYN_BLOCK) void k_inverse_dynamics_inertia_vjp(const DevBody* __restrict__ bodies, DevModel mdl, int flags, int64_t B,
                                                                            const double* __restrict__ state, const double* __restrict__ accel,
                                                                            const double* __restrict__ gtau,
                                                                            const DevInertiaParam* __restrict__ params, int count,
                                                                            double* __restrict__ gparams, int accumulate, double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
  if (b >= B) return;
  idInertiaVjpWorld(bodies, mdl.nb, mdl.n, mdl.gravity, flags, B, b, state, accel, gtau, params, count, gparams, accumulate, ws);
}

__global__ __launch_bounds__(DYN_BLOCK) void k_mass_matrix(const DevBody* __restrict__ bodies, DevModel mdl, int64_t B,
                                                           const double* __restrict__ state, double* __restrict__ M, double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
  if (b >= B) return;
  massMatrixWorld(bodies, mdl.nb, mdl.n, B, b, state, M, ws);
}

// a = M(q)^-1 (tau - C(q, v)): the articulated-body algorithm's three sweeps on the [body][FD_SLOTS][B] workspace.
__global__ __launch_bounds__(DYN_BLOCK) void k_forward_dynamics(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs, DevModel mdl,
                                                                int flags, int64_t B, const double* __restrict__ state,
                                                                const double* __restrict__ tau, double* __restrict__ accel, double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
  if (b >= B) return;
  fdForwardWorld(bodies, dofs, mdl.nb, mdl.n, mdl.gravity, mdl.dt, flags, B, b, state, tau, accel, ws);
}

// First launch of nbl_forward_dynamics_backward: a again, lambda = M^-1 grad_accel, grad_tau (+)= lambda, neglam = -lambda; the second
// launch is k_inverse_dynamics_vjp at (q, v, a) with the cotangent neglam.
__global__ __launch_bounds__(DYN_BLOCK) void k_forward_dynamics_lambda(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs,
                                                                       DevModel mdl, int flags, int64_t B, const double* __restrict__ state,
                                                                       const double* __restrict__ tau, const double* __restrict__ gaccel,
                                                                       double* __restrict__ accel, double* __restrict__ neglam,
                                                                       double* __restrict__ gtau, int accumulate, double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
  if (b >= B) return;
  fdLambdaWorld(bodies, dofs, mdl.nb, mdl.n, mdl.gravity, mdl.dt, flags, B, b, state, tau, gaccel, accel, neglam, gtau, accumulate, ws);
}

// Y [R][n][B] = M(q)^-1 X [R][n][B];  X null (R = n): Y = M(q)^-1 itself, [n * n][B], both triangles from one computation.
__global__ __launch_bounds__(DYN_BLOCK) void k_minv_apply(const DevBody* __restrict__ bodies, DevModel mdl, int64_t B, int R,
                                                          const double* __restrict__ state, const double* __restrict__ X, double* __restrict__ Y,
                                                          double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
  if (b >= B) return;
  minvApplyWorld(bodies, mdl.nb, mdl.n, B, b, state, R, X, Y, ws);
}

// ---- the same with wrenches on body frames (a wrench set = the entries of a kinematics map; dynamics_dev.hpp) ------------------------------
__global__ __launch_bounds__(DYN_BLOCK) void k_inverse_dynamics_wrench(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs,
                                                                       DevModel mdl, int flags, int64_t B, const double* __restrict__ state,
                                                                       const double* __restrict__ accel, const DevKinEntry* __restrict__ entries,
                                                                       const int32_t* __restrict__ path, int count,
                                                                       const double* __restrict__ wrench, double* __restrict__ tau,
                                                                       double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
  if (b >= B) return;
  idForwardWorldT<true>(bodies, dofs, mdl.nb, mdl.n, mdl.gravity, mdl.dt, flags, B, b, state, accel, tau, ws, entries, path, count, wrench);
}

// grad_state, grad_accel and grad_wrench [6 E][B] (any may be null); wx [nb][3][B]: the moments of world-frame wrenches on their way up
__global__ __launch_bounds__(DYN_BLOCK) void k_inverse_dynamics_wrench_vjp(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs,
                                                                           DevModel mdl, int flags, int64_t B, const double* __restrict__ state,
                                                                           const double* __restrict__ accel, const DevKinEntry* __restrict__ entries,
                                                                           const int32_t* __restrict__ path, int count,
                                                                           const double* __restrict__ wrench, const double* __restrict__ gtau,
                                                                           double* __restrict__ gstate, double* __restrict__ gaccel,
                                                                           double* __restrict__ gwrench, int accumulate, double* __restrict__ ws,
                                                                           double* __restrict__ wx) {
  const int64_t b = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
  if (b >= B) return;
  idVjpWorldT<true>(bodies, dofs, mdl.nb, mdl.n, mdl.gravity, mdl.dt, flags, B, b, state, accel, gtau, gstate, gaccel, accumulate, ws, entries, path,
                    count, wrench, gwrench, wx);
}

__global__ __launch_bounds__(DYN_BLOCK) void k_forward_dynamics_wrench(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs,
                                                                       DevModel mdl, int flags, int64_t B, const double* __restrict__ state,
                                                                       const double* __restrict__ tau, const DevKinEntry* __restrict__ entries,
                                                                       const int32_t* __restrict__ path, int count,
                                                                       const double* __restrict__ wrench, double* __restrict__ accel,
                                                                       double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
  if (b >= B) return;
  fdForwardWorldT<true>(bodies, dofs, mdl.nb, mdl.n, mdl.gravity, mdl.dt, flags, B, b, state, tau, accel, ws, entries, path, count, wrench);
}

// First launch of nbl_forward_dynamics_wrench_backward; the second is k_inverse_dynamics_wrench_vjp at (q, v, a) with the cotangent neglam.
__global__ __launch_bounds__(DYN_BLOCK) void k_forward_dynamics_wrench_lambda(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs,
                                                                              DevModel mdl, int flags, int64_t B, const double* __restrict__ state,
                                                                              const double* __restrict__ tau, const DevKinEntry* __restrict__ entries,
                                                                              const int32_t* __restrict__ path, int count,
                                                                              const double* __restrict__ wrench, const double* __restrict__ gaccel,
                                                                              double* __restrict__ accel, double* __restrict__ neglam,
                                                                              double* __restrict__ gtau, int accumulate, double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
  if (b >= B) return;
  fdLambdaWrenchWorld(bodies, dofs, mdl.nb, mdl.n, mdl.gravity, mdl.dt, flags, B, b, state, tau, gaccel, accel, neglam, gtau, accumulate, ws, entries,
                      path, count, wrench);
}

// The contact wrenches and joint torques of Skeleton::getContactInverseDynamics / getMultipleContactInverseDynamics; xs [E][12][B].
__global__ __launch_bounds__(DYN_BLOCK) void k_contact_inverse_dynamics(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs,
                                                                        DevModel mdl, int flags, int mode, int64_t B,
                                                                        const double* __restrict__ state, const double* __restrict__ accel,
                                                                        const DevKinEntry* __restrict__ entries, const int32_t* __restrict__ path,
                                                                        int count, const double* __restrict__ guess, double* __restrict__ wout,
                                                                        double* __restrict__ tau, double* __restrict__ ws, double* __restrict__ xs) {
  const int64_t b = (int64_t)blockIdx.x * DYN_BLOCK + threadIdx.x;
  if (b >= B) return;
  cidWorld(bodies, dofs, mdl.nb, mdl.n, mdl.gravity, mdl.dt, flags, mode, B, b, state, accel, entries, path, count, guess, wout, tau, ws, xs);
}

}  // namespace NBL_NS
