// taskspace.hip — task-space Jacobians, their time derivative and task-space accelerations of the rows of a kinematics map for B worlds
// (nbl_task_jacobian / _vjp, nbl_task_jacobian_deriv, nbl_task_accel / _vjp): the device side of nimblephysics_amd/taskspace.py
// (task_jacobian, task_jacobian_deriv, task_jacobian_dot_times_v, map_to_acc).  The math is in taskspace_dev.hpp.
//
// ONE WORLD PER LANE, like the kinematics kernels: every [row][B] / [dof][B] access of a wavefront is one coalesced line, the entries,
// their ancestor chains and the body constants are wave-uniform (scalar loads).  The forward kernels and the reverse pass of J keep an
// entry's running transform, twist and wrench in registers and need no workspace; the reverse pass of the acceleration sweeps the whole
// tree through the caller's workspace laid out [body][slot][B], like the sensor kernels.  No LDS, no atomics, no cross-lane operations:
// a world's bits do not depend on B or on its place in the batch.  B may be (T + 1) x worlds: 64-bit world indices throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "taskspace_dev.hpp"

namespace NBL_NS {

constexpr int TASK_BLOCK = 64;

__global__ __launch_bounds__(TASK_BLOCK) void k_task_jacobian(const DevBody* __restrict__ bodies, const DevKinEntry* __restrict__ entries,
                                                              const int32_t* __restrict__ path, int count, int n, int64_t B,
                                                              const double* __restrict__ state, double* __restrict__ J) {
  const int64_t b = (int64_t)blockIdx.x * TASK_BLOCK + threadIdx.x;
  if (b >= B) return;
  taskJacobianWorld(bodies, entries, path, count, n, B, b, state, J);
}

__global__ __launch_bounds__(TASK_BLOCK) void k_task_jacobian_deriv(const DevBody* __restrict__ bodies, const DevKinEntry* __restrict__ entries,
                                                                    const int32_t* __restrict__ path, int count, int n, int64_t B,
                                                                    const double* __restrict__ state, double* __restrict__ Jd) {
  const int64_t b = (int64_t)blockIdx.x * TASK_BLOCK + threadIdx.x;
  if (b >= B) return;
  taskJacobianDerivWorld(bodies, entries, path, count, n, B, b, state, Jd);
}

__global__ __launch_bounds__(TASK_BLOCK) void k_task_jacobian_vjp(const DevBody* __restrict__ bodies, const DevKinEntry* __restrict__ entries,
                                                                  const int32_t* __restrict__ path, int count, int n, int64_t B,
                                                                  const double* __restrict__ state, const double* __restrict__ G,
                                                                  double* __restrict__ gq, int accumulate) {
  const int64_t b = (int64_t)blockIdx.x * TASK_BLOCK + threadIdx.x;
  if (b >= B) return;
  taskJacobianVjpWorld(bodies, entries, path, count, n, B, b, state, G, gq, accumulate);
}

__global__ __launch_bounds__(TASK_BLOCK) void k_task_accel(const DevBody* __restrict__ bodies, const DevKinEntry* __restrict__ entries,
                                                           const int32_t* __restrict__ path, int count, int n, int64_t B,
                                                           const double* __restrict__ state, const double* __restrict__ accel,
                                                           double* __restrict__ bias, double* __restrict__ xdd) {
  const int64_t b = (int64_t)blockIdx.x * TASK_BLOCK + threadIdx.x;
  if (b >= B) return;
  if (bias) taskAccelWorld(bodies, entries, path, count, n, B, b, state, nullptr, bias);
  if (xdd) taskAccelWorld(bodies, entries, path, count, n, B, b, state, accel, xdd);
}

__global__ __launch_bounds__(TASK_BLOCK) void k_task_accel_vjp(const DevBody* __restrict__ bodies, DevModel mdl,
                                                               const DevKinEntry* __restrict__ entries, const int32_t* __restrict__ path,
                                                               int count, int64_t B, const double* __restrict__ state,
                                                               const double* __restrict__ accel, const double* __restrict__ gout,
                                                               double* __restrict__ gstate, double* __restrict__ gaccel, int accumulate,
                                                               double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * TASK_BLOCK + threadIdx.x;
  if (b >= B) return;
  taskAccelVjpWorld(bodies, mdl.nb, mdl.n, entries, path, count, B, b, state, accel, gout, gstate, gaccel, accumulate, ws);
}

}  // namespace NBL_NS
