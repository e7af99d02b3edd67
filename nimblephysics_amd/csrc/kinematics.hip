// kinematics.hip — world-space kinematics of body frames for B worlds (nbl_kinematics_forward / nbl_kinematics_backward): the device side
// of IKMapping::getPositions / getVelocities and of the vector-Jacobian products of map_to_pos / map_to_vel (dart/neural/IKMapping.cpp,
// python/nimblephysics/mapping.py).  The math is in kinematics_dev.hpp.
//
// ONE WORLD PER LANE, like the tree kernels of kernels.hip: every [row][B] / [dof][B] access of a wavefront is one coalesced line, the
// entries, their ancestor chains and the body constants are wave-uniform (scalar loads), and the running transform and wrench of an
// entry stay in registers.  The work per world is a few dozen joint transforms, so nothing is staged in LDS.  B may be (T + 1) x worlds
// (a whole rollout in one launch): 64-bit world indices throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kinematics_dev.hpp"

namespace NBL_NS {

constexpr int KIN_BLOCK = 64;

__global__ __launch_bounds__(KIN_BLOCK) void k_kinematics_fwd(const DevBody* __restrict__ bodies, const DevKinEntry* __restrict__ entries,
                                                              const int32_t* __restrict__ path, int count, int n, int64_t B,
                                                              const double* __restrict__ state, double* __restrict__ pos, double* __restrict__ vel) {
  const int64_t b = (int64_t)blockIdx.x * KIN_BLOCK + threadIdx.x;
  if (b >= B) return;
  kinForwardWorld(bodies, entries, path, count, n, B, b, state, pos, vel);
}

__global__ __launch_bounds__(KIN_BLOCK) void k_kinematics_vjp(const DevBody* __restrict__ bodies, const DevKinEntry* __restrict__ entries,
                                                              const int32_t* __restrict__ path, int count, int n, int64_t B,
                                                              const double* __restrict__ state, const double* __restrict__ gpos,
                                                              const double* __restrict__ gvel, double* __restrict__ gstate, int accumulate) {
  const int64_t b = (int64_t)blockIdx.x * KIN_BLOCK + threadIdx.x;
  if (b >= B) return;
  kinVjpWorld(bodies, entries, path, count, n, B, b, state, gpos, gvel, gstate, accumulate);
}

}  // namespace NBL_NS
