// centroidal.hip — centre of mass, its velocity, acceleration and Jacobian, momentum and energies of a body set for B worlds
// (nbl_centroidal_forward / _backward): the device side of Skeleton::getCOM, getCOMLinearVelocity, getCOMLinearAcceleration,
// getCOMLinearJacobian, computeKineticEnergy and computePotentialEnergy (Skeleton.cpp:13598-13810) and of their vector-Jacobian product
// (nimblephysics_amd/centroidal.py).  The math is in centroidal_dev.hpp.
//
// ONE WORLD PER LANE, like the dynamics kernels: the body constants and the set's masks are wave-uniform, the per-body T / W / V / A and
// their adjoints live in the caller's workspace laid out [body][slot][B].  No LDS, no atomics, no cross-lane operations: a world's bits do
// not depend on B or on its place in the batch.  B may be (T + 1) x worlds: 64-bit world indices throughout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "centroidal_dev.hpp"

namespace NBL_NS {

constexpr int CEN_BLOCK = 64;

__global__ __launch_bounds__(CEN_BLOCK) void k_centroidal(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs, DevModel mdl,
                                                          DevBodySet set, int flags, int64_t B, const double* __restrict__ state,
                                                          const double* __restrict__ accel, double* __restrict__ com,
                                                          double* __restrict__ comVel, double* __restrict__ comAcc, double* __restrict__ mom,
                                                          double* __restrict__ ke, double* __restrict__ pe, double* __restrict__ Jcom,
                                                          double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * CEN_BLOCK + threadIdx.x;
  if (b >= B) return;
  cenForwardWorld(bodies, dofs, mdl.nb, mdl.n, mdl.gravity, set, flags, B, b, state, accel, com, comVel, comAcc, mom, ke, pe, Jcom, ws);
}

__global__ __launch_bounds__(CEN_BLOCK) void k_centroidal_vjp(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs, DevModel mdl,
                                                              DevBodySet set, int flags, int64_t B, const double* __restrict__ state,
                                                              const double* __restrict__ accel, const double* __restrict__ gcom,
                                                              const double* __restrict__ gvel, const double* __restrict__ gacc,
                                                              const double* __restrict__ gmom, const double* __restrict__ gke,
                                                              const double* __restrict__ gpe, double* __restrict__ gstate,
                                                              double* __restrict__ gaccel, int accumulate, double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * CEN_BLOCK + threadIdx.x;
  if (b >= B) return;
  cenVjpWorld(bodies, dofs, mdl.nb, mdl.n, mdl.gravity, set, flags, B, b, state, accel, gcom, gvel, gacc, gmom, gke, gpe, gstate, gaccel,
              accumulate, ws);
}

}  // namespace NBL_NS
