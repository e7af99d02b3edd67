// ik.hip — batched inverse kinematics (nbl_ik_solve): the device side of IKMapping::setPositions (dart/neural/IKMapping.cpp:86-119,
// math::solveIK / refineIK, dart/math/IKSolver.cpp:195-493) for B independent worlds.  The math is in ik_dev.hpp.
//
// ONE WORLD PER LANE, like the kinematics and dynamics kernels: a lane runs its own world's whole solve - both phases, every branch of
// refineIK's ladder - and leaves the loop when ITS world terminates; lanes of a wavefront that finish early idle until the slowest one is
// done.  The model, the entries and their ancestor chains are wave-uniform (scalar loads).  The iterate, the dense Jacobian [P][n], the
// normal matrix (min(P, n) on a side, factored in place) and the step live in the caller's workspace laid out [slot][B]: every access of
// a wavefront is one coalesced line, and because every index into them is computed nothing of the solver is a private array (no scratch)
// and nothing is staged in LDS (a world's state is IkLayout's 3 n + P + min(P, n) + P n + min(P, n)^2 doubles - 7.9 kB on Atlas-20 with
// four spatial entries -, 64 of them do not fit).  No atomics, no cross-lane operations: results do not depend on B or on a world's place in the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ik_dev.hpp"

namespace NBL_NS {

constexpr int IK_BLOCK = 64;

__global__ __launch_bounds__(IK_BLOCK) void k_ik_solve(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs,
                                                       const DevKinEntry* __restrict__ entries, const int32_t* __restrict__ path, int count,
                                                       int nb, int n, int P, int64_t B, const double* __restrict__ target,
                                                       const double* __restrict__ q_init, IkConfig cfg, double* __restrict__ q_out,
                                                       double* __restrict__ loss, int32_t* __restrict__ steps, double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * IK_BLOCK + threadIdx.x;
  if (b >= B) return;
  ikSolveWorld(bodies, dofs, entries, path, count, nb, n, P, B, b, target, q_init, cfg, q_out, loss, steps, ws);
}

}  // namespace NBL_NS
