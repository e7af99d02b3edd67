// ik_grad.hip — the reverse pass of the batched inverse kinematics (nbl_ik_solve_vjp): grad_target from grad_q at the positions
// nbl_ik_solve returned, for B independent worlds.  The math is in ik_grad_dev.hpp.
//
// ONE WORLD PER LANE with the launch shape of k_ik_solve (ik.hip), for its reasons: the dense Jacobian [P][n] and the normal matrix
// (min(P, |F|) on a side, factored in place) live in the caller's workspace laid out [slot][B] - IkLayout, the solver's own layout and
// size -, so every access of a wavefront is one coalesced line, every index is computed (no private array, no scratch beyond ikEval's),
// and nothing is staged in LDS (64 worlds' matrices do not fit).  A world costs one Jacobian and one factorisation - about one step of the
// solver's several hundred -, so lanes of a wavefront diverge only in the side of their systems (|F| differs where limits are hit).
// No atomics, no cross-lane operations: results do not depend on B or on a world's place in the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ik_grad_dev.hpp"

namespace NBL_NS {

constexpr int IK_GRAD_BLOCK = 64;

__global__ __launch_bounds__(IK_GRAD_BLOCK) void k_ik_solve_vjp(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs,
                                                                const DevKinEntry* __restrict__ entries, const int32_t* __restrict__ path,
                                                                int count, int nb, int n, int P, int64_t B, const double* __restrict__ q,
                                                                const double* __restrict__ grad_q, double mu,
                                                                double* __restrict__ grad_target, int accumulate,
                                                                int32_t* __restrict__ free_count, double* __restrict__ ws) {
  const int64_t b = (int64_t)blockIdx.x * IK_GRAD_BLOCK + threadIdx.x;
  if (b >= B) return;
  ikVjpWorld(bodies, dofs, entries, path, count, nb, n, P, B, b, q, grad_q, mu, grad_target, accumulate, free_count, ws);
}

}  // namespace NBL_NS
