// Host build of the reverse pass of the product's inverse kinematics (nimblephysics_amd/csrc/ik_grad_dev.hpp: what k_ik_solve_vjp runs
// per lane) for tests/test_ik_grad_host.py and tests/test_gpu_ik_grad.py.  Test harness only; the model is built as ik_shim.cpp builds it.
#include <vector>

#include "ik_grad_dev.hpp"
#include "model_shim.hpp"

using namespace NBL_NS;

using namespace shim_model;

extern "C" {
void* shim_ikg_model(const nbl_model_desc* d) { return makeModel(d); }
void shim_ikg_free(void* h) { delete (ShimModel*)h; }

// nbl_ik_solve_vjp on the host: entries as nbl_kin_map_create takes them, the arrays as nbl_ik_solve_vjp takes them (free_count may be
// null).  Returns P.
int shim_ikg_vjp(void* h, int count, const int* kind, const int* body, const double* T, int64_t B, const double* q, const double* grad_q,
                 double mu, double* grad_target, int accumulate, int32_t* free_count) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimMap k = makeMap(m, count, kind, body, T);
  std::vector<double> ws((size_t)ikLayout(m.n, k.P).total * B, NAN);     // NaN: a slot read before it is written shows
  for (int64_t b = 0; b < B; b++)
    ikVjpWorld(m.bodies.data(), m.dofs.data(), k.e.data(), k.path.data(), count, (int)m.bodies.size(), m.n, k.P, B, b, q, grad_q, mu,
               grad_target, accumulate, free_count, ws.data());
  return k.P;
}
}
