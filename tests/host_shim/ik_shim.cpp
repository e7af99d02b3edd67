// Host build of the product's inverse kinematics (nimblephysics_amd/csrc/ik_dev.hpp) for tests/test_ik_host.py and tools/ik_bench.py.
// Test harness only.  The device body table is restated here from nbl_model_create / expandBallJoints (nimble_amd.hip), in
// model_shim.hpp; the per-coordinate limits come from the description's pos_lo / pos_hi.
#include <thread>
#include <vector>

#include "ik_dev.hpp"
#include "model_shim.hpp"

using namespace NBL_NS;

using namespace shim_model;

namespace {
IkCtx makeCtx(const ShimModel& m, const ShimMap& k, int64_t B, int64_t b, const double* target, double* ws) {
  IkCtx c;
  c.bodies = m.bodies.data(); c.dofs = m.dofs.data(); c.entries = k.e.data(); c.path = k.path.data();
  c.count = (int)k.e.size(); c.nb = (int)m.bodies.size(); c.B = B; c.b = b; c.target = target; c.ws = ws; c.L = ikLayout(m.n, k.P);
  return c;
}
}  // namespace

extern "C" {
void* shim_ik_model(const nbl_model_desc* d) { return makeModel(d); }
void shim_ik_free(void* h) { delete (ShimModel*)h; }

// nbl_ik_solve on the host: entries as nbl_kin_map_create takes them, the arrays as nbl_ik_solve takes them; `threads` host threads
// share the worlds.  Returns P.
int shim_ik_solve(void* h, int count, const int* kind, const int* body, const double* T, int64_t B, const double* target, const double* q_init,
                  const nbl_ik_config* cfg, double* q_out, double* loss, int32_t* steps, int threads) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimMap k = makeMap(m, count, kind, body, T);
  IkConfig c;
  c.convergenceThreshold = cfg->convergence_threshold; c.maxStepCount = cfg->max_step_count; c.damping = cfg->least_squares_damping;
  c.startClamped = cfg->start_clamped; c.lineSearch = cfg->line_search; c.dontExitTranspose = cfg->dont_exit_transpose;
  std::vector<double> ws((size_t)ikLayout(m.n, k.P).total * B, NAN);     // NaN: a slot read before it is written shows
  auto run = [&](int64_t b0, int64_t b1) {
    for (int64_t b = b0; b < b1; b++)
      ikSolveWorld(m.bodies.data(), m.dofs.data(), k.e.data(), k.path.data(), count, (int)m.bodies.size(), m.n, k.P, B, b, target, q_init, c,
                   q_out, loss, steps, ws.data());
  };
  if (threads <= 1) {
    run(0, B);
  } else {
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++) pool.emplace_back(run, B * t / threads, B * (t + 1) / threads);
    for (auto& t : pool) t.join();
  }
  return k.P;
}

// One eval at q [n][B]: diff [P][B] against target, the dense Jacobian J [P * n][B] (row-major P x n per world), the squared error err [B].
int shim_ik_eval(void* h, int count, const int* kind, const int* body, const double* T, int64_t B, const double* q, const double* target,
                 double* diff, double* J, double* err) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimMap k = makeMap(m, count, kind, body, T);
  const IkLayout L = ikLayout(m.n, k.P);
  std::vector<double> ws((size_t)L.total * B, NAN);
  for (int64_t b = 0; b < B; b++) {
    IkCtx c = makeCtx(m, k, B, b, target, ws.data());
    for (int d = 0; d < m.n; d++) IKW(c, L.pos + d) = q[(int64_t)d * B + b];
    for (int i = 0; i < k.P * m.n; i++) IKW(c, L.J + i) = 0.0;
    err[b] = ikEval<true>(c, L.pos);
    for (int p = 0; p < k.P; p++) diff[(int64_t)p * B + b] = IKW(c, L.diff + p);
    for (int i = 0; i < k.P * m.n; i++) J[(int64_t)i * B + b] = IKW(c, L.J + i);
  }
  return k.P;
}

// Skeleton::clampPositionsToLimits as ikClamp states it, in place on q [n][B].
void shim_ik_clamp(void* h, int64_t B, double* q) {
  const ShimModel& m = *(const ShimModel*)h;
  ShimMap k;
  const IkLayout L = ikLayout(m.n, 0);
  std::vector<double> ws((size_t)L.total * B, NAN);
  for (int64_t b = 0; b < B; b++) {
    IkCtx c = makeCtx(m, k, B, b, nullptr, ws.data());
    for (int d = 0; d < m.n; d++) IKW(c, L.pos + d) = q[(int64_t)d * B + b];
    ikClamp(c, L.pos);
    for (int d = 0; d < m.n; d++) q[(int64_t)d * B + b] = IKW(c, L.pos + d);
  }
}
}
