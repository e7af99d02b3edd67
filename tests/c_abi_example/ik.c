/* Batched inverse kinematics from plain C99: nbl_ik_solve on the Atlas-20 model of atlas20_ground_model.h with ONE linear entry on the
 * left foot (body 8 of the description: pelvis, two torso links, then the six links of the left leg), B worlds.  The targets are the
 * foot positions nbl_kinematics_forward gives at known joint positions; the solve starts from zero.  Prints "ik loss" for the test to
 * read.  Exit status 0 = every world's returned loss is below its initial loss, q_out is finite, and the argument errors answer as the
 * header says. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <hip/hip_runtime_api.h>
#include "nimble_amd.h"
#include "atlas20_ground_model.h"

#define CHECK(x) do { int rc_ = (x); if (rc_ != 0) { fprintf(stderr, "%s failed (%d): %s\n", #x, rc_, nbl_last_error()); return 1; } } while (0)
#define HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
#define EXPECT(x, code) do { int rc_ = (x); if (rc_ != (code) || !nbl_last_error()[0]) { fprintf(stderr, "%s returned %d, expected %d\n", #x, rc_, (code)); return 1; } } while (0)

int main(int argc, char** argv) {
  const int64_t B = argc > 1 ? atoll(argv[1]) : 8;
  const int n = MDL_N_DOFS, P = 3;
  nbl_model_desc d;
  mdl_fill(&d);
  nbl_model* m = NULL;
  CHECK(nbl_model_create(&d, 0, &m));
  const int32_t kind = NBL_KIN_LINEAR, body = 8;
  nbl_kin_map* k = NULL;
  CHECK(nbl_kin_map_create(m, 1, &kind, &body, NULL, &k));
  if (nbl_kin_map_dim(k) != P) { fprintf(stderr, "map rows\n"); return 1; }
  const size_t wsBytes = nbl_ik_workspace_bytes(m, k, B);
  if (wsBytes == 0 || nbl_ik_workspace_bytes(NULL, k, B) != 0 || nbl_ik_workspace_bytes(m, NULL, B) != 0) { fprintf(stderr, "workspace bytes\n"); return 1; }
  double *state, *target, *start, *qout, *loss;
  int32_t* steps;
  void* ws;
  HIP(hipMalloc((void**)&state, 2 * n * B * sizeof(double))); HIP(hipMalloc((void**)&target, P * B * sizeof(double)));
  HIP(hipMalloc((void**)&start, P * B * sizeof(double))); HIP(hipMalloc((void**)&qout, n * B * sizeof(double)));
  HIP(hipMalloc((void**)&loss, B * sizeof(double))); HIP(hipMalloc((void**)&steps, B * sizeof(int32_t)));
  HIP(hipMalloc(&ws, wsBytes));
  /* known joint positions (DOF-major [row][B]; leg joints inside their limits), velocities zero */
  double* hs = (double*)calloc(2 * n * B, sizeof(double));
  for (int r = 0; r < n; r++)
    for (int64_t b = 0; b < B; b++) hs[r * B + b] = 0.15 * sin(1.0 + 3.0 * (double)b + 7.0 * r);
  HIP(hipMemcpy(state, hs, 2 * n * B * sizeof(double), hipMemcpyHostToDevice));
  CHECK(nbl_kinematics_forward(m, k, B, state, target, NULL, NULL));
  HIP(hipMemset(state, 0, 2 * n * B * sizeof(double)));
  CHECK(nbl_kinematics_forward(m, k, B, state, start, NULL, NULL));       /* the foot at q = 0: the initial loss */
  nbl_ik_config cfg;
  memset(&cfg, 0xff, sizeof(cfg));
  nbl_ik_default_config(&cfg);
  if (cfg.max_step_count != 100 || cfg.least_squares_damping != 0.01 || cfg.convergence_threshold != 1e-7 || cfg.start_clamped != 0 ||
      cfg.line_search != 1 || cfg.dont_exit_transpose != 0) { fprintf(stderr, "default config\n"); return 1; }
  CHECK(nbl_ik_solve(m, k, B, target, NULL, &cfg, qout, loss, steps, ws, wsBytes, NULL));
  HIP(hipDeviceSynchronize());
  double* ht = (double*)malloc(P * B * sizeof(double));
  double* h0 = (double*)malloc(P * B * sizeof(double));
  double* hq = (double*)malloc(n * B * sizeof(double));
  double* hl = (double*)malloc(B * sizeof(double));
  int32_t* hn = (int32_t*)malloc(B * sizeof(int32_t));
  HIP(hipMemcpy(ht, target, P * B * sizeof(double), hipMemcpyDeviceToHost)); HIP(hipMemcpy(h0, start, P * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hq, qout, n * B * sizeof(double), hipMemcpyDeviceToHost)); HIP(hipMemcpy(hl, loss, B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hn, steps, B * sizeof(int32_t), hipMemcpyDeviceToHost));
  double worst = 0, worstRatio = 0;
  int maxSteps = 0;
  for (int64_t b = 0; b < B; b++) {
    double l0 = 0;
    for (int p = 0; p < P; p++) l0 += (h0[p * B + b] - ht[p * B + b]) * (h0[p * B + b] - ht[p * B + b]);
    for (int r = 0; r < n; r++)
      if (!isfinite(hq[r * B + b])) { fprintf(stderr, "q_out not finite (world %lld)\n", (long long)b); return 1; }
    if (!(hl[b] < l0)) { fprintf(stderr, "world %lld: loss %g not below the initial loss %g\n", (long long)b, hl[b], l0); return 1; }
    if (hn[b] < 2 || hn[b] > 20 + cfg.max_step_count) { fprintf(stderr, "world %lld: %d evaluations\n", (long long)b, hn[b]); return 1; }
    if (hl[b] > worst) worst = hl[b];
    if (hl[b] / l0 > worstRatio) worstRatio = hl[b] / l0;
    if (hn[b] > maxSteps) maxSteps = hn[b];
  }
  printf("ik loss worst %.3e worst ratio to the initial loss %.3e most evaluations %d\n", worst, worstRatio, maxSteps);
  /* argument errors: nothing is launched */
  nbl_ik_config bad = cfg;
  EXPECT(nbl_ik_solve(NULL, k, B, target, NULL, &cfg, qout, loss, steps, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_ik_solve(m, NULL, B, target, NULL, &cfg, qout, loss, steps, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_ik_solve(m, k, B, NULL, NULL, &cfg, qout, loss, steps, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_ik_solve(m, k, B, target, NULL, &cfg, NULL, loss, steps, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_ik_solve(m, k, -1, target, NULL, &cfg, qout, loss, steps, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_ik_solve(m, k, B, target, NULL, &cfg, qout, loss, steps, ws, wsBytes - 1, NULL), NBL_E_WORKSPACE);
  bad.max_step_count = 0;
  EXPECT(nbl_ik_solve(m, k, B, target, NULL, &bad, qout, loss, steps, ws, wsBytes, NULL), NBL_E_BADARG);
  bad.max_step_count = 100001;
  EXPECT(nbl_ik_solve(m, k, B, target, NULL, &bad, qout, loss, steps, ws, wsBytes, NULL), NBL_E_BADARG);
  bad = cfg; bad.least_squares_damping = 0.0;
  EXPECT(nbl_ik_solve(m, k, B, target, NULL, &bad, qout, loss, steps, ws, wsBytes, NULL), NBL_E_UNSUPPORTED);
  bad = cfg; bad.convergence_threshold = -1.0;
  EXPECT(nbl_ik_solve(m, k, B, target, NULL, &bad, qout, loss, steps, ws, wsBytes, NULL), NBL_E_BADARG);
  CHECK(nbl_ik_solve(m, k, 0, NULL, NULL, &cfg, NULL, NULL, NULL, NULL, 0, NULL));      /* B = 0: a no-op */
  CHECK(nbl_ik_solve(m, k, B, target, NULL, NULL, qout, NULL, NULL, ws, wsBytes, NULL)); /* config NULL, no loss / steps */
  HIP(hipDeviceSynchronize());
  nbl_kin_map_destroy(k);
  nbl_model_destroy(m);
  return 0;
}
