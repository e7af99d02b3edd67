/* The inertia-parameter gradients of the dynamics calls from plain C99: nbl_inverse_dynamics_backward_inertia and
 * nbl_forward_dynamics_backward_inertia on the Atlas-20 model of atlas20_ground_model.h, B worlds, with the mass of every body registered
 * (nbl_set_inertia_params: dG_p = G_p / m_p, the direction in which INERTIA_MASS moves a body's spatial inertia).  Checks from the
 * library's own outputs
 *   the Euler identity  sum_p m_p d tau_i / d m_p == tau_i  (tau is homogeneous of degree 1 in the masses; n launches with the unit
 *     cotangents e_i against nbl_inverse_dynamics_forward), to 1e-12 relative;
 *   forward dynamics:  grad_params == -(inverse-dynamics inertia gradient at (q, v, a) with the cotangent lambda),  a from
 *     nbl_forward_dynamics_forward, lambda = nbl_inv_mass_apply(grad_accel);
 *   a wrench set of one entry with a zero wrench gives what no set gives; accumulate adds;
 * then the argument errors; prints "max residuals" for the test to read.  Exit status 0 = all checks passed. */
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

/* G / m of body i, row-major 6 x 6: G = [[I + m C C^T, m C], [m C^T, m 1]], C = skew(com) */
static void mass_direction(int i, double* D) {
  const double m = MDL_mass[i];
  const double* c = MDL_com + 3 * i;
  const double* I = MDL_inertia + 6 * i;
  const double Ic[3][3] = {{I[0], I[3], I[4]}, {I[3], I[1], I[5]}, {I[4], I[5], I[2]}};
  const double Cx[3][3] = {{0, -c[2], c[1]}, {c[2], 0, -c[0]}, {-c[1], c[0], 0}};
  memset(D, 0, 36 * sizeof(double));
  for (int r = 0; r < 3; r++)
    for (int k = 0; k < 3; k++) {
      double cct = 0;
      for (int j = 0; j < 3; j++) cct += Cx[r][j] * Cx[k][j];
      D[6 * r + k] = Ic[r][k] / m + cct;
      D[6 * r + 3 + k] = Cx[r][k];
      D[6 * (3 + r) + k] = Cx[k][r];
    }
  D[6 * 3 + 3] = D[6 * 4 + 4] = D[6 * 5 + 5] = 1.0;
}

int main(int argc, char** argv) {
  const int64_t B = argc > 1 ? atoll(argv[1]) : 8;
  const int n = MDL_N_DOFS, P = MDL_N_BODIES;
  nbl_model_desc d;
  memset(&d, 0, sizeof(d));
  mdl_fill(&d);
  nbl_model* m = NULL;
  CHECK(nbl_model_create(&d, 0, &m));
  int32_t bodies[MDL_N_BODIES];
  double dG[MDL_N_BODIES * 36];
  for (int i = 0; i < P; i++) { bodies[i] = i; mass_direction(i, dG + 36 * i); }
  if (nbl_num_inertia_params(m) != 0) { fprintf(stderr, "parameters before registration\n"); return 1; }
  const int32_t kind[1] = {NBL_KIN_SPATIAL}, kbody[1] = {MDL_N_BODIES - 1};
  nbl_kin_map* km = NULL;
  CHECK(nbl_kin_map_create(m, 1, kind, kbody, NULL, &km));
  const size_t fdBytes = nbl_forward_dynamics_workspace_bytes(m, B), idBytes = nbl_dynamics_workspace_bytes(m, B), wrBytes = nbl_wrench_workspace_bytes(m, km, B);
  if (idBytes == 0 || fdBytes < idBytes || wrBytes < fdBytes) { fprintf(stderr, "workspace bytes\n"); return 1; }
  double *state, *accel, *tau, *g, *cot, *lam, *a, *gp, *gpFd, *gpWr, *gpId, *wrench;
  void* ws;
  HIP(hipMalloc((void**)&state, 2 * n * B * sizeof(double))); HIP(hipMalloc((void**)&accel, n * B * sizeof(double)));
  HIP(hipMalloc((void**)&tau, n * B * sizeof(double))); HIP(hipMalloc((void**)&g, n * B * sizeof(double)));
  HIP(hipMalloc((void**)&cot, n * B * sizeof(double))); HIP(hipMalloc((void**)&lam, n * B * sizeof(double)));
  HIP(hipMalloc((void**)&a, n * B * sizeof(double))); HIP(hipMalloc((void**)&gp, (size_t)n * P * B * sizeof(double)));
  HIP(hipMalloc((void**)&gpFd, P * B * sizeof(double))); HIP(hipMalloc((void**)&gpWr, P * B * sizeof(double)));
  HIP(hipMalloc((void**)&gpId, P * B * sizeof(double))); HIP(hipMalloc((void**)&wrench, 6 * B * sizeof(double)));
  HIP(hipMalloc(&ws, wrBytes));                       /* the largest of the three sizes serves every call */
  HIP(hipMemset(wrench, 0, 6 * B * sizeof(double)));
  double* hs = (double*)malloc(2 * n * B * sizeof(double));
  double* ha = (double*)malloc(n * B * sizeof(double));
  double* hg = (double*)malloc(n * B * sizeof(double));
  double* hc = (double*)calloc(n * B, sizeof(double));
  for (int r = 0; r < 2 * n; r++)
    for (int64_t b = 0; b < B; b++) hs[r * B + b] = r < n ? 0.4 * sin(1.0 + 3.0 * (double)b + 7.0 * r) : 0.8 * cos(2.0 + 5.0 * (double)b + 11.0 * (r - n));
  for (int r = 0; r < n; r++)
    for (int64_t b = 0; b < B; b++) { ha[r * B + b] = 2.0 * sin(0.5 + (double)b + 1.3 * r); hg[r * B + b] = cos(0.25 + 2.0 * (double)b + 0.7 * r); }
  HIP(hipMemcpy(state, hs, 2 * n * B * sizeof(double), hipMemcpyHostToDevice));
  HIP(hipMemcpy(accel, ha, n * B * sizeof(double), hipMemcpyHostToDevice));
  HIP(hipMemcpy(g, hg, n * B * sizeof(double), hipMemcpyHostToDevice));
  /* nothing registered: a no-op that succeeds, whatever grad_params is */
  CHECK(nbl_inverse_dynamics_backward_inertia(m, B, state, accel, 0, g, NULL, 0, ws, wrBytes, NULL));
  CHECK(nbl_set_inertia_params(m, P, bodies, dG));
  if (nbl_num_inertia_params(m) != P) { fprintf(stderr, "nbl_num_inertia_params\n"); return 1; }

  /* the Euler identity: row i of the Jacobian by the unit cotangent e_i */
  CHECK(nbl_inverse_dynamics_forward(m, B, state, accel, 0, tau, ws, wrBytes, NULL));
  for (int i = 0; i < n; i++) {
    memset(hc, 0, n * B * sizeof(double));
    for (int64_t b = 0; b < B; b++) hc[i * B + b] = 1.0;
    HIP(hipMemcpy(cot, hc, n * B * sizeof(double), hipMemcpyHostToDevice));
    CHECK(nbl_inverse_dynamics_backward_inertia(m, B, state, accel, 0, cot, gp + (size_t)i * P * B, 0, ws, wrBytes, NULL));
  }
  /* forward dynamics: the call, the same through a wrench set with a zero wrench, and its two halves by hand */
  CHECK(nbl_forward_dynamics_backward_inertia(m, NULL, B, state, accel, NULL, NBL_ID_JOINT_FORCES, g, gpFd, 0, ws, wrBytes, NULL));
  CHECK(nbl_forward_dynamics_backward_inertia(m, km, B, state, accel, wrench, NBL_ID_JOINT_FORCES, g, gpWr, 0, ws, wrBytes, NULL));
  CHECK(nbl_forward_dynamics_forward(m, B, state, accel, NBL_ID_JOINT_FORCES, a, ws, wrBytes, NULL));      /* (accel serves as tau here) */
  CHECK(nbl_inv_mass_apply(m, B, 1, state, g, lam, ws, wrBytes, NULL));
  CHECK(nbl_inverse_dynamics_backward_inertia(m, B, state, a, NBL_ID_JOINT_FORCES, lam, gpId, 0, ws, wrBytes, NULL));
  HIP(hipDeviceSynchronize());
  double* ht = (double*)malloc(n * B * sizeof(double));
  double* hgp = (double*)malloc((size_t)n * P * B * sizeof(double));
  double* hfd = (double*)malloc(P * B * sizeof(double));
  double* hwr = (double*)malloc(P * B * sizeof(double));
  double* hid = (double*)malloc(P * B * sizeof(double));
  double* hacc = (double*)malloc(P * B * sizeof(double));
  HIP(hipMemcpy(ht, tau, n * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hgp, gp, (size_t)n * P * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hfd, gpFd, P * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hwr, gpWr, P * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hid, gpId, P * B * sizeof(double), hipMemcpyDeviceToHost));
  double resEuler = 0, scaleTau = 1, resFd = 0, resWr = 0, scaleFd = 1;
  for (int i = 0; i < n; i++)
    for (int64_t b = 0; b < B; b++) {
      double e = 0;
      for (int p = 0; p < P; p++) e += MDL_mass[p] * hgp[((size_t)i * P + p) * B + b];
      if (fabs(e - ht[i * B + b]) > resEuler) resEuler = fabs(e - ht[i * B + b]);
      if (fabs(ht[i * B + b]) > scaleTau) scaleTau = fabs(ht[i * B + b]);
    }
  for (int64_t k = 0; k < P * B; k++) {
    if (!(hfd[k] == hfd[k])) { fprintf(stderr, "grad_params has a NaN\n"); return 1; }
    if (fabs(hfd[k] + hid[k]) > resFd) resFd = fabs(hfd[k] + hid[k]);
    if (fabs(hfd[k] - hwr[k]) > resWr) resWr = fabs(hfd[k] - hwr[k]);
    if (fabs(hfd[k]) > scaleFd) scaleFd = fabs(hfd[k]);
  }
  /* accumulate adds */
  CHECK(nbl_forward_dynamics_backward_inertia(m, NULL, B, state, accel, NULL, NBL_ID_JOINT_FORCES, g, gpFd, 1, ws, wrBytes, NULL));
  HIP(hipDeviceSynchronize());
  HIP(hipMemcpy(hacc, gpFd, P * B * sizeof(double), hipMemcpyDeviceToHost));
  double resAcc = 0;
  for (int64_t k = 0; k < P * B; k++)
    if (fabs(hacc[k] - 2.0 * hfd[k]) > resAcc) resAcc = fabs(hacc[k] - 2.0 * hfd[k]);
  printf("max residuals euler %.3e forward %.3e wrench set %.3e accumulate %.3e |tau| %.3e |grad_params| %.3e\n", resEuler / scaleTau, resFd / scaleFd,
         resWr / scaleFd, resAcc / scaleFd, scaleTau, scaleFd);
  if (!(resEuler <= 1e-12 * scaleTau)) { fprintf(stderr, "sum_p m_p d tau / d m_p != tau\n"); return 1; }
  if (!(resFd <= 1e-10 * scaleFd)) { fprintf(stderr, "forward-dynamics gradient != -(inverse-dynamics gradient at (q, v, a), lambda)\n"); return 1; }
  if (!(resWr <= 1e-12 * scaleFd)) { fprintf(stderr, "a zero wrench changed the gradient\n"); return 1; }
  if (!(resAcc <= 1e-12 * scaleFd)) { fprintf(stderr, "accumulate does not add\n"); return 1; }
  if (!(scaleFd > 1.0)) { fprintf(stderr, "grad_params is zero\n"); return 1; }
  /* argument errors */
  EXPECT(nbl_inverse_dynamics_backward_inertia(NULL, B, state, accel, 0, g, gpId, 0, ws, wrBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_inverse_dynamics_backward_inertia(m, -1, state, accel, 0, g, gpId, 0, ws, wrBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_inverse_dynamics_backward_inertia(m, B, state, accel, 8, g, gpId, 0, ws, wrBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_inverse_dynamics_backward_inertia(m, B, state, accel, 0, g, NULL, 0, ws, wrBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_inverse_dynamics_backward_inertia(m, B, state, accel, 0, g, gpId, 0, ws, idBytes - 1, NULL), NBL_E_WORKSPACE);
  EXPECT(nbl_forward_dynamics_backward_inertia(m, NULL, B, state, accel, NULL, 0, g, NULL, 0, ws, wrBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_forward_dynamics_backward_inertia(m, NULL, B, state, accel, NULL, NBL_WRENCH_WORLD, g, gpId, 0, ws, wrBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_forward_dynamics_backward_inertia(m, NULL, B, state, accel, NULL, 0, g, gpId, 0, ws, fdBytes - 1, NULL), NBL_E_WORKSPACE);
  EXPECT(nbl_forward_dynamics_backward_inertia(m, km, B, state, accel, NULL, 0, g, gpId, 0, ws, wrBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_forward_dynamics_backward_inertia(m, km, B, state, accel, wrench, 0, g, NULL, 0, ws, wrBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_forward_dynamics_backward_inertia(m, km, B, state, accel, wrench, 0, g, gpId, 0, ws, wrBytes - 1, NULL), NBL_E_WORKSPACE);
  CHECK(nbl_forward_dynamics_backward_inertia(m, km, 0, state, accel, wrench, 0, g, gpId, 0, ws, wrBytes, NULL));
  nbl_kin_map_destroy(km);
  nbl_model_destroy(m);
  return 0;
}
