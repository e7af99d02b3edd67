/* The forward-dynamics and inverse-mass-matrix entry points from plain C99: nbl_forward_dynamics_forward / _backward,
 * nbl_inv_mass_matrix and nbl_inv_mass_apply on the Atlas-20 model of atlas20_ground_model.h, B worlds.  Checks from the library's own
 * outputs that  ID(q, v, FD(q, v, tau)) == tau  (nbl_inverse_dynamics_forward),  Minv M == I  (nbl_mass_matrix), that Minv is bitwise
 * symmetric, and that grad_tau == Minv g == nbl_inv_mass_apply(g); then the argument errors; prints "max residuals" for the test to read.
 * Exit status 0 = all checks passed. */
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
  const int n = MDL_N_DOFS;
  nbl_model_desc d;
  mdl_fill(&d);
  nbl_model* m = NULL;
  CHECK(nbl_model_create(&d, 0, &m));
  const size_t wsBytes = nbl_forward_dynamics_workspace_bytes(m, B), idBytes = nbl_dynamics_workspace_bytes(m, B);
  if (wsBytes == 0 || wsBytes < idBytes || nbl_forward_dynamics_workspace_bytes(NULL, B) != 0) { fprintf(stderr, "workspace bytes\n"); return 1; }
  double *state, *tau, *accel, *back, *M, *Minv, *g, *gstate, *gtau, *lam;
  void* ws;
  HIP(hipMalloc((void**)&state, 2 * n * B * sizeof(double))); HIP(hipMalloc((void**)&tau, n * B * sizeof(double)));
  HIP(hipMalloc((void**)&accel, n * B * sizeof(double))); HIP(hipMalloc((void**)&back, n * B * sizeof(double)));
  HIP(hipMalloc((void**)&M, (size_t)n * n * B * sizeof(double))); HIP(hipMalloc((void**)&Minv, (size_t)n * n * B * sizeof(double)));
  HIP(hipMalloc((void**)&g, n * B * sizeof(double))); HIP(hipMalloc((void**)&gstate, 2 * n * B * sizeof(double)));
  HIP(hipMalloc((void**)&gtau, n * B * sizeof(double))); HIP(hipMalloc((void**)&lam, n * B * sizeof(double)));
  HIP(hipMalloc(&ws, wsBytes));                       /* the larger of the two sizes serves both families of calls */
  double* hs = (double*)malloc(2 * n * B * sizeof(double));
  double* ht = (double*)malloc(n * B * sizeof(double));
  double* hg = (double*)malloc(n * B * sizeof(double));
  /* DOF-major layout [row][B]: rows 0 .. n-1 = q, rows n .. 2n-1 = v */
  for (int r = 0; r < 2 * n; r++)
    for (int64_t b = 0; b < B; b++) hs[r * B + b] = r < n ? 0.4 * sin(1.0 + 3.0 * (double)b + 7.0 * r) : 0.8 * cos(2.0 + 5.0 * (double)b + 11.0 * (r - n));
  for (int r = 0; r < n; r++)
    for (int64_t b = 0; b < B; b++) { ht[r * B + b] = 2.0 * sin(0.5 + (double)b + 1.3 * r); hg[r * B + b] = cos(0.25 + 2.0 * (double)b + 0.7 * r); }
  HIP(hipMemcpy(state, hs, 2 * n * B * sizeof(double), hipMemcpyHostToDevice));
  HIP(hipMemcpy(tau, ht, n * B * sizeof(double), hipMemcpyHostToDevice));
  HIP(hipMemcpy(g, hg, n * B * sizeof(double), hipMemcpyHostToDevice));
  CHECK(nbl_forward_dynamics_forward(m, B, state, tau, NBL_ID_JOINT_FORCES, accel, ws, wsBytes, NULL));
  CHECK(nbl_inverse_dynamics_forward(m, B, state, accel, NBL_ID_JOINT_FORCES, back, ws, wsBytes, NULL));
  CHECK(nbl_mass_matrix(m, B, state, M, ws, wsBytes, NULL));
  CHECK(nbl_inv_mass_matrix(m, B, state, Minv, ws, wsBytes, NULL));
  CHECK(nbl_forward_dynamics_backward(m, B, state, tau, NBL_ID_JOINT_FORCES, g, gstate, gtau, 0, ws, wsBytes, NULL));
  CHECK(nbl_inv_mass_apply(m, B, 1, state, g, lam, ws, wsBytes, NULL));
  HIP(hipDeviceSynchronize());
  double* hM = (double*)malloc((size_t)n * n * B * sizeof(double));
  double* hMi = (double*)malloc((size_t)n * n * B * sizeof(double));
  double* hb = (double*)malloc(n * B * sizeof(double));
  double* hgt = (double*)malloc(n * B * sizeof(double));
  double* hl = (double*)malloc(n * B * sizeof(double));
  double* hgs = (double*)malloc(2 * n * B * sizeof(double));
  HIP(hipMemcpy(hM, M, (size_t)n * n * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hMi, Minv, (size_t)n * n * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hb, back, n * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hgt, gtau, n * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hl, lam, n * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hgs, gstate, 2 * n * B * sizeof(double), hipMemcpyDeviceToHost));
  double resTau = 0, resEye = 0, resLam = 0, scaleTau = 1, scaleLam = 1, gsMax = 0;
  int asym = 0, apart = 0;
  for (int64_t b = 0; b < B; b++)
    for (int i = 0; i < n; i++) {
      double t = 0;
      for (int j = 0; j < n; j++) {
        double e = 0;
        for (int k = 0; k < n; k++) e += hMi[((size_t)i * n + k) * B + b] * hM[((size_t)k * n + j) * B + b];
        if (fabs(e - (i == j ? 1.0 : 0.0)) > resEye) resEye = fabs(e - (i == j ? 1.0 : 0.0));
        t += hMi[((size_t)i * n + j) * B + b] * hg[j * B + b];
        if (hMi[((size_t)i * n + j) * B + b] != hMi[((size_t)j * n + i) * B + b]) asym++;
      }
      if (fabs(hb[i * B + b] - ht[i * B + b]) > resTau) resTau = fabs(hb[i * B + b] - ht[i * B + b]);
      if (fabs(t - hgt[i * B + b]) > resLam) resLam = fabs(t - hgt[i * B + b]);
      if (fabs(hl[i * B + b] - hgt[i * B + b]) > 1e-10 * fabs(hgt[i * B + b]) + 1e-12) apart++;   /* the same recursion: nbl_inv_mass_apply(g) is grad_tau */
      if (fabs(ht[i * B + b]) > scaleTau) scaleTau = fabs(ht[i * B + b]);
      if (fabs(hgt[i * B + b]) > scaleLam) scaleLam = fabs(hgt[i * B + b]);
    }
  for (int64_t k = 0; k < 2 * n * B; k++) {
    if (!(hgs[k] == hgs[k])) { fprintf(stderr, "grad_state has a NaN\n"); return 1; }
    if (fabs(hgs[k]) > gsMax) gsMax = fabs(hgs[k]);
  }
  printf("max residuals %.3e %.3e %.3e asymmetric %d apart %d |grad_state| %.3e\n", resTau / scaleTau, resEye, resLam / scaleLam, asym, apart, gsMax);
  if (!(resTau <= 1e-10 * scaleTau)) { fprintf(stderr, "ID(FD(tau)) != tau\n"); return 1; }
  if (!(resEye <= 1e-10)) { fprintf(stderr, "Minv M != I\n"); return 1; }
  if (!(resLam <= 1e-10 * scaleLam)) { fprintf(stderr, "grad_tau != Minv g\n"); return 1; }
  if (apart) { fprintf(stderr, "nbl_inv_mass_apply(g) != grad_tau (%d entries)\n", apart); return 1; }
  if (asym) { fprintf(stderr, "Minv is not bitwise symmetric (%d entries)\n", asym); return 1; }
  if (!(gsMax > 0)) { fprintf(stderr, "grad_state is zero\n"); return 1; }
  /* argument errors */
  EXPECT(nbl_forward_dynamics_forward(NULL, B, state, tau, 0, accel, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_forward_dynamics_forward(m, -1, state, tau, 0, accel, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_forward_dynamics_forward(m, B, state, tau, 8, accel, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_forward_dynamics_forward(m, B, state, tau, 0, accel, ws, wsBytes - 1, NULL), NBL_E_WORKSPACE);
  EXPECT(nbl_forward_dynamics_backward(m, B, state, tau, 0, g, gstate, gtau, 0, ws, wsBytes / 2, NULL), NBL_E_WORKSPACE);
  EXPECT(nbl_inv_mass_apply(m, B, 0, state, g, lam, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_inv_mass_matrix(m, B, NULL, Minv, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_inv_mass_matrix(m, B, state, Minv, ws, 0, NULL), NBL_E_WORKSPACE);
  CHECK(nbl_inv_mass_matrix(m, 0, state, Minv, ws, wsBytes, NULL));
  nbl_model_destroy(m);
  return 0;
}
