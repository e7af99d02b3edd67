/* The joint-space dynamics entry points from plain C99: nbl_mass_matrix, nbl_inverse_dynamics_forward (with accelerations,
 * and with accel = NULL: the Coriolis-and-gravity vector) and nbl_inverse_dynamics_backward on the Atlas-20 model of
 * atlas20_ground_model.h, B worlds.  Checks from the library's own outputs that  M a + C == tau  and that  grad_accel == M^T g,
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

int main(int argc, char** argv) {
  const int64_t B = argc > 1 ? atoll(argv[1]) : 8;
  const int n = MDL_N_DOFS;
  if ((nbl_version() & 0xffff) < 5) { fprintf(stderr, "ABI minor %d < 5\n", nbl_version() & 0xffff); return 1; }
  nbl_model_desc d;
  mdl_fill(&d);
  nbl_model* m = NULL;
  CHECK(nbl_model_create(&d, 0, &m));
  const size_t wsBytes = nbl_dynamics_workspace_bytes(m, B);
  if (wsBytes == 0 || nbl_dynamics_workspace_bytes(NULL, B) != 0) { fprintf(stderr, "workspace bytes\n"); return 1; }
  double *state, *accel, *tau, *cg, *M, *g, *gstate, *gaccel;
  void* ws;
  HIP(hipMalloc((void**)&state, 2 * n * B * sizeof(double))); HIP(hipMalloc((void**)&accel, n * B * sizeof(double)));
  HIP(hipMalloc((void**)&tau, n * B * sizeof(double))); HIP(hipMalloc((void**)&cg, n * B * sizeof(double)));
  HIP(hipMalloc((void**)&M, (size_t)n * n * B * sizeof(double))); HIP(hipMalloc((void**)&g, n * B * sizeof(double)));
  HIP(hipMalloc((void**)&gstate, 2 * n * B * sizeof(double))); HIP(hipMalloc((void**)&gaccel, n * B * sizeof(double)));
  HIP(hipMalloc(&ws, wsBytes));
  double* hs = (double*)malloc(2 * n * B * sizeof(double));
  double* ha = (double*)malloc(n * B * sizeof(double));
  double* hg = (double*)malloc(n * B * sizeof(double));
  /* DOF-major layout [row][B]: rows 0 .. n-1 = q, rows n .. 2n-1 = v */
  for (int r = 0; r < 2 * n; r++)
    for (int64_t b = 0; b < B; b++) hs[r * B + b] = r < n ? 0.4 * sin(1.0 + 3.0 * (double)b + 7.0 * r) : 0.8 * cos(2.0 + 5.0 * (double)b + 11.0 * (r - n));
  for (int r = 0; r < n; r++)
    for (int64_t b = 0; b < B; b++) { ha[r * B + b] = 2.0 * sin(0.5 + (double)b + 1.3 * r); hg[r * B + b] = cos(0.25 + 2.0 * (double)b + 0.7 * r); }
  HIP(hipMemcpy(state, hs, 2 * n * B * sizeof(double), hipMemcpyHostToDevice));
  HIP(hipMemcpy(accel, ha, n * B * sizeof(double), hipMemcpyHostToDevice));
  HIP(hipMemcpy(g, hg, n * B * sizeof(double), hipMemcpyHostToDevice));
  CHECK(nbl_mass_matrix(m, B, state, M, ws, wsBytes, NULL));
  CHECK(nbl_inverse_dynamics_forward(m, B, state, NULL, 0, cg, ws, wsBytes, NULL));
  CHECK(nbl_inverse_dynamics_forward(m, B, state, accel, 0, tau, ws, wsBytes, NULL));
  CHECK(nbl_inverse_dynamics_backward(m, B, state, accel, 0, g, gstate, gaccel, 0, ws, wsBytes, NULL));
  HIP(hipDeviceSynchronize());
  double* hM = (double*)malloc((size_t)n * n * B * sizeof(double));
  double* ht = (double*)malloc(n * B * sizeof(double));
  double* hc = (double*)malloc(n * B * sizeof(double));
  double* hga = (double*)malloc(n * B * sizeof(double));
  HIP(hipMemcpy(hM, M, (size_t)n * n * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(ht, tau, n * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hc, cg, n * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hga, gaccel, n * B * sizeof(double), hipMemcpyDeviceToHost));
  double resTau = 0, resGa = 0, scaleTau = 1, scaleGa = 1;
  int asym = 0;
  for (int64_t b = 0; b < B; b++)
    for (int i = 0; i < n; i++) {
      double s = hc[i * B + b], t = 0;
      for (int j = 0; j < n; j++) {
        s += hM[((size_t)i * n + j) * B + b] * ha[j * B + b];
        t += hM[((size_t)j * n + i) * B + b] * hg[j * B + b];
        if (hM[((size_t)i * n + j) * B + b] != hM[((size_t)j * n + i) * B + b]) asym++;
      }
      if (fabs(s - ht[i * B + b]) > resTau) resTau = fabs(s - ht[i * B + b]);
      if (fabs(t - hga[i * B + b]) > resGa) resGa = fabs(t - hga[i * B + b]);
      if (fabs(ht[i * B + b]) > scaleTau) scaleTau = fabs(ht[i * B + b]);
      if (fabs(hga[i * B + b]) > scaleGa) scaleGa = fabs(hga[i * B + b]);
    }
  printf("max residuals %.3e %.3e asymmetric %d\n", resTau / scaleTau, resGa / scaleGa, asym);
  if (!(resTau <= 1e-10 * scaleTau)) { fprintf(stderr, "M a + C != tau\n"); return 1; }
  if (!(resGa <= 1e-10 * scaleGa)) { fprintf(stderr, "grad_accel != M^T g\n"); return 1; }
  if (asym) { fprintf(stderr, "M is not bitwise symmetric (%d entries)\n", asym); return 1; }
  /* argument errors */
  EXPECT(nbl_inverse_dynamics_forward(NULL, B, state, accel, 0, tau, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_inverse_dynamics_forward(m, -1, state, accel, 0, tau, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_inverse_dynamics_forward(m, B, state, accel, 8, tau, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_inverse_dynamics_forward(m, B, state, accel, 0, tau, ws, wsBytes - 1, NULL), NBL_E_WORKSPACE);
  EXPECT(nbl_inverse_dynamics_backward(m, B, state, accel, 0, g, gstate, gaccel, 0, ws, wsBytes / 2, NULL), NBL_E_WORKSPACE);
  EXPECT(nbl_mass_matrix(m, B, NULL, M, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_mass_matrix(m, B, state, M, ws, 0, NULL), NBL_E_WORKSPACE);
  CHECK(nbl_mass_matrix(m, 0, state, M, ws, wsBytes, NULL));
  nbl_model_destroy(m);
  return 0;
}
