/* Wrenches on bodies and contact inverse dynamics from plain C99: nbl_contact_inverse_dynamics, nbl_forward_dynamics_wrench_forward and
 * nbl_inverse_dynamics_wrench_forward on the Atlas-20 model of atlas20_ground_model.h with a wrench set on its two feet (bodies 8 and 14
 * of the description), B worlds.  Checks from the library's own outputs that the torques of the min-torque contact solve have zero root
 * rows, that forward dynamics with the returned (tau, wrenches) reproduces the accelerations (the reference's sumError), that inverse
 * dynamics with those wrenches returns tau outside the root rows and 0 +- rounding in them, and that a NULL set gives the bits of
 * nbl_inverse_dynamics_forward; then the argument errors; prints "max residuals" for the test to read.  Exit status 0 = all checks passed. */
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
  const int n = MDL_N_DOFS, E = 2;
  nbl_model_desc d;
  mdl_fill(&d);
  nbl_model* m = NULL;
  CHECK(nbl_model_create(&d, 0, &m));
  const int32_t kinds[2] = {NBL_KIN_SPATIAL, NBL_KIN_SPATIAL}, feet[2] = {8, 14}, linear[1] = {NBL_KIN_LINEAR};
  nbl_kin_map *k = NULL, *klin = NULL;
  CHECK(nbl_kin_map_create(m, E, kinds, feet, NULL, &k));
  CHECK(nbl_kin_map_create(m, 1, linear, feet, NULL, &klin));
  const size_t wsBytes = nbl_wrench_workspace_bytes(m, k, B);
  if (wsBytes < nbl_forward_dynamics_workspace_bytes(m, B) || nbl_wrench_workspace_bytes(NULL, k, B) != 0 ||
      nbl_wrench_workspace_bytes(m, NULL, B) >= wsBytes) { fprintf(stderr, "workspace bytes\n"); return 1; }
  double *state, *accel, *W, *tau, *back, *tid, *plain, *plain0;
  void* ws;
  HIP(hipMalloc((void**)&state, 2 * n * B * sizeof(double))); HIP(hipMalloc((void**)&accel, n * B * sizeof(double)));
  HIP(hipMalloc((void**)&W, 6 * E * B * sizeof(double))); HIP(hipMalloc((void**)&tau, n * B * sizeof(double)));
  HIP(hipMalloc((void**)&back, n * B * sizeof(double))); HIP(hipMalloc((void**)&tid, n * B * sizeof(double)));
  HIP(hipMalloc((void**)&plain, n * B * sizeof(double))); HIP(hipMalloc((void**)&plain0, n * B * sizeof(double)));
  HIP(hipMalloc(&ws, wsBytes));
  double* hs = (double*)malloc(2 * n * B * sizeof(double));
  double* ha = (double*)malloc(n * B * sizeof(double));
  for (int r = 0; r < 2 * n; r++)
    for (int64_t b = 0; b < B; b++) hs[r * B + b] = r < n ? 0.4 * sin(1.0 + 3.0 * (double)b + 7.0 * r) : 0.8 * cos(2.0 + 5.0 * (double)b + 11.0 * (r - n));
  for (int r = 0; r < n; r++)
    for (int64_t b = 0; b < B; b++) ha[r * B + b] = 2.0 * sin(0.5 + (double)b + 1.3 * r);
  HIP(hipMemcpy(state, hs, 2 * n * B * sizeof(double), hipMemcpyHostToDevice));
  HIP(hipMemcpy(accel, ha, n * B * sizeof(double), hipMemcpyHostToDevice));
  CHECK(nbl_contact_inverse_dynamics(m, k, B, state, accel, NULL, NBL_CID_MIN_TORQUE, NBL_ID_JOINT_FORCES, W, tau, ws, wsBytes, NULL));
  CHECK(nbl_forward_dynamics_wrench_forward(m, k, B, state, tau, W, NBL_ID_JOINT_FORCES, back, ws, wsBytes, NULL));
  CHECK(nbl_inverse_dynamics_wrench_forward(m, k, B, state, accel, W, NBL_ID_JOINT_FORCES, tid, ws, wsBytes, NULL));
  CHECK(nbl_inverse_dynamics_wrench_forward(m, NULL, B, state, accel, NULL, NBL_ID_JOINT_FORCES, plain0, ws, wsBytes, NULL));
  CHECK(nbl_inverse_dynamics_forward(m, B, state, accel, NBL_ID_JOINT_FORCES, plain, ws, wsBytes, NULL));
  HIP(hipDeviceSynchronize());
  double* hW = (double*)malloc(6 * E * B * sizeof(double));
  double* ht = (double*)malloc(n * B * sizeof(double));
  double* hb = (double*)malloc(n * B * sizeof(double));
  double* hi = (double*)malloc(n * B * sizeof(double));
  double* hp = (double*)malloc(n * B * sizeof(double));
  double* hp0 = (double*)malloc(n * B * sizeof(double));
  HIP(hipMemcpy(hW, W, 6 * E * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(ht, tau, n * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hb, back, n * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hi, tid, n * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hp, plain, n * B * sizeof(double), hipMemcpyDeviceToHost));
  HIP(hipMemcpy(hp0, plain0, n * B * sizeof(double), hipMemcpyDeviceToHost));
  double resAcc = 0, resTau = 0, scaleAcc = 1, scaleTau = 1, wMax = 0;
  int rootNonZero = 0, differ = 0;
  for (int64_t b = 0; b < B; b++)
    for (int i = 0; i < n; i++) {
      const int64_t x = i * B + b;
      if (i < 6 && ht[x] != 0.0) rootNonZero++;
      if (fabs(hb[x] - ha[x]) > resAcc) resAcc = fabs(hb[x] - ha[x]);
      if (fabs(hi[x] - ht[x]) > resTau) resTau = fabs(hi[x] - ht[x]);
      if (fabs(ha[x]) > scaleAcc) scaleAcc = fabs(ha[x]);
      if (fabs(hp[x]) > scaleTau) scaleTau = fabs(hp[x]);
      if (memcmp(&hp[x], &hp0[x], sizeof(double)) != 0) differ++;
    }
  for (int64_t x = 0; x < 6 * E * B; x++) {
    if (!(hW[x] == hW[x])) { fprintf(stderr, "a wrench is NaN\n"); return 1; }
    if (fabs(hW[x]) > wMax) wMax = fabs(hW[x]);
  }
  printf("max residuals %.3e %.3e root rows not zero %d differ %d |wrench| %.3e\n", resAcc / scaleAcc, resTau / scaleTau, rootNonZero, differ, wMax);
  if (rootNonZero) { fprintf(stderr, "root rows of tau are not 0\n"); return 1; }
  if (!(resAcc <= 1e-9 * scaleAcc)) { fprintf(stderr, "FD(tau, W) != a\n"); return 1; }
  if (!(resTau <= 1e-10 * scaleTau)) { fprintf(stderr, "ID(a, W) != tau\n"); return 1; }
  if (differ) { fprintf(stderr, "a NULL wrench set does not give the bits of nbl_inverse_dynamics_forward (%d entries)\n", differ); return 1; }
  if (!(wMax > 0)) { fprintf(stderr, "the wrenches are zero\n"); return 1; }
  /* argument errors */
  EXPECT(nbl_contact_inverse_dynamics(m, NULL, B, state, accel, NULL, NBL_CID_MIN_TORQUE, 0, W, tau, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_contact_inverse_dynamics(m, k, B, state, accel, NULL, NBL_CID_MIN_TORQUE, NBL_WRENCH_WORLD, W, tau, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_contact_inverse_dynamics(m, k, B, state, accel, NULL, NBL_CID_SINGLE, 0, W, tau, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_contact_inverse_dynamics(m, k, B, state, accel, NULL, NBL_CID_NEAREST, 0, W, tau, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_contact_inverse_dynamics(m, k, B, state, accel, NULL, 3, 0, W, tau, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_contact_inverse_dynamics(m, klin, B, state, accel, NULL, NBL_CID_SINGLE, 0, W, tau, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_contact_inverse_dynamics(m, k, B, state, accel, NULL, NBL_CID_MIN_TORQUE, 0, W, tau, ws, wsBytes - 1, NULL), NBL_E_WORKSPACE);
  EXPECT(nbl_inverse_dynamics_wrench_forward(m, k, B, state, accel, NULL, 0, tid, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_inverse_dynamics_wrench_forward(m, k, B, state, accel, W, 16, tid, ws, wsBytes, NULL), NBL_E_BADARG);
  EXPECT(nbl_inverse_dynamics_forward(m, B, state, accel, NBL_WRENCH_WORLD, tid, ws, wsBytes, NULL), NBL_E_BADARG);
  CHECK(nbl_contact_inverse_dynamics(m, k, 0, NULL, NULL, NULL, NBL_CID_MIN_TORQUE, 0, NULL, NULL, NULL, 0, NULL));
  nbl_kin_map_destroy(klin);
  nbl_kin_map_destroy(k);
  nbl_model_destroy(m);
  return 0;
}
