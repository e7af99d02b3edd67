// Host build of the product's forward dynamics and inverse mass matrix (the second half of nimblephysics_amd/csrc/dynamics_dev.hpp) for
// tests/test_fdyn_host.py.  Test harness only.  The device body table comes from dyn_shim.cpp (shim_dyn_model), included as it is.
#include "dyn_shim.cpp"

extern "C" {
int shim_fdyn_slots(void) { return FD_SLOTS; }

// accel [n][B] = M^-1 (tau - C) of state [2n][B] and tau [n][B] (null: 0)
void shim_fdyn_forward(void* h, int64_t B, const double* state, const double* tau, int flags, double* accel) {
  const ShimModel& m = *(const ShimModel*)h;
  const int nb = (int)m.bodies.size();
  std::vector<double> ws((size_t)nb * FD_SLOTS * B, NAN);      // NaN: a slot read before it is written shows
  for (int64_t b = 0; b < B; b++) fdForwardWorld(m.bodies.data(), m.dofs.data(), nb, m.n, m.gravity, m.dt, flags, B, b, state, tau, accel, ws.data());
}

// the reverse pass as nbl_forward_dynamics_backward runs it: fdLambdaWorld, then idVjpWorld at (q, v, a) with the cotangent -lambda on the
// same tree slots.  gstate [2n][B] / gtau [n][B]: either may be null.
void shim_fdyn_backward(void* h, int64_t B, const double* state, const double* tau, int flags, const double* gaccel, double* gstate, double* gtau,
                        int accumulate) {
  const ShimModel& m = *(const ShimModel*)h;
  const int nb = (int)m.bodies.size();
  static_assert(DYN_SLOTS <= FD_SLOTS, "idVjpWorld runs on the forward-dynamics tree slots");
  std::vector<double> ws((size_t)nb * FD_SLOTS * B, NAN), accel((size_t)m.n * B, NAN), neglam((size_t)m.n * B, NAN);
  for (int64_t b = 0; b < B; b++)
    fdLambdaWorld(m.bodies.data(), m.dofs.data(), nb, m.n, m.gravity, m.dt, flags, B, b, state, tau, gaccel, accel.data(), neglam.data(), gtau, accumulate,
                  ws.data());
  if (gstate)
    for (int64_t b = 0; b < B; b++)
      idVjpWorld(m.bodies.data(), m.dofs.data(), nb, m.n, m.gravity, m.dt, flags, B, b, state, accel.data(), neglam.data(), gstate, nullptr, accumulate,
                 ws.data());
}

// Y [R][n][B] = M^-1 X [R][n][B];  X null (R = n): Y = M^-1, [n * n][B]
void shim_fdyn_minv(void* h, int64_t B, int R, const double* state, const double* X, double* Y) {
  const ShimModel& m = *(const ShimModel*)h;
  const int nb = (int)m.bodies.size();
  std::vector<double> ws((size_t)nb * FD_SLOTS * B, NAN);
  for (int64_t b = 0; b < B; b++) minvApplyWorld(m.bodies.data(), nb, m.n, B, b, state, R, X, Y, ws.data());
}
}
