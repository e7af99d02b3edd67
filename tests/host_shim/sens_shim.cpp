// Host build of the product's inertial-sensor code (nimblephysics_amd/csrc/sensors_dev.hpp) for tests/test_sensors_host.py and for the
// stand-alone sanitizer program sens_main.cpp.  Test harness only.  The device body table comes from dyn_shim.cpp (shim_dyn_model), the
// sensor set is the wrench set of wrench_shim.cpp (shim_wrench_set: spatial entries resolved as nbl_kin_map_create resolves them).
#include "wrench_shim.cpp"

#include "sensors_dev.hpp"

extern "C" {
int shim_sens_slots(void) { return CEN_SLOTS; }

// state [2n][B], accel [n][B], field [3][B]; gyro, acc, mag [3 S][B] (any may be null)
void shim_sens_forward(void* h, void* set, int64_t B, const double* state, const double* accel, const double* field, double* gyro, double* acc,
                       double* mag) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimWrenchSet& s = *(const ShimWrenchSet*)set;
  const int nb = (int)m.bodies.size();
  std::vector<double> ws((size_t)nb * CEN_SLOTS * B, NAN);     // NaN: a slot read before it is written shows
  for (int64_t b = 0; b < B; b++)
    sensForwardWorld(m.bodies.data(), nb, m.n, m.gravity, s.entries.data(), s.path.data(), (int)s.entries.size(), B, b, state, accel, field, gyro,
                     acc, mag, ws.data());
}

void shim_sens_vjp(void* h, void* set, int64_t B, const double* state, const double* accel, const double* field, const double* ggyro,
                   const double* gacc, const double* gmag, double* gstate, double* gaccel, double* gfield, int accumulate) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimWrenchSet& s = *(const ShimWrenchSet*)set;
  const int nb = (int)m.bodies.size();
  std::vector<double> ws((size_t)nb * CEN_SLOTS * B, NAN);
  for (int64_t b = 0; b < B; b++)
    sensVjpWorld(m.bodies.data(), nb, m.n, m.gravity, s.entries.data(), s.path.data(), (int)s.entries.size(), B, b, state, accel, field, ggyro,
                 gacc, gmag, gstate, gaccel, gfield, accumulate, ws.data());
}
}
