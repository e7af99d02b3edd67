// Host build of the product's inertia-parameter gradient of inverse dynamics (idInertiaVjpWorld of nimblephysics_amd/csrc/dynamics_dev.hpp)
// for tests/test_dynamics_mass_host.py.  Test harness only.  The device body table comes from dyn_shim.cpp (shim_dyn_model), included as
// it is; the parameter table is restated from nbl_set_inertia_params_on (nimble_amd.hip): the carrying device body and the symmetric
// half of dG.
#include "dyn_shim.cpp"

extern "C" {
// state [2n][B], accel [n][B] or null, gtau [n][B]; `count` parameters on the bodies `bodies` (indices of the description the model was
// made from) with the directions dG [count][36]; gparams [count][B] (= or +=).
void shim_dynmass_run(void* h, int64_t B, const double* state, const double* accel, int flags, const double* gtau, int count,
                      const int32_t* bodies, const double* dG, double* gparams, int accumulate) {
  const ShimModel& m = *(const ShimModel*)h;
  const int nb = (int)m.bodies.size();
  std::vector<DevInertiaParam> table(count);
  for (int p = 0; p < count; p++) {
    table[p].body = m.bodyMap[bodies[p]];
    table[p].pad = 0;
    const double* D = dG + 36 * (size_t)p;
    int idx = 0;
    for (int r = 0; r < 6; r++)
      for (int c = r; c < 6; c++) table[p].dG[idx++] = 0.5 * (D[6 * r + c] + D[6 * c + r]);
  }
  std::vector<double> ws((size_t)nb * DYN_SLOTS * B, NAN);     // NaN: a slot read before it is written shows
  for (int64_t b = 0; b < B; b++)
    idInertiaVjpWorld(m.bodies.data(), nb, m.n, m.gravity, flags, B, b, state, accel, gtau, table.data(), count, gparams, accumulate, ws.data());
}
}
