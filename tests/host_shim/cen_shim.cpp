// Host build of the product's centre-of-mass family (nimblephysics_amd/csrc/centroidal_dev.hpp) for tests/test_centroidal_host.py and
// for the stand-alone sanitizer program cen_main.cpp.  Test harness only.  The device body table comes from dyn_shim.cpp; the body set is
// restated here from nbl_body_set_create (nimble_amd.hip): the mass on the body that carries T_cj, the springs on the whole chain.
#include "dyn_shim.cpp"

#include "centroidal_dev.hpp"

extern "C" {
// bodies: `count` indices of the description the model was made from (count 0: every body); masks[0] = mass, masks[1] = joints;
// moments (may be null): [bodies of the description][3], the origin moments of nbl_body_set_origin_moments -> origin [3 * 64] per device body
void shim_cen_set(void* h, int count, const int32_t* bodies, uint64_t* masks, const double* moments, double* origin) {
  const ShimModel& m = *(const ShimModel*)h;
  masks[0] = masks[1] = 0;
  for (int k = 0; k < 3 * CEN_MAX_BODIES; k++) origin[k] = 0.0;
  if (moments)
    for (size_t k = 0; k < m.bodyMap.size(); k++)
      for (int c = 0; c < 3; c++) origin[3 * m.bodyMap[k] + c] = moments[3 * k + c];
  const int total = count > 0 ? count : (int)m.bodyMap.size();
  for (int k = 0; k < total; k++) {
    int i = m.bodyMap[count > 0 ? bodies[k] : k];
    masks[0] |= 1ull << i;
    masks[1] |= 1ull << i;
    while ((m.bodies[i].jtype == JT_BALL || m.bodies[i].jtype == JT_FREEC) && m.bodies[i].ballComp > 0) {
      i = m.bodies[i].parent;
      masks[1] |= 1ull << i;
    }
  }
}
double shim_cen_mass(void* h, uint64_t mass) {
  const ShimModel& m = *(const ShimModel*)h;
  return cenTotalMass(m.bodies.data(), (int)m.bodies.size(), mass);
}
int shim_cen_slots(void) { return CEN_SLOTS; }

void shim_cen_forward(void* h, uint64_t mass, uint64_t joints, int64_t B, const double* state, const double* accel, int flags, const double* origin, double* com,
                      double* vel, double* acc, double* mom, double* ke, double* pe, double* Jcom) {
  const ShimModel& m = *(const ShimModel*)h;
  const int nb = (int)m.bodies.size();
  std::vector<double> ws((size_t)nb * CEN_SLOTS * B, NAN);     // NaN: a slot read before it is written shows
  DevBodySet set{};
  set.mass = mass; set.joints = joints;
  if (origin) std::memcpy(set.originMoment, origin, sizeof(set.originMoment));
  for (int64_t b = 0; b < B; b++)
    cenForwardWorld(m.bodies.data(), m.dofs.data(), nb, m.n, m.gravity, set, flags, B, b, state, accel, com, vel, acc, mom, ke, pe, Jcom, ws.data());
}

void shim_cen_vjp(void* h, uint64_t mass, uint64_t joints, int64_t B, const double* state, const double* accel, int flags, const double* origin, const double* gcom,
                  const double* gvel, const double* gacc, const double* gmom, const double* gke, const double* gpe, double* gstate,
                  double* gaccel, int accumulate) {
  const ShimModel& m = *(const ShimModel*)h;
  const int nb = (int)m.bodies.size();
  std::vector<double> ws((size_t)nb * CEN_SLOTS * B, NAN);
  DevBodySet set{};
  set.mass = mass; set.joints = joints;
  if (origin) std::memcpy(set.originMoment, origin, sizeof(set.originMoment));
  for (int64_t b = 0; b < B; b++)
    cenVjpWorld(m.bodies.data(), m.dofs.data(), nb, m.n, m.gravity, set, flags, B, b, state, accel, gcom, gvel, gacc, gmom, gke, gpe, gstate,
                gaccel, accumulate, ws.data());
}
}
