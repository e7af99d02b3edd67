// Host build of the product's task-space code (nimblephysics_amd/csrc/taskspace_dev.hpp) for tests/test_taskspace_host.py and for the
// stand-alone sanitizer program task_main.cpp.  Test harness only.  The device body table comes from dyn_shim.cpp (shim_dyn_model); the
// entries are resolved as nbl_kin_map_create resolves them (kinds, rows in entry order, the ancestor chain of the device body that carries
// T_cj, root first).
#include "wrench_shim.cpp"

#include "taskspace_dev.hpp"

extern "C" {
// kind [count]: KIN_SPATIAL / KIN_LINEAR / KIN_ANGULAR; body [count]: indices into the model description (-1: the world); T_offset [count][12]
void* shim_task_set(void* h, int count, const int32_t* kind, const int32_t* body, const double* T_offset) {
  ShimWrenchSet* s = (ShimWrenchSet*)shim_wrench_set(h, count, body, T_offset);
  int row = 0;
  for (int k = 0; k < count; k++) {
    s->entries[k].kind = kind[k];
    s->entries[k].row = row;
    row += kinRows(kind[k]);
  }
  return s;
}
int shim_task_rows(void* set) {
  const ShimWrenchSet& s = *(const ShimWrenchSet*)set;
  return s.entries.empty() ? 0 : s.entries.back().row + kinRows(s.entries.back().kind);
}

// state [2n][B]; J, Jdot [R n][B] (either may be null)
void shim_task_jacobian(void* h, void* set, int64_t B, const double* state, double* J, double* Jdot) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimWrenchSet& s = *(const ShimWrenchSet*)set;
  for (int64_t b = 0; b < B; b++) {
    if (J) taskJacobianWorld(m.bodies.data(), s.entries.data(), s.path.data(), (int)s.entries.size(), m.n, B, b, state, J);
    if (Jdot) taskJacobianDerivWorld(m.bodies.data(), s.entries.data(), s.path.data(), (int)s.entries.size(), m.n, B, b, state, Jdot);
  }
}

// G [R n][B] -> gq [n][B]
void shim_task_jacobian_vjp(void* h, void* set, int64_t B, const double* state, const double* G, double* gq, int accumulate) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimWrenchSet& s = *(const ShimWrenchSet*)set;
  for (int64_t b = 0; b < B; b++)
    taskJacobianVjpWorld(m.bodies.data(), s.entries.data(), s.path.data(), (int)s.entries.size(), m.n, B, b, state, G, gq, accumulate);
}

// out [R][B]: J accel + Jdot v, or - accel null - Jdot v
void shim_task_accel(void* h, void* set, int64_t B, const double* state, const double* accel, double* out) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimWrenchSet& s = *(const ShimWrenchSet*)set;
  for (int64_t b = 0; b < B; b++)
    taskAccelWorld(m.bodies.data(), s.entries.data(), s.path.data(), (int)s.entries.size(), m.n, B, b, state, accel, out);
}

void shim_task_accel_vjp(void* h, void* set, int64_t B, const double* state, const double* accel, const double* gout, double* gstate,
                         double* gaccel, int accumulate) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimWrenchSet& s = *(const ShimWrenchSet*)set;
  const int nb = (int)m.bodies.size();
  std::vector<double> ws((size_t)nb * CEN_SLOTS * B, NAN);     // NaN: a slot read before it is written shows
  for (int64_t b = 0; b < B; b++)
    taskAccelVjpWorld(m.bodies.data(), nb, m.n, s.entries.data(), s.path.data(), (int)s.entries.size(), B, b, state, accel, gout, gstate, gaccel,
                      accumulate, ws.data());
}
}
