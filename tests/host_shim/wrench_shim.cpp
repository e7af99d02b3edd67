// Host build of the product's wrench code (nimblephysics_amd/csrc/dynamics_dev.hpp: inverse and forward dynamics with wrenches on body
// frames, their reverse passes, contact inverse dynamics) for tests/test_wrench_host.py.  Test harness only.  The device body table comes
// from dyn_shim.cpp (shim_dyn_model), the plain forward-dynamics entry points from fdyn_shim.cpp, both included as they are; the entries
// are resolved as nbl_kin_map_create does it (the ancestor chain of the device body that carries T_cj, root first).
#include "fdyn_shim.cpp"

namespace {
struct ShimWrenchSet {
  std::vector<DevKinEntry> entries;
  std::vector<int32_t> path;
};
}  // namespace

extern "C" {
// body [count]: indices into the model description (-1: the world); T_offset [count][12] (null: identity)
void* shim_wrench_set(void* h, int count, const int32_t* body, const double* T_offset) {
  const ShimModel& m = *(const ShimModel*)h;
  ShimWrenchSet* s = new ShimWrenchSet();
  for (int k = 0; k < count; k++) {
    DevKinEntry e;
    std::memset(&e, 0, sizeof(e));
    e.kind = KIN_SPATIAL;
    e.row = 6 * k;
    for (int c = 0; c < 12; c++) e.T[c] = T_offset ? T_offset[12 * k + c] : I12[c];
    std::vector<int32_t> chain;
    for (int i = body[k] < 0 ? -1 : m.bodyMap[body[k]]; i >= 0; i = m.bodies[i].parent) chain.push_back(i);
    e.pathBegin = (int32_t)s->path.size();
    e.pathLen = (int32_t)chain.size();
    s->path.insert(s->path.end(), chain.rbegin(), chain.rend());
    s->entries.push_back(e);
  }
  return s;
}
void shim_wrench_set_free(void* s) { delete (ShimWrenchSet*)s; }

// tau [n][B] = M a + C - sum_e J_e^T W_e
void shim_wrench_id(void* h, void* set, int64_t B, const double* state, const double* accel, const double* wrench, int flags, double* tau) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimWrenchSet& s = *(const ShimWrenchSet*)set;
  const int nb = (int)m.bodies.size();
  std::vector<double> ws((size_t)nb * DYN_SLOTS * B, NAN);
  for (int64_t b = 0; b < B; b++)
    idForwardWorldT<true>(m.bodies.data(), m.dofs.data(), nb, m.n, m.gravity, m.dt, flags, B, b, state, accel, tau, ws.data(), s.entries.data(),
                          s.path.data(), (int)s.entries.size(), wrench);
}

// the reverse pass: gstate [2n][B], gaccel [n][B], gwrench [6 E][B] (any may be null)
void shim_wrench_id_vjp(void* h, void* set, int64_t B, const double* state, const double* accel, const double* wrench, int flags, const double* gtau,
                        double* gstate, double* gaccel, double* gwrench, int accumulate) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimWrenchSet& s = *(const ShimWrenchSet*)set;
  const int nb = (int)m.bodies.size();
  std::vector<double> ws((size_t)nb * DYN_SLOTS * B, NAN), wx((size_t)nb * 3 * B, NAN);
  for (int64_t b = 0; b < B; b++)
    idVjpWorldT<true>(m.bodies.data(), m.dofs.data(), nb, m.n, m.gravity, m.dt, flags, B, b, state, accel, gtau, gstate, gaccel, accumulate, ws.data(),
                      s.entries.data(), s.path.data(), (int)s.entries.size(), wrench, gwrench, wx.data());
}

// accel [n][B] = M^-1 (tau + sum_e J_e^T W_e - C)
void shim_wrench_fd(void* h, void* set, int64_t B, const double* state, const double* tau, const double* wrench, int flags, double* accel) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimWrenchSet& s = *(const ShimWrenchSet*)set;
  const int nb = (int)m.bodies.size();
  std::vector<double> ws((size_t)nb * FD_SLOTS * B, NAN);
  for (int64_t b = 0; b < B; b++)
    fdForwardWorldT<true>(m.bodies.data(), m.dofs.data(), nb, m.n, m.gravity, m.dt, flags, B, b, state, tau, accel, ws.data(), s.entries.data(),
                          s.path.data(), (int)s.entries.size(), wrench);
}

// the reverse pass as nbl_forward_dynamics_wrench_backward runs it: fdLambdaWrenchWorld, then idVjpWorldT<true> at (q, v, a) with -lambda
void shim_wrench_fd_vjp(void* h, void* set, int64_t B, const double* state, const double* tau, const double* wrench, int flags, const double* gaccel,
                        double* gstate, double* gtau, double* gwrench, int accumulate) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimWrenchSet& s = *(const ShimWrenchSet*)set;
  const int nb = (int)m.bodies.size(), E = (int)s.entries.size();
  std::vector<double> ws((size_t)nb * FD_SLOTS * B, NAN), accel((size_t)m.n * B, NAN), neglam((size_t)m.n * B, NAN), wx((size_t)nb * 3 * B, NAN);
  for (int64_t b = 0; b < B; b++)
    fdLambdaWrenchWorld(m.bodies.data(), m.dofs.data(), nb, m.n, m.gravity, m.dt, flags, B, b, state, tau, gaccel, accel.data(), neglam.data(), gtau,
                        accumulate, ws.data(), s.entries.data(), s.path.data(), E, wrench);
  if (gstate || gwrench)
    for (int64_t b = 0; b < B; b++)
      idVjpWorldT<true>(m.bodies.data(), m.dofs.data(), nb, m.n, m.gravity, m.dt, flags, B, b, state, accel.data(), neglam.data(), gstate, nullptr,
                        accumulate, ws.data(), s.entries.data(), s.path.data(), E, wrench, gwrench, wx.data());
}

// the root body nbl_contact_inverse_dynamics requires (-1: NBL_E_UNSUPPORTED)
int shim_wrench_cid_root(void* h, void* set) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimWrenchSet& s = *(const ShimWrenchSet*)set;
  return cidRoot(m.bodies.data(), s.entries.data(), s.path.data(), (int)s.entries.size());
}

// contact inverse dynamics: wout [6 E][B], tau [n][B].  The caller has checked what nbl_contact_inverse_dynamics checks (one free root).
void shim_wrench_cid(void* h, void* set, int64_t B, const double* state, const double* accel, const double* guess, int mode, int flags, double* wout,
                     double* tau) {
  const ShimModel& m = *(const ShimModel*)h;
  const ShimWrenchSet& s = *(const ShimWrenchSet*)set;
  const int nb = (int)m.bodies.size(), E = (int)s.entries.size();
  std::vector<double> ws((size_t)nb * DYN_SLOTS * B, NAN), xs((size_t)E * 12 * B, NAN);
  for (int64_t b = 0; b < B; b++)
    cidWorld(m.bodies.data(), m.dofs.data(), nb, m.n, m.gravity, m.dt, flags, mode, B, b, state, accel, s.entries.data(), s.path.data(), E, guess, wout,
             tau, ws.data(), xs.data());
}
}
