// nimble_amd_tree.hip — the 43 contact-independent entry points of include/nimble_amd.h: world-space kinematics, inverse and forward dynamics,
// mass matrix and its inverse, wrenches, contact inverse dynamics, inertia-parameter gradients, IK, centroidal quantities, sensors,
// task-space Jacobians and accelerations and the reverse pass of IK.
//
// None of them depends on the contact capacity, so they are built ONCE (device namespace nbl_tree) and not once per instantiation of the
// contact stage (abi_variants.h): every call works on the capacity-independent base of the handle, nbl_tree_model (tree_model_host.hpp),
// whichever instantiation owns it.  Thin like nimble_amd.hip: checks, then launches on the caller's stream.
#ifdef NBL_TREE_STANDALONE
// included at the end of nimble_amd.hip built without NBL_VARIANT_SUFFIX (the stand-alone library): the handle is that file's own struct,
// which derives from the base, and errors go to that file's fail()
static nbl_tree_model* treeOf(const nbl_model* m) { return const_cast<nbl_model*>(m); }
#else
#include <hip/hip_runtime.h>

#include <cmath>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "dispatch_handle.hpp"   // the linked library's handle; treeOf(handle) is its base, ownError the text nbl_last_error returns
#include "tree_model_host.hpp"
static int fail(int code, const std::string& msg) { return ownError(code, msg.c_str()); }
#endif
#include "kinematics.hip"
#include "dynamics.hip"
#include "centroidal.hip"
#include "sensors.hip"
#include "taskspace.hip"
#include "ik.hip"
#include "ik_grad.hip"

using namespace NBL_NS;

// A kinematics map and a body set remember the model they were made against - device, DOFs, device bodies and the contact capacity of the
// instantiation that owns it - and every call refuses one made for another model.
struct nbl_kin_map {
  int capacity = 0, device = 0;
  int count = 0, P = 0, n = 0, nb = 0;   // entries, mapped rows, DOFs and device bodies of the model it was made for
  void* dBuf = nullptr;                  // [count] DevKinEntry, then the ancestor chains (int32 device bodies, root -> entry body)
  DevKinEntry* dEntries = nullptr;
  int32_t* dPath = nullptr;
  std::vector<DevKinEntry> hEntries;     // host copies: what the wrench calls check before they launch
  std::vector<int32_t> hPath;
};
struct nbl_body_set {
  int capacity = 0, device = 0, n = 0, nb = 0;   // the model it was made for
  DevBodySet set{};
};

// What every call refuses first, in this order: a missing map or set (`ifNull`: the calls that need one say so), one made on a model of
// another instantiation, a null model.  The calls' own checks follow.  (The task-space calls and nbl_ik_solve_vjp name a null model before
// the map, as they always have: handleCheck(h), then mapCheck.)
static int32_t handleCheck(const nbl_model* h) { return h ? NBL_OK : fail(NBL_E_BADARG, "null model"); }
static int32_t handleCheck(const nbl_model* h, const nbl_kin_map* k, const char* ifNull) {
  if (!k && ifNull) return fail(NBL_E_BADARG, ifNull);
  if (h && k && k->capacity != treeOf(h)->capacity) return fail(NBL_E_BADARG, "the kinematics map was made for another model");
  return handleCheck(h);
}
static int32_t handleCheck(const nbl_model* h, const nbl_body_set* s) {
  if (!s) return fail(NBL_E_BADARG, "null body set");
  if (h && s->capacity != treeOf(h)->capacity) return fail(NBL_E_BADARG, "the body set was made for another model");
  return handleCheck(h);
}

// ---- the checks and the launch line the calls below share; each runs after handleCheck, on m = treeOf(h) ----
static int32_t batchCheck(int64_t B) {   // (B = 0 is not refused: a call that takes it as a no-op returns NBL_OK after this)
  return B < 0 ? fail(NBL_E_BADARG, "B must not be negative (got " + std::to_string(B) + ")") : NBL_OK;
}
static int32_t gridCheck(int64_t B, int block) {
  return (B + block - 1) / block > (int64_t)0x7fffffff ? fail(NBL_E_BADARG, "B too large for one launch") : NBL_OK;
}
// `label`: the family in the message, `fn`: the function that says how many bytes are needed
static int32_t workspaceCheck(const char* label, const char* fn, int64_t B, const void* workspace, size_t workspace_bytes, size_t need) {
  if (!workspace) return fail(NBL_E_BADARG, "null workspace");
  if (workspace_bytes < need)
    return fail(NBL_E_WORKSPACE, std::string(label) + " workspace too small for B = " + std::to_string(B) + ": " + std::to_string(workspace_bytes) +
                                     " bytes given, " + fn + "() = " + std::to_string(need));
  return NBL_OK;
}
// a map, wrench set or sensor set that was made for this model; null: `ifNull` says so (nullptr: a set with no entries, accepted)
static int32_t mapCheck(const nbl_tree_model* m, const nbl_kin_map* k, const char* ifNull = nullptr) {
  if (!k) return ifNull ? fail(NBL_E_BADARG, ifNull) : NBL_OK;
  if (k->capacity != m->capacity || k->n != m->n || k->nb != m->nb || k->device != m->device)
    return fail(NBL_E_BADARG, "the kinematics map was made for another model");
  return NBL_OK;
}
// a wrench set or a sensor set (`what`) has whole frames only
static int32_t spatialCheck(const nbl_kin_map* k, const std::string& what) {
  for (int e = 0; k && e < k->count; e++)
    if (k->hEntries[e].kind != KIN_SPATIAL)
      return fail(NBL_E_BADARG, "entry " + std::to_string(e) + " of the " + what + " set is not NBL_KIN_SPATIAL: a " + what + " needs a whole frame");
  return NBL_OK;
}
// `kernel` with one world per lane: a 1-D grid of `block`-lane blocks over the B worlds, on the caller's stream (B, stream: the entry point's)
#define LAUNCH(kernel, block, ...)                                                                                                       \
  do {                                                                                                                                   \
    hipLaunchKernelGGL(kernel, dim3((unsigned)((B + (block) - 1) / (block))), dim3(block), 0, (hipStream_t)stream, __VA_ARGS__);         \
    HIP_TRY(hipGetLastError());                                                                                                          \
  } while (0)
// the entries, ancestor chains and entry count of a map as the kernels take them; k NULL: a set with no entries
#define MAP_ARGS(k) (const DevKinEntry*)((k) ? (k)->dEntries : nullptr), (const int32_t*)((k) ? (k)->dPath : nullptr), (int)((k) ? (k)->count : 0)

extern "C" {

// ---- world-space kinematics of body frames (IKMapping, map_to_pos / map_to_vel; csrc/kinematics.hip) ----------------------------------
int32_t nbl_kin_map_create(nbl_model* h, int32_t count, const int32_t* kind, const int32_t* body, const double* T_offset, nbl_kin_map** out) {
  if (!h || !out || !kind || !body) return fail(NBL_E_BADARG, "null argument");
  nbl_tree_model* const m = treeOf(h);
  *out = nullptr;
  if (count < 1) return fail(NBL_E_BADARG, "a kinematics map needs at least one entry");
  if (count > KIN_MAX_ENTRIES)
    return fail(NBL_E_BADARG, "a kinematics map holds at most " + std::to_string(KIN_MAX_ENTRIES) + " entries (" +
                                  std::to_string(6 * KIN_MAX_ENTRIES) + " rows); got " + std::to_string(count));
  std::vector<DevKinEntry> he(count);
  std::vector<int32_t> path;
  int row = 0;
  for (int k = 0; k < count; k++) {
    if (kind[k] != NBL_KIN_SPATIAL && kind[k] != NBL_KIN_LINEAR && kind[k] != NBL_KIN_ANGULAR)
      return fail(NBL_E_BADARG, "entry " + std::to_string(k) + ": kind must be NBL_KIN_SPATIAL, NBL_KIN_LINEAR or NBL_KIN_ANGULAR");
    if (body[k] < -1 || body[k] >= m->userBodies)
      return fail(NBL_E_BADARG, "entry " + std::to_string(k) + ": body " + std::to_string(body[k]) + " out of range [-1, " + std::to_string(m->userBodies) + ")");
    DevKinEntry& e = he[k];
    std::memset(&e, 0, sizeof(e));
    e.kind = kind[k];
    e.row = row;
    row += kinRows(kind[k]);
    static const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
    for (int c = 0; c < 12; c++) e.T[c] = T_offset ? T_offset[12 * k + c] : I12[c];
    for (int c = 0; c < 12; c++)
      if (!std::isfinite(e.T[c])) return fail(NBL_E_BADARG, "entry " + std::to_string(k) + ": non-finite offset transform");
    // the ancestor chain of the device body that carries T_cj (the z body of a ball triple, the last body of a free chain), root first
    std::vector<int32_t> chain;
    for (int i = body[k] < 0 ? -1 : m->deviceBody(body[k]); i >= 0; i = m->hBodies[i].parent) chain.push_back(i);
    e.pathBegin = (int32_t)path.size();
    e.pathLen = (int32_t)chain.size();
    path.insert(path.end(), chain.rbegin(), chain.rend());
  }
  nbl_kin_map* km = new nbl_kin_map();
  km->capacity = m->capacity; km->device = m->device; km->count = count; km->P = row; km->n = m->n; km->nb = m->nb;
  const size_t eb = sizeof(DevKinEntry) * count, bytes = eb + sizeof(int32_t) * std::max<size_t>(path.size(), 1);
  std::vector<char> img(bytes, 0);
  std::memcpy(img.data(), he.data(), eb);
  if (!path.empty()) std::memcpy(img.data() + eb, path.data(), sizeof(int32_t) * path.size());
  {
    DeviceGuard guard(m->device);
    hipError_t e = guard.ok ? hipMalloc(&km->dBuf, bytes) : hipErrorInvalidDevice;
    if (e == hipSuccess) e = hipMemcpy(km->dBuf, img.data(), bytes, hipMemcpyHostToDevice);   // (registration time: synchronous)
    if (e != hipSuccess) {
      const std::string msg = std::string("kinematics map upload: ") + hipGetErrorString(e);
      if (km->dBuf) (void)hipFree(km->dBuf);
      delete km;
      return fail(NBL_E_HIP, msg);
    }
  }
  km->dEntries = (DevKinEntry*)km->dBuf;
  km->dPath = (int32_t*)((char*)km->dBuf + eb);
  km->hEntries = he;
  km->hPath = path;
  *out = km;
  return NBL_OK;
}

void nbl_kin_map_destroy(nbl_kin_map* k) {
  if (!k) return;
  if (k->dBuf) {
    DeviceGuard guard(k->device);
    (void)hipFree(k->dBuf);   // (waits for launches that still read it)
  }
  delete k;
}

int32_t nbl_kin_map_dim(const nbl_kin_map* k) { return k ? k->P : 0; }

static int32_t kinCheck(const nbl_tree_model* m, const nbl_kin_map* k, int64_t B, const double* state) {
  if (!state) return fail(NBL_E_BADARG, "null argument");
  if (const int32_t rc = mapCheck(m, k)) return rc;
  if (B <= 0) return fail(NBL_E_BADARG, "B must be positive");
  return gridCheck(B, KIN_BLOCK);
}

int32_t nbl_kinematics_forward(nbl_model* h, const nbl_kin_map* k, int64_t B, const double* state, double* pos, double* vel, void* stream) {
  if (const int32_t refused = handleCheck(h, k, "null kinematics map")) return refused;
  nbl_tree_model* const m = treeOf(h);
  const int32_t rc = kinCheck(m, k, B, state);
  if (rc != NBL_OK) return rc;
  if (!pos && !vel) return NBL_OK;
  LAUNCH(k_kinematics_fwd, KIN_BLOCK, (const DevBody*)m->dBodies, MAP_ARGS(k), m->n, B, state, pos, vel);
  return NBL_OK;
}

int32_t nbl_kinematics_backward(nbl_model* h, const nbl_kin_map* k, int64_t B, const double* state, const double* grad_pos,
                                const double* grad_vel, double* grad_state, int32_t accumulate, void* stream) {
  if (const int32_t refused = handleCheck(h, k, "null kinematics map")) return refused;
  nbl_tree_model* const m = treeOf(h);
  const int32_t rc = kinCheck(m, k, B, state);
  if (rc != NBL_OK) return rc;
  if (!grad_state) return fail(NBL_E_BADARG, "null argument");
  LAUNCH(k_kinematics_vjp, KIN_BLOCK, (const DevBody*)m->dBodies, MAP_ARGS(k), m->n, B, state, grad_pos, grad_vel, grad_state, accumulate ? 1 : 0);
  return NBL_OK;
}

// ---- joint-space dynamics quantities (inverse dynamics, Coriolis and gravity, mass matrix; csrc/dynamics.hip) --------------------------
static size_t dynWorkspaceBytes(const nbl_tree_model* m, int64_t B) {
  if (!m || B <= 0) return 0;
  return sizeof(double) * (size_t)m->nb * DYN_SLOTS * (size_t)B;
}
size_t nbl_dynamics_workspace_bytes(const nbl_model* h, int64_t B) { return h ? dynWorkspaceBytes(treeOf(h), B) : 0; }

// workspace of the forward-dynamics calls: [nb][FD_SLOTS][B] tree slots (the reverse pass's k_inverse_dynamics_vjp reuses them: DYN_SLOTS <=
// FD_SLOTS), then the recomputed acceleration [n][B] and -lambda [n][B] of nbl_forward_dynamics_backward
static_assert(DYN_SLOTS <= FD_SLOTS, "the reverse pass runs k_inverse_dynamics_vjp on the forward-dynamics tree slots");
static size_t fdynWorkspaceBytes(const nbl_tree_model* m, int64_t B) {
  if (!m || B <= 0) return 0;
  return sizeof(double) * ((size_t)m->nb * FD_SLOTS + 2 * (size_t)m->n) * (size_t)B;
}

// the checks of the dynamics calls without a wrench set; fd: a forward-dynamics call (its workspace is the larger one)
static int32_t dynCheck(const nbl_tree_model* m, bool fd, int64_t B, const double* state, const void* out, const void* workspace, size_t workspace_bytes) {
  if (const int32_t rc = batchCheck(B)) return rc;
  if (B == 0) return NBL_OK;
  if (!state || !out) return fail(NBL_E_BADARG, "null argument");
  if (const int32_t rc = gridCheck(B, DYN_BLOCK)) return rc;
  return fd ? workspaceCheck("forward-dynamics", "nbl_forward_dynamics_workspace_bytes", B, workspace, workspace_bytes, fdynWorkspaceBytes(m, B))
            : workspaceCheck("dynamics", "nbl_dynamics_workspace_bytes", B, workspace, workspace_bytes, dynWorkspaceBytes(m, B));
}
static int32_t dynFlags(int32_t flags) {
  if (flags & ~DYN_FLAG_MASK) return fail(NBL_E_BADARG, "unknown flag bits " + std::to_string(flags & ~DYN_FLAG_MASK) + " (NBL_ID_*)");
  return NBL_OK;
}

int32_t nbl_inverse_dynamics_forward(nbl_model* h, int64_t B, const double* state, const double* accel, int32_t flags, double* tau,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h)) return refused;
  nbl_tree_model* const m = treeOf(h);
  int32_t rc = dynCheck(m, false, B, state, tau, workspace, workspace_bytes);
  if (rc == NBL_OK) rc = dynFlags(flags);
  if (rc != NBL_OK || B == 0) return rc;
  DeviceGuard guard(m->device);
  LAUNCH(k_inverse_dynamics, DYN_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, (int)flags, B, state, accel, tau,
         (double*)workspace);
  return NBL_OK;
}

int32_t nbl_inverse_dynamics_backward(nbl_model* h, int64_t B, const double* state, const double* accel, int32_t flags,
                                      const double* grad_tau, double* grad_state, double* grad_accel, int32_t accumulate, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h)) return refused;
  nbl_tree_model* const m = treeOf(h);
  int32_t rc = dynCheck(m, false, B, state, grad_tau, workspace, workspace_bytes);
  if (rc == NBL_OK) rc = dynFlags(flags);
  if (rc != NBL_OK || B == 0) return rc;
  if (!grad_state && !grad_accel) return NBL_OK;
  DeviceGuard guard(m->device);
  LAUNCH(k_inverse_dynamics_vjp, DYN_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, (int)flags, B, state, accel, grad_tau,
         grad_state, grad_accel, accumulate ? 1 : 0, (double*)workspace);
  return NBL_OK;
}

int32_t nbl_mass_matrix(nbl_model* h, int64_t B, const double* state, double* M, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h)) return refused;
  nbl_tree_model* const m = treeOf(h);
  const int32_t rc = dynCheck(m, false, B, state, M, workspace, workspace_bytes);
  if (rc != NBL_OK || B == 0) return rc;
  DeviceGuard guard(m->device);
  HIP_TRY(hipMemsetAsync(M, 0, sizeof(double) * (size_t)m->n * m->n * (size_t)B, (hipStream_t)stream));   // unrelated DOFs: the kernel writes the rest
  LAUNCH(k_mass_matrix, DYN_BLOCK, (const DevBody*)m->dBodies, m->mdl, B, state, M, (double*)workspace);
  return NBL_OK;
}

// ---- forward dynamics and the inverse mass matrix (articulated-body algorithm; csrc/dynamics.hip) ---------------------------------------
size_t nbl_forward_dynamics_workspace_bytes(const nbl_model* h, int64_t B) { return h ? fdynWorkspaceBytes(treeOf(h), B) : 0; }

int32_t nbl_forward_dynamics_forward(nbl_model* h, int64_t B, const double* state, const double* tau, int32_t flags, double* accel,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h)) return refused;
  nbl_tree_model* const m = treeOf(h);
  int32_t rc = dynCheck(m, true, B, state, accel, workspace, workspace_bytes);
  if (rc == NBL_OK) rc = dynFlags(flags);
  if (rc != NBL_OK || B == 0) return rc;
  DeviceGuard guard(m->device);
  LAUNCH(k_forward_dynamics, DYN_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, (int)flags, B, state, tau, accel,
         (double*)workspace);
  return NBL_OK;
}

int32_t nbl_forward_dynamics_backward(nbl_model* h, int64_t B, const double* state, const double* tau, int32_t flags, const double* grad_accel,
                                      double* grad_state, double* grad_tau, int32_t accumulate, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  if (const int32_t refused = handleCheck(h)) return refused;
  nbl_tree_model* const m = treeOf(h);
  int32_t rc = dynCheck(m, true, B, state, grad_accel, workspace, workspace_bytes);
  if (rc == NBL_OK) rc = dynFlags(flags);
  if (rc != NBL_OK || B == 0) return rc;
  if (!grad_state && !grad_tau) return NBL_OK;
  DeviceGuard guard(m->device);
  double* ws = (double*)workspace;
  double* accel = ws + (size_t)m->nb * FD_SLOTS * (size_t)B;
  double* neglam = accel + (size_t)m->n * (size_t)B;
  LAUNCH(k_forward_dynamics_lambda, DYN_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, (int)flags, B, state, tau, grad_accel,
         accel, neglam, grad_tau, accumulate ? 1 : 0, ws);
  if (grad_state) {   // grad_state (+)= -(d ID / d [q; v])^T lambda at (q, v, a): inverse dynamics is the exact inverse function
    LAUNCH(k_inverse_dynamics_vjp, DYN_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, (int)flags, B, state, (const double*)accel,
           (const double*)neglam, grad_state, (double*)nullptr, accumulate ? 1 : 0, ws);
  }
  return NBL_OK;
}

int32_t nbl_inv_mass_apply(nbl_model* h, int64_t B, int32_t R, const double* state, const double* X, double* Y, void* workspace,
                           size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h)) return refused;
  nbl_tree_model* const m = treeOf(h);
  const int32_t rc = dynCheck(m, true, B, state, Y, workspace, workspace_bytes);
  if (rc != NBL_OK) return rc;
  if (R < 1) return fail(NBL_E_BADARG, "R must be at least 1 (got " + std::to_string(R) + ")");
  if (B == 0) return NBL_OK;
  if (!X && R != m->n) return fail(NBL_E_BADARG, "X may be null (the identity) only with R = n");
  DeviceGuard guard(m->device);
  LAUNCH(k_minv_apply, DYN_BLOCK, (const DevBody*)m->dBodies, m->mdl, B, (int)R, state, X, Y, (double*)workspace);
  return NBL_OK;
}

int32_t nbl_inv_mass_matrix(nbl_model* h, int64_t B, const double* state, double* Minv, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h)) return refused;
  nbl_tree_model* const m = treeOf(h);
  const int32_t rc = dynCheck(m, true, B, state, Minv, workspace, workspace_bytes);
  if (rc != NBL_OK || B == 0) return rc;
  DeviceGuard guard(m->device);
  LAUNCH(k_minv_apply, DYN_BLOCK, (const DevBody*)m->dBodies, m->mdl, B, (int)m->n, state, (const double*)nullptr, Minv, (double*)workspace);
  return NBL_OK;
}

// ---- wrenches on body frames in the dynamics calls, contact inverse dynamics (csrc/dynamics.hip) -----------------------------------------
// workspace: the forward-dynamics layout ([nb][FD_SLOTS][B] tree slots, accel [n][B], -lambda [n][B]), then the moments of world-frame
// wrenches [nb][3][B] and the root-to-entry transforms of the contact solve [E][12][B]
static size_t wrenchCount(const nbl_kin_map* k) { return k ? (size_t)k->count : 0; }
static size_t wrenchWorkspaceBytes(const nbl_tree_model* m, const nbl_kin_map* k, int64_t B) {
  if (!m || B <= 0) return 0;
  return sizeof(double) * ((size_t)m->nb * (FD_SLOTS + 3) + 2 * (size_t)m->n + 12 * wrenchCount(k)) * (size_t)B;
}
size_t nbl_wrench_workspace_bytes(const nbl_model* h, const nbl_kin_map* k, int64_t B) {
  return (h && (!k || k->capacity == treeOf(h)->capacity)) ? wrenchWorkspaceBytes(treeOf(h), k, B) : 0;
}

// the checks the wrench calls share; k NULL: a set with no entries
static int32_t wrenchCheck(const nbl_tree_model* m, const nbl_kin_map* k, int64_t B, const double* state, const void* out, const double* wrench,
                           int32_t flags, int32_t flagMask, const void* workspace, size_t workspace_bytes) {
  if (const int32_t rc = mapCheck(m, k)) return rc;
  if (const int32_t rc = spatialCheck(k, "wrench")) return rc;
  if (flags & ~flagMask) return fail(NBL_E_BADARG, "unknown flag bits " + std::to_string(flags & ~flagMask) + " (NBL_ID_*, NBL_WRENCH_WORLD)");
  if (const int32_t rc = batchCheck(B)) return rc;
  if (B == 0) return NBL_OK;
  if (!state || !out) return fail(NBL_E_BADARG, "null argument");
  if (k && !wrench) return fail(NBL_E_BADARG, "null wrench array for a set of " + std::to_string(k->count) + " entries");
  if (const int32_t rc = gridCheck(B, DYN_BLOCK)) return rc;
  return workspaceCheck("wrench", "nbl_wrench_workspace_bytes", B, workspace, workspace_bytes, wrenchWorkspaceBytes(m, k, B));
}

int32_t nbl_inverse_dynamics_wrench_forward(nbl_model* h, const nbl_kin_map* k, int64_t B, const double* state, const double* accel,
                                            const double* wrench, int32_t flags, double* tau, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  if (const int32_t refused = handleCheck(h, k, nullptr)) return refused;
  nbl_tree_model* const m = treeOf(h);
  const int32_t rc = wrenchCheck(m, k, B, state, tau, wrench, flags, DYN_FLAG_MASK | DYN_WRENCH_WORLD, workspace, workspace_bytes);
  if (rc != NBL_OK || B == 0) return rc;
  DeviceGuard guard(m->device);
  LAUNCH(k_inverse_dynamics_wrench, DYN_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, (int)flags, B, state, accel, MAP_ARGS(k),
         wrench, tau, (double*)workspace);
  return NBL_OK;
}

int32_t nbl_inverse_dynamics_wrench_backward(nbl_model* h, const nbl_kin_map* k, int64_t B, const double* state, const double* accel,
                                             const double* wrench, int32_t flags, const double* grad_tau, double* grad_state, double* grad_accel,
                                             double* grad_wrench, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h, k, nullptr)) return refused;
  nbl_tree_model* const m = treeOf(h);
  const int32_t rc = wrenchCheck(m, k, B, state, grad_tau, wrench, flags, DYN_FLAG_MASK | DYN_WRENCH_WORLD, workspace, workspace_bytes);
  if (rc != NBL_OK || B == 0) return rc;
  if (!grad_state && !grad_accel && !grad_wrench) return NBL_OK;
  DeviceGuard guard(m->device);
  double* ws = (double*)workspace;
  double* wx = ws + ((size_t)m->nb * FD_SLOTS + 2 * (size_t)m->n) * (size_t)B;
  LAUNCH(k_inverse_dynamics_wrench_vjp, DYN_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, (int)flags, B, state, accel,
         MAP_ARGS(k), wrench, grad_tau, grad_state, grad_accel, grad_wrench, accumulate ? 1 : 0, ws, wx);
  return NBL_OK;
}

int32_t nbl_forward_dynamics_wrench_forward(nbl_model* h, const nbl_kin_map* k, int64_t B, const double* state, const double* tau,
                                            const double* wrench, int32_t flags, double* accel, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  if (const int32_t refused = handleCheck(h, k, nullptr)) return refused;
  nbl_tree_model* const m = treeOf(h);
  const int32_t rc = wrenchCheck(m, k, B, state, accel, wrench, flags, DYN_FLAG_MASK | DYN_WRENCH_WORLD, workspace, workspace_bytes);
  if (rc != NBL_OK || B == 0) return rc;
  DeviceGuard guard(m->device);
  LAUNCH(k_forward_dynamics_wrench, DYN_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, (int)flags, B, state, tau, MAP_ARGS(k),
         wrench, accel, (double*)workspace);
  return NBL_OK;
}

int32_t nbl_forward_dynamics_wrench_backward(nbl_model* h, const nbl_kin_map* k, int64_t B, const double* state, const double* tau,
                                             const double* wrench, int32_t flags, const double* grad_accel, double* grad_state, double* grad_tau,
                                             double* grad_wrench, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h, k, nullptr)) return refused;
  nbl_tree_model* const m = treeOf(h);
  const int32_t rc = wrenchCheck(m, k, B, state, grad_accel, wrench, flags, DYN_FLAG_MASK | DYN_WRENCH_WORLD, workspace, workspace_bytes);
  if (rc != NBL_OK || B == 0) return rc;
  if (!grad_state && !grad_tau && !grad_wrench) return NBL_OK;
  DeviceGuard guard(m->device);
  double* ws = (double*)workspace;
  double* accel = ws + (size_t)m->nb * FD_SLOTS * (size_t)B;
  double* neglam = accel + (size_t)m->n * (size_t)B;
  double* wx = neglam + (size_t)m->n * (size_t)B;
  LAUNCH(k_forward_dynamics_wrench_lambda, DYN_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, (int)flags, B, state, tau,
         MAP_ARGS(k), wrench, grad_accel, accel, neglam, grad_tau, accumulate ? 1 : 0, ws);
  if (grad_state || grad_wrench) {   // grad_state (+)= -(d ID / d [q; v])^T lambda, grad_wrench (+)= J lambda, at (q, v, a) with the same wrenches
    LAUNCH(k_inverse_dynamics_wrench_vjp, DYN_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, (int)flags, B, state,
           (const double*)accel, MAP_ARGS(k), wrench, (const double*)neglam, grad_state, (double*)nullptr, grad_wrench, accumulate ? 1 : 0, ws, wx);
  }
  return NBL_OK;
}

// ---- gradients of the dynamics calls to the registered inertia parameters (k_inverse_dynamics_inertia_vjp; csrc/dynamics.hip) ------------
// The table is the one nbl_set_inertia_params[_on] uploaded; none registered: nothing to write, success.
int32_t nbl_inverse_dynamics_backward_inertia(nbl_model* h, int64_t B, const double* state, const double* accel, int32_t flags,
                                              const double* grad_tau, double* grad_params, int32_t accumulate, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h)) return refused;
  nbl_tree_model* const m = treeOf(h);
  int32_t rc = dynCheck(m, false, B, state, grad_tau, workspace, workspace_bytes);
  if (rc == NBL_OK) rc = dynFlags(flags);
  if (rc != NBL_OK || B == 0 || m->nParams == 0) return rc;
  if (!grad_params) return fail(NBL_E_BADARG, "null grad_params for " + std::to_string(m->nParams) + " registered inertia parameters");
  DeviceGuard guard(m->device);
  LAUNCH(k_inverse_dynamics_inertia_vjp, DYN_BLOCK, (const DevBody*)m->dBodies, m->mdl, (int)flags, B, state, accel, grad_tau,
         (const DevInertiaParam*)m->dParams, m->nParams, grad_params, accumulate ? 1 : 0, (double*)workspace);
  return NBL_OK;
}

// Two launches like nbl_forward_dynamics[_wrench]_backward: a again and -lambda = -M^-1 grad_accel, then the inertia contraction at
// (q, v, a) with the cotangent -lambda on the same tree slots.
int32_t nbl_forward_dynamics_backward_inertia(nbl_model* h, const nbl_kin_map* k, int64_t B, const double* state, const double* tau,
                                              const double* wrench, int32_t flags, const double* grad_accel, double* grad_params,
                                              int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h, k, nullptr)) return refused;
  nbl_tree_model* const m = treeOf(h);
  int32_t rc;
  if (k) {
    rc = wrenchCheck(m, k, B, state, grad_accel, wrench, flags, DYN_FLAG_MASK | DYN_WRENCH_WORLD, workspace, workspace_bytes);
  } else {
    rc = dynCheck(m, true, B, state, grad_accel, workspace, workspace_bytes);
    if (rc == NBL_OK) rc = dynFlags(flags);
  }
  if (rc != NBL_OK || B == 0 || m->nParams == 0) return rc;
  if (!grad_params) return fail(NBL_E_BADARG, "null grad_params for " + std::to_string(m->nParams) + " registered inertia parameters");
  DeviceGuard guard(m->device);
  double* ws = (double*)workspace;
  double* accel = ws + (size_t)m->nb * FD_SLOTS * (size_t)B;
  double* neglam = accel + (size_t)m->n * (size_t)B;
  if (k)
    LAUNCH(k_forward_dynamics_wrench_lambda, DYN_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, (int)flags, B, state, tau,
           MAP_ARGS(k), wrench, grad_accel, accel, neglam, (double*)nullptr, 0, ws);
  else
    LAUNCH(k_forward_dynamics_lambda, DYN_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, (int)flags, B, state, tau, grad_accel,
           accel, neglam, (double*)nullptr, 0, ws);
  LAUNCH(k_inverse_dynamics_inertia_vjp, DYN_BLOCK, (const DevBody*)m->dBodies, m->mdl, (int)(flags & DYN_FLAG_MASK), B, state, (const double*)accel,
         (const double*)neglam, (const DevInertiaParam*)m->dParams, m->nParams, grad_params, accumulate ? 1 : 0, ws);
  return NBL_OK;
}

int32_t nbl_contact_inverse_dynamics(nbl_model* h, const nbl_kin_map* k, int64_t B, const double* state, const double* accel,
                                     const double* wrench_guess, int32_t mode, int32_t flags, double* wrench_out, double* tau, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h, k, nullptr)) return refused;
  nbl_tree_model* const m = treeOf(h);
  if (!k) return fail(NBL_E_BADARG, "null kinematics map: contact inverse dynamics needs at least one contact body");
  if (mode != NBL_CID_SINGLE && mode != NBL_CID_NEAREST && mode != NBL_CID_MIN_TORQUE)
    return fail(NBL_E_BADARG, "mode must be NBL_CID_SINGLE, NBL_CID_NEAREST or NBL_CID_MIN_TORQUE (got " + std::to_string(mode) + ")");
  // (wrench_out stands in for the wrench array of the shared check: it is as long)
  const int32_t rc = wrenchCheck(m, k, B, state, tau, wrench_out, flags, DYN_FLAG_MASK, workspace, workspace_bytes);
  if (rc != NBL_OK) return rc;
  if (mode == NBL_CID_SINGLE && k->count != 1)
    return fail(NBL_E_BADARG, "NBL_CID_SINGLE takes one contact body (the set has " + std::to_string(k->count) + ")");
  if (cidRoot(m->hBodies.data(), k->hEntries.data(), k->hPath.data(), k->count) < 0)
    return fail(NBL_E_UNSUPPORTED, "contact inverse dynamics needs every contact body below ONE free joint at the root of its tree "
                                   "(Skeleton::getContactInverseDynamics returns zeros otherwise)");
  if (B == 0) return NBL_OK;
  if (mode == NBL_CID_NEAREST && !wrench_guess) return fail(NBL_E_BADARG, "NBL_CID_NEAREST needs wrench_guess");
  if (!accel) return fail(NBL_E_BADARG, "null argument");
  DeviceGuard guard(m->device);
  double* ws = (double*)workspace;
  double* xs = ws + ((size_t)m->nb * (FD_SLOTS + 3) + 2 * (size_t)m->n) * (size_t)B;
  LAUNCH(k_contact_inverse_dynamics, DYN_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, (int)flags, (int)mode, B, state, accel,
         MAP_ARGS(k), mode == NBL_CID_NEAREST ? wrench_guess : (const double*)nullptr, wrench_out, tau, ws, xs);
  return NBL_OK;
}

// ---- batched inverse kinematics (IKMapping::setPositions = math::solveIK with one restart; csrc/ik.hip) ---------------------------------
void nbl_ik_default_config(nbl_ik_config* c) {   // math::IKConfig (IKSolver.hpp:31-38)
  if (!c) return;
  c->convergence_threshold = 1e-7; c->max_step_count = 100; c->least_squares_damping = 0.01;
  c->start_clamped = 0; c->line_search = 1; c->dont_exit_transpose = 0;
}

static size_t ikWorkspaceBytes(const nbl_tree_model* m, const nbl_kin_map* k, int64_t B) {
  if (!m || !k || B <= 0) return 0;
  return sizeof(double) * (size_t)ikLayout(m->n, k->P).total * (size_t)B;
}
size_t nbl_ik_workspace_bytes(const nbl_model* h, const nbl_kin_map* k, int64_t B) {
  return (h && k && k->capacity == treeOf(h)->capacity) ? ikWorkspaceBytes(treeOf(h), k, B) : 0;
}

int32_t nbl_ik_solve(nbl_model* h, const nbl_kin_map* k, int64_t B, const double* target, const double* q_init, const nbl_ik_config* config,
                     double* q_out, double* loss, int32_t* steps, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h, k, "null kinematics map")) return refused;
  nbl_tree_model* const m = treeOf(h);
  if (const int32_t rc = mapCheck(m, k)) return rc;
  if (const int32_t rc = batchCheck(B)) return rc;
  IkConfig cfg;
  if (config) {
    cfg.convergenceThreshold = config->convergence_threshold; cfg.maxStepCount = config->max_step_count;
    cfg.damping = config->least_squares_damping; cfg.startClamped = config->start_clamped ? 1 : 0;
    cfg.lineSearch = config->line_search ? 1 : 0; cfg.dontExitTranspose = config->dont_exit_transpose ? 1 : 0;
  } else {   // IKMapping::setPositions: IKConfig().setMaxStepCount(500)
    cfg.convergenceThreshold = 1e-7; cfg.maxStepCount = 500; cfg.damping = 0.01; cfg.startClamped = 0; cfg.lineSearch = 1; cfg.dontExitTranspose = 0;
  }
  if (cfg.maxStepCount < 1) return fail(NBL_E_BADARG, "max_step_count must be at least 1 (got " + std::to_string(cfg.maxStepCount) + ")");
  if (cfg.maxStepCount > IK_MAX_STEP_COUNT)
    return fail(NBL_E_BADARG, "max_step_count above " + std::to_string(IK_MAX_STEP_COUNT) + " (got " + std::to_string(cfg.maxStepCount) +
                                  "): a lane runs its world's whole solve in one launch");
  if (!(cfg.damping >= 0.0) || !(cfg.convergenceThreshold >= 0.0)) return fail(NBL_E_BADARG, "least_squares_damping and convergence_threshold must not be negative");
  if (cfg.damping == 0.0)
    return fail(NBL_E_UNSUPPORTED, "least_squares_damping = 0 (the reference's complete orthogonal decomposition) is outside the device path");
  if (B == 0) return NBL_OK;
  if (!target || !q_out || !workspace) return fail(NBL_E_BADARG, "null argument");
  if (const int32_t rc = gridCheck(B, IK_BLOCK)) return rc;
  if (const int32_t rc = workspaceCheck("IK", "nbl_ik_workspace_bytes", B, workspace, workspace_bytes, ikWorkspaceBytes(m, k, B))) return rc;
  DeviceGuard guard(m->device);
  LAUNCH(k_ik_solve, IK_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, MAP_ARGS(k), m->nb, m->n, k->P, B, target, q_init, cfg, q_out,
         loss, steps, (double*)workspace);
  return NBL_OK;
}

// ---- the reverse pass of inverse kinematics (csrc/ik_grad.hip); its scratch has the solver's layout: J, the normal matrix, three vectors ----
size_t nbl_ik_grad_workspace_bytes(const nbl_model* h, const nbl_kin_map* k, int64_t B) { return nbl_ik_workspace_bytes(h, k, B); }

int32_t nbl_ik_solve_vjp(nbl_model* h, const nbl_kin_map* k, int64_t B, const double* q, const double* grad_q, double grad_damping,
                         double* grad_target, int32_t accumulate, int32_t* free_count, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h)) return refused;   // (a null model before a null map, unlike nbl_ik_solve)
  nbl_tree_model* const m = treeOf(h);
  if (const int32_t rc = mapCheck(m, k, "null kinematics map")) return rc;
  if (const int32_t rc = batchCheck(B)) return rc;
  if (!(grad_damping >= 0.0)) return fail(NBL_E_BADARG, "grad_damping must not be negative");
  if (grad_damping == 0.0)
    return fail(NBL_E_UNSUPPORTED, "grad_damping = 0 (a pseudo-inverse of a possibly singular Jacobian) is outside the device path");
  if (B == 0) return NBL_OK;
  if (!q || !grad_q || !grad_target || !workspace) return fail(NBL_E_BADARG, "null argument");
  if (const int32_t rc = gridCheck(B, IK_GRAD_BLOCK)) return rc;
  if (const int32_t rc = workspaceCheck("IK gradient", "nbl_ik_grad_workspace_bytes", B, workspace, workspace_bytes, ikWorkspaceBytes(m, k, B))) return rc;
  DeviceGuard guard(m->device);
  LAUNCH(k_ik_solve_vjp, IK_GRAD_BLOCK, (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, MAP_ARGS(k), m->nb, m->n, k->P, B, q, grad_q,
         grad_damping, grad_target, accumulate ? 1 : 0, free_count, (double*)workspace);
  return NBL_OK;
}

// ---- centre of mass, momentum and energy of a body set (csrc/centroidal.hip) -----------------------------------------------------------------
int32_t nbl_body_set_create(nbl_model* h, int32_t count, const int32_t* bodies, nbl_body_set** out) {
  if (!h || !out) return fail(NBL_E_BADARG, "null argument");
  nbl_tree_model* const m = treeOf(h);
  *out = nullptr;
  if (count < 0 || (count > 0 && !bodies)) return fail(NBL_E_BADARG, "a body set needs `count` body indices (or none: every body)");
  if (m->nb > CEN_MAX_BODIES)
    return fail(NBL_E_UNSUPPORTED, "body sets are masks over at most " + std::to_string(CEN_MAX_BODIES) + " internal bodies; the model has " + std::to_string(m->nb));
  DevBodySet set{};
  auto add = [&](int body) {
    int i = m->deviceBody(body);
    set.mass |= 1ull << i;
    set.joints |= 1ull << i;
    // the whole chain of a ball joint / a free joint below the root: its coordinates sit on the bodies before the one that carries T_cj
    while ((m->hBodies[i].jtype == JT_BALL || m->hBodies[i].jtype == JT_FREEC) && m->hBodies[i].ballComp > 0) {
      i = m->hBodies[i].parent;
      set.joints |= 1ull << i;
    }
  };
  if (count == 0) {
    for (int i = 0; i < m->userBodies; i++) add(i);
  } else {
    for (int k = 0; k < count; k++) {
      if (bodies[k] < 0 || bodies[k] >= m->userBodies)
        return fail(NBL_E_BADARG, "entry " + std::to_string(k) + ": body " + std::to_string(bodies[k]) + " out of range [0, " + std::to_string(m->userBodies) + ")");
      for (int f = 0; f < k; f++)
        if (bodies[f] == bodies[k]) return fail(NBL_E_BADARG, "body " + std::to_string(bodies[k]) + " is named twice (entries " + std::to_string(f) + " and " + std::to_string(k) + ")");
      add(bodies[k]);
    }
  }
  if (!(cenTotalMass(m->hBodies.data(), m->nb, set.mass) > 0.0)) return fail(NBL_E_BADARG, "the body set has no mass");
  nbl_body_set* s = new nbl_body_set();
  s->capacity = m->capacity; s->device = m->device; s->n = m->n; s->nb = m->nb; s->set = set;
  *out = s;
  return NBL_OK;
}

void nbl_body_set_destroy(nbl_body_set* s) { delete s; }

int32_t nbl_body_set_origin_moments(nbl_model* h, nbl_body_set* s, int32_t count, const int32_t* bodies, const double* moments) {
  if (const int32_t refused = handleCheck(h, s)) return refused;
  nbl_tree_model* const m = treeOf(h);
  if (!m || !s || count < 0 || (count > 0 && (!bodies || !moments))) return fail(NBL_E_BADARG, "null argument");
  if (s->n != m->n || s->nb != m->nb || s->device != m->device) return fail(NBL_E_BADARG, "the body set was made for another model");
  for (int k = 0; k < count; k++) {
    if (bodies[k] < 0 || bodies[k] >= m->userBodies) return fail(NBL_E_BADARG, "entry " + std::to_string(k) + ": body out of range");
    for (int c = 0; c < 3; c++)
      if (!std::isfinite(moments[3 * k + c])) return fail(NBL_E_BADARG, "entry " + std::to_string(k) + ": non-finite moment");
  }
  for (int k = 0; k < count; k++)
    for (int c = 0; c < 3; c++) s->set.originMoment[3 * m->deviceBody(bodies[k]) + c] = moments[3 * k + c];
  return NBL_OK;
}

double nbl_body_set_mass(nbl_model* h, const nbl_body_set* s) {
  if (!h || !s) { (void)fail(NBL_E_BADARG, "null argument"); return 0.0; }
  nbl_tree_model* const m = treeOf(h);
  if (s->capacity != m->capacity) { (void)fail(NBL_E_BADARG, "the body set was made for another model"); return 0.0; }
  if (s->n != m->n || s->nb != m->nb || s->device != m->device) { (void)fail(NBL_E_BADARG, "the body set was made for another model"); return 0.0; }
  return cenTotalMass(m->hBodies.data(), m->nb, s->set.mass);
}

static size_t cenWorkspaceBytes(const nbl_tree_model* m, int64_t B) {
  if (!m || B <= 0) return 0;
  return sizeof(double) * (size_t)m->nb * CEN_SLOTS * (size_t)B;
}
size_t nbl_centroidal_workspace_bytes(const nbl_model* h, int64_t B) { return h ? cenWorkspaceBytes(treeOf(h), B) : 0; }

static int32_t cenCheck(const nbl_tree_model* m, const nbl_body_set* s, int64_t B, const double* state, int32_t flags, const void* workspace,
                        size_t workspace_bytes) {
  if (s->n != m->n || s->nb != m->nb || s->device != m->device) return fail(NBL_E_BADARG, "the body set was made for another model");
  if (const int32_t rc = batchCheck(B)) return rc;
  if (flags & ~CEN_FLAG_MASK) return fail(NBL_E_BADARG, "unknown flag bits " + std::to_string(flags & ~CEN_FLAG_MASK) + " (NBL_CEN_*)");
  if (B == 0) return NBL_OK;
  if (!state) return fail(NBL_E_BADARG, "null argument");
  if (const int32_t rc = gridCheck(B, CEN_BLOCK)) return rc;
  if (!(cenTotalMass(m->hBodies.data(), m->nb, s->set.mass) > 0.0)) return fail(NBL_E_BADARG, "the body set has no mass");
  return workspaceCheck("centroidal", "nbl_centroidal_workspace_bytes", B, workspace, workspace_bytes, cenWorkspaceBytes(m, B));
}

int32_t nbl_centroidal_forward(nbl_model* h, const nbl_body_set* set, int64_t B, const double* state, const double* accel, int32_t flags,
                               double* com, double* com_vel, double* com_acc, double* momentum, double* ke, double* pe, double* Jcom,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h, set)) return refused;
  nbl_tree_model* const m = treeOf(h);
  const int32_t rc = cenCheck(m, set, B, state, flags, workspace, workspace_bytes);
  if (rc != NBL_OK) return rc;
  if (com_acc && !accel) return fail(NBL_E_BADARG, "com_acc needs the accelerations (accel is null)");
  if (B == 0 || !(com || com_vel || com_acc || momentum || ke || pe || Jcom)) return NBL_OK;
  DeviceGuard guard(m->device);
  hipStream_t s = (hipStream_t)stream;
  m->timingNow = m->timing;
  TIMED(K_CENTROIDAL, hipLaunchKernelGGL(k_centroidal, dim3((unsigned)((B + CEN_BLOCK - 1) / CEN_BLOCK)), dim3(CEN_BLOCK), 0, s,
                                         (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, set->set, (int)flags, B, state, accel, com,
                                         com_vel, com_acc, momentum, ke, pe, Jcom, (double*)workspace));
  m->timingNow = false;
  HIP_TRY(hipGetLastError());
  return NBL_OK;
}

int32_t nbl_centroidal_backward(nbl_model* h, const nbl_body_set* set, int64_t B, const double* state, const double* accel, int32_t flags,
                                const double* g_com, const double* g_com_vel, const double* g_com_acc, const double* g_momentum,
                                const double* g_ke, const double* g_pe, double* grad_state, double* grad_accel, int32_t accumulate,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h, set)) return refused;
  nbl_tree_model* const m = treeOf(h);
  const int32_t rc = cenCheck(m, set, B, state, flags, workspace, workspace_bytes);
  if (rc != NBL_OK) return rc;
  if (g_com_acc && !accel) return fail(NBL_E_BADARG, "g_com_acc needs the accelerations (accel is null)");
  if (B == 0 || (!grad_state && !grad_accel)) return NBL_OK;
  DeviceGuard guard(m->device);
  hipStream_t s = (hipStream_t)stream;
  m->timingNow = m->timing;
  TIMED(K_CENTROIDAL_VJP, hipLaunchKernelGGL(k_centroidal_vjp, dim3((unsigned)((B + CEN_BLOCK - 1) / CEN_BLOCK)), dim3(CEN_BLOCK), 0, s,
                                             (const DevBody*)m->dBodies, (const DevDof*)m->dDofs, m->mdl, set->set, (int)flags, B, state, accel,
                                             g_com, g_com_vel, g_com_acc, g_momentum, g_ke, g_pe, grad_state, grad_accel, accumulate ? 1 : 0,
                                             (double*)workspace));
  m->timingNow = false;
  HIP_TRY(hipGetLastError());
  return NBL_OK;
}

// ---- gyroscope, accelerometer and magnetometer readings of a sensor set (csrc/sensors.hip) ---------------------------------------------------
size_t nbl_sensors_workspace_bytes(const nbl_model* h, int64_t B) { return nbl_centroidal_workspace_bytes(h, B); }

// the checks the two sensor calls share; a sensor set is a kinematics map of NBL_KIN_SPATIAL entries, like a wrench set
static int32_t sensCheck(const nbl_tree_model* m, const nbl_kin_map* k, int64_t B, const double* state, const void* workspace, size_t workspace_bytes) {
  if (const int32_t rc = mapCheck(m, k)) return rc;
  if (const int32_t rc = spatialCheck(k, "sensor")) return rc;
  if (const int32_t rc = batchCheck(B)) return rc;
  if (B == 0) return NBL_OK;
  if (!state) return fail(NBL_E_BADARG, "null argument");
  if (const int32_t rc = gridCheck(B, SENS_BLOCK)) return rc;
  return workspaceCheck("sensor", "nbl_sensors_workspace_bytes", B, workspace, workspace_bytes, cenWorkspaceBytes(m, B));
}

int32_t nbl_sensors_forward(nbl_model* h, const nbl_kin_map* k, int64_t B, const double* state, const double* accel, const double* field,
                            double* gyro, double* acc, double* mag, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h, k, "null sensor set")) return refused;
  nbl_tree_model* const m = treeOf(h);
  const int32_t rc = sensCheck(m, k, B, state, workspace, workspace_bytes);
  if (rc != NBL_OK) return rc;
  if (acc && !accel) return fail(NBL_E_BADARG, "acc needs the accelerations (accel is null)");
  if (mag && !field) return fail(NBL_E_BADARG, "mag needs the magnetic field (field is null)");
  if (B == 0 || !(gyro || acc || mag)) return NBL_OK;
  DeviceGuard guard(m->device);
  LAUNCH(k_sensors, SENS_BLOCK, (const DevBody*)m->dBodies, m->mdl, MAP_ARGS(k), B, state, accel, field, gyro, acc, mag, (double*)workspace);
  return NBL_OK;
}

int32_t nbl_sensors_backward(nbl_model* h, const nbl_kin_map* k, int64_t B, const double* state, const double* accel, const double* field,
                             const double* g_gyro, const double* g_acc, const double* g_mag, double* grad_state, double* grad_accel,
                             double* grad_field, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  if (const int32_t refused = handleCheck(h, k, "null sensor set")) return refused;
  nbl_tree_model* const m = treeOf(h);
  const int32_t rc = sensCheck(m, k, B, state, workspace, workspace_bytes);
  if (rc != NBL_OK) return rc;
  if (g_acc && !accel) return fail(NBL_E_BADARG, "g_acc needs the accelerations (accel is null)");
  if (g_mag && !field) return fail(NBL_E_BADARG, "g_mag needs the magnetic field (field is null)");
  if (B == 0 || (!grad_state && !grad_accel && !grad_field)) return NBL_OK;
  DeviceGuard guard(m->device);
  LAUNCH(k_sensors_vjp, SENS_BLOCK, (const DevBody*)m->dBodies, m->mdl, MAP_ARGS(k), B, state, accel, field, g_gyro, g_acc, g_mag, grad_state,
         grad_accel, grad_field, accumulate ? 1 : 0, (double*)workspace);
  return NBL_OK;
}

// ---- task-space Jacobians, their time derivative and task-space accelerations (csrc/taskspace.hip) ------------------------------------------
size_t nbl_task_workspace_bytes(const nbl_model* h, int64_t B) { return nbl_centroidal_workspace_bytes(h, B); }

// the checks the five calls share: a null model first, then the map
static int32_t taskCheck(const nbl_model* h, const nbl_kin_map* k, int64_t B, int32_t rows, int32_t n, const double* state) {
  if (const int32_t refused = handleCheck(h)) return refused;
  const nbl_tree_model* const m = treeOf(h);
  if (const int32_t rc = mapCheck(m, k, "null kinematics map")) return rc;
  if (rows != k->P) return fail(NBL_E_BADARG, "rows = " + std::to_string(rows) + ", the kinematics map has " + std::to_string(k->P));
  if (n != m->n) return fail(NBL_E_BADARG, "n = " + std::to_string(n) + ", the model has " + std::to_string(m->n) + " DOFs");
  if (const int32_t rc = batchCheck(B)) return rc;
  if (B == 0) return NBL_OK;
  if (!state) return fail(NBL_E_BADARG, "null argument");
  return gridCheck(B, TASK_BLOCK);
}

int32_t nbl_task_jacobian(nbl_model* h, const nbl_kin_map* k, int64_t B, int32_t rows, int32_t n, const double* state, double* J, void* stream) {
  const int32_t rc = taskCheck(h, k, B, rows, n, state);
  if (rc != NBL_OK || B == 0) return rc;
  if (!J) return fail(NBL_E_BADARG, "null argument");
  nbl_tree_model* const m = treeOf(h);
  DeviceGuard guard(m->device);
  LAUNCH(k_task_jacobian, TASK_BLOCK, (const DevBody*)m->dBodies, MAP_ARGS(k), m->n, B, state, J);
  return NBL_OK;
}

int32_t nbl_task_jacobian_deriv(nbl_model* h, const nbl_kin_map* k, int64_t B, int32_t rows, int32_t n, const double* state, double* Jdot,
                                void* stream) {
  const int32_t rc = taskCheck(h, k, B, rows, n, state);
  if (rc != NBL_OK || B == 0) return rc;
  if (!Jdot) return fail(NBL_E_BADARG, "null argument");
  nbl_tree_model* const m = treeOf(h);
  DeviceGuard guard(m->device);
  LAUNCH(k_task_jacobian_deriv, TASK_BLOCK, (const DevBody*)m->dBodies, MAP_ARGS(k), m->n, B, state, Jdot);
  return NBL_OK;
}

int32_t nbl_task_jacobian_vjp(nbl_model* h, const nbl_kin_map* k, int64_t B, int32_t rows, int32_t n, const double* state, const double* G,
                              double* grad_q, int32_t accumulate, void* stream) {
  const int32_t rc = taskCheck(h, k, B, rows, n, state);
  if (rc != NBL_OK || B == 0) return rc;
  if (!G || !grad_q) return fail(NBL_E_BADARG, "null argument");
  nbl_tree_model* const m = treeOf(h);
  DeviceGuard guard(m->device);
  LAUNCH(k_task_jacobian_vjp, TASK_BLOCK, (const DevBody*)m->dBodies, MAP_ARGS(k), m->n, B, state, G, grad_q, accumulate ? 1 : 0);
  return NBL_OK;
}

int32_t nbl_task_accel(nbl_model* h, const nbl_kin_map* k, int64_t B, int32_t rows, int32_t n, const double* state, const double* accel,
                       double* bias, double* xdd, void* stream) {
  const int32_t rc = taskCheck(h, k, B, rows, n, state);
  if (rc != NBL_OK) return rc;
  if (xdd && !accel) return fail(NBL_E_BADARG, "xdd needs the accelerations (accel is null)");
  if (B == 0 || (!bias && !xdd)) return NBL_OK;
  nbl_tree_model* const m = treeOf(h);
  DeviceGuard guard(m->device);
  LAUNCH(k_task_accel, TASK_BLOCK, (const DevBody*)m->dBodies, MAP_ARGS(k), m->n, B, state, accel, bias, xdd);
  return NBL_OK;
}

int32_t nbl_task_accel_vjp(nbl_model* h, const nbl_kin_map* k, int64_t B, int32_t rows, int32_t n, const double* state, const double* accel,
                           const double* g_out, double* grad_state, double* grad_accel, int32_t accumulate, void* workspace,
                           size_t workspace_bytes, void* stream) {
  const int32_t rc = taskCheck(h, k, B, rows, n, state);
  if (rc != NBL_OK) return rc;
  if (grad_accel && !accel) return fail(NBL_E_BADARG, "grad_accel needs the accelerations (accel is null)");
  if (B == 0 || (!grad_state && !grad_accel)) return NBL_OK;
  if (!g_out) return fail(NBL_E_BADARG, "null argument");
  nbl_tree_model* const m = treeOf(h);
  if (const int32_t refused = workspaceCheck("task-space", "nbl_task_workspace_bytes", B, workspace, workspace_bytes, cenWorkspaceBytes(m, B)))
    return refused;
  DeviceGuard guard(m->device);
  LAUNCH(k_task_accel_vjp, TASK_BLOCK, (const DevBody*)m->dBodies, m->mdl, MAP_ARGS(k), B, state, accel, g_out, grad_state, grad_accel,
         accumulate ? 1 : 0, (double*)workspace);
  return NBL_OK;
}

}  // extern "C"
