// tree_model_host.hpp — the part of a model handle that does not depend on the contact capacity, and the host helpers every unit that
// launches kernels on a handle shares.
//
// nbl_model of an instantiation of the contact stage (nimble_amd.hip, abi_variants.h) DERIVES from nbl_tree_model; the unit of the
// contact-independent calls (nimble_amd_tree.hip, built once) sees a handle of any instantiation through this base alone.  Host code:
// the including file provides `fail(int code, const std::string& msg)`, which HIP_TRY reports through.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "model_dev.hpp"

#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) return fail(NBL_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
  } while (0)

enum KernelId { K_FWD = 0, K_DETECT, K_BWD, K_RECOMPUTE, K_BWD_FINAL, K_SOLVE_COOP, K_BWD_A_COOP, K_ROWS_COOP, K_BWD_B_COOP, K_FWD_COOP, K_RECOMPUTE_COOP, K_BWD_FINAL_COOP, K_TREE_TO_LANES, K_CASCADE_COOP, K_CASCADE_FINAL, K_BWD_BOUNCE, K_CASCADE_FUSED, K_FWD_DETECT, K_CENTROIDAL, K_CENTROIDAL_VJP, K_COUNT };
inline const char* const kKernelNames[K_COUNT] = {"k_step_forward", "k_contact_detect",
                                                  "k_step_backward", "k_bwd_recompute",
                                                  "k_bwd_final", "k_contact_solve_coop", "k_bwd_contact_a_coop", "k_contact_rows_coop", "k_bwd_contact_b_coop", "k_step_forward_coop", "k_bwd_recompute_coop",
                                                  "k_bwd_final_coop", "k_tree_to_lanes", "k_contact_cascade_stages", "k_contact_cascade_final", "k_bwd_bounce", "k_contact_cascade_fused", "k_forward_detect_coop",
                                                  "k_centroidal", "k_centroidal_vjp"};
struct TimedLaunch {
  hipEvent_t start, stop;
  int kernel;
};

struct nbl_tree_model {
  int capacity = 0;                  // contact slots per world of the instantiation that owns the handle (8, 16, 64 or 128)
  int device = 0;
  nbl_shared::DevModel mdl;
  nbl_shared::DevBody* dBodies = nullptr;
  nbl_shared::DevDof* dDofs = nullptr;
  int nb = 0, n = 0;
  std::vector<nbl_shared::DevBody> hBodies;   // host copy of the body constants (nbl_set_body_inertia patches one entry)
  int userBodies = 0;                // bodies of the caller's description; bodyMap: caller's body index -> device body (empty: identity;
  std::vector<int32_t> bodyMap;      // models with ball joints carry two extra massless bodies per ball joint, expandBallJoints)
  int deviceBody(int body) const { return bodyMap.empty() ? body : bodyMap[body]; }
  nbl_shared::DevInertiaParam* dParams = nullptr; // registered inertia parameters (nbl_set_inertia_params)
  int nParams = 0;
  bool timing = false;      // kernel timing requested
  bool timingNow = false;   // ... and this call is one of the sampled ones
  std::vector<TimedLaunch> pending;
  double kMs[K_COUNT] = {0};
  int64_t kCount[K_COUNT] = {0};
};

// keeps the calling thread's current device across an entry point that has to work on the model's device
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) ok = hipSetDevice(dev) == hipSuccess; }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

static void beginTiming(nbl_tree_model* m, hipStream_t s, int kernel) {
  if (!m->timingNow) return;
  TimedLaunch t;
  hipEventCreate(&t.start);
  hipEventCreate(&t.stop);
  t.kernel = kernel;
  hipEventRecord(t.start, s);
  m->pending.push_back(t);
}
static void endTiming(nbl_tree_model* m, hipStream_t s) {
  if (!m->timingNow) return;
  hipEventRecord(m->pending.back().stop, s);
}
// NBL_DEBUG_SYNC=1 (developer switch): wait for every kernel and name it on stderr - a device fault then points at its launch
static const bool g_dbgSync = getenv("NBL_DEBUG_SYNC") && atoi(getenv("NBL_DEBUG_SYNC")) != 0;
#define TIMED(kid, launch) do { beginTiming(m, s, kid); launch; endTiming(m, s); \
    if (g_dbgSync) { const hipError_t de_ = hipStreamSynchronize(s); fprintf(stderr, "[nbl] %s: %s\n", kKernelNames[kid], hipGetErrorString(de_)); } } while (0)
