// nimble_amd_dispatch.cpp — the entry points of include/nimble_amd.h over the instantiations of the library (abi_variants.h):
// a model is given, when it is created, to the 24-row build (max_contacts <= 8, <= 16 colliders, <= 32 collider pairs: every
// BASELINE config), to the 48-row build (up to 16 contacts, 32 colliders, 64 pairs per world) or to the GENERAL build (up to 64
// contacts = 192 LCP rows, 64 colliders, 512 pairs: rows looped over instead of mapped to lanes - there so that no legal world
// gets a truncated answer; 2 M world-steps/s on eight-contact worlds since round 6; a fourth instantiation is the same code with 384 rows); every later call goes to the build that owns the handle.  Host code only; no HIP call of its own.
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>

#include "../../include/nimble_amd.h"
#define NBL_DISPATCHER
#include "abi_variants.h"

// the same signatures as include/nimble_amd.h with the handle as void* (C linkage: no type in the symbol)
#define NBL_DECLARE_VARIANT(S)                                                                                                              \
  const char* nbl_last_error##S(void);                                                                                                     \
  int32_t nbl_version##S(void);                                                                                                            \
  int32_t nbl_device_count##S(void);                                                                                                       \
  int32_t nbl_model_create##S(const nbl_model_desc*, int32_t, void**);                                                                     \
  void nbl_model_destroy##S(void*);                                                                                                        \
  int32_t nbl_model_num_dofs##S(const void*);                                                                                              \
  int32_t nbl_model_num_action##S(const void*);                                                                                            \
  int32_t nbl_model_lcp_rows##S(const void*);                                                                                              \
  int32_t nbl_model_max_contacts##S(const void*);                                                                                          \
  size_t nbl_workspace_bytes##S(const void*, int64_t);                                                                                     \
  size_t nbl_saved_bytes##S(const void*, int64_t);                                                                                         \
  int32_t nbl_step_forward##S(void*, int64_t, const double*, const double*, const double*, double*, double*, void*, uint32_t*, void*,      \
                              size_t, void*);                                                                                              \
  int32_t nbl_step_backward##S(void*, int64_t, const void*, const double*, double*, double*, void*, size_t, void*);                        \
  int32_t nbl_set_body_inertia##S(void*, int32_t, double, const double*, const double*);                                                   \
  int32_t nbl_set_body_inertias##S(void*, int32_t, const int32_t*, const double*, const double*, const double*, void*);                    \
  int32_t nbl_set_inertia_params##S(void*, int32_t, const int32_t*, const double*);                                                        \
  int32_t nbl_set_inertia_params_on##S(void*, int32_t, const int32_t*, const double*, void*);                                              \
  int32_t nbl_num_inertia_params##S(const void*);                                                                                          \
  int32_t nbl_backward_inertia##S(void*, int64_t, const void*, double*, int32_t, void*, size_t, void*);                                    \
  size_t nbl_rollout_workspace_bytes##S(const void*, int64_t);                                                                             \
  int32_t nbl_rollout_forward##S(void*, int64_t, int32_t, const double*, const double*, int64_t, double*, void*, uint32_t*, int32_t,       \
                                 void*, size_t, void*);                                                                                    \
  int32_t nbl_rollout_backward##S(void*, int64_t, int32_t, const void*, const double*, double*, double*, void*, size_t, void*);            \
  int32_t nbl_rollout_backward_inertia##S(void*, int64_t, int32_t, const void*, const double*, double*, double*, double*, void*, size_t,   \
                                          void*);                                                                                          \
  size_t nbl_rollout_checkpoint_bytes##S(const void*, int64_t, int32_t, int32_t);                                                          \
  int32_t nbl_rollout_forward_checkpointed##S(void*, int64_t, int32_t, int32_t, const double*, const double*, int64_t, double*, void*,     \
                                              void*, uint32_t*, int32_t, void*, size_t, void*);                                            \
  int32_t nbl_rollout_backward_checkpointed##S(void*, int64_t, int32_t, int32_t, double*, const double*, int64_t, void*, const void*,      \
                                               int32_t, const double*, double*, double*, double*, void*, size_t, void*);                   \
  int32_t nbl_selftest_lcp_dantzig_timed##S(int32_t, int32_t, const double*, const double*, const double*, const double*, const int32_t*,  \
                                            double*, int32_t*, int32_t, double*);                                                          \
  int32_t nbl_selftest_pinv_rows##S(int32_t, int32_t, const double*, const int32_t*, int32_t, double*, int32_t*, int32_t, double*);        \
  int32_t nbl_selftest_stage0_rows##S(int32_t, int32_t, const double*, const double*, const double*, const uint64_t*, const uint64_t*,     \
                                      const uint64_t*, const double*, const int32_t*, const double*, double*, double*, int32_t*, double*,  \
                                      int32_t*, double*);                                                                                  \
  int32_t nbl_selftest_lcp_cascade##S(int32_t, int32_t, const double*, const double*, const double*, int32_t, const double*, const uint8_t*, double,   \
                                      double*, int32_t*, uint32_t*, double*);                                                              \
  int32_t nbl_selftest_lcp_cascade_rows##S(int32_t, int32_t, const double*, const double*, const double*, const double*, const uint8_t*,   \
                                           int32_t, const double*, const uint8_t*, double, double*, int32_t*, uint32_t*, double*);         \
  int32_t nbl_transpose_to_soa##S(const double*, double*, int64_t, int32_t, void*);                                                        \
  int32_t nbl_transpose_from_soa##S(const double*, double*, int64_t, int32_t, void*);                                                      \
  int32_t nbl_set_launch_lanes##S(void*, int32_t, int32_t);                                                                                \
  int32_t nbl_set_slices##S(void*, int32_t);                                                                                               \
  int32_t nbl_slices_for##S(const void*, int64_t);                                                                                         \
  int32_t nbl_set_deferred_join##S(void*, int32_t);                                                                                        \
  int32_t nbl_slice_stream##S(void*, int64_t, int32_t, void**, int64_t*, int64_t*);                                                        \
  int32_t nbl_join_slices##S(void*, void*);                                                                                                \
  int32_t nbl_fork_slices##S(void*, void*);                                                                                                \
  int32_t nbl_set_timing##S(void*, int32_t);                                                                                               \
  int32_t nbl_get_timing##S(void*, double*, int64_t*, double*, int64_t*);                                                                  \
  int32_t nbl_kernel_count##S(void);                                                                                                       \
  const char* nbl_kernel_name##S(int32_t);                                                                                                 \
  int32_t nbl_kernel_timing##S(void*, int32_t, double*, int64_t*);                                                                         \
  int32_t nbl_kin_map_create##S(void*, int32_t, const int32_t*, const int32_t*, const double*, void**);                                    \
  void nbl_kin_map_destroy##S(void*);                                                                                                      \
  int32_t nbl_kin_map_dim##S(const void*);                                                                                                 \
  int32_t nbl_kinematics_forward##S(void*, const void*, int64_t, const double*, double*, double*, void*);                                  \
  int32_t nbl_kinematics_backward##S(void*, const void*, int64_t, const double*, const double*, const double*, double*, int32_t, void*); \
  size_t nbl_dynamics_workspace_bytes##S(const void*, int64_t);                                                                            \
  int32_t nbl_inverse_dynamics_forward##S(void*, int64_t, const double*, const double*, int32_t, double*, void*, size_t, void*);           \
  int32_t nbl_inverse_dynamics_backward##S(void*, int64_t, const double*, const double*, int32_t, const double*, double*, double*, int32_t, \
                                           void*, size_t, void*);                                                                          \
  int32_t nbl_mass_matrix##S(void*, int64_t, const double*, double*, void*, size_t, void*);                                                \
  size_t nbl_forward_dynamics_workspace_bytes##S(const void*, int64_t);                                                                    \
  int32_t nbl_forward_dynamics_forward##S(void*, int64_t, const double*, const double*, int32_t, double*, void*, size_t, void*);           \
  int32_t nbl_forward_dynamics_backward##S(void*, int64_t, const double*, const double*, int32_t, const double*, double*, double*, int32_t, \
                                           void*, size_t, void*);                                                                          \
  int32_t nbl_inv_mass_apply##S(void*, int64_t, int32_t, const double*, const double*, double*, void*, size_t, void*);                     \
  int32_t nbl_inv_mass_matrix##S(void*, int64_t, const double*, double*, void*, size_t, void*);                                            \
  void nbl_ik_default_config##S(nbl_ik_config*);                                                                                           \
  size_t nbl_ik_workspace_bytes##S(const void*, const void*, int64_t);                                                                     \
  int32_t nbl_ik_solve##S(void*, const void*, int64_t, const double*, const double*, const nbl_ik_config*, double*, double*, int32_t*,     \
                          void*, size_t, void*);                                                                                             \
  size_t nbl_wrench_workspace_bytes##S(const void*, const void*, int64_t);                                                                 \
  int32_t nbl_inverse_dynamics_wrench_forward##S(void*, const void*, int64_t, const double*, const double*, const double*, int32_t,        \
                                                 double*, void*, size_t, void*);                                                             \
  int32_t nbl_inverse_dynamics_wrench_backward##S(void*, const void*, int64_t, const double*, const double*, const double*, int32_t,       \
                                                  const double*, double*, double*, double*, int32_t, void*, size_t, void*);                  \
  int32_t nbl_forward_dynamics_wrench_forward##S(void*, const void*, int64_t, const double*, const double*, const double*, int32_t,        \
                                                 double*, void*, size_t, void*);                                                             \
  int32_t nbl_forward_dynamics_wrench_backward##S(void*, const void*, int64_t, const double*, const double*, const double*, int32_t,       \
                                                  const double*, double*, double*, double*, int32_t, void*, size_t, void*);                  \
  int32_t nbl_contact_inverse_dynamics##S(void*, const void*, int64_t, const double*, const double*, const double*, int32_t, int32_t,      \
                                          double*, double*, void*, size_t, void*);                                                            \
  int32_t nbl_contact_readout##S(void*, int64_t, const void*, int32_t*, int32_t*, int32_t*, double*, void*);                              \
  int32_t nbl_contact_readout_rows##S(void*, int64_t, const void*, int32_t*, double*, int32_t*, void*);                                   \
  int32_t nbl_contact_body_wrenches##S(void*, int64_t, const void*, int32_t, const int32_t*, double*, void*);                              \
  int32_t nbl_body_set_create##S(void*, int32_t, const int32_t*, void**);                                                                  \
  void nbl_body_set_destroy##S(void*);                                                                                                     \
  double nbl_body_set_mass##S(void*, const void*);                                                                                         \
  int32_t nbl_body_set_origin_moments##S(void*, void*, int32_t, const int32_t*, const double*);                                            \
  size_t nbl_centroidal_workspace_bytes##S(const void*, int64_t);                                                                          \
  int32_t nbl_centroidal_forward##S(void*, const void*, int64_t, const double*, const double*, int32_t, double*, double*, double*, double*, \
                                    double*, double*, double*, void*, size_t, void*);                                                      \
  int32_t nbl_centroidal_backward##S(void*, const void*, int64_t, const double*, const double*, int32_t, const double*, const double*,     \
                                     const double*, const double*, const double*, const double*, double*, double*, int32_t, void*, size_t, \
                                     void*);                                                                                               \
  size_t nbl_sensors_workspace_bytes##S(const void*, int64_t);                                                                             \
  int32_t nbl_sensors_forward##S(void*, const void*, int64_t, const double*, const double*, const double*, double*, double*, double*,      \
                                 void*, size_t, void*);                                                                                    \
  int32_t nbl_sensors_backward##S(void*, const void*, int64_t, const double*, const double*, const double*, const double*, const double*,  \
                                  const double*, double*, double*, double*, int32_t, void*, size_t, void*);                                \
  int32_t nbl_inverse_dynamics_backward_inertia##S(void*, int64_t, const double*, const double*, int32_t, const double*, double*, int32_t, \
                                                   void*, size_t, void*);                                                                  \
  int32_t nbl_forward_dynamics_backward_inertia##S(void*, const void*, int64_t, const double*, const double*, const double*, int32_t,      \
                                                   const double*, double*, int32_t, void*, size_t, void*);

extern "C" {
NBL_DECLARE_VARIANT(_c8)
NBL_DECLARE_VARIANT(_c16)
NBL_DECLARE_VARIANT(_c64)
NBL_DECLARE_VARIANT(_c128)
}

// one table of entry points per instantiation
struct Variant {
  int id;   // 8, 16 or 64: the contact slots per world of the instantiation
  const char* (*last_error)(void);
  int32_t (*model_create)(const nbl_model_desc*, int32_t, void**);
  void (*model_destroy)(void*);
  int32_t (*model_num_dofs)(const void*);
  int32_t (*model_num_action)(const void*);
  int32_t (*model_lcp_rows)(const void*);
  int32_t (*model_max_contacts)(const void*);
  size_t (*workspace_bytes)(const void*, int64_t);
  size_t (*saved_bytes)(const void*, int64_t);
  int32_t (*step_forward)(void*, int64_t, const double*, const double*, const double*, double*, double*, void*, uint32_t*, void*, size_t, void*);
  int32_t (*step_backward)(void*, int64_t, const void*, const double*, double*, double*, void*, size_t, void*);
  int32_t (*set_body_inertia)(void*, int32_t, double, const double*, const double*);
  int32_t (*set_body_inertias)(void*, int32_t, const int32_t*, const double*, const double*, const double*, void*);
  int32_t (*set_inertia_params)(void*, int32_t, const int32_t*, const double*);
  int32_t (*set_inertia_params_on)(void*, int32_t, const int32_t*, const double*, void*);
  int32_t (*num_inertia_params)(const void*);
  int32_t (*backward_inertia)(void*, int64_t, const void*, double*, int32_t, void*, size_t, void*);
  size_t (*rollout_workspace_bytes)(const void*, int64_t);
  int32_t (*rollout_forward)(void*, int64_t, int32_t, const double*, const double*, int64_t, double*, void*, uint32_t*, int32_t, void*, size_t, void*);
  int32_t (*rollout_backward)(void*, int64_t, int32_t, const void*, const double*, double*, double*, void*, size_t, void*);
  int32_t (*rollout_backward_inertia)(void*, int64_t, int32_t, const void*, const double*, double*, double*, double*, void*, size_t, void*);
  size_t (*rollout_checkpoint_bytes)(const void*, int64_t, int32_t, int32_t);
  int32_t (*rollout_forward_checkpointed)(void*, int64_t, int32_t, int32_t, const double*, const double*, int64_t, double*, void*, void*, uint32_t*, int32_t,
                                          void*, size_t, void*);
  int32_t (*rollout_backward_checkpointed)(void*, int64_t, int32_t, int32_t, double*, const double*, int64_t, void*, const void*, int32_t, const double*,
                                           double*, double*, double*, void*, size_t, void*);
  int32_t (*selftest_lcp_dantzig_timed)(int32_t, int32_t, const double*, const double*, const double*, const double*, const int32_t*, double*, int32_t*,
                                        int32_t, double*);
  int32_t (*selftest_pinv_rows)(int32_t, int32_t, const double*, const int32_t*, int32_t, double*, int32_t*, int32_t, double*);
  int32_t (*set_launch_lanes)(void*, int32_t, int32_t);
  int32_t (*set_slices)(void*, int32_t);
  int32_t (*slices_for)(const void*, int64_t);
  int32_t (*set_deferred_join)(void*, int32_t);
  int32_t (*slice_stream)(void*, int64_t, int32_t, void**, int64_t*, int64_t*);
  int32_t (*join_slices)(void*, void*);
  int32_t (*fork_slices)(void*, void*);
  int32_t (*set_timing)(void*, int32_t);
  int32_t (*get_timing)(void*, double*, int64_t*, double*, int64_t*);
  int32_t (*kernel_timing)(void*, int32_t, double*, int64_t*);
  int32_t (*kin_map_create)(void*, int32_t, const int32_t*, const int32_t*, const double*, void**);
  void (*kin_map_destroy)(void*);
  int32_t (*kin_map_dim)(const void*);
  int32_t (*kinematics_forward)(void*, const void*, int64_t, const double*, double*, double*, void*);
  int32_t (*kinematics_backward)(void*, const void*, int64_t, const double*, const double*, const double*, double*, int32_t, void*);
  size_t (*dynamics_workspace_bytes)(const void*, int64_t);
  int32_t (*inverse_dynamics_forward)(void*, int64_t, const double*, const double*, int32_t, double*, void*, size_t, void*);
  int32_t (*inverse_dynamics_backward)(void*, int64_t, const double*, const double*, int32_t, const double*, double*, double*, int32_t, void*, size_t, void*);
  int32_t (*mass_matrix)(void*, int64_t, const double*, double*, void*, size_t, void*);
  size_t (*ik_workspace_bytes)(const void*, const void*, int64_t);
  int32_t (*ik_solve)(void*, const void*, int64_t, const double*, const double*, const nbl_ik_config*, double*, double*, int32_t*, void*, size_t, void*);
  size_t (*forward_dynamics_workspace_bytes)(const void*, int64_t);
  int32_t (*forward_dynamics_forward)(void*, int64_t, const double*, const double*, int32_t, double*, void*, size_t, void*);
  int32_t (*forward_dynamics_backward)(void*, int64_t, const double*, const double*, int32_t, const double*, double*, double*, int32_t, void*, size_t, void*);
  int32_t (*inv_mass_apply)(void*, int64_t, int32_t, const double*, const double*, double*, void*, size_t, void*);
  int32_t (*inv_mass_matrix)(void*, int64_t, const double*, double*, void*, size_t, void*);
  size_t (*wrench_workspace_bytes)(const void*, const void*, int64_t);
  int32_t (*inverse_dynamics_wrench_forward)(void*, const void*, int64_t, const double*, const double*, const double*, int32_t, double*, void*, size_t, void*);
  int32_t (*inverse_dynamics_wrench_backward)(void*, const void*, int64_t, const double*, const double*, const double*, int32_t, const double*, double*, double*, double*, int32_t, void*, size_t, void*);
  int32_t (*forward_dynamics_wrench_forward)(void*, const void*, int64_t, const double*, const double*, const double*, int32_t, double*, void*, size_t, void*);
  int32_t (*forward_dynamics_wrench_backward)(void*, const void*, int64_t, const double*, const double*, const double*, int32_t, const double*, double*, double*, double*, int32_t, void*, size_t, void*);
  int32_t (*contact_inverse_dynamics)(void*, const void*, int64_t, const double*, const double*, const double*, int32_t, int32_t, double*, double*, void*, size_t, void*);
  int32_t (*contact_readout)(void*, int64_t, const void*, int32_t*, int32_t*, int32_t*, double*, void*);
  int32_t (*contact_readout_rows)(void*, int64_t, const void*, int32_t*, double*, int32_t*, void*);
  int32_t (*contact_body_wrenches)(void*, int64_t, const void*, int32_t, const int32_t*, double*, void*);
  int32_t (*body_set_create)(void*, int32_t, const int32_t*, void**);
  void (*body_set_destroy)(void*);
  double (*body_set_mass)(void*, const void*);
  int32_t (*body_set_origin_moments)(void*, void*, int32_t, const int32_t*, const double*);
  size_t (*centroidal_workspace_bytes)(const void*, int64_t);
  int32_t (*centroidal_forward)(void*, const void*, int64_t, const double*, const double*, int32_t, double*, double*, double*, double*, double*, double*, double*, void*, size_t, void*);
  int32_t (*centroidal_backward)(void*, const void*, int64_t, const double*, const double*, int32_t, const double*, const double*, const double*, const double*, const double*, const double*, double*, double*, int32_t, void*, size_t, void*);
  size_t (*sensors_workspace_bytes)(const void*, int64_t);
  int32_t (*sensors_forward)(void*, const void*, int64_t, const double*, const double*, const double*, double*, double*, double*, void*, size_t, void*);
  int32_t (*sensors_backward)(void*, const void*, int64_t, const double*, const double*, const double*, const double*, const double*, const double*, double*, double*, double*, int32_t, void*, size_t, void*);
  int32_t (*inverse_dynamics_backward_inertia)(void*, int64_t, const double*, const double*, int32_t, const double*, double*, int32_t, void*, size_t, void*);
  int32_t (*forward_dynamics_backward_inertia)(void*, const void*, int64_t, const double*, const double*, const double*, int32_t, const double*, double*, int32_t, void*, size_t, void*);
};
#define NBL_VARIANT_TABLE(ID, S)                                                                                                              \
  {ID, nbl_last_error##S, nbl_model_create##S, nbl_model_destroy##S, nbl_model_num_dofs##S, nbl_model_num_action##S, nbl_model_lcp_rows##S,    \
   nbl_model_max_contacts##S, nbl_workspace_bytes##S, nbl_saved_bytes##S, nbl_step_forward##S, nbl_step_backward##S, nbl_set_body_inertia##S, \
   nbl_set_body_inertias##S, nbl_set_inertia_params##S, nbl_set_inertia_params_on##S, nbl_num_inertia_params##S, nbl_backward_inertia##S,     \
   nbl_rollout_workspace_bytes##S, nbl_rollout_forward##S, nbl_rollout_backward##S, nbl_rollout_backward_inertia##S,                          \
   nbl_rollout_checkpoint_bytes##S, nbl_rollout_forward_checkpointed##S, nbl_rollout_backward_checkpointed##S,                               \
   nbl_selftest_lcp_dantzig_timed##S, nbl_selftest_pinv_rows##S, nbl_set_launch_lanes##S, nbl_set_slices##S, nbl_slices_for##S,               \
   nbl_set_deferred_join##S, nbl_slice_stream##S, nbl_join_slices##S, nbl_fork_slices##S,                                                                         \
   nbl_set_timing##S, nbl_get_timing##S, nbl_kernel_timing##S, nbl_kin_map_create##S, nbl_kin_map_destroy##S, nbl_kin_map_dim##S,          \
   nbl_kinematics_forward##S, nbl_kinematics_backward##S, nbl_dynamics_workspace_bytes##S, nbl_inverse_dynamics_forward##S,                 \
   nbl_inverse_dynamics_backward##S, nbl_mass_matrix##S, nbl_ik_workspace_bytes##S, nbl_ik_solve##S,                        \
   nbl_forward_dynamics_workspace_bytes##S, nbl_forward_dynamics_forward##S, nbl_forward_dynamics_backward##S, nbl_inv_mass_apply##S,       \
   nbl_inv_mass_matrix##S, nbl_wrench_workspace_bytes##S, nbl_inverse_dynamics_wrench_forward##S,                                          \
   nbl_inverse_dynamics_wrench_backward##S, nbl_forward_dynamics_wrench_forward##S, nbl_forward_dynamics_wrench_backward##S,                \
   nbl_contact_inverse_dynamics##S, nbl_contact_readout##S, nbl_contact_readout_rows##S, nbl_contact_body_wrenches##S,       \
   nbl_body_set_create##S, nbl_body_set_destroy##S, nbl_body_set_mass##S, nbl_body_set_origin_moments##S,         \
   nbl_centroidal_workspace_bytes##S, nbl_centroidal_forward##S, nbl_centroidal_backward##S,                         \
   nbl_sensors_workspace_bytes##S, nbl_sensors_forward##S, nbl_sensors_backward##S,                                  \
   nbl_inverse_dynamics_backward_inertia##S, nbl_forward_dynamics_backward_inertia##S}
constexpr int kNumVariants = 4;
static const Variant kVariants[kNumVariants] = {NBL_VARIANT_TABLE(8, _c8), NBL_VARIANT_TABLE(16, _c16), NBL_VARIANT_TABLE(64, _c64),
                                                     NBL_VARIANT_TABLE(128, _c128)};

struct nbl_model {
  const Variant* v;   // the instantiation that owns `impl`
  void* impl;
};
struct nbl_kin_map {
  const Variant* v;   // the instantiation of the model it was made against
  void* impl;
};
struct nbl_body_set {
  const Variant* v;   // the instantiation of the model it was made against
  void* impl;
};

namespace {
thread_local const Variant* g_errVariant = nullptr;   // whose message nbl_last_error returns: nullptr = the dispatcher's own
thread_local std::string g_err;
int ownError(int code, const char* msg) {
  g_err = msg;
  g_errVariant = nullptr;
  return code;
}
int noted(const nbl_model* m, int rc) {   // remember which instantiation holds the text of a failure
  if (rc != NBL_OK) g_errVariant = m->v;
  return rc;
}
}  // namespace

// int-returning entry point on a handle: FN = the table entry, then its arguments after the implementation handle
#define NBL_FWD(m, FN, ...) (!(m) ? ownError(NBL_E_BADARG, "null model") : noted((m), (m)->v->FN((m)->impl, ##__VA_ARGS__)))
#define NBL_GET(m, FN, ...) (!(m) ? 0 : (m)->v->FN((m)->impl, ##__VA_ARGS__))

extern "C" {

const char* nbl_last_error(void) { return g_errVariant ? g_errVariant->last_error() : g_err.c_str(); }
int32_t nbl_version(void) { return nbl_version_c8(); }
int32_t nbl_device_count(void) { return nbl_device_count_c8(); }

int32_t nbl_model_create(const nbl_model_desc* d, int32_t device, nbl_model** out) {
  if (!d || !out) return ownError(NBL_E_BADARG, "null argument");
  *out = nullptr;
  void* impl = nullptr;
  // the smallest instantiation that holds the model: contact slots first (a model without colliders and without enforced joint limits has no
  // contact stage: the 24-row build whatever max_contacts says), then whatever an instantiation answers NBL_E_CAPACITY to (its collider /
  // collider-pair budget: 16 / 32, 32 / 64, 64 / 512, 64 / 512).  The two general instantiations differ in their row budget only (192 / 384 rows:
  // the size of the per-world scratch and record): 64 slots unless the model asks for more
  const bool contactStage = d->n_boxes > 0 || d->dof_limit_enforced != nullptr;
  int first = 0;
  if (contactStage && d->max_contacts > 64) first = 3;
  else if (contactStage && (d->max_contacts > 16 || d->n_boxes > 32)) first = 2;
  else if (contactStage && (d->max_contacts > 8 || d->n_boxes > 16)) first = 1;
  // developer knob: NBL_MIN_VARIANT=0..3 starts the search at a later instantiation (never an earlier one: that would truncate)
  if (const char* e = getenv("NBL_MIN_VARIANT")) { const int f = atoi(e); if (f > first && f < kNumVariants) first = f; }
  int32_t rc = NBL_E_CAPACITY;
  const Variant* v = nullptr;
  for (int k = first; k < kNumVariants && rc == NBL_E_CAPACITY; k++) {
    v = &kVariants[k];
    rc = v->model_create(d, device, &impl);
    g_errVariant = v;
  }
  if (rc == NBL_E_CAPACITY) rc = NBL_E_UNSUPPORTED;
  if (rc != NBL_OK) return rc;
  nbl_model* m = new nbl_model();
  m->v = v;
  m->impl = impl;
  *out = m;
  return NBL_OK;
}

void nbl_model_destroy(nbl_model* m) {
  if (!m) return;
  m->v->model_destroy(m->impl);
  delete m;
}

int32_t nbl_model_num_dofs(const nbl_model* m) { return NBL_GET(m, model_num_dofs); }
int32_t nbl_model_num_action(const nbl_model* m) { return NBL_GET(m, model_num_action); }
int32_t nbl_model_lcp_rows(const nbl_model* m) { return NBL_GET(m, model_lcp_rows); }
int32_t nbl_model_max_contacts(const nbl_model* m) { return NBL_GET(m, model_max_contacts); }
size_t nbl_workspace_bytes(const nbl_model* m, int64_t B) { return NBL_GET(m, workspace_bytes, B); }
size_t nbl_saved_bytes(const nbl_model* m, int64_t B) { return NBL_GET(m, saved_bytes, B); }

int32_t nbl_step_forward(nbl_model* m, int64_t B, const double* state, const double* action, const double* lcp_cache_in, double* next_state,
                         double* lcp_cache_out, void* saved, uint32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  return NBL_FWD(m, step_forward, B, state, action, lcp_cache_in, next_state, lcp_cache_out, saved, status, workspace, workspace_bytes, stream);
}
int32_t nbl_step_backward(nbl_model* m, int64_t B, const void* saved, const double* grad_next_state, double* grad_state, double* grad_action,
                          void* workspace, size_t workspace_bytes, void* stream) {
  return NBL_FWD(m, step_backward, B, saved, grad_next_state, grad_state, grad_action, workspace, workspace_bytes, stream);
}

int32_t nbl_set_body_inertia(nbl_model* m, int32_t body, double mass, const double* com, const double* inertia) {
  return NBL_FWD(m, set_body_inertia, body, mass, com, inertia);
}
int32_t nbl_set_body_inertias(nbl_model* m, int32_t count, const int32_t* bodies, const double* mass, const double* com, const double* inertia,
                              void* stream) {
  return NBL_FWD(m, set_body_inertias, count, bodies, mass, com, inertia, stream);
}
int32_t nbl_set_inertia_params(nbl_model* m, int32_t count, const int32_t* bodies, const double* dG) { return NBL_FWD(m, set_inertia_params, count, bodies, dG); }
int32_t nbl_set_inertia_params_on(nbl_model* m, int32_t count, const int32_t* bodies, const double* dG, void* stream) {
  return NBL_FWD(m, set_inertia_params_on, count, bodies, dG, stream);
}
int32_t nbl_num_inertia_params(const nbl_model* m) { return NBL_GET(m, num_inertia_params); }
int32_t nbl_backward_inertia(nbl_model* m, int64_t B, const void* saved, double* grad_params, int32_t accumulate, void* workspace,
                             size_t workspace_bytes, void* stream) {
  return NBL_FWD(m, backward_inertia, B, saved, grad_params, accumulate, workspace, workspace_bytes, stream);
}

size_t nbl_rollout_workspace_bytes(const nbl_model* m, int64_t B) { return NBL_GET(m, rollout_workspace_bytes, B); }
int32_t nbl_rollout_forward(nbl_model* m, int64_t B, int32_t T, const double* state0, const double* actions, int64_t action_stride, double* states,
                            void* saved, uint32_t* status, int32_t warm_start, void* workspace, size_t workspace_bytes, void* stream) {
  return NBL_FWD(m, rollout_forward, B, T, state0, actions, action_stride, states, saved, status, warm_start, workspace, workspace_bytes, stream);
}
int32_t nbl_rollout_backward(nbl_model* m, int64_t B, int32_t T, const void* saved, const double* grad_states, double* grad_state0,
                             double* grad_actions, void* workspace, size_t workspace_bytes, void* stream) {
  return NBL_FWD(m, rollout_backward, B, T, saved, grad_states, grad_state0, grad_actions, workspace, workspace_bytes, stream);
}
int32_t nbl_rollout_backward_inertia(nbl_model* m, int64_t B, int32_t T, const void* saved, const double* grad_states, double* grad_state0,
                                     double* grad_actions, double* grad_params, void* workspace, size_t workspace_bytes, void* stream) {
  return NBL_FWD(m, rollout_backward_inertia, B, T, saved, grad_states, grad_state0, grad_actions, grad_params, workspace, workspace_bytes, stream);
}
size_t nbl_rollout_checkpoint_bytes(const nbl_model* m, int64_t B, int32_t T, int32_t segment) { return NBL_GET(m, rollout_checkpoint_bytes, B, T, segment); }
int32_t nbl_rollout_forward_checkpointed(nbl_model* m, int64_t B, int32_t T, int32_t segment, const double* state0, const double* actions,
                                         int64_t action_stride, double* states, void* saved, void* checkpoints, uint32_t* status,
                                         int32_t warm_start, void* workspace, size_t workspace_bytes, void* stream) {
  return NBL_FWD(m, rollout_forward_checkpointed, B, T, segment, state0, actions, action_stride, states, saved, checkpoints, status, warm_start, workspace,
                 workspace_bytes, stream);
}
int32_t nbl_rollout_backward_checkpointed(nbl_model* m, int64_t B, int32_t T, int32_t segment, double* states, const double* actions,
                                          int64_t action_stride, void* saved, const void* checkpoints, int32_t warm_start,
                                          const double* grad_states, double* grad_state0, double* grad_actions, double* grad_params,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  return NBL_FWD(m, rollout_backward_checkpointed, B, T, segment, states, actions, action_stride, saved, checkpoints, warm_start, grad_states, grad_state0,
                 grad_actions, grad_params, workspace, workspace_bytes, stream);
}

// ---- self-tests: the problem size picks the instantiation whose device code runs ----
int32_t nbl_selftest_lcp_dantzig_timed(int32_t count, int32_t n, const double* A, const double* b, const double* lo, const double* hi,
                                       const int32_t* findex, double* x, int32_t* rc, int32_t reps, double* ms_per_launch) {
  const Variant* v = &kVariants[n > 192 ? 3 : (n > 48 ? 2 : (n > 24 ? 1 : 0))];     // (n > 48: the general driver, gen_dantzig_dev.hpp; n > 192: its 384-row build)
  g_errVariant = v;
  return v->selftest_lcp_dantzig_timed(count, n, A, b, lo, hi, findex, x, rc, reps, ms_per_launch);
}
int32_t nbl_selftest_lcp_dantzig(int32_t count, int32_t n, const double* A, const double* b, const double* lo, const double* hi,
                                 const int32_t* findex, double* x, int32_t* rc) {
  return nbl_selftest_lcp_dantzig_timed(count, n, A, b, lo, hi, findex, x, rc, 1, nullptr);
}
int32_t nbl_selftest_lcp_cascade(int32_t count, int32_t m, const double* A, const double* b, const double* mu, int32_t have_cache,
                                 const double* x_cache, const uint8_t* on, double fallback_cfm, double* x, int32_t* cls, uint32_t* st, double* cfm) {
  g_errVariant = &kVariants[2];       // (the general instantiation's code, whatever the size)
  return nbl_selftest_lcp_cascade_c64(count, m, A, b, mu, have_cache, x_cache, on, fallback_cfm, x, cls, st, cfm);
}
int32_t nbl_selftest_lcp_cascade_rows(int32_t count, int32_t m, const double* A, const double* b, const double* mu, const double* bound,
                                      const uint8_t* lim, int32_t have_cache, const double* x_cache, const uint8_t* on, double fallback_cfm,
                                      double* x, int32_t* cls, uint32_t* st, double* cfm) {
  g_errVariant = &kVariants[2];       // (the general instantiation's code, whatever the size)
  return nbl_selftest_lcp_cascade_rows_c64(count, m, A, b, mu, bound, lim, have_cache, x_cache, on, fallback_cfm, x, cls, st, cfm);
}
int32_t nbl_selftest_pinv_rows(int32_t count, int32_t rows, const double* Q, const int32_t* cTrue, int32_t route, double* P, int32_t* rank,
                               int32_t reps, double* ms_per_launch) {
  if (rows != 24 && rows != 48) return ownError(NBL_E_BADARG, "rows must be 24 or 48");
  const Variant* v = &kVariants[rows == 48 ? 1 : 0];
  g_errVariant = v;
  return v->selftest_pinv_rows(count, rows, Q, cTrue, route, P, rank, reps, ms_per_launch);
}
int32_t nbl_selftest_pinv(int32_t count, const double* Q, const int32_t* cTrue, int32_t route, double* P, int32_t* rank, int32_t reps,
                          double* ms_per_launch) {
  return nbl_selftest_pinv_rows(count, 24, Q, cTrue, route, P, rank, reps, ms_per_launch);
}
int32_t nbl_selftest_stage0_rows(int32_t count, int32_t rows, const double* A, const double* b, const double* mu, const uint64_t* mask,
                                 const uint64_t* lim_mask, const uint64_t* neg_mask, const double* cfm, const int32_t* have_cache,
                                 const double* x_cache, double* x, double* x0, int32_t* cls, double* e_out, int32_t* ok, double* pinv) {
  if (rows != 24 && rows != 48) return ownError(NBL_E_BADARG, "rows must be 24 or 48");
  g_errVariant = &kVariants[rows == 48 ? 1 : 0];
  return rows == 48 ? nbl_selftest_stage0_rows_c16(count, rows, A, b, mu, mask, lim_mask, neg_mask, cfm, have_cache, x_cache, x, x0, cls, e_out, ok, pinv)
                    : nbl_selftest_stage0_rows_c8(count, rows, A, b, mu, mask, lim_mask, neg_mask, cfm, have_cache, x_cache, x, x0, cls, e_out, ok, pinv);
}

int32_t nbl_transpose_to_soa(const double* src_bd, double* dst_db, int64_t B, int32_t d, void* stream) {
  g_errVariant = &kVariants[0];
  return nbl_transpose_to_soa_c8(src_bd, dst_db, B, d, stream);
}
int32_t nbl_transpose_from_soa(const double* src_db, double* dst_bd, int64_t B, int32_t d, void* stream) {
  g_errVariant = &kVariants[0];
  return nbl_transpose_from_soa_c8(src_db, dst_bd, B, d, stream);
}

int32_t nbl_set_launch_lanes(nbl_model* m, int32_t tree_lanes, int32_t lcp_lanes) { return NBL_FWD(m, set_launch_lanes, tree_lanes, lcp_lanes); }
int32_t nbl_set_slices(nbl_model* m, int32_t slices) { return NBL_FWD(m, set_slices, slices); }
int32_t nbl_slices_for(const nbl_model* m, int64_t B) { return NBL_GET(m, slices_for, B); }
int32_t nbl_set_deferred_join(nbl_model* m, int32_t enabled) { return NBL_FWD(m, set_deferred_join, enabled); }
int32_t nbl_slice_stream(nbl_model* m, int64_t B, int32_t slice, void** stream, int64_t* first_world, int64_t* end_world) {
  return NBL_FWD(m, slice_stream, B, slice, stream, first_world, end_world);
}
int32_t nbl_join_slices(nbl_model* m, void* stream) { return NBL_FWD(m, join_slices, stream); }
int32_t nbl_fork_slices(nbl_model* m, void* stream) { return NBL_FWD(m, fork_slices, stream); }
int32_t nbl_set_timing(nbl_model* m, int32_t enabled) { return NBL_FWD(m, set_timing, enabled); }
int32_t nbl_get_timing(nbl_model* m, double* fwd_ms_sum, int64_t* fwd_count, double* bwd_ms_sum, int64_t* bwd_count) {
  return NBL_FWD(m, get_timing, fwd_ms_sum, fwd_count, bwd_ms_sum, bwd_count);
}
int32_t nbl_kernel_count(void) { return nbl_kernel_count_c8(); }
const char* nbl_kernel_name(int32_t i) { return nbl_kernel_name_c8(i); }
int32_t nbl_kernel_timing(nbl_model* m, int32_t i, double* ms_sum, int64_t* count) { return NBL_FWD(m, kernel_timing, i, ms_sum, count); }

int32_t nbl_kin_map_create(nbl_model* m, int32_t count, const int32_t* kind, const int32_t* body, const double* T_offset, nbl_kin_map** out) {
  if (!m || !out) return ownError(NBL_E_BADARG, "null argument");
  *out = nullptr;
  void* impl = nullptr;
  const int32_t rc = noted(m, m->v->kin_map_create(m->impl, count, kind, body, T_offset, &impl));
  if (rc != NBL_OK) return rc;
  *out = new nbl_kin_map{m->v, impl};
  return NBL_OK;
}
void nbl_kin_map_destroy(nbl_kin_map* k) {
  if (!k) return;
  k->v->kin_map_destroy(k->impl);
  delete k;
}
int32_t nbl_kin_map_dim(const nbl_kin_map* k) { return k ? k->v->kin_map_dim(k->impl) : 0; }
int32_t nbl_kinematics_forward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, double* pos, double* vel, void* stream) {
  if (!k) return ownError(NBL_E_BADARG, "null kinematics map");
  if (m && k->v != m->v) return ownError(NBL_E_BADARG, "the kinematics map was made for another model");
  return NBL_FWD(m, kinematics_forward, k->impl, B, state, pos, vel, stream);
}
int32_t nbl_kinematics_backward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* grad_pos, const double* grad_vel,
                                double* grad_state, int32_t accumulate, void* stream) {
  if (!k) return ownError(NBL_E_BADARG, "null kinematics map");
  if (m && k->v != m->v) return ownError(NBL_E_BADARG, "the kinematics map was made for another model");
  return NBL_FWD(m, kinematics_backward, k->impl, B, state, grad_pos, grad_vel, grad_state, accumulate, stream);
}

size_t nbl_dynamics_workspace_bytes(const nbl_model* m, int64_t B) { return m ? m->v->dynamics_workspace_bytes(m->impl, B) : 0; }
int32_t nbl_inverse_dynamics_forward(nbl_model* m, int64_t B, const double* state, const double* accel, int32_t flags, double* tau,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  return NBL_FWD(m, inverse_dynamics_forward, B, state, accel, flags, tau, workspace, workspace_bytes, stream);
}
int32_t nbl_inverse_dynamics_backward(nbl_model* m, int64_t B, const double* state, const double* accel, int32_t flags, const double* grad_tau,
                                      double* grad_state, double* grad_accel, int32_t accumulate, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  return NBL_FWD(m, inverse_dynamics_backward, B, state, accel, flags, grad_tau, grad_state, grad_accel, accumulate, workspace, workspace_bytes,
                 stream);
}
int32_t nbl_mass_matrix(nbl_model* m, int64_t B, const double* state, double* M, void* workspace, size_t workspace_bytes, void* stream) {
  return NBL_FWD(m, mass_matrix, B, state, M, workspace, workspace_bytes, stream);
}

size_t nbl_forward_dynamics_workspace_bytes(const nbl_model* m, int64_t B) { return m ? m->v->forward_dynamics_workspace_bytes(m->impl, B) : 0; }
int32_t nbl_forward_dynamics_forward(nbl_model* m, int64_t B, const double* state, const double* tau, int32_t flags, double* accel,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  return NBL_FWD(m, forward_dynamics_forward, B, state, tau, flags, accel, workspace, workspace_bytes, stream);
}
int32_t nbl_forward_dynamics_backward(nbl_model* m, int64_t B, const double* state, const double* tau, int32_t flags, const double* grad_accel,
                                      double* grad_state, double* grad_tau, int32_t accumulate, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  return NBL_FWD(m, forward_dynamics_backward, B, state, tau, flags, grad_accel, grad_state, grad_tau, accumulate, workspace, workspace_bytes,
                 stream);
}
int32_t nbl_inv_mass_apply(nbl_model* m, int64_t B, int32_t R, const double* state, const double* X, double* Y, void* workspace,
                           size_t workspace_bytes, void* stream) {
  return NBL_FWD(m, inv_mass_apply, B, R, state, X, Y, workspace, workspace_bytes, stream);
}
int32_t nbl_inv_mass_matrix(nbl_model* m, int64_t B, const double* state, double* Minv, void* workspace, size_t workspace_bytes, void* stream) {
  return NBL_FWD(m, inv_mass_matrix, B, state, Minv, workspace, workspace_bytes, stream);
}

// the wrench calls: a NULL map is a wrench set with no entries
#define NBL_WRENCH_MAP_CHECK(m, k) \
  if ((m) && (k) && (k)->v != (m)->v) return ownError(NBL_E_BADARG, "the kinematics map was made for another model")
size_t nbl_wrench_workspace_bytes(const nbl_model* m, const nbl_kin_map* k, int64_t B) {
  return (m && (!k || k->v == m->v)) ? m->v->wrench_workspace_bytes(m->impl, k ? k->impl : nullptr, B) : 0;
}
int32_t nbl_inverse_dynamics_wrench_forward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* accel,
                                            const double* wrench, int32_t flags, double* tau, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  NBL_WRENCH_MAP_CHECK(m, k);
  return NBL_FWD(m, inverse_dynamics_wrench_forward, k ? k->impl : nullptr, B, state, accel, wrench, flags, tau, workspace, workspace_bytes, stream);
}
int32_t nbl_inverse_dynamics_wrench_backward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* accel,
                                             const double* wrench, int32_t flags, const double* grad_tau, double* grad_state, double* grad_accel,
                                             double* grad_wrench, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  NBL_WRENCH_MAP_CHECK(m, k);
  return NBL_FWD(m, inverse_dynamics_wrench_backward, k ? k->impl : nullptr, B, state, accel, wrench, flags, grad_tau, grad_state, grad_accel,
                 grad_wrench, accumulate, workspace, workspace_bytes, stream);
}
int32_t nbl_forward_dynamics_wrench_forward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* tau,
                                            const double* wrench, int32_t flags, double* accel, void* workspace, size_t workspace_bytes,
                                            void* stream) {
  NBL_WRENCH_MAP_CHECK(m, k);
  return NBL_FWD(m, forward_dynamics_wrench_forward, k ? k->impl : nullptr, B, state, tau, wrench, flags, accel, workspace, workspace_bytes, stream);
}
int32_t nbl_forward_dynamics_wrench_backward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* tau,
                                             const double* wrench, int32_t flags, const double* grad_accel, double* grad_state, double* grad_tau,
                                             double* grad_wrench, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  NBL_WRENCH_MAP_CHECK(m, k);
  return NBL_FWD(m, forward_dynamics_wrench_backward, k ? k->impl : nullptr, B, state, tau, wrench, flags, grad_accel, grad_state, grad_tau,
                 grad_wrench, accumulate, workspace, workspace_bytes, stream);
}
int32_t nbl_contact_inverse_dynamics(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* accel,
                                     const double* wrench_guess, int32_t mode, int32_t flags, double* wrench_out, double* tau, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  NBL_WRENCH_MAP_CHECK(m, k);
  return NBL_FWD(m, contact_inverse_dynamics, k ? k->impl : nullptr, B, state, accel, wrench_guess, mode, flags, wrench_out, tau, workspace,
                 workspace_bytes, stream);
}

int32_t nbl_inverse_dynamics_backward_inertia(nbl_model* m, int64_t B, const double* state, const double* accel, int32_t flags,
                                              const double* grad_tau, double* grad_params, int32_t accumulate, void* workspace,
                                              size_t workspace_bytes, void* stream) {
  return NBL_FWD(m, inverse_dynamics_backward_inertia, B, state, accel, flags, grad_tau, grad_params, accumulate, workspace, workspace_bytes, stream);
}
int32_t nbl_forward_dynamics_backward_inertia(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* tau,
                                              const double* wrench, int32_t flags, const double* grad_accel, double* grad_params,
                                              int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  NBL_WRENCH_MAP_CHECK(m, k);
  return NBL_FWD(m, forward_dynamics_backward_inertia, k ? k->impl : nullptr, B, state, tau, wrench, flags, grad_accel, grad_params, accumulate,
                 workspace, workspace_bytes, stream);
}

int32_t nbl_contact_readout(nbl_model* m, int64_t B, const void* saved, int32_t* count, int32_t* n_limit_rows, int32_t* n_friction_rows,
                            double* contacts, void* stream) {
  return NBL_FWD(m, contact_readout, B, saved, count, n_limit_rows, n_friction_rows, contacts, stream);
}
int32_t nbl_contact_readout_rows(nbl_model* m, int64_t B, const void* saved, int32_t* n_rows, double* impulse, int32_t* mapping, void* stream) {
  return NBL_FWD(m, contact_readout_rows, B, saved, n_rows, impulse, mapping, stream);
}
int32_t nbl_contact_body_wrenches(nbl_model* m, int64_t B, const void* saved, int32_t E, const int32_t* bodies, double* wrench, void* stream) {
  return NBL_FWD(m, contact_body_wrenches, B, saved, E, bodies, wrench, stream);
}

int32_t nbl_body_set_create(nbl_model* m, int32_t count, const int32_t* bodies, nbl_body_set** out) {
  if (!m || !out) return ownError(NBL_E_BADARG, "null argument");
  *out = nullptr;
  void* impl = nullptr;
  const int32_t rc = noted(m, m->v->body_set_create(m->impl, count, bodies, &impl));
  if (rc != NBL_OK) return rc;
  *out = new nbl_body_set{m->v, impl};
  return NBL_OK;
}
void nbl_body_set_destroy(nbl_body_set* s) {
  if (!s) return;
  s->v->body_set_destroy(s->impl);
  delete s;
}
double nbl_body_set_mass(nbl_model* m, const nbl_body_set* s) {
  if (!m || !s) { (void)ownError(NBL_E_BADARG, "null argument"); return 0.0; }
  if (s->v != m->v) { (void)ownError(NBL_E_BADARG, "the body set was made for another model"); return 0.0; }
  g_errVariant = m->v;   // (a refusal's text is the instantiation's)
  return m->v->body_set_mass(m->impl, s->impl);
}
int32_t nbl_body_set_origin_moments(nbl_model* m, nbl_body_set* s, int32_t count, const int32_t* bodies, const double* moments) {
  if (!s) return ownError(NBL_E_BADARG, "null body set");
  if (m && s->v != m->v) return ownError(NBL_E_BADARG, "the body set was made for another model");
  return NBL_FWD(m, body_set_origin_moments, s->impl, count, bodies, moments);
}
size_t nbl_centroidal_workspace_bytes(const nbl_model* m, int64_t B) { return m ? m->v->centroidal_workspace_bytes(m->impl, B) : 0; }
int32_t nbl_centroidal_forward(nbl_model* m, const nbl_body_set* s, int64_t B, const double* state, const double* accel, int32_t flags,
                               double* com, double* com_vel, double* com_acc, double* momentum, double* ke, double* pe, double* Jcom,
                               void* workspace, size_t workspace_bytes, void* stream) {
  if (!s) return ownError(NBL_E_BADARG, "null body set");
  if (m && s->v != m->v) return ownError(NBL_E_BADARG, "the body set was made for another model");
  return NBL_FWD(m, centroidal_forward, s->impl, B, state, accel, flags, com, com_vel, com_acc, momentum, ke, pe, Jcom, workspace, workspace_bytes,
                 stream);
}
int32_t nbl_centroidal_backward(nbl_model* m, const nbl_body_set* s, int64_t B, const double* state, const double* accel, int32_t flags,
                                const double* g_com, const double* g_com_vel, const double* g_com_acc, const double* g_momentum,
                                const double* g_ke, const double* g_pe, double* grad_state, double* grad_accel, int32_t accumulate,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!s) return ownError(NBL_E_BADARG, "null body set");
  if (m && s->v != m->v) return ownError(NBL_E_BADARG, "the body set was made for another model");
  return NBL_FWD(m, centroidal_backward, s->impl, B, state, accel, flags, g_com, g_com_vel, g_com_acc, g_momentum, g_ke, g_pe, grad_state,
                 grad_accel, accumulate, workspace, workspace_bytes, stream);
}

size_t nbl_sensors_workspace_bytes(const nbl_model* m, int64_t B) { return m ? m->v->sensors_workspace_bytes(m->impl, B) : 0; }
int32_t nbl_sensors_forward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* accel, const double* field,
                            double* gyro, double* acc, double* mag, void* workspace, size_t workspace_bytes, void* stream) {
  if (!k) return ownError(NBL_E_BADARG, "null sensor set");
  if (m && k->v != m->v) return ownError(NBL_E_BADARG, "the kinematics map was made for another model");
  return NBL_FWD(m, sensors_forward, k->impl, B, state, accel, field, gyro, acc, mag, workspace, workspace_bytes, stream);
}
int32_t nbl_sensors_backward(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* state, const double* accel, const double* field,
                             const double* g_gyro, const double* g_acc, const double* g_mag, double* grad_state, double* grad_accel,
                             double* grad_field, int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream) {
  if (!k) return ownError(NBL_E_BADARG, "null sensor set");
  if (m && k->v != m->v) return ownError(NBL_E_BADARG, "the kinematics map was made for another model");
  return NBL_FWD(m, sensors_backward, k->impl, B, state, accel, field, g_gyro, g_acc, g_mag, grad_state, grad_accel, grad_field, accumulate,
                 workspace, workspace_bytes, stream);
}

void nbl_ik_default_config(nbl_ik_config* c) { nbl_ik_default_config_c8(c); }   // (the same in every instantiation)
size_t nbl_ik_workspace_bytes(const nbl_model* m, const nbl_kin_map* k, int64_t B) {
  return (m && k && k->v == m->v) ? m->v->ik_workspace_bytes(m->impl, k->impl, B) : 0;
}
int32_t nbl_ik_solve(nbl_model* m, const nbl_kin_map* k, int64_t B, const double* target, const double* q_init, const nbl_ik_config* config,
                     double* q_out, double* loss, int32_t* steps, void* workspace, size_t workspace_bytes, void* stream) {
  if (!k) return ownError(NBL_E_BADARG, "null kinematics map");
  if (m && k->v != m->v) return ownError(NBL_E_BADARG, "the kinematics map was made for another model");
  return NBL_FWD(m, ik_solve, k->impl, B, target, q_init, config, q_out, loss, steps, workspace, workspace_bytes, stream);
}

}  // extern "C"
