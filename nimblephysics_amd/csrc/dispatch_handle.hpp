// dispatch_handle.hpp — private to nimble_amd_dispatch.cpp and nimble_amd_tree.hip: the model handle callers of the linked library hold.
#pragma once
#include "../../include/nimble_amd.h"

struct Variant;          // the entry points of one instantiation of the contact stage (nimble_amd_dispatch.cpp)
struct nbl_tree_model;   // the capacity-independent base of that instantiation's handle (tree_model_host.hpp)

struct nbl_model {
  const Variant* v;      // the instantiation that owns `impl`
  void* impl;
  nbl_tree_model* tree;  // points INTO impl: what nbl_set_body_inertia[s] / nbl_set_inertia_params[_on] change there, the dynamics calls see
};

// the text nbl_last_error returns for a refusal that no instantiation made; returns `code`
int ownError(int code, const char* msg);

inline nbl_tree_model* treeOf(const nbl_model* m) { return m->tree; }
