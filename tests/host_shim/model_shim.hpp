// Host restatement of the device body table for the host_shim builds (test harness only): what nbl_model_create / expandBallJoints
// (nimble_amd.hip) make of a model description - ball joints and free joints below the root become chains of coincident single-axis
// bodies, the caller's bodies map to the last body of a chain -, the per-coordinate limits, and the entries of nbl_kin_map_create.
// One copy for the shims that include it (ik_shim.cpp); kin_shim.cpp and dyn_shim.cpp predate it and carry their own.
#pragma once
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "kinematics_dev.hpp"
#include "nimble_amd.h"

namespace shim_model {
using namespace NBL_NS;

struct ShimModel {
  std::vector<DevBody> bodies;
  std::vector<DevDof> dofs;
  std::vector<int> bodyMap;
  int n = 0;
};
struct ShimMap {
  std::vector<DevKinEntry> e;
  std::vector<int32_t> path;
  int P = 0;
};
static const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};

inline void push(ShimModel& m, int parent, int jt, int dofOff, const double* Tpj, const double* Tcj, const double* ax, int comp, double pitch) {
  DevBody b;
  std::memset(&b, 0, sizeof(b));
  b.parent = parent; b.jtype = jt; b.dofOff = dofOff; b.ndof = jt == JT_FREE ? 6 : 1; b.ballComp = comp; b.freeIdx = -1;
  for (int k = 0; k < 12; k++) { b.Tpj[k] = Tpj[k]; b.Tcj[k] = Tcj[k]; }
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) b.TcjInv[3 * r + c] = b.Tcj[3 * c + r];
  for (int r = 0; r < 3; r++) b.TcjInv[9 + r] = -(b.Tcj[r] * b.Tcj[9] + b.Tcj[3 + r] * b.Tcj[10] + b.Tcj[6 + r] * b.Tcj[11]);
  for (int k = 0; k < 3; k++) b.axis[k] = ax[k];
  const double* R = b.Tcj;
  const double* p = b.Tcj + 9;
  double Ra[3];
  for (int r = 0; r < 3; r++) Ra[r] = R[3 * r] * ax[0] + R[3 * r + 1] * ax[1] + R[3 * r + 2] * ax[2];
  const bool rot = jt == JT_REVOLUTE || jt == JT_BALL || jt == JT_SCREW || (jt == JT_FREEC && comp < 3);
  const bool lin = jt == JT_PRISMATIC || (jt == JT_FREEC && comp >= 3);
  if (rot) {
    b.S[0] = Ra[0]; b.S[1] = Ra[1]; b.S[2] = Ra[2];
    b.S[3] = p[1] * Ra[2] - p[2] * Ra[1]; b.S[4] = p[2] * Ra[0] - p[0] * Ra[2]; b.S[5] = p[0] * Ra[1] - p[1] * Ra[0];
  } else if (lin) {
    b.S[3] = Ra[0]; b.S[4] = Ra[1]; b.S[5] = Ra[2];
  }
  if (jt == JT_SCREW) {
    b.screwRate = pitch / (2.0 * M_PI);
    for (int k = 0; k < 3; k++) b.S[3 + k] += b.screwRate * Ra[k];
  }
  m.bodies.push_back(b);
}

inline ShimMap makeMap(const ShimModel& m, int count, const int* kind, const int* body, const double* T) {
  ShimMap k;
  k.e.resize(count);
  int row = 0;
  for (int i = 0; i < count; i++) {
    std::memset(&k.e[i], 0, sizeof(DevKinEntry));
    k.e[i].kind = kind[i]; k.e[i].row = row; row += kinRows(kind[i]);
    for (int c = 0; c < 12; c++) k.e[i].T[c] = T ? T[12 * i + c] : I12[c];
    std::vector<int32_t> chain;
    for (int j = body[i] < 0 ? -1 : m.bodyMap[body[i]]; j >= 0; j = m.bodies[j].parent) chain.push_back(j);
    k.e[i].pathBegin = (int32_t)k.path.size(); k.e[i].pathLen = (int32_t)chain.size();
    k.path.insert(k.path.end(), chain.rbegin(), chain.rend());
  }
  if (k.path.empty()) k.path.push_back(0);
  k.P = row;
  return k;
}

inline ShimModel* makeModel(const nbl_model_desc* d) {
  ShimModel* m = new ShimModel();
  m->n = d->n_dofs;
  m->bodyMap.assign(d->n_bodies, -1);
  for (int i = 0; i < d->n_bodies; i++) {
    const int par = d->parent[i] < 0 ? -1 : m->bodyMap[d->parent[i]];
    const int jt = d->joint_type[i];
    const double pitch = d->pitch ? d->pitch[i] : 0.1;
    if ((jt == NBL_JOINT_FREE && d->parent[i] >= 0) || jt == NBL_JOINT_BALL) {
      const int nc = jt == NBL_JOINT_BALL ? 3 : 6;
      for (int k = 0; k < nc; k++) {
        const double ax[3] = {k % 3 == 0 ? 1.0 : 0.0, k % 3 == 1 ? 1.0 : 0.0, k % 3 == 2 ? 1.0 : 0.0};
        push(*m, k == 0 ? par : (int)m->bodies.size() - 1, jt == NBL_JOINT_BALL ? JT_BALL : JT_FREEC, d->dof_offset[i] + k,
             k == 0 ? d->T_pj + 12 * i : I12, k == nc - 1 ? d->T_cj + 12 * i : I12, ax, k, pitch);
      }
    } else {
      push(*m, par, jt, d->dof_offset[i], d->T_pj + 12 * i, d->T_cj + 12 * i, d->axis + 3 * i, 0, pitch);
    }
    m->bodyMap[i] = (int)m->bodies.size() - 1;
  }
  m->dofs.resize(d->n_dofs);
  const double inf = std::numeric_limits<double>::infinity();
  for (int j = 0; j < d->n_dofs; j++) {
    DevDof& f = m->dofs[j];
    std::memset(&f, 0, sizeof(f));
    f.posLo = d->pos_lo ? d->pos_lo[j] : -inf;
    f.posHi = d->pos_hi ? d->pos_hi[j] : inf;
    f.actionIndex = -1;
  }
  return m;
}

}  // namespace shim_model
