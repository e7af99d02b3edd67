// Host build of the product's world-space kinematics (nimblephysics_amd/csrc/kinematics_dev.hpp) for tests/test_kinematics_host.py.
// Test harness only.  The device body table is restated here from nbl_model_create / expandBallJoints (nimble_amd.hip): ball joints
// and free joints below the root become chains of coincident single-axis bodies, the caller's bodies map to the last body of a chain.
#include <cstring>
#include <vector>

#include "kinematics_dev.hpp"
#include "nimble_amd.h"

using namespace NBL_NS;

namespace {
struct ShimModel {
  std::vector<DevBody> bodies;
  std::vector<int> bodyMap;
  int n = 0;
};
const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};

void push(ShimModel& m, int parent, int jt, int dofOff, const double* Tpj, const double* Tcj, const double* ax, int comp, double pitch) {
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
}  // namespace

extern "C" {
void* shim_kin_model(const nbl_model_desc* d) {
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
  return m;
}
void shim_kin_free(void* h) { delete (ShimModel*)h; }

// entries as nbl_kin_map_create takes them; pos / vel / gstate may be null (gstate: the VJP with grad_pos / grad_vel, overwritten)
int shim_kin_run(void* h, int count, const int* kind, const int* body, const double* T, int64_t B, const double* state, double* pos,
                 double* vel, const double* gpos, const double* gvel, double* gstate) {
  const ShimModel& m = *(const ShimModel*)h;
  std::vector<DevKinEntry> e(count);
  std::vector<int32_t> path;
  int row = 0;
  for (int k = 0; k < count; k++) {
    std::memset(&e[k], 0, sizeof(DevKinEntry));
    e[k].kind = kind[k]; e[k].row = row; row += kinRows(kind[k]);
    for (int c = 0; c < 12; c++) e[k].T[c] = T[12 * k + c];
    std::vector<int32_t> chain;
    for (int i = body[k] < 0 ? -1 : m.bodyMap[body[k]]; i >= 0; i = m.bodies[i].parent) chain.push_back(i);
    e[k].pathBegin = (int32_t)path.size(); e[k].pathLen = (int32_t)chain.size();
    path.insert(path.end(), chain.rbegin(), chain.rend());
  }
  for (int64_t b = 0; b < B; b++) {
    if (pos || vel) kinForwardWorld(m.bodies.data(), e.data(), path.data(), count, m.n, B, b, state, pos, vel);
    if (gstate) kinVjpWorld(m.bodies.data(), e.data(), path.data(), count, m.n, B, b, state, gpos, gvel, gstate, 0);
  }
  return row;
}
}
