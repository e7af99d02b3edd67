// Host build of the product's joint-space dynamics (nimblephysics_amd/csrc/dynamics_dev.hpp) for tests/test_dynamics_host.py.
// Test harness only.  The device body table is restated here from nbl_model_create / expandBallJoints (nimble_amd.hip): ball joints
// and free joints below the root become chains of coincident single-axis bodies whose last body carries the mass.
#include <cmath>
#include <cstring>
#include <vector>

#include "dynamics_dev.hpp"
#include "nimble_amd.h"

using namespace NBL_NS;

namespace {
struct ShimModel {
  std::vector<DevBody> bodies;
  std::vector<DevDof> dofs;
  std::vector<int> bodyMap;
  int n = 0;
  double gravity[3], dt;
};
const double I12[12] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};

// spatial inertia (Inertia.cpp:1368-1383), packed symmetric (upper triangle, row by row)
void packSpatialInertia(double m, const double* c, const double* I, double* out21) {
  double Ic[3][3] = {{I[0], I[3], I[4]}, {I[3], I[1], I[5]}, {I[4], I[5], I[2]}};
  double Cx[3][3] = {{0, -c[2], c[1]}, {c[2], 0, -c[0]}, {-c[1], c[0], 0}};
  double G[6][6];
  std::memset(G, 0, sizeof(G));
  for (int r = 0; r < 3; r++)
    for (int cc = 0; cc < 3; cc++) {
      double cct = 0;
      for (int k = 0; k < 3; k++) cct += Cx[r][k] * Cx[cc][k];
      G[r][cc] = Ic[r][cc] + m * cct;
      G[r][3 + cc] = m * Cx[r][cc];
      G[3 + r][cc] = m * Cx[cc][r];
    }
  G[3][3] = G[4][4] = G[5][5] = m;
  int idx = 0;
  for (int r = 0; r < 6; r++)
    for (int cc = r; cc < 6; cc++) out21[idx++] = G[r][cc];
}

void push(ShimModel& m, int parent, int jt, int dofOff, const double* Tpj, const double* Tcj, const double* ax, int comp, double pitch,
          double mass, const double* com, const double* inertia) {
  static const double z6[6] = {0, 0, 0, 0, 0, 0};
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
  packSpatialInertia(mass, com ? com : z6, inertia ? inertia : z6, b.G);
  m.bodies.push_back(b);
}
}  // namespace

extern "C" {
void* shim_dyn_model(const nbl_model_desc* d) {
  ShimModel* m = new ShimModel();
  m->n = d->n_dofs;
  m->dt = d->dt;
  for (int k = 0; k < 3; k++) m->gravity[k] = d->gravity[k];
  m->bodyMap.assign(d->n_bodies, -1);
  for (int i = 0; i < d->n_bodies; i++) {
    const int par = d->parent[i] < 0 ? -1 : m->bodyMap[d->parent[i]];
    const int jt = d->joint_type[i];
    const double pitch = d->pitch ? d->pitch[i] : 0.1;
    if ((jt == NBL_JOINT_FREE && d->parent[i] >= 0) || jt == NBL_JOINT_BALL) {
      const int nc = jt == NBL_JOINT_BALL ? 3 : 6;
      for (int k = 0; k < nc; k++) {
        const double ax[3] = {k % 3 == 0 ? 1.0 : 0.0, k % 3 == 1 ? 1.0 : 0.0, k % 3 == 2 ? 1.0 : 0.0};
        const bool last = k == nc - 1;
        push(*m, k == 0 ? par : (int)m->bodies.size() - 1, jt == NBL_JOINT_BALL ? JT_BALL : JT_FREEC, d->dof_offset[i] + k,
             k == 0 ? d->T_pj + 12 * i : I12, last ? d->T_cj + 12 * i : I12, ax, k, pitch, last ? d->mass[i] : 0.0,
             last ? d->com + 3 * i : nullptr, last ? d->inertia + 6 * i : nullptr);
      }
    } else {
      push(*m, par, jt, d->dof_offset[i], d->T_pj + 12 * i, d->T_cj + 12 * i, d->axis + 3 * i, 0, pitch, d->mass[i], d->com + 3 * i,
           d->inertia + 6 * i);
    }
    m->bodyMap[i] = (int)m->bodies.size() - 1;
  }
  m->dofs.resize(d->n_dofs);
  for (int j = 0; j < d->n_dofs; j++) {
    DevDof& f = m->dofs[j];
    std::memset(&f, 0, sizeof(f));
    f.damping = d->damping ? d->damping[j] : 0.0;
    f.spring = d->spring ? d->spring[j] : 0.0;
    f.rest = d->rest ? d->rest[j] : 0.0;
    f.actionIndex = -1;
  }
  return m;
}
void shim_dyn_free(void* h) { delete (ShimModel*)h; }
int shim_dyn_slots(void) { return DYN_SLOTS; }
int shim_dyn_bodies(void* h) { return (int)((const ShimModel*)h)->bodies.size(); }

// state [2n][B], accel [n][B] or null; tau [n][B] (null: skipped).  With gtau: the reverse pass into gstate [2n][B] / gaccel [n][B]
// (either may be null).  M [n * n][B] (null: skipped).
void shim_dyn_run(void* h, int64_t B, const double* state, const double* accel, int flags, double* tau, const double* gtau, double* gstate,
                  double* gaccel, int accumulate, double* M) {
  const ShimModel& m = *(const ShimModel*)h;
  const int nb = (int)m.bodies.size();
  std::vector<double> ws((size_t)nb * DYN_SLOTS * B, NAN);     // NaN: a slot read before it is written shows
  if (M) std::memset(M, 0, sizeof(double) * (size_t)m.n * m.n * B);
  for (int64_t b = 0; b < B; b++) {
    if (tau) idForwardWorld(m.bodies.data(), m.dofs.data(), nb, m.n, m.gravity, m.dt, flags, B, b, state, accel, tau, ws.data());
    if (gtau) idVjpWorld(m.bodies.data(), m.dofs.data(), nb, m.n, m.gravity, m.dt, flags, B, b, state, accel, gtau, gstate, gaccel, accumulate, ws.data());
    if (M) massMatrixWorld(m.bodies.data(), nb, m.n, B, b, state, M, ws.data());
  }
}
}
