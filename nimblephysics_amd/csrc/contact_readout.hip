// contact_readout.hip — what a step's contacts WERE, decoded from its saved record for B worlds (nbl_contact_readout,
// nbl_contact_readout_rows, nbl_contact_body_wrenches): the device side of World::getLastCollisionResult (dart/collision/Contact.hpp:90-147,
// Contact::force as ContactConstraint::applyImpulse fills it, ContactConstraint.cpp:630-684) and of BackpropSnapshot's
// getContactConstraintImpulses / getContactConstraintMappings (BackpropSnapshot.cpp:1601-1705).
//
// ONE WORLD PER LANE, like kinematics.hip: every row of the record's first block is lane-interleaved [row][B] (SavedLayout), so each read
// of a wavefront is one coalesced line, and the outputs are [row][B] too.  Read-only on the record: nothing of the step, its records or
// its results changes.  No atomics, no workspace, no LDS; every sum runs in contact order inside the lane that owns the world, so the
// results are bit-reproducible and do not depend on B or on a world's place in the batch.  The small per-call tables (device body ->
// description body, the bodies of a wrench set) travel by value in the kernel arguments.
//
// Body positions of the wrench kernel: the forward kinematics is RECOMPUTED from the record's q down the ancestor chain of every named
// body (jointRelTransform of kinematics_dev.hpp, the arithmetic of the narrow phase's own chains) instead of read from the record's tree
// block - that block is absent with NBL_SAVE_TREE=0 and comes in two layouts (compact world-major / lane-interleaved), the q rows are
// always there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kinematics_dev.hpp"

namespace NBL_NS {

constexpr int CO_BLOCK = 64;
// rows of a contact slot in the table of nbl_contact_readout (= NBL_CO_* of include/nimble_amd.h)
constexpr int CO_POINT = 0, CO_NORMAL = 3, CO_DEPTH = 6, CO_TYPE = 7, CO_COLLIDER_A = 8, CO_COLLIDER_B = 9, CO_BODY_A = 10, CO_BODY_B = 11;
constexpr int CO_IMPULSE = 12, CO_CLASS = 15, CO_FORCE = 18, CO_FIELDS = 21;
constexpr double CO_CLASS_EMPTY = -1.0;              // the tangent slots of a frictionless contact (no LCP row there)
constexpr int CO_MAP_CLAMPING = -1, CO_MAP_NOT_CLAMPING = -2, CO_MAP_NONE = -4;   // neural::ConstraintMapping (ConstrainedGroupGradientMatrices.hpp:33-39)
constexpr int CO_MAX_BODIES = 64;                    // the contact path's cap on device bodies (nbl_model_create), and on the bodies of a wrench set
struct CoBodyTable { int8_t v[CO_MAX_BODIES]; };

DEV double coRec(const double* __restrict__ saved, int row, int64_t B, int64_t b) { return saved[(int64_t)row * B + b]; }

// The constraints of world b in the record: nAll slots in use, of which the first nTrue are collider contacts; the joint-limit rows
// (CT_LIMIT) and the joint-friction rows (CT_JFRIC) are appended after them (contactDetectBody, contactRowsGen).  Everything read from the
// record is clamped before it is used as an index: a record that no step has written yet decodes to garbage, never to a wild address.
struct CoCounts { int nAll, nTrue, nLim, nFric; };
DEV CoCounts coCounts(const DevContactModel* __restrict__ cm, const double* __restrict__ saved, const SavedLayout& lay, int64_t B, int64_t b) {
  CoCounts k;
  const int cap = cm->maxContacts < MAX_CONTACTS ? cm->maxContacts : MAX_CONTACTS;
  const double ncD = coRec(saved, lay.nc, B, b);                   // (+ 0.5: contacts were dropped, NBL_ST_CONTACT_OVERFLOW)
  k.nAll = (ncD >= 0.0 && ncD < (double)cap + 1.0) ? (int)ncD : 0;
  if (k.nAll > cap) k.nAll = cap;
  k.nTrue = k.nLim = k.nFric = 0;
  for (int c = 0; c < k.nAll; c++) {
    const int type = (int)coRec(saved, lay.contacts + c * CR_SIZE + CR_TYPE, B, b);
    if (type == CT_LIMIT) k.nLim++;
    else if (type == CT_JFRIC) k.nFric++;
    else if (k.nLim + k.nFric == 0) k.nTrue++;
  }
  return k;
}

// One collider contact of the record: geometry, the two colliders and their device bodies, the three impulses and row classes (the
// tangent slots of a frictionless contact, mu = min(mu_A, mu_B) <= 1e-3, are EMPTY: impulse 0, class CO_CLASS_EMPTY), and the force
// (n l0 + t1 l1 + t2 l2) / dt with the tangent basis of the row kernels (tangentBasis, contact_kernels.hip).
struct CoContact { V3 p, n, f; double depth, type, lam[3], cls[3]; int bxA, bxB, bodyA, bodyB; };
DEV CoContact coContact(const DevContactModel* __restrict__ cm, const double* __restrict__ saved, const SavedLayout& lay, double dt, int slot,
                        int64_t B, int64_t b) {
  CoContact c;
  const int r0 = lay.contacts + slot * CR_SIZE;
  c.p = mk3(coRec(saved, r0 + CR_POINT, B, b), coRec(saved, r0 + CR_POINT + 1, B, b), coRec(saved, r0 + CR_POINT + 2, B, b));
  c.n = mk3(coRec(saved, r0 + CR_NORMAL, B, b), coRec(saved, r0 + CR_NORMAL + 1, B, b), coRec(saved, r0 + CR_NORMAL + 2, B, b));
  c.depth = coRec(saved, r0 + CR_DEPTH, B, b);
  c.type = coRec(saved, r0 + CR_TYPE, B, b);
  const int nBx = cm->nBoxes > 0 ? cm->nBoxes : 1;
  const int a = (int)coRec(saved, r0 + CR_BOXA, B, b), bb = (int)coRec(saved, r0 + CR_BOXB, B, b);
  c.bxA = (unsigned)a < (unsigned)nBx ? a : 0;
  c.bxB = (unsigned)bb < (unsigned)nBx ? bb : 0;
  c.bodyA = cm->boxes[c.bxA].body; c.bodyB = cm->boxes[c.bxB].body;
  const bool fric = fmin(cm->boxes[c.bxA].mu, cm->boxes[c.bxB].mu) > 1e-3;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const bool live = k == 0 || fric;
    c.lam[k] = live ? coRec(saved, lay.x + 3 * slot + k, B, b) : 0.0;
    c.cls[k] = live ? coRec(saved, lay.cls + 3 * slot + k, B, b) : CO_CLASS_EMPTY;
  }
  V3 t1, t2;
  tangentBasis(c.n, t1, t2);
  auto overDt = [&](V3 v) -> V3 { return mk3(v.x / dt, v.y / dt, v.z / dt); };   // (term by term, as applyImpulse accumulates it)
  c.f = overDt(c.lam[0] * c.n);
  if (fric) c.f = c.f + overDt(c.lam[1] * t1) + overDt(c.lam[2] * t2);
  return c;
}

__global__ __launch_bounds__(CO_BLOCK) void k_contact_readout(const DevContactModel* __restrict__ cm, CoBodyTable userOf, SavedLayout lay, int slots,
                                                              double dt, int64_t B, const double* __restrict__ saved, int32_t* __restrict__ count,
                                                              int32_t* __restrict__ nLimitRows, int32_t* __restrict__ nFrictionRows,
                                                              double* __restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x * CO_BLOCK + threadIdx.x;
  if (b >= B) return;
  const CoCounts k = coCounts(cm, saved, lay, B, b);
  if (count) count[b] = k.nTrue;
  if (nLimitRows) nLimitRows[b] = k.nLim;
  if (nFrictionRows) nFrictionRows[b] = k.nFric;
  if (!out) return;
  auto userBody = [&](int body) -> double { return body < 0 ? -1.0 : (double)userOf.v[body & (CO_MAX_BODIES - 1)]; };
  for (int slot = 0; slot < slots; slot++) {
    double f[CO_FIELDS];
#pragma unroll
    for (int e = 0; e < CO_FIELDS; e++) f[e] = 0.0;                 // slots past the world's contacts: zeros
    if (slot < k.nTrue) {
      const CoContact c = coContact(cm, saved, lay, dt, slot, B, b);
      f[CO_POINT] = c.p.x; f[CO_POINT + 1] = c.p.y; f[CO_POINT + 2] = c.p.z;
      f[CO_NORMAL] = c.n.x; f[CO_NORMAL + 1] = c.n.y; f[CO_NORMAL + 2] = c.n.z;
      f[CO_DEPTH] = c.depth; f[CO_TYPE] = c.type;
      f[CO_COLLIDER_A] = (double)c.bxA; f[CO_COLLIDER_B] = (double)c.bxB;
      f[CO_BODY_A] = userBody(c.bodyA); f[CO_BODY_B] = userBody(c.bodyB);
#pragma unroll
      for (int e = 0; e < 3; e++) { f[CO_IMPULSE + e] = c.lam[e]; f[CO_CLASS + e] = c.cls[e]; }
      f[CO_FORCE] = c.f.x; f[CO_FORCE + 1] = c.f.y; f[CO_FORCE + 2] = c.f.z;
    }
#pragma unroll
    for (int e = 0; e < CO_FIELDS; e++) out[((int64_t)e * slots + slot) * B + b] = f[e];
  }
}

// The live LCP rows of world b in the reference's order (constraint by constraint: a contact with friction has three rows, a frictionless
// one, a joint-limit row and a joint-friction row one), compacted: impulse [3 slots][B] in the reference's sign (an upper-limit row is
// carried negated in the record: model_dev.hpp) and mapping [3 slots][B]: CLAMPING -1, NOT_CLAMPING -2, or - a friction row on its bound -
// the compacted index of its contact's normal row; rows past nRows[b]: impulse 0, mapping CO_MAP_NONE.
__global__ __launch_bounds__(CO_BLOCK) void k_contact_readout_rows(const DevContactModel* __restrict__ cm, SavedLayout lay, int slots, int64_t B,
                                                                   const double* __restrict__ saved, int32_t* __restrict__ nRows,
                                                                   double* __restrict__ impulse, int32_t* __restrict__ mapping) {
  const int64_t b = (int64_t)blockIdx.x * CO_BLOCK + threadIdx.x;
  if (b >= B) return;
  const CoCounts k = coCounts(cm, saved, lay, B, b);
  const int cap = 3 * slots, nBx = cm->nBoxes > 0 ? cm->nBoxes : 1;
  int r = 0;
  for (int c = 0; c < k.nAll && c < slots; c++) {
    const int r0 = lay.contacts + c * CR_SIZE;
    const int type = (int)coRec(saved, r0 + CR_TYPE, B, b);
    const bool pseudo = type == CT_LIMIT || type == CT_JFRIC;
    const int a = (int)coRec(saved, r0 + CR_BOXA, B, b), bb = (int)coRec(saved, r0 + CR_BOXB, B, b);
    const bool fric = !pseudo && fmin(cm->boxes[(unsigned)a < (unsigned)nBx ? a : 0].mu, cm->boxes[(unsigned)bb < (unsigned)nBx ? bb : 0].mu) > 1e-3;
    const double sigma = type == CT_LIMIT ? coRec(saved, r0 + CR_EA_FIXED + 1, B, b) : 1.0;
    const int normalRow = r, dim = fric ? 3 : 1;
    for (int kk = 0; kk < dim && r < cap; kk++, r++) {
      const double X = coRec(saved, lay.x + 3 * c + kk, B, b), cv = coRec(saved, lay.cls + 3 * c + kk, B, b);
      // (3: a joint-limit row that was clamping - the record sets it apart because the backward pass gives it a zero constraint-force
      //  column; as a row of the LCP it is clamping.  A joint-friction row on its fixed bound has no normal row to point to: not clamping)
      const int map = (cv == 1.0 || cv == 3.0) ? CO_MAP_CLAMPING : ((!pseudo && kk > 0 && (cv == 2.0 || cv == -2.0)) ? normalRow : CO_MAP_NOT_CLAMPING);
      if (impulse) impulse[(int64_t)r * B + b] = kk == 0 ? sigma * X : X;
      if (mapping) mapping[(int64_t)r * B + b] = map;
    }
  }
  if (nRows) nRows[b] = r;
  for (; r < cap; r++) {
    if (impulse) impulse[(int64_t)r * B + b] = 0.0;
    if (mapping) mapping[(int64_t)r * B + b] = CO_MAP_NONE;
  }
}

// (a model without a contact stage has no rows: its mapping table is all CO_MAP_NONE)
__global__ __launch_bounds__(CO_BLOCK) void k_contact_fill_i32(int32_t* __restrict__ dst, int64_t count, int32_t value) {
  const int64_t i = (int64_t)blockIdx.x * CO_BLOCK + threadIdx.x;
  if (i < count) dst[i] = value;
}

// wrench [6 E][B]: rows 6 e .. 6 e + 5 = [torque(3); force(3)], world coordinates, at the origin of the frame of device body ent.v[e]: the
// sum over the world's collider contacts of + force on the body of collider A and - force on the body of collider B
// (ContactConstraint::applyImpulse: + lambda mSpatialNormalA on A, mSpatialNormalB = - that wrench on B), with the moment
// (point - p_body) x force.  Joint-limit and joint-friction rows are generalized forces, not body wrenches: they contribute nothing.
__global__ __launch_bounds__(CO_BLOCK) void k_contact_body_wrenches(const DevBody* __restrict__ bodies, const DevContactModel* __restrict__ cm,
                                                                    CoBodyTable ent, int E, SavedLayout lay, double dt, int64_t B,
                                                                    const double* __restrict__ saved, double* __restrict__ wrench) {
  const int64_t b = (int64_t)blockIdx.x * CO_BLOCK + threadIdx.x;
  if (b >= B) return;
  const CoCounts k = coCounts(cm, saved, lay, B, b);
  const double* q = saved + (int64_t)lay.q * B;
  for (int e = 0; e < E; e++) {
    const int body = ent.v[e & (CO_MAX_BODIES - 1)];
    V3 tq = mk3(0, 0, 0), fr = mk3(0, 0, 0);
    bool touched = false;
    for (int c = 0; c < k.nTrue; c++) {
      const int r0 = lay.contacts + c * CR_SIZE;
      const int nBx = cm->nBoxes > 0 ? cm->nBoxes : 1;
      const int a = (int)coRec(saved, r0 + CR_BOXA, B, b), bb = (int)coRec(saved, r0 + CR_BOXB, B, b);
      const int bA = cm->boxes[(unsigned)a < (unsigned)nBx ? a : 0].body, bB = cm->boxes[(unsigned)bb < (unsigned)nBx ? bb : 0].body;
      touched = touched || bA == body || bB == body;
    }
    if (touched) {
      // BodyNode::mWorldTransform at the record's q: the product of the joint transforms down the ancestor chain, root first
      uint64_t chain = cm->ancestors[body];
      T12 TW = jointRelTransform(bodies[__builtin_ctzll(chain)], q, B, b);
      chain &= chain - 1;
      while (chain) {
        TW = mulT(TW, jointRelTransform(bodies[__builtin_ctzll(chain)], q, B, b));
        chain &= chain - 1;
      }
      for (int c = 0; c < k.nTrue; c++) {
        const CoContact ct = coContact(cm, saved, lay, dt, c, B, b);
        const double sgn = (ct.bodyA == body ? 1.0 : 0.0) - (ct.bodyB == body ? 1.0 : 0.0);
        if (sgn == 0.0) continue;
        const V3 f = sgn * ct.f;
        tq = tq + cross(ct.p - TW.p, f);
        fr = fr + f;
      }
    }
    const int64_t r = 6 * (int64_t)e;
    wrench[r * B + b] = tq.x; wrench[(r + 1) * B + b] = tq.y; wrench[(r + 2) * B + b] = tq.z;
    wrench[(r + 3) * B + b] = fr.x; wrench[(r + 4) * B + b] = fr.y; wrench[(r + 5) * B + b] = fr.z;
  }
}

}  // namespace NBL_NS
