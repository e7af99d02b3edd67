// kinematics_dev.hpp — per-body joint transforms, twists and relative Jacobians of the device model, and the world-space
// kinematics of body frames built on them (csrc/kinematics.hip: IKMapping / map_to_pos / map_to_vel, dart/neural/IKMapping.cpp).
//
// Plain C++ on the spatial algebra of spatial_dev.hpp (no intrinsics, no LDS, no cross-lane operations), so that the tests compile this
// header for the host with g++ (tests/host_shim/kin_shim.cpp).  The joint helpers (cT .. jointRelTransform, applyHt) are shared with the tree kernels of
// kernels.hip, which include this header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "model_dev.hpp"
#include "spatial_dev.hpp"

namespace NBL_NS {

DEV T12 cT(const double* t) {  // wave-uniform constant -> scalar loads
  T12 T;
#pragma unroll
  for (int k = 0; k < 9; k++) T.R.m[k] = t[k];
  T.p = mk3(t[9], t[10], t[11]);
  return T;
}
DEV S6 cS6(const double* g) {
  S6 A;
#pragma unroll
  for (int k = 0; k < 21; k++) A.a[k] = g[k];
  return A;
}
DEV V6 cV6(const double* s) { return mk6(mk3(s[0], s[1], s[2]), mk3(s[3], s[4], s[5])); }

// joint twist S*dq in the child frame
DEV V6 jointTwist(const DevBody& bd, const double* __restrict__ v, int64_t B, int64_t b) {
  if (bd.jtype == JT_FREE) {
    V6 x = mk6(mk3(v[(bd.dofOff + 0) * B + b], v[(bd.dofOff + 1) * B + b], v[(bd.dofOff + 2) * B + b]),
               mk3(v[(bd.dofOff + 3) * B + b], v[(bd.dofOff + 4) * B + b], v[(bd.dofOff + 5) * B + b]));
    return AdT(cT(bd.Tcj), x);  // S = Ad(T_cj), FreeJoint.cpp:1049-1056
  }
  return v[bd.dofOff * B + b] * cV6(bd.S);
}

// T_parent->child of one body at the positions q ([n][B]): T_pj Q(q) T_cj^-1 with Q of the joint type (RevoluteJoint.cpp:203-211,
// PrismaticJoint, ScrewJoint.cpp:217-232, FreeJoint.cpp:74-81, BallJoint.cpp:91-95; ball joints and free joints below the root are
// chains of coincident single-axis bodies whose first one carries the exponential map).  The same expressions as the tree kernels'
// first sweep; used by the narrow phase when it runs next to the forward tree kernel instead of after it.
DEV T12 jointRelTransform(const DevBody& bd, const double* __restrict__ q, int64_t B, int64_t b) {
  T12 Q;
  if (bd.jtype == JT_REVOLUTE) {
    const double qi = q[bd.dofOff * B + b];
    Q.R = expAngular(mk3(bd.axis[0] * qi, bd.axis[1] * qi, bd.axis[2] * qi));
    Q.p = mk3(0, 0, 0);
  } else if (bd.jtype == JT_PRISMATIC) {
    const double qi = q[bd.dofOff * B + b];
    Q.R = eye3();
    Q.p = mk3(bd.axis[0] * qi, bd.axis[1] * qi, bd.axis[2] * qi);
  } else if (bd.jtype == JT_SCREW) {
    const double qi = q[bd.dofOff * B + b], hq = bd.screwRate * qi;
    Q.R = expAngular(mk3(bd.axis[0] * qi, bd.axis[1] * qi, bd.axis[2] * qi));
    Q.p = mk3(bd.axis[0] * hq, bd.axis[1] * hq, bd.axis[2] * hq);
  } else if (bd.jtype == JT_FREEC) {
    const int o = bd.dofOff;
    Q.R = bd.ballComp == 0 ? expMapRot(mk3(q[(o + 0) * B + b], q[(o + 1) * B + b], q[(o + 2) * B + b])) : eye3();
    Q.p = bd.ballComp == 0 ? mk3(q[(o + 3) * B + b], q[(o + 4) * B + b], q[(o + 5) * B + b]) : mk3(0, 0, 0);
  } else if (bd.jtype == JT_BALL) {
    Q.R = bd.ballComp == 0 ? expMapRot(mk3(q[(bd.dofOff + 0) * B + b], q[(bd.dofOff + 1) * B + b], q[(bd.dofOff + 2) * B + b])) : eye3();
    Q.p = mk3(0, 0, 0);
  } else {
    Q.R = expMapRot(mk3(q[(bd.dofOff + 0) * B + b], q[(bd.dofOff + 1) * B + b], q[(bd.dofOff + 2) * B + b]));
    Q.p = mk3(q[(bd.dofOff + 3) * B + b], q[(bd.dofOff + 4) * B + b], q[(bd.dofOff + 5) * B + b]);
  }
  return mulT(mulT(cT(bd.Tpj), Q), cT(bd.TcjInv));
}

// Position-space Jacobian transpose of joint i applied to a body-frame adjoint xi:  H_i^T xi
// (H = S for 1-DOF joints; free joint: Ad(T_cj) blkdiag(expMapJac(r)^T, R^T), FreeJoint.cpp:790-823)
DEV void applyHt(const DevBody& bd, const double* __restrict__ q, int64_t B, int64_t b, V6 xi, double* out) {
  if (bd.jtype == JT_BALL) {
    // ball joint (BallJoint.cpp:282-289): H = [expMapJac(q)^T; 0] in the frame of the x body of the triple; xi = THAT body's adjoint
    const int d0 = bd.dofOff - bd.ballComp;
    const V3 y = mul(expMapJac(mk3(q[(int64_t)(d0 + 0) * B + b], q[(int64_t)(d0 + 1) * B + b], q[(int64_t)(d0 + 2) * B + b])), xi.w);
    out[0] = bd.ballComp == 0 ? y.x : (bd.ballComp == 1 ? y.y : y.z);
    return;
  }
  if (bd.jtype == JT_FREEC) {
    // free joint below the root (FreeJoint.cpp:790-823): H = blkdiag(expMapJac(r)^T, R^T) in the frame of the first of its six bodies
    const int d0 = bd.dofOff - bd.ballComp, cmp = bd.ballComp;
    const V3 r = mk3(q[(int64_t)(d0 + 0) * B + b], q[(int64_t)(d0 + 1) * B + b], q[(int64_t)(d0 + 2) * B + b]);
    out[0] = cmp < 3 ? pick3(mul(expMapJac(r), xi.w), cmp) : pick3(mul(expMapRot(r), xi.v), cmp - 3);
    return;
  }
  if (bd.jtype != JT_FREE) { out[0] = dot(cV6(bd.S), xi); return; }
  const int o = bd.dofOff;
  V6 y = dAdT(cT(bd.Tcj), xi);
  V3 r = mk3(q[(o + 0) * B + b], q[(o + 1) * B + b], q[(o + 2) * B + b]);
  V3 qbr = mul(expMapJac(r), y.w), qbp = mul(expMapRot(r), y.v);
  out[0] = qbr.x; out[1] = qbr.y; out[2] = qbr.z; out[3] = qbp.x; out[4] = qbp.y; out[5] = qbp.z;
}

// ---- world-space kinematics of body frames (IKMapping.cpp:146-232, 371-473) ----------------------------------------------------
// An ENTRY is a frame fixed in one device body: F = W_body T_offset.  Its rows (in the order the entries were added):
//   KIN_SPATIAL  logMap(R_F), p_F  |  [w; v]          KIN_LINEAR  p_F  |  v          KIN_ANGULAR  logMap(R_F)  |  w
// with w the angular velocity and v the velocity of the frame's origin, both in world coordinates (getSpatialVelocity(World, World),
// Frame.cpp:163-178).  The bodies an entry depends on are listed root -> body at registration (path[pathBegin .. pathBegin + pathLen));
// pathLen = 0: a frame fixed in the world (a constant).
constexpr int KIN_SPATIAL = 0, KIN_LINEAR = 1, KIN_ANGULAR = 2;   // = NBL_KIN_*
constexpr int KIN_MAX_ENTRIES = 64;                               // P <= 6 * 64 = 384 rows
struct DevKinEntry {
  int32_t kind, row, pathBegin, pathLen;   // row: first of the entry's rows in the mapped vector
  double T[12];                            // the entry frame in the body frame (R row-major, p)
};
__host__ __device__ constexpr int kinRows(int kind) { return kind == KIN_SPATIAL ? 6 : 3; }

// World transform W of the entry's body and, with VEL, its body-frame twist V: the first sweep of the tree kernels restricted to one
// ancestor chain (T = T_pj Q(q) T_cj^-1, W = W_parent T, V = S dq + AdInvT(T, V_parent)).
template <bool VEL>
DEV void kinWalk(const DevBody* __restrict__ bodies, const int32_t* __restrict__ path, const DevKinEntry& e, const double* __restrict__ q,
                 const double* __restrict__ v, int64_t B, int64_t b, T12& W, V6& V) {
  W.R = eye3(); W.p = mk3(0, 0, 0); V = zero6();
  for (int j = 0; j < e.pathLen; j++) {
    const DevBody& bd = bodies[path[e.pathBegin + j]];
    const T12 T = jointRelTransform(bd, q, B, b);
    if (j == 0) {
      W = T;
      if (VEL) V = jointTwist(bd, v, B, b);
    } else {
      W = mulT(W, T);
      if (VEL) V = jointTwist(bd, v, B, b) + AdInvT(T, V);
    }
  }
}

// Forward: pos [P][B] and / or vel [P][B] (either may be null) of world b.  state = [q; v], [2n][B].
DEV void kinForwardWorld(const DevBody* __restrict__ bodies, const DevKinEntry* __restrict__ entries, const int32_t* __restrict__ path,
                         int count, int n, int64_t B, int64_t b, const double* __restrict__ state, double* __restrict__ pos,
                         double* __restrict__ vel) {
  const double* q = state;
  const double* v = state + (int64_t)n * B;
  for (int k = 0; k < count; k++) {
    const DevKinEntry& e = entries[k];
    T12 W;
    V6 V;
    if (vel) kinWalk<true>(bodies, path, e, q, v, B, b, W, V);
    else kinWalk<false>(bodies, path, e, q, v, B, b, W, V);
    const T12 O = cT(e.T);
    const T12 F = mulT(W, O);
    const int64_t r = e.row;
    if (pos) {
      if (e.kind != KIN_LINEAR) {
        const V3 lr = logMap(F.R);
        pos[r * B + b] = lr.x; pos[(r + 1) * B + b] = lr.y; pos[(r + 2) * B + b] = lr.z;
      }
      if (e.kind != KIN_ANGULAR) {
        const int64_t rl = e.kind == KIN_SPATIAL ? r + 3 : r;
        pos[rl * B + b] = F.p.x; pos[(rl + 1) * B + b] = F.p.y; pos[(rl + 2) * B + b] = F.p.z;
      }
    }
    if (vel) {
      const V6 Vf = AdInvT(O, V);                        // body-frame twist of the entry frame
      if (e.kind != KIN_LINEAR) {
        const V3 w = mul(F.R, Vf.w);
        vel[r * B + b] = w.x; vel[(r + 1) * B + b] = w.y; vel[(r + 2) * B + b] = w.z;
      }
      if (e.kind != KIN_ANGULAR) {
        const int64_t rl = e.kind == KIN_SPATIAL ? r + 3 : r;
        const V3 u = mul(F.R, Vf.v);
        vel[rl * B + b] = u.x; vel[(rl + 1) * B + b] = u.y; vel[(rl + 2) * B + b] = u.z;
      }
    }
  }
}

// Vector-Jacobian product of world b: grad_state [2n][B] (= or +=) Jpos^T grad_pos in the position block and Jvel^T grad_vel in the
// velocity block (either cotangent may be null: that block gets nothing).  Jpos is the exact derivative of the rows above
// (getWorldPositionJacobian, Skeleton.cpp:11010-11060: the joints' position screws, the angular rows through dLogMap), Jvel the world
// Jacobian (getWorldJacobian).  Every entry turns its cotangent into a wrench on its frame (body coordinates), which is carried down its
// ancestor chain (xi_parent = AdInvT(T)^T xi) and dotted with every joint's relative Jacobian on the way: H (applyHt) for positions, S for
// velocities.  A ball joint's (a free joint's below the root) position gradient acts through the first body of its triple (sextuple) and
// is emitted there for all of its coordinates.  No atomics: the lane owns the world, the sums run in entry order, leaf -> root.
DEV void kinVjpWorld(const DevBody* __restrict__ bodies, const DevKinEntry* __restrict__ entries, const int32_t* __restrict__ path,
                     int count, int n, int64_t B, int64_t b, const double* __restrict__ state, const double* __restrict__ gpos,
                     const double* __restrict__ gvel, double* __restrict__ gstate, int accumulate) {
  const double* q = state;
  double* gq = gstate;
  double* gv = gstate + (int64_t)n * B;
  if (!accumulate)
    for (int d = 0; d < 2 * n; d++) gstate[(int64_t)d * B + b] = 0.0;
  for (int k = 0; k < count; k++) {
    const DevKinEntry& e = entries[k];
    if (e.pathLen == 0) continue;                         // a frame fixed in the world
    T12 W;
    V6 V;
    kinWalk<false>(bodies, path, e, q, q, B, b, W, V);
    const T12 O = cT(e.T);
    const T12 F = mulT(W, O);
    const int64_t r = e.row, rl = e.kind == KIN_SPATIAL ? r + 3 : r;
    V6 xiP = zero6(), xiV = zero6();                      // cotangents as wrenches on F, body coordinates
    if (gpos) {
      if (e.kind != KIN_LINEAR) {
        // d logMap(R)[R [dw]] = <Rb, R [dw]> = dw . vee(N - N^T), N = R^T Rb  (Rb: reverse mode of logMap)
        const M3 Rb = logMap_vjp(F.R, mk3(gpos[r * B + b], gpos[(r + 1) * B + b], gpos[(r + 2) * B + b]));
        const M3 N = mulAtB(F.R, Rb);
        xiP.w = mk3(N.m[7] - N.m[5], N.m[2] - N.m[6], N.m[3] - N.m[1]);
      }
      if (e.kind != KIN_ANGULAR) xiP.v = tmul(F.R, mk3(gpos[rl * B + b], gpos[(rl + 1) * B + b], gpos[(rl + 2) * B + b]));
      xiP = dAdInvT(O, xiP);
    }
    if (gvel) {
      if (e.kind != KIN_LINEAR) xiV.w = tmul(F.R, mk3(gvel[r * B + b], gvel[(r + 1) * B + b], gvel[(r + 2) * B + b]));
      if (e.kind != KIN_ANGULAR) xiV.v = tmul(F.R, mk3(gvel[rl * B + b], gvel[(rl + 1) * B + b], gvel[(rl + 2) * B + b]));
      xiV = dAdInvT(O, xiV);
    }
    for (int j = e.pathLen - 1; j >= 0; j--) {
      const int i = path[e.pathBegin + j];
      const DevBody& bd = bodies[i];
      const int64_t o = bd.dofOff;
      if (gpos) {
        double h[6];
        if (bd.jtype == JT_FREE) {
          applyHt(bd, q, B, b, xiP, h);
          gq[o * B + b] += h[0]; gq[(o + 1) * B + b] += h[1]; gq[(o + 2) * B + b] += h[2];
          gq[(o + 3) * B + b] += h[3]; gq[(o + 4) * B + b] += h[4]; gq[(o + 5) * B + b] += h[5];
        } else if (bd.jtype == JT_BALL || bd.jtype == JT_FREEC) {
          if (bd.ballComp == 0) {
            const int nc = bd.jtype == JT_BALL ? 3 : 6;
            for (int c = 0; c < nc; c++) {
              applyHt(bodies[i + c], q, B, b, xiP, h);
              gq[(o + c) * B + b] += h[0];
            }
          }
        } else {
          applyHt(bd, q, B, b, xiP, h);
          gq[o * B + b] += h[0];
        }
      }
      if (gvel) {
        if (bd.jtype == JT_FREE) {
          double y[6];
          toArr(dAdT(cT(bd.Tcj), xiV), y);                // S = Ad(T_cj), FreeJoint.cpp:1049-1056
          gv[o * B + b] += y[0]; gv[(o + 1) * B + b] += y[1]; gv[(o + 2) * B + b] += y[2];
          gv[(o + 3) * B + b] += y[3]; gv[(o + 4) * B + b] += y[4]; gv[(o + 5) * B + b] += y[5];
        } else {
          gv[o * B + b] += dot(cV6(bd.S), xiV);
        }
      }
      if (j > 0) {
        const T12 T = jointRelTransform(bd, q, B, b);
        if (gpos) xiP = dAdInvT(T, xiP);
        if (gvel) xiV = dAdInvT(T, xiV);
      }
    }
  }
}

}  // namespace NBL_NS
