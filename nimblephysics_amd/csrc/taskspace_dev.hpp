// taskspace_dev.hpp — second-order world-space kinematics of the rows of a kinematics map for one world: the dense task Jacobian J
// (map_to_vel = J v), its time derivative Jdot along the motion, the bias acceleration c = Jdot v, the task-space acceleration
// xdd = J a + c, and the exact reverse passes of J and of xdd (BodyNode::getJacobian / getJacobianClassicDeriv / getLinearJacobianDeriv /
// getAngularJacobianDeriv, dart/dynamics/BodyNode.cpp; the rows, their order and their frames are kinForwardWorld's, kinematics_dev.hpp).
// csrc/taskspace.hip runs them one world per lane.
//
// Plain C++ on sensors_dev.hpp / centroidal_dev.hpp / dynamics_dev.hpp (no intrinsics, no LDS, no atomics, no cross-lane operations), so
// that the tests compile this header for the host with g++ (tests/host_shim/task_shim.cpp).
//
// THE ROWS of an entry with frame F = W_body T_offset, body twist V and gravity-free body acceleration A (both in body coordinates, the
// first RNEA sweep: A = AdInvT(T, A_parent) + ad(V, S dq) + S ddq, chainAccel on ball and free chains), Vf = AdInvT(T_offset, V),
// Af = AdInvT(T_offset, A):
//   velocity      angular  R_F Vf.w        linear  R_F Vf.v                           (kinForwardWorld)
//   acceleration  angular  R_F Af.w        linear  R_F (Af.v + Vf.w x Vf.v)           (the classical acceleration of F's origin)
// each the time derivative of the velocity row above it.  No gravity.
//
// THE JACOBIAN.  Every coordinate k has a screw S_k that is constant in the frame of the body it moves (S = Ad(T_cj) for a free root; a
// ball or free chain's axes are fixed in the chain's last body), so its column is the screw carried into F, col = AdInvT(T_(body -> F), S_k),
// rotated into the world: one walk up the entry's ancestor chain.  A coordinate that is no ancestor's has a zero column, WRITTEN here.
// In world coordinates X_k = Ad(W_body) S_k and dX_k/dt = ad(Vs, X_k) with Vs the world twist of the body X_k is fixed in (for the bodies
// of a ball / free chain: the chain's LAST body - this is where the joint's Sdot v term comes from), so with p, u the position and
// velocity of F's origin
//   Jdot  angular  ad(Vs, X_k).w       linear  ad(Vs, X_k).v + ad(Vs, X_k).w x p + X_k.w x u.
//
// THE REVERSE PASS OF J.  <G, J> = sum_k <Phi_k, X_k> + the dependence on p, with Phi_k the wrench [g_ang + p x g_lin; g_lin] of column k.
// A coordinate l of an ancestor-or-self of body(k) moves X_k by ad(Hs_l, X_k) (Hs_l its world position screw: applyHt) and every
// coordinate on the chain moves p, so  g_q[l] = Hs_l . (- sum_(k at or below l) dad(X_k, Phi_k) + [p x m; m]),  m = sum_k g_lin_k x X_k.w.
// Carried leaf -> root in body coordinates like kinVjpWorld's xiP.
//
// THE REVERSE PASS OF xdd seeds, per entry, the adjoints of A, V and of the body's world pose (delta W = W hat(eta)) of the centroidal /
// sensor reverse pass, with ua = R_F^T g_ang, ub = R_F^T g_lin:
//   Ab += dAdInvT(T_offset, [ua; ub])      Vb += dAdInvT(T_offset, [Vf.v x ub; ub x Vf.w])
//   Pb += [R_offset (Af.w x ua + (Af.v + Vf.w x Vf.v) x ub); 0]
// and carries them leaf -> root through sensBodyUp.  Nothing is left out: d(J a + Jdot v)/dq is part of it.
//
// WORKSPACE (the reverse pass of xdd only): the centroidal one, ws[(body * CEN_SLOTS + slot) * B + world].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sensors_dev.hpp"

namespace NBL_NS {

DEV bool taskIsChain(const DevBody& bd) { return bd.jtype == JT_BALL || bd.jtype == JT_FREEC; }
DEV int taskNdof(const DevBody& bd) { return bd.jtype == JT_FREE ? 6 : 1; }
// screw of coordinate c of the body, in the body's frame
DEV V6 taskScrew(const DevBody& bd, int c) {
  if (bd.jtype != JT_FREE) return cV6(bd.S);
  double e[6] = {0, 0, 0, 0, 0, 0};
  e[c] = 1.0;
  return AdT(cT(bd.Tcj), fromArr(e));
}
// angular / linear rows of an entry in a vector [R][B] and in a matrix [R n][B] (row-major R x n per world)
DEV int64_t taskAngRow(const DevKinEntry& e) { return e.row; }
DEV int64_t taskLinRow(const DevKinEntry& e) { return e.kind == KIN_SPATIAL ? e.row + 3 : e.row; }
DEV void taskStCol(double* __restrict__ M, const DevKinEntry& e, int n, int64_t d, int64_t B, int64_t b, V3 ang, V3 lin) {
  if (e.kind != KIN_LINEAR) {
    const int64_t r = taskAngRow(e);
    M[(r * n + d) * B + b] = ang.x; M[((r + 1) * n + d) * B + b] = ang.y; M[((r + 2) * n + d) * B + b] = ang.z;
  }
  if (e.kind != KIN_ANGULAR) {
    const int64_t r = taskLinRow(e);
    M[(r * n + d) * B + b] = lin.x; M[((r + 1) * n + d) * B + b] = lin.y; M[((r + 2) * n + d) * B + b] = lin.z;
  }
}
DEV V3 taskLdCol(const double* __restrict__ M, int64_t r, int n, int64_t d, int64_t B, int64_t b) {
  return mk3(M[(r * n + d) * B + b], M[((r + 1) * n + d) * B + b], M[((r + 2) * n + d) * B + b]);
}
DEV void taskZeroRows(double* __restrict__ M, const DevKinEntry& e, int n, int64_t B, int64_t b) {
  const int64_t r0 = (int64_t)e.row * n, r1 = r0 + (int64_t)kinRows(e.kind) * n;
  for (int64_t x = r0; x < r1; x++) M[x * B + b] = 0.0;
}

// W, V and the gravity-free A of the entry's body: kinWalk with the acceleration of the first RNEA sweep (cenBodyDown on one chain).
DEV void taskWalk(const DevBody* __restrict__ bodies, const int32_t* __restrict__ path, const DevKinEntry& e, const double* __restrict__ q,
                  const double* __restrict__ v, const double* __restrict__ accel, int64_t B, int64_t b, T12& W, V6& V, V6& A) {
  W.R = eye3(); W.p = mk3(0, 0, 0); V = zero6(); A = zero6();
  for (int j = 0; j < e.pathLen; j++) {
    const DevBody& bd = bodies[path[e.pathBegin + j]];
    const T12 T = jointRelTransform(bd, q, B, b);
    const V6 s = jointTwist(bd, v, B, b);
    const V6 sa = jointAccelTwist(bd, v, accel, B, b);
    if (j == 0) {
      W = T;
      V = s;
      A = ad(V, s) + sa;
    } else {
      W = mulT(W, T);
      V = AdInvT(T, V) + s;
      A = AdInvT(T, A) + (ad(V, s) + sa);
    }
  }
}

// xdd [R][B] of world b: J a + Jdot v, or - accel null - the bias acceleration Jdot v.  state = [q; v], [2n][B]; accel [n][B].
DEV void taskAccelWorld(const DevBody* __restrict__ bodies, const DevKinEntry* __restrict__ entries, const int32_t* __restrict__ path, int count,
                        int n, int64_t B, int64_t b, const double* __restrict__ state, const double* __restrict__ accel, double* __restrict__ out) {
  const double* q = state;
  const double* v = state + (int64_t)n * B;
  for (int k = 0; k < count; k++) {
    const DevKinEntry& e = entries[k];
    T12 W;
    V6 V, A;
    taskWalk(bodies, path, e, q, v, accel, B, b, W, V, A);
    const T12 O = cT(e.T);
    const M3 RF = mul(W.R, O.R);
    const V6 Vf = AdInvT(O, V), Af = AdInvT(O, A);
    if (e.kind != KIN_LINEAR) cenSt3(out + taskAngRow(e) * B + b, B, mul(RF, Af.w));
    if (e.kind != KIN_ANGULAR) cenSt3(out + taskLinRow(e) * B + b, B, mul(RF, Af.v + cross(Vf.w, Vf.v)));
  }
}

// J [R n][B] (row-major R x n per world) of world b, zero columns written.
DEV void taskJacobianWorld(const DevBody* __restrict__ bodies, const DevKinEntry* __restrict__ entries, const int32_t* __restrict__ path, int count,
                           int n, int64_t B, int64_t b, const double* __restrict__ state, double* __restrict__ J) {
  const double* q = state;
  for (int k = 0; k < count; k++) {
    const DevKinEntry& e = entries[k];
    taskZeroRows(J, e, n, B, b);
    if (e.pathLen == 0) continue;                         // a frame fixed in the world
    T12 W;
    V6 V;
    kinWalk<false>(bodies, path, e, q, q, B, b, W, V);
    const T12 O = cT(e.T);
    const M3 RF = mul(W.R, O.R);
    T12 X = O;                                            // the entry frame in the frame of the body at hand
    for (int j = e.pathLen - 1; j >= 0; j--) {
      const DevBody& bd = bodies[path[e.pathBegin + j]];
      const int nd = taskNdof(bd);
      for (int c = 0; c < nd; c++) {
        const V6 col = AdInvT(X, taskScrew(bd, c));
        taskStCol(J, e, n, bd.dofOff + c, B, b, mul(RF, col.w), mul(RF, col.v));
      }
      if (j > 0) X = mulT(jointRelTransform(bd, q, B, b), X);
    }
  }
}

// Jdot [R n][B] of world b: d/dt of taskJacobianWorld's J along the motion (q moving with v), zero columns written.
DEV void taskJacobianDerivWorld(const DevBody* __restrict__ bodies, const DevKinEntry* __restrict__ entries, const int32_t* __restrict__ path,
                                int count, int n, int64_t B, int64_t b, const double* __restrict__ state, double* __restrict__ Jd) {
  const double* q = state;
  const double* v = state + (int64_t)n * B;
  for (int k = 0; k < count; k++) {
    const DevKinEntry& e = entries[k];
    taskZeroRows(Jd, e, n, B, b);
    if (e.pathLen == 0) continue;
    T12 W;
    V6 V;
    kinWalk<true>(bodies, path, e, q, v, B, b, W, V);
    const T12 O = cT(e.T);
    const T12 F = mulT(W, O);
    const V3 u = mul(F.R, AdInvT(O, V).v);                 // velocity of F's origin
    T12 Wj;
    V6 Vb = zero6();
    for (int j = 0; j < e.pathLen; j++) {
      const int i = path[e.pathBegin + j];
      const DevBody& bd = bodies[i];
      const T12 T = jointRelTransform(bd, q, B, b);
      const V6 s = jointTwist(bd, v, B, b);
      if (j == 0) { Wj = T; Vb = s; }
      else { Wj = mulT(Wj, T); Vb = AdInvT(T, Vb) + s; }
      V6 Vs = AdT(Wj, Vb);                                // world twist of the body this body's screws are fixed in
      if (taskIsChain(bd)) {                              // ... the last body of a ball / free chain: add the later axes' rates
        const int nc = bd.jtype == JT_BALL ? 3 : 6;
        T12 Wc = Wj;
        for (int c = bd.ballComp + 1; c < nc; c++) {
          const DevBody& bc = bodies[i + (c - bd.ballComp)];
          Wc = mulT(Wc, jointRelTransform(bc, q, B, b));
          Vs = Vs + AdT(Wc, jointTwist(bc, v, B, b));
        }
      }
      const int nd = taskNdof(bd);
      for (int c = 0; c < nd; c++) {
        const V6 Xk = AdT(Wj, taskScrew(bd, c));
        const V6 Xd = ad(Vs, Xk);
        taskStCol(Jd, e, n, bd.dofOff + c, B, b, Xd.w, Xd.v + cross(Xd.w, F.p) + cross(Xk.w, u));
      }
    }
  }
}

// The exact reverse pass of taskJacobianWorld for world b: gq [n][B] (= or +=) d<G, J>/dq, G [R n][B].  See the head of this file.
DEV void taskJacobianVjpWorld(const DevBody* __restrict__ bodies, const DevKinEntry* __restrict__ entries, const int32_t* __restrict__ path,
                              int count, int n, int64_t B, int64_t b, const double* __restrict__ state, const double* __restrict__ G,
                              double* __restrict__ gq, int accumulate) {
  const double* q = state;
  if (!accumulate)
    for (int d = 0; d < n; d++) gq[(int64_t)d * B + b] = 0.0;
  for (int k = 0; k < count; k++) {
    const DevKinEntry& e = entries[k];
    if (e.pathLen == 0) continue;
    T12 W;
    V6 V;
    kinWalk<false>(bodies, path, e, q, q, B, b, W, V);
    const T12 O = cT(e.T);
    const M3 RF = mul(W.R, O.R);
    const bool ang = e.kind != KIN_LINEAR, lin = e.kind != KIN_ANGULAR;
    const int64_t ra = taskAngRow(e), rl = taskLinRow(e);
    // m = sum_k g_lin_k x X_k.w over the whole chain, in the coordinates of F
    V3 mF = mk3(0, 0, 0);
    T12 X = O;
    if (lin)
      for (int j = e.pathLen - 1; j >= 0; j--) {
        const DevBody& bd = bodies[path[e.pathBegin + j]];
        const int nd = taskNdof(bd);
        for (int c = 0; c < nd; c++) {
          const V6 col = AdInvT(X, taskScrew(bd, c));
          mF = mF + cross(tmul(RF, taskLdCol(G, rl, n, bd.dofOff + c, B, b)), col.w);
        }
        if (j > 0) X = mulT(jointRelTransform(bd, q, B, b), X);
      }
    V6 xi = dAdInvT(O, mk6(mk3(0, 0, 0), mF));             // a wrench on the body at hand, body coordinates
    X = O;
    for (int j = e.pathLen - 1; j >= 0; j--) {
      const int i = path[e.pathBegin + j];
      const DevBody& bd = bodies[i];
      const int64_t o = bd.dofOff;
      const int nd = taskNdof(bd);
      for (int c = 0; c < nd; c++) {
        const V6 phiF = mk6(ang ? tmul(RF, taskLdCol(G, ra, n, o + c, B, b)) : mk3(0, 0, 0),
                            lin ? tmul(RF, taskLdCol(G, rl, n, o + c, B, b)) : mk3(0, 0, 0));
        xi = xi - dad(taskScrew(bd, c), dAdInvT(X, phiF));
      }
      double h[6];
      if (bd.jtype == JT_FREE) {
        applyHt(bd, q, B, b, xi, h);
#pragma unroll
        for (int c = 0; c < 6; c++) gq[(o + c) * B + b] += h[c];
      } else if (taskIsChain(bd)) {
        if (bd.ballComp == 0) {
          const int nc = bd.jtype == JT_BALL ? 3 : 6;
          for (int c = 0; c < nc; c++) {
            applyHt(bodies[i + c], q, B, b, xi, h);
            gq[(o + c) * B + b] += h[0];
          }
        }
      } else {
        applyHt(bd, q, B, b, xi, h);
        gq[o * B + b] += h[0];
      }
      if (j > 0) {
        const T12 T = jointRelTransform(bd, q, B, b);
        xi = dAdInvT(T, xi);
        X = mulT(T, X);
      }
    }
  }
}

// The exact reverse pass of taskAccelWorld for world b: grad_state [2n][B] and grad_accel [n][B] (either may be null) receive (= or +=) the
// cotangent gout [R][B] pulled back.  accel null: the reverse pass of the bias acceleration.  See the head of this file.
DEV void taskAccelVjpWorld(const DevBody* __restrict__ bodies, int nb, int n, const DevKinEntry* __restrict__ entries,
                           const int32_t* __restrict__ path, int count, int64_t B, int64_t b, const double* __restrict__ state,
                           const double* __restrict__ accel, const double* __restrict__ gout, double* __restrict__ gstate,
                           double* __restrict__ gaccel, int accumulate, double* __restrict__ ws) {
  const double* q = state;
  const double* v = state + (int64_t)n * B;
  double* gq = gstate;
  double* gv = gstate ? gstate + (int64_t)n * B : nullptr;
  if (!accumulate) {
    if (gstate) for (int d = 0; d < 2 * n; d++) gstate[(int64_t)d * B + b] = 0.0;
    if (gaccel) for (int d = 0; d < n; d++) gaccel[(int64_t)d * B + b] = 0.0;
  }
  if (!gstate && !gaccel) return;
  for (int i = 0; i < nb; i++) {
    T12 T, W;
    V6 V, A;
    cenBodyDown(bodies[i], i, q, v, accel, true, true, B, b, ws, T, W, V, A);
    dynStT(cenSlot(ws, i, CEN_T, B, b), B, T);
    dynSt6(cenSlot(ws, i, CEN_PB, B, b), B, zero6());
    dynSt6(cenSlot(ws, i, CEN_VB, B, b), B, zero6());
    dynSt6(cenSlot(ws, i, CEN_AB, B, b), B, zero6());
  }
  for (int k = 0; k < count; k++) {
    const DevKinEntry& e = entries[k];
    if (e.pathLen == 0) continue;                         // a frame fixed in the world: a constant
    const int i = wrenchBody(path, e);
    const T12 O = cT(e.T);
    const M3 RF = mul(dynLdT(cenSlot(ws, i, CEN_W, B, b), B).R, O.R);
    const V6 Vf = AdInvT(O, dynLd6(cenSlot(ws, i, CEN_V, B, b), B)), Af = AdInvT(O, dynLd6(cenSlot(ws, i, CEN_A, B, b), B));
    const V3 ua = e.kind != KIN_LINEAR ? tmul(RF, cenLd3(gout + taskAngRow(e) * B + b, B)) : mk3(0, 0, 0);
    const V3 ub = e.kind != KIN_ANGULAR ? tmul(RF, cenLd3(gout + taskLinRow(e) * B + b, B)) : mk3(0, 0, 0);
    dynAdd6(cenSlot(ws, i, CEN_AB, B, b), B, dAdInvT(O, mk6(ua, ub)));
    dynAdd6(cenSlot(ws, i, CEN_VB, B, b), B, dAdInvT(O, mk6(cross(Vf.v, ub), cross(ub, Vf.w))));
    dynAdd6(cenSlot(ws, i, CEN_PB, B, b), B, mk6(mul(O.R, cross(Af.w, ua) + cross(Af.v + cross(Vf.w, Vf.v), ub)), mk3(0, 0, 0)));
  }
  for (int i = nb - 1; i >= 0; i--) {
    const T12 T = dynLdT(cenSlot(ws, i, CEN_T, B, b), B);
    const V6 V = dynLd6(cenSlot(ws, i, CEN_V, B, b), B);
    const V6 A = dynLd6(cenSlot(ws, i, CEN_A, B, b), B);
    const V6 Ab = dynLd6(cenSlot(ws, i, CEN_AB, B, b), B);
    const V6 Vb = dynLd6(cenSlot(ws, i, CEN_VB, B, b), B);
    const V6 Pb = dynLd6(cenSlot(ws, i, CEN_PB, B, b), B);
    sensBodyUp(bodies, i, q, v, accel, true, true, B, b, T, V, A, Ab, Vb, Pb, gq, gv, gaccel, ws);
  }
}

}  // namespace NBL_NS
