// centroidal_dev.hpp — whole-body quantities of a set of bodies of the device model for one world: total mass, centre of mass, its
// velocity, acceleration and velocity Jacobian, the momentum about the centre of mass, kinetic and potential energy
// (Skeleton::getMass / getCOM / getCOMLinearVelocity / getCOMLinearAcceleration / getCOMLinearJacobian / computeKineticEnergy /
// computePotentialEnergy, dart/dynamics/Skeleton.cpp:13598-13810; BodyNode::getLinearMomentum / getAngularMomentum / computeKineticEnergy /
// computePotentialEnergy, BodyNode.cpp:2357-2391; GenericJoint::computePotentialEnergy, GenericJoint.hpp:1598-1610), and their exact
// reverse-mode pass.  csrc/centroidal.hip runs them one world per lane.
//
// THE MOMENTUM OF THE SET IS THIS PROJECT'S EXTENSION: the reference has the momenta per body only (BodyNode.cpp:2378-2391); here they are
// summed over the set,  [angular about the set's centre of mass; linear]  in world coordinates.
//
// Plain C++ on spatial_dev.hpp / kinematics_dev.hpp / dynamics_dev.hpp (no intrinsics, no LDS, no atomics, no cross-lane operations), so
// that the tests compile this header for the host with g++ (tests/host_shim/cen_shim.cpp).
//
// A BODY SET is a 64-bit mask over device bodies (`mass`: the bodies whose inertia counts; a ball / free chain carries its mass on the body
// that carries T_cj) and a second one (`joints`: the bodies whose coordinates' springs count - the whole chain of such a joint).
//
// ONE SWEEP root -> leaf gives every output: W_i = W_parent T_i, V_i = AdInvT(T_i, V_parent) + S dq, and - with accelerations - the
// gravity-free A_i of the first RNEA sweep (dynSweepDown; chainAccel on ball and free chains).  With h_i = G_i V_i and
// F_i = G_i A_i - dad(V_i, h_i) (the body's own force without gravity), over the bodies of the set:
//   com      = sum (m p + R mc) / M                 com_vel = sum R m (v + w x c) / M           com_acc = sum R lin(F) / M
//   momentum = [sum (R ang(h) + p x R lin(h)) - com x P;  P = sum R lin(h)]                      ke = sum V.h / 2
//   pe       = -g . sum (m p + R mc)   (CEN_PE_BODY_ORIGIN: -g . sum (m p + R mo), the reference's rule; mo = 0 unless welded bodies were merged)  + sum_d k_d (q_d - rest_d)^2 / 2
//   Jcom column of a coordinate with relative screw S = [w; v] on body i:  R_i (m_sub v + w x mc_sub) / M, (m_sub, mc_sub) the mass and first
//   moment of the set's bodies in the subtree of i, in the frame of i - one sweep leaf -> root.  A coordinate that moves no body of the set
//   has m_sub = 0: the KERNEL writes its zero column, no host zero-fill is needed.
//
// THE REVERSE PASS seeds, per body of the set, the adjoints of A, V and of the body's world pose (a wrench Pb on the body frame:
// delta W = W hat(eta)) and carries them leaf -> root exactly as idVjpWorldT carries Ab and Vb and kinVjpWorld carries xiP:
//   Fb = [0; R^T g_acc / M]                     hb = [R^T g_k;  R^T (g_vel / M + g_P + g_k x (p - com))]      (g_mom = [g_k; g_P])
//   Ab = G Fb      Vb = dad(Fb, h) - G ad(V, Fb) + G hb + g_ke h
//   Pb = dad(hb, h) + dad(Fb, F) + G [0; R^T (g_com / M + g_k x P / M - g_pe g)]     (body origin rule: - g_pe m [0; R^T g] instead)
// dad(Fb, F) = [lin(F) x R^T g_acc / M; 0] is the explicit dR term of com_acc.  Then per joint, as there:
//   grad_accel = S^T Ab,  Vb -= dad(S dq, Ab),  grad_v = S^T (Vb + dad(V, Ab)) (+ chainAccelVjp),
//   grad_q = H^T (dad(X A_parent, Ab) + dad(X V_parent, Vb) + Pb)                 (applyHt: expMapJac for ball and free coordinates).
// Nothing is left out: the velocity- and acceleration-level outputs carry their full position dependence.
//
// WORKSPACE  ws[(body * CEN_SLOTS + slot) * B + world], like the dynamics one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dynamics_dev.hpp"

namespace NBL_NS {

constexpr int CEN_PE_BODY_ORIGIN = 1, CEN_NO_SPRINGS = 2;   // = NBL_CEN_*
constexpr int CEN_FLAG_MASK = 3;
constexpr int CEN_T = 0;       // 12  relative transform
constexpr int CEN_W = 12;      // 12  world transform
constexpr int CEN_V = 24;      // 6   body twist
constexpr int CEN_A = 30;      // 6   body acceleration, gravity-free
constexpr int CEN_AB = 36;     // 6   reverse pass: adjoint of A;  forward pass (Jcom): [0] m_sub, [1..3] mc_sub
constexpr int CEN_VB = 42;     // 6   adjoint of V
constexpr int CEN_PB = 48;     // 6   adjoint of the world pose (a wrench on the body frame)
constexpr int CEN_SLOTS = 54;
constexpr int CEN_MAX_BODIES = 64;

struct DevBodySet {
  uint64_t mass, joints;
  // CEN_PE_BODY_ORIGIN on a model whose caller merged welded bodies: per device body the first moment  sum_k m_k o_k  of the origins o_k of
  // the merged BodyNodes' frames, in the body's frame (nbl_body_set_origin_moments).  Zero: the body's own origin.
  double originMoment[3 * CEN_MAX_BODIES];
};
DEV V3 cenOriginMoment(const DevBodySet& set, int i) { return mk3(set.originMoment[3 * i], set.originMoment[3 * i + 1], set.originMoment[3 * i + 2]); }

DEV double* cenSlot(double* ws, int body, int slot, int64_t B, int64_t b) { return ws + ((int64_t)body * CEN_SLOTS + slot) * B + b; }
DEV V3 cenLd3(const double* p, int64_t B) { return mk3(p[0], p[B], p[2 * B]); }
DEV void cenSt3(double* p, int64_t B, V3 x) { p[0] = x.x; p[B] = x.y; p[2 * B] = x.z; }
DEV V3 cenLdOpt3(const double* p, int64_t B, int64_t b) { return p ? cenLd3(p + b, B) : mk3(0, 0, 0); }
DEV bool cenIn(uint64_t mask, int i) { return ((mask >> i) & 1ull) != 0; }
// mass and first moment m c of a packed spatial inertia (packSpatialInertia: the upper right block is m [c]x)
DEV double cenMassOf(const double* G) { return G[15]; }
DEV V3 cenMomentOf(const double* G) { return mk3(G[13], G[5], G[8]); }

// Total mass of the set at the inertias in `bodies`, summed in body order (the host getter runs the same loop on its copy).
__host__ __device__ inline double cenTotalMass(const DevBody* bodies, int nb, uint64_t mask) {
  double M = 0.0;
  for (int i = 0; i < nb; i++)
    if ((mask >> i) & 1ull) M += bodies[i].G[15];
  return M;
}

// T, W, V (VEL) and A (ACC) of body i from its parent's slots; stored for the later sweeps.
DEV void cenBodyDown(const DevBody& bd, int i, const double* __restrict__ q, const double* __restrict__ v, const double* __restrict__ accel,
                     bool vel, bool acc, int64_t B, int64_t b, double* __restrict__ ws, T12& T, T12& W, V6& V, V6& A) {
  T = jointRelTransform(bd, q, B, b);
  W = bd.parent >= 0 ? mulT(dynLdT(cenSlot(ws, bd.parent, CEN_W, B, b), B), T) : T;
  V = zero6();
  A = zero6();
  if (vel) {
    const V6 s = jointTwist(bd, v, B, b);
    V = bd.parent >= 0 ? AdInvT(T, dynLd6(cenSlot(ws, bd.parent, CEN_V, B, b), B)) + s : s;
    dynSt6(cenSlot(ws, i, CEN_V, B, b), B, V);
    if (acc) {
      A = ad(V, s) + jointAccelTwist(bd, v, accel, B, b);
      if (bd.parent >= 0) A = AdInvT(T, dynLd6(cenSlot(ws, bd.parent, CEN_A, B, b), B)) + A;
      dynSt6(cenSlot(ws, i, CEN_A, B, b), B, A);
    }
  }
  dynStT(cenSlot(ws, i, CEN_W, B, b), B, W);
}

// joint spring energy of the set's coordinates (GenericJoint.hpp:1598-1610) and, with gq, its gradient times gpe
DEV double cenSprings(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs, int nb, uint64_t joints, const double* __restrict__ q,
                      int64_t B, int64_t b, double gpe, double* __restrict__ gq) {
  double e = 0.0;
  for (int i = 0; i < nb; i++) {
    if (!cenIn(joints, i)) continue;
    const DevBody& bd = bodies[i];
    for (int k = 0; k < bd.ndof; k++) {
      const int64_t d = bd.dofOff + k;
      const DevDof& f = dofs[d];
      const double x = q[d * B + b] - f.rest;
      e += 0.5 * f.spring * x * x;
      if (gq) gq[d * B + b] += gpe * f.spring * x;
    }
  }
  return e;
}

// Every output that is not null, of world b.  state = [q; v], [2n][B]; accel [n][B] (needed by comAcc only).
// com, comVel, comAcc [3][B]; mom [6][B]; ke, pe [B]; Jcom [3 n][B] (row-major 3 x n per world).
DEV void cenForwardWorld(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs, int nb, int n, const double* g3, const DevBodySet& set,
                         int flags, int64_t B, int64_t b, const double* __restrict__ state, const double* __restrict__ accel,
                         double* __restrict__ com, double* __restrict__ comVel, double* __restrict__ comAcc, double* __restrict__ mom,
                         double* __restrict__ ke, double* __restrict__ pe, double* __restrict__ Jcom, double* __restrict__ ws) {
  const double* q = state;
  const double* v = state + (int64_t)n * B;
  const bool acc = comAcc != nullptr, vel = acc || comVel || mom || ke;
  const double iM = 1.0 / cenTotalMass(bodies, nb, set.mass);
  V3 sc = mk3(0, 0, 0), sp = sc, sv = sc, sa = sc, P = sc, L0 = sc;
  double keS = 0.0;
  for (int i = 0; i < nb; i++) {
    const DevBody& bd = bodies[i];
    T12 T, W;
    V6 V, A;
    cenBodyDown(bd, i, q, v, accel, vel, acc, B, b, ws, T, W, V, A);
    const bool in = cenIn(set.mass, i);
    const double m = cenMassOf(bd.G);
    const V3 mc = cenMomentOf(bd.G);
    if (Jcom) {
      dynStT(cenSlot(ws, i, CEN_T, B, b), B, T);
      double* p = cenSlot(ws, i, CEN_AB, B, b);
      p[0] = in ? m : 0.0;
      cenSt3(p + B, B, in ? mc : mk3(0, 0, 0));
    }
    if (!in) continue;
    sc = sc + (m * W.p + mul(W.R, mc));
    sp = sp + (m * W.p + mul(W.R, cenOriginMoment(set, i)));
    if (vel) {
      const S6 G = cS6(bd.G);
      const V6 h = mul(G, V);
      sv = sv + mul(W.R, m * V.v + cross(V.w, mc));
      const V3 f = mul(W.R, h.v);
      P = P + f;
      L0 = L0 + (mul(W.R, h.w) + cross(W.p, f));
      keS += 0.5 * dot(V, h);
      if (acc) sa = sa + mul(W.R, (mul(G, A) - dad(V, h)).v);
    }
  }
  const V3 c = iM * sc;
  if (com) cenSt3(com + b, B, c);
  if (comVel) cenSt3(comVel + b, B, iM * sv);
  if (comAcc) cenSt3(comAcc + b, B, iM * sa);
  if (mom) dynSt6(mom + b, B, mk6(L0 - cross(c, P), P));
  if (ke) ke[b] = keS;
  if (pe) {
    const V3 g = mk3(g3[0], g3[1], g3[2]);
    double e = -dot(g, (flags & CEN_PE_BODY_ORIGIN) ? sp : sc);
    if (!(flags & CEN_NO_SPRINGS)) e += cenSprings(bodies, dofs, nb, set.joints, q, B, b, 0.0, nullptr);
    pe[b] = e;
  }
  if (Jcom)
    for (int i = nb - 1; i >= 0; i--) {
      const DevBody& bd = bodies[i];
      const double* p = cenSlot(ws, i, CEN_AB, B, b);
      const double ms = p[0];
      const V3 mcs = cenLd3(p + B, B);
      const M3 R = dynLdT(cenSlot(ws, i, CEN_W, B, b), B).R;
      const int64_t o = bd.dofOff;
      if (bd.jtype == JT_FREE) {
        const T12 Tcj = cT(bd.Tcj);
        for (int k = 0; k < 6; k++) {
          double e[6] = {0, 0, 0, 0, 0, 0};
          e[k] = 1.0;
          const V6 S = AdT(Tcj, fromArr(e));
          const V3 col = iM * mul(R, ms * S.v + cross(S.w, mcs));
          Jcom[(o + k) * B + b] = col.x; Jcom[(n + o + k) * B + b] = col.y; Jcom[(2 * (int64_t)n + o + k) * B + b] = col.z;
        }
      } else {
        const V6 S = cV6(bd.S);
        const V3 col = iM * mul(R, ms * S.v + cross(S.w, mcs));
        Jcom[o * B + b] = col.x; Jcom[(n + o) * B + b] = col.y; Jcom[(2 * (int64_t)n + o) * B + b] = col.z;
      }
      if (bd.parent >= 0) {
        const T12 T = dynLdT(cenSlot(ws, i, CEN_T, B, b), B);
        double* pp = cenSlot(ws, bd.parent, CEN_AB, B, b);
        const V3 up = mul(T.R, mcs) + ms * T.p;
        pp[0] += ms; pp[B] += up.x; pp[2 * B] += up.y; pp[3 * B] += up.z;
      }
    }
}

// The exact reverse pass of cenForwardWorld for world b: grad_state [2n][B] and grad_accel [n][B] (either may be null) receive (= or +=)
// the cotangents gcom, gvel, gacc [3][B], gmom [6][B], gke, gpe [B] (any may be null) pulled back.  See the head of this file.
DEV void cenVjpWorld(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs, int nb, int n, const double* g3, const DevBodySet& set,
                     int flags, int64_t B, int64_t b, const double* __restrict__ state, const double* __restrict__ accel,
                     const double* __restrict__ gcom, const double* __restrict__ gvel, const double* __restrict__ gacc,
                     const double* __restrict__ gmom, const double* __restrict__ gke, const double* __restrict__ gpe,
                     double* __restrict__ gstate, double* __restrict__ gaccel, int accumulate, double* __restrict__ ws) {
  const double* q = state;
  const double* v = state + (int64_t)n * B;
  double* gq = gstate;
  double* gv = gstate ? gstate + (int64_t)n * B : nullptr;
  if (!accumulate) {
    if (gstate) for (int d = 0; d < 2 * n; d++) gstate[(int64_t)d * B + b] = 0.0;
    if (gaccel) for (int d = 0; d < n; d++) gaccel[(int64_t)d * B + b] = 0.0;
  }
  const bool acc = gacc != nullptr, vel = acc || gvel || gmom || gke;
  const double iM = 1.0 / cenTotalMass(bodies, nb, set.mass);
  V3 sc = mk3(0, 0, 0), P = sc;
  for (int i = 0; i < nb; i++) {
    const DevBody& bd = bodies[i];
    T12 T, W;
    V6 V, A;
    cenBodyDown(bd, i, q, v, accel, vel, acc, B, b, ws, T, W, V, A);
    dynStT(cenSlot(ws, i, CEN_T, B, b), B, T);
    dynSt6(cenSlot(ws, i, CEN_PB, B, b), B, zero6());
    if (vel) dynSt6(cenSlot(ws, i, CEN_VB, B, b), B, zero6());
    if (acc) dynSt6(cenSlot(ws, i, CEN_AB, B, b), B, zero6());
    if (!cenIn(set.mass, i)) continue;
    sc = sc + (cenMassOf(bd.G) * W.p + mul(W.R, cenMomentOf(bd.G)));
    if (gmom) P = P + mul(W.R, mul(cS6(bd.G), V).v);
  }
  const V3 c = iM * sc;
  const V3 g = mk3(g3[0], g3[1], g3[2]);
  const V3 gk = cenLdOpt3(gmom, B, b), gP = gmom ? cenLd3(gmom + 3 * B + b, B) : mk3(0, 0, 0);
  const V3 gvl = iM * cenLdOpt3(gvel, B, b) + gP, gal = iM * cenLdOpt3(gacc, B, b);
  const double gk_e = gke ? gke[b] : 0.0, gp_e = gpe ? gpe[b] : 0.0;
  const bool origin = (flags & CEN_PE_BODY_ORIGIN) != 0;
  // cotangent of sum (m p + R mc), and of sum m p under the body-origin rule
  const V3 gsc = iM * (cenLdOpt3(gcom, B, b) + cross(gk, P)) - (origin ? 0.0 : gp_e) * g;
  const V3 gsp = -(origin ? gp_e : 0.0) * g;
  for (int i = nb - 1; i >= 0; i--) {
    const DevBody& bd = bodies[i];
    const int64_t o = bd.dofOff;
    const T12 T = dynLdT(cenSlot(ws, i, CEN_T, B, b), B);
    const V6 V = vel ? dynLd6(cenSlot(ws, i, CEN_V, B, b), B) : zero6();
    const V6 A = acc ? dynLd6(cenSlot(ws, i, CEN_A, B, b), B) : zero6();
    V6 Ab = acc ? dynLd6(cenSlot(ws, i, CEN_AB, B, b), B) : zero6();
    V6 Vb = vel ? dynLd6(cenSlot(ws, i, CEN_VB, B, b), B) : zero6();
    V6 Pb = dynLd6(cenSlot(ws, i, CEN_PB, B, b), B);
    if (cenIn(set.mass, i)) {
      const T12 W = dynLdT(cenSlot(ws, i, CEN_W, B, b), B);
      const S6 G = cS6(bd.G);
      Pb = Pb + mul(G, mk6(mk3(0, 0, 0), tmul(W.R, gsc)));
      if (origin) {
        const V3 gl = tmul(W.R, gsp);
        Pb = Pb + mk6(cross(cenOriginMoment(set, i), gl), cenMassOf(bd.G) * gl);
      }
      if (vel) {
        const V6 h = mul(G, V);
        const V6 hb = mk6(tmul(W.R, gk), tmul(W.R, gvl + cross(gk, W.p - c)));
        Vb = Vb + mul(G, hb) + gk_e * h;
        Pb = Pb + dad(hb, h);
        if (acc) {
          const V6 Fb = mk6(mk3(0, 0, 0), tmul(W.R, gal));
          Ab = Ab + mul(G, Fb);
          Vb = Vb + dad(Fb, h) - mul(G, ad(V, Fb));
          Pb = Pb + dad(Fb, mul(G, A) - dad(V, h));
        }
      }
    }
    const V6 s = vel ? jointTwist(bd, v, B, b) : zero6();
    if (acc) {
      Vb = Vb - dad(s, Ab);
      if ((bd.jtype == JT_BALL || bd.jtype == JT_FREEC) && bd.ballComp != 0) dynSt6(cenSlot(ws, i, CEN_AB, B, b), B, Ab);   // read again at the chain's first body
      if (gaccel) {
        if (bd.jtype == JT_FREE) {
          double y[6];
          toArr(dAdT(cT(bd.Tcj), Ab), y);
#pragma unroll
          for (int k = 0; k < 6; k++) gaccel[(o + k) * B + b] += y[k];
        } else {
          gaccel[o * B + b] += dot(cV6(bd.S), Ab);
        }
      }
    }
    if (gv && vel) {
      const V6 sb = acc ? Vb + dad(V, Ab) : Vb;
      if (bd.jtype == JT_FREE) {
        double y[6];
        toArr(dAdT(cT(bd.Tcj), sb), y);
#pragma unroll
        for (int k = 0; k < 6; k++) gv[(o + k) * B + b] += y[k];
      } else {
        gv[o * B + b] += dot(cV6(bd.S), sb);
      }
      if (acc && (bd.jtype == JT_BALL || bd.jtype == JT_FREEC) && bd.ballComp == 0) {   // the chain's last visit: grad of a_chain -> v through c(v)
        const int nc = bd.jtype == JT_BALL ? 3 : 6;
        double ga[6];
        ga[0] = dot(cV6(bd.S), Ab);
        for (int k = 1; k < nc; k++) ga[k] = dot(cV6(bodies[i + k].S), dynLd6(cenSlot(ws, i + k, CEN_AB, B, b), B));
        chainAccelVjp((int)o, nc, v, ga, gv, B, b);
      }
    }
    if (gq) {
      const bool chainTail = (bd.jtype == JT_BALL || bd.jtype == JT_FREEC) && bd.ballComp != 0;   // constant transform: nothing to emit
      if (!chainTail) {
        V6 xi = Pb;
        if (vel && bd.parent >= 0) xi = xi + dad(V - s, Vb);                                        // X V_parent
        if (acc && bd.parent >= 0) xi = xi + dad(A - ad(V, s) - jointAccelTwist(bd, v, accel, B, b), Ab);   // X A_parent
        double h[6];
        if (bd.jtype == JT_FREE) {
          applyHt(bd, q, B, b, xi, h);
#pragma unroll
          for (int k = 0; k < 6; k++) gq[(o + k) * B + b] += h[k];
        } else if (bd.jtype == JT_BALL || bd.jtype == JT_FREEC) {
          const int nc = bd.jtype == JT_BALL ? 3 : 6;
          for (int k = 0; k < nc; k++) {
            applyHt(bodies[i + k], q, B, b, xi, h);
            gq[(o + k) * B + b] += h[0];
          }
        } else {
          applyHt(bd, q, B, b, xi, h);
          gq[o * B + b] += h[0];
        }
      }
    }
    if (bd.parent >= 0) {
      dynAdd6(cenSlot(ws, bd.parent, CEN_PB, B, b), B, dAdInvT(T, Pb));
      if (vel) dynAdd6(cenSlot(ws, bd.parent, CEN_VB, B, b), B, dAdInvT(T, Vb));
      if (acc) dynAdd6(cenSlot(ws, bd.parent, CEN_AB, B, b), B, dAdInvT(T, Ab));
    }
  }
  if (gq && gpe && !(flags & CEN_NO_SPRINGS)) (void)cenSprings(bodies, dofs, nb, set.joints, q, B, b, gp_e, gq);
}

}  // namespace NBL_NS
