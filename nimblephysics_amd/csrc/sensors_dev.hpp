// sensors_dev.hpp — readings of inertial sensors fixed in bodies of the device model for one world: gyroscopes, accelerometers and
// magnetometers (Skeleton::getGyroReadings / getAccelerometerReadings / getMagnetometerReadings, dart/dynamics/Skeleton.cpp:8082-8460;
// www/docs/accs-and-gyros.rst), and their exact reverse-mode pass.  csrc/sensors.hip runs them one world per lane.
//
// Plain C++ on centroidal_dev.hpp / dynamics_dev.hpp (no intrinsics, no LDS, no atomics, no cross-lane operations), so that the tests
// compile this header for the host with g++ (tests/host_shim/sens_shim.cpp).
//
// A SENSOR SET is a list of KIN_SPATIAL entries (kinematics_dev.hpp), like a wrench set: entry e names the frame (R_bs, p_bs) = e.T fixed
// in the last body i of its path (pathLen = 0: fixed in the world).  With the body's twist V = [w; v] and its gravity-free spatial
// acceleration A = [al; a], both in body coordinates (cenBodyDown), its world rotation R, the gravity g and a world field m:
//   gyro = R_bs^T w
//   acc  = R_bs^T (a + al x p_bs + w x (v + w x p_bs) - R^T g)         (the proper acceleration of the sensor's origin)
//   mag  = R_bs^T R^T m
// Rows 3 e .. 3 e + 2 of each output.  A sensor in the world reads gyro 0, acc -R_bs^T g, mag R_bs^T m.
//
// THE REVERSE PASS seeds, per entry, the adjoints of A, V and of the body's world pose (delta W = W hat(eta)) with the cotangents turned
// into the body frame, ug = R_bs g_gyro, ua = R_bs g_acc, um = R_bs g_mag, and u = v + w x p_bs:
//   Ab += [p_bs x ua;  ua]
//   Vb += [ug + u x ua + p_bs x (ua x w);  ua x w]
//   Pb += [(R^T g) x ua + um x (R^T m);  0]                             grad_field += R um
// and carries them leaf -> root through sensBodyUp, the joint step of the centroidal reverse pass.  Nothing is left out: the velocity
// products' dependence on q and v and that of R^T g on q are part of it; ball and free coordinates go through applyHt.
//
// WORKSPACE: the centroidal one, ws[(body * CEN_SLOTS + slot) * B + world].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "centroidal_dev.hpp"

namespace NBL_NS {

// Every output that is not null, of world b.  state = [q; v], [2n][B]; accel [n][B] (needed by accOut only); field [3][B] (needed by
// magOut only); gyro, accOut, magOut [3 count][B].
DEV void sensForwardWorld(const DevBody* __restrict__ bodies, int nb, int n, const double* g3, const DevKinEntry* __restrict__ entries,
                          const int32_t* __restrict__ path, int count, int64_t B, int64_t b, const double* __restrict__ state,
                          const double* __restrict__ accel, const double* __restrict__ field, double* __restrict__ gyro,
                          double* __restrict__ accOut, double* __restrict__ magOut, double* __restrict__ ws) {
  const double* q = state;
  const double* v = state + (int64_t)n * B;
  const bool acc = accOut != nullptr, vel = acc || gyro;
  for (int i = 0; i < nb; i++) {
    T12 T, W;
    V6 V, A;
    cenBodyDown(bodies[i], i, q, v, accel, vel, acc, B, b, ws, T, W, V, A);
  }
  const V3 g = mk3(g3[0], g3[1], g3[2]);
  const V3 m = cenLdOpt3(field, B, b);
  for (int k = 0; k < count; k++) {
    const DevKinEntry& e = entries[k];
    const T12 O = cT(e.T);
    const bool fixed = e.pathLen == 0;
    const int i = fixed ? 0 : wrenchBody(path, e);
    const M3 R = fixed ? eye3() : dynLdT(cenSlot(ws, i, CEN_W, B, b), B).R;
    const V6 V = vel && !fixed ? dynLd6(cenSlot(ws, i, CEN_V, B, b), B) : zero6();
    const int64_t r = 3 * (int64_t)k;
    if (gyro) cenSt3(gyro + r * B + b, B, tmul(O.R, V.w));
    if (accOut) {
      const V6 A = fixed ? zero6() : dynLd6(cenSlot(ws, i, CEN_A, B, b), B);
      cenSt3(accOut + r * B + b, B, tmul(O.R, A.v + cross(A.w, O.p) + cross(V.w, V.v + cross(V.w, O.p)) - tmul(R, g)));
    }
    if (magOut) cenSt3(magOut + r * B + b, B, tmul(O.R, tmul(R, m)));
  }
}

// The joint of body i in the reverse pass: the adjoints Ab, Vb, Pb of its A, V and world pose (complete: every child has added its share)
// give the gradients of the joint's coordinates and go on to the parent's slots.  The joint step of cenVjpWorld, restated here: calling
// one shared function from both changed the code generated for k_centroidal_vjp.
DEV void sensBodyUp(const DevBody* __restrict__ bodies, int i, const double* __restrict__ q, const double* __restrict__ v,
                    const double* __restrict__ accel, bool vel, bool acc, int64_t B, int64_t b, const T12& T, const V6& V, const V6& A, V6 Ab, V6 Vb,
                    V6 Pb, double* __restrict__ gq, double* __restrict__ gv, double* __restrict__ gaccel, double* __restrict__ ws) {
  const DevBody& bd = bodies[i];
  const int64_t o = bd.dofOff;
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

// The exact reverse pass of sensForwardWorld for world b: grad_state [2n][B], grad_accel [n][B] and grad_field [3][B] (any may be null)
// receive (= or +=) the cotangents ggyro, gacc, gmag [3 count][B] (any may be null) pulled back.  See the head of this file.
DEV void sensVjpWorld(const DevBody* __restrict__ bodies, int nb, int n, const double* g3, const DevKinEntry* __restrict__ entries,
                      const int32_t* __restrict__ path, int count, int64_t B, int64_t b, const double* __restrict__ state,
                      const double* __restrict__ accel, const double* __restrict__ field, const double* __restrict__ ggyro,
                      const double* __restrict__ gacc, const double* __restrict__ gmag, double* __restrict__ gstate,
                      double* __restrict__ gaccel, double* __restrict__ gfield, int accumulate, double* __restrict__ ws) {
  const double* q = state;
  const double* v = state + (int64_t)n * B;
  double* gq = gstate;
  double* gv = gstate ? gstate + (int64_t)n * B : nullptr;
  if (!accumulate) {
    if (gstate) for (int d = 0; d < 2 * n; d++) gstate[(int64_t)d * B + b] = 0.0;
    if (gaccel) for (int d = 0; d < n; d++) gaccel[(int64_t)d * B + b] = 0.0;
    if (gfield) cenSt3(gfield + b, B, mk3(0, 0, 0));
  }
  const bool acc = gacc != nullptr, vel = acc || ggyro;
  for (int i = 0; i < nb; i++) {
    T12 T, W;
    V6 V, A;
    cenBodyDown(bodies[i], i, q, v, accel, vel, acc, B, b, ws, T, W, V, A);
    dynStT(cenSlot(ws, i, CEN_T, B, b), B, T);
    dynSt6(cenSlot(ws, i, CEN_PB, B, b), B, zero6());
    if (vel) dynSt6(cenSlot(ws, i, CEN_VB, B, b), B, zero6());
    if (acc) dynSt6(cenSlot(ws, i, CEN_AB, B, b), B, zero6());
  }
  const V3 g = mk3(g3[0], g3[1], g3[2]);
  const V3 m = cenLdOpt3(field, B, b);
  V3 gf = mk3(0, 0, 0);
  for (int k = 0; k < count; k++) {
    const DevKinEntry& e = entries[k];
    const T12 O = cT(e.T);
    const int64_t r = 3 * (int64_t)k;
    const V3 um = gmag ? mul(O.R, cenLd3(gmag + r * B + b, B)) : mk3(0, 0, 0);
    if (e.pathLen == 0) {                                     // fixed in the world: a constant but for the field
      gf = gf + um;
      continue;
    }
    const int i = wrenchBody(path, e);
    const M3 R = dynLdT(cenSlot(ws, i, CEN_W, B, b), B).R;
    gf = gf + mul(R, um);
    V3 pw = cross(um, tmul(R, m));
    if (vel) {
      const V6 V = dynLd6(cenSlot(ws, i, CEN_V, B, b), B);
      V6 Vb = mk6(ggyro ? mul(O.R, cenLd3(ggyro + r * B + b, B)) : mk3(0, 0, 0), mk3(0, 0, 0));
      if (acc) {
        const V3 ua = mul(O.R, cenLd3(gacc + r * B + b, B));
        const V3 uw = cross(ua, V.w);
        Vb = Vb + mk6(cross(V.v + cross(V.w, O.p), ua) + cross(O.p, uw), uw);
        dynAdd6(cenSlot(ws, i, CEN_AB, B, b), B, mk6(cross(O.p, ua), ua));
        pw = pw + cross(tmul(R, g), ua);
      }
      dynAdd6(cenSlot(ws, i, CEN_VB, B, b), B, Vb);
    }
    dynAdd6(cenSlot(ws, i, CEN_PB, B, b), B, mk6(pw, mk3(0, 0, 0)));
  }
  if (gfield && gmag) {
    double* p = gfield + b;
    p[0] += gf.x; p[B] += gf.y; p[2 * B] += gf.z;
  }
  if (!gstate && !gaccel) return;
  for (int i = nb - 1; i >= 0; i--) {
    const T12 T = dynLdT(cenSlot(ws, i, CEN_T, B, b), B);
    const V6 V = vel ? dynLd6(cenSlot(ws, i, CEN_V, B, b), B) : zero6();
    const V6 A = acc ? dynLd6(cenSlot(ws, i, CEN_A, B, b), B) : zero6();
    const V6 Ab = acc ? dynLd6(cenSlot(ws, i, CEN_AB, B, b), B) : zero6();
    const V6 Vb = vel ? dynLd6(cenSlot(ws, i, CEN_VB, B, b), B) : zero6();
    const V6 Pb = dynLd6(cenSlot(ws, i, CEN_PB, B, b), B);
    sensBodyUp(bodies, i, q, v, accel, vel, acc, B, b, T, V, A, Ab, Vb, Pb, gq, gv, gaccel, ws);
  }
}

}  // namespace NBL_NS
