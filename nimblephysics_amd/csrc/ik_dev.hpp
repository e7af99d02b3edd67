// ik_dev.hpp — inverse kinematics of one world: the reference's math::solveIK / refineIK (dart/math/IKSolver.cpp:195-493) as
// IKMapping::setPositions drives it (dart/neural/IKMapping.cpp:86-119), on the rows of kinematics_dev.hpp and their exact position
// Jacobian (IKMapping::getPosJacobian), with Skeleton::clampPositionsToLimits (Skeleton.cpp:3642-3740) on the device model's limits.
//
// Plain C++ like kinematics_dev.hpp and dynamics_dev.hpp (no intrinsics, no LDS, no cross-lane operations, no atomics): the tests compile
// this header for the host with g++ (tests/host_shim/ik_shim.cpp).  ONE WORLD PER LANE; everything a world keeps between steps lives in the
// caller's workspace laid out [slot][B] (IkLayout), every index into it is computed, so nothing of it is a private array.
//
// Restated operation by operation: solveIK with ONE restart (20 steps of refineIK, then max_step_count steps from that result) and
// refineIK's whole branch ladder (lr, transpose mode, line search, clamping, the forced clamping of the last steps).
// Departures, both stated in include/nimble_amd.h:
//   * the damped-least-squares step.  The reference factors J J^T + lambda I when n < P and J^T J + lambda I otherwise: the LARGER of the
//     two.  Both give the same step, J^T (J J^T + lambda I)^-1 = (J^T J + lambda I)^-1 J^T; this code factors the SMALLER one (min(P, n)
//     on a side; for P = n the reference's) with an in-place Cholesky (llt) and two triangular solves.  lambda = 0 (the reference's
//     complete orthogonal decomposition) is refused by the caller;
//   * the loss returned is the squared error AT the returned positions, from one evaluation after the loop (refineIK's lastError belongs
//     to an earlier iterate, solveIK returns the 20-step phase's).
// clampPositionsToLimits builds 2 pi candidates for revolute coordinates, but its selection loop tests the LAST candidate in every
// condition and so always keeps the FIRST, the coordinate as it came (the last candidate is never below the lower limit: its own loop ended
// there; if it is inside the limits the first is taken and the loop left; if it is above, the violation is the same number for every
// candidate and only the first is strictly smaller than infinity).  What the routine does to a coordinate is therefore the plain clamp,
// and that is what ikClamp does - without the reference's unbounded `while` loops, which a lane must not run on a diverged iterate.
// tests/ik_numpy.py restates the routine literally, loops included, and tests/test_ik_host.py compares.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kinematics_dev.hpp"

namespace NBL_NS {

struct IkConfig {             // = nbl_ik_config
  double convergenceThreshold;
  int32_t maxStepCount;
  double damping;
  int32_t startClamped, lineSearch, dontExitTranspose;
};
constexpr int IK_RESTART_STEPS = 20;   // IKSolver.cpp:249
constexpr int IK_MAX_STEP_COUNT = 100000;   // the caller refuses more: one launch holds a wavefront for its slowest world's whole solve (setPositions uses 500)

// Workspace slots of one world: the solver's state between steps, 3 n + P + min(P, n) + P n + min(P, n)^2 doubles with m = min(P, n)
// (984 = 7.9 kB on Atlas-20, n = 20, with four spatial entries, P = 24).
struct IkLayout {
  int32_t n, P, m;                                   // m: side of the normal matrix
  int32_t pos, last, diff, J, A, y, delta, total;    // pos / last / delta [n], diff [P], J [P][n], A [m][m], y [m]
};
__host__ __device__ inline IkLayout ikLayout(int n, int P) {
  IkLayout L;
  L.n = n; L.P = P; L.m = P < n ? P : n;
  L.pos = 0; L.last = L.pos + n; L.delta = L.last + n; L.diff = L.delta + n; L.y = L.diff + P;
  L.J = L.y + L.m; L.A = L.J + P * n; L.total = L.A + L.m * L.m;
  return L;
}

struct IkCtx {
  const DevBody* bodies; const DevDof* dofs; const DevKinEntry* entries; const int32_t* path;
  int count, nb;
  int64_t B, b;
  const double* target;   // [P][B]
  double* ws;             // [L.total][B]
  IkLayout L;
};
#define IKW(c, slot) (c).ws[(int64_t)(slot) * (c).B + (c).b]

// Skeleton::clampPositionsToLimits on the coordinates at slot `base`: the clamp to [posLo, posHi] per coordinate (see the header comment
// for the 2 pi candidates), then logMap(expMapRot(.)) of the rotation coordinates of free and ball joints.
DEV void ikClamp(const IkCtx& c, int base) {
  for (int d = 0; d < c.L.n; d++) {
    double p = IKW(c, base + d);
    const double lo = c.dofs[d].posLo, hi = c.dofs[d].posHi;
    if (p > hi) p = hi;
    if (p < lo) p = lo;
    IKW(c, base + d) = p;
  }
  for (int i = 0; i < c.nb; i++) {
    const DevBody& bd = c.bodies[i];
    if (bd.jtype == JT_FREE || ((bd.jtype == JT_BALL || bd.jtype == JT_FREEC) && bd.ballComp == 0)) {
      const int o = base + bd.dofOff;
      const V3 r = logMap(expMapRot(mk3(IKW(c, o), IKW(c, o + 1), IKW(c, o + 2))));
      IKW(c, o) = r.x; IKW(c, o + 1) = r.y; IKW(c, o + 2) = r.z;
    }
  }
}

// eval of IKMapping::setPositions (IKMapping.cpp:108-112): diff = rows(q) - target, returned squared norm; with JAC also J = getPosJacobian,
// dense [P][n].  Every entry's ancestor chain is walked ONCE, leaf -> root, with the wrenches of all of the entry's rows (the unit
// cotangents of kinVjpWorld) carried together; every joint on the way emits its columns: H^T xi (applyHt) per row.  The entries of J off
// the chains are zero and are never written: ikSolveWorld zeroes J once.
template <bool JAC>
DEV double ikEval(const IkCtx& c, int base) {
  const int64_t B = c.B, b = c.b;
  const double* q = c.ws + (int64_t)base * B;
  const int n = c.L.n;
  double err = 0.0;
  for (int k = 0; k < c.count; k++) {
    const DevKinEntry& e = c.entries[k];
    T12 W;
    V6 V;
    kinWalk<false>(c.bodies, c.path, e, q, q, B, b, W, V);
    const T12 O = cT(e.T);
    const T12 F = mulT(W, O);
    const int r = e.row, rl = e.kind == KIN_SPATIAL ? r + 3 : r;
    if (e.kind != KIN_LINEAR) {
      const V3 lg = logMap(F.R);
      const double d0 = lg.x - c.target[(int64_t)r * B + b], d1 = lg.y - c.target[(int64_t)(r + 1) * B + b], d2 = lg.z - c.target[(int64_t)(r + 2) * B + b];
      IKW(c, c.L.diff + r) = d0; IKW(c, c.L.diff + r + 1) = d1; IKW(c, c.L.diff + r + 2) = d2;
      err += d0 * d0; err += d1 * d1; err += d2 * d2;
    }
    if (e.kind != KIN_ANGULAR) {
      const double d0 = F.p.x - c.target[(int64_t)rl * B + b], d1 = F.p.y - c.target[(int64_t)(rl + 1) * B + b], d2 = F.p.z - c.target[(int64_t)(rl + 2) * B + b];
      IKW(c, c.L.diff + rl) = d0; IKW(c, c.L.diff + rl + 1) = d1; IKW(c, c.L.diff + rl + 2) = d2;
      err += d0 * d0; err += d1 * d1; err += d2 * d2;
    }
    if (!JAC || e.pathLen == 0) continue;
    // the rows' unit cotangents as wrenches on F, body coordinates (kinVjpWorld): xi[0..2] the first three rows, xi[3..5] a spatial entry's linear rows
    const int nr = kinRows(e.kind);
    V6 xi[6];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const V3 ea = mk3(a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0);
      V6 ang = zero6(), lin = zero6();
      if (e.kind != KIN_LINEAR) {
        const M3 Rb = logMap_vjp(F.R, ea);
        const M3 N = mulAtB(F.R, Rb);
        ang.w = mk3(N.m[7] - N.m[5], N.m[2] - N.m[6], N.m[3] - N.m[1]);
        ang = dAdInvT(O, ang);
      }
      if (e.kind != KIN_ANGULAR) {
        lin.v = tmul(F.R, ea);
        lin = dAdInvT(O, lin);
      }
      xi[a] = e.kind == KIN_LINEAR ? lin : ang;
      xi[3 + a] = lin;
    }
    for (int j = e.pathLen - 1; j >= 0; j--) {
      const int i = c.path[e.pathBegin + j];
      const DevBody& bd = c.bodies[i];
      const int o = bd.dofOff;
#pragma unroll
      for (int a = 0; a < 6; a++) {
        if (a >= nr) continue;
        const int jr = c.L.J + (r + a) * n;
        double h[6];
        if (bd.jtype == JT_FREE) {
          applyHt(bd, q, B, b, xi[a], h);
          IKW(c, jr + o) = h[0]; IKW(c, jr + o + 1) = h[1]; IKW(c, jr + o + 2) = h[2];
          IKW(c, jr + o + 3) = h[3]; IKW(c, jr + o + 4) = h[4]; IKW(c, jr + o + 5) = h[5];
        } else if (bd.jtype == JT_BALL || bd.jtype == JT_FREEC) {
          if (bd.ballComp == 0) {
            const int nc = bd.jtype == JT_BALL ? 3 : 6;
            for (int cc = 0; cc < nc; cc++) {
              applyHt(c.bodies[i + cc], q, B, b, xi[a], h);
              IKW(c, jr + o + cc) = h[0];
            }
          }
        } else {
          applyHt(bd, q, B, b, xi[a], h);
          IKW(c, jr + o) = h[0];
        }
      }
      if (j > 0) {
        const T12 T = jointRelTransform(bd, q, B, b);
#pragma unroll
        for (int a = 0; a < 6; a++)
          if (a < nr) xi[a] = dAdInvT(T, xi[a]);
      }
    }
  }
  return err;
}

// In-place Cholesky A = L L^T of the m x m matrix at slot L.A (lower triangle), then L L^T y = y.
DEV void ikCholSolve(const IkCtx& c) {
  const int m = c.L.m, A = c.L.A, y = c.L.y;
  for (int j = 0; j < m; j++) {
    double s = IKW(c, A + j * m + j);
    for (int k = 0; k < j; k++) { const double l = IKW(c, A + j * m + k); s -= l * l; }
    const double d = sqrt(s);
    IKW(c, A + j * m + j) = d;
    for (int i = j + 1; i < m; i++) {
      double t = IKW(c, A + i * m + j);
      for (int k = 0; k < j; k++) t -= IKW(c, A + i * m + k) * IKW(c, A + j * m + k);
      IKW(c, A + i * m + j) = t / d;
    }
  }
  for (int i = 0; i < m; i++) {
    double t = IKW(c, y + i);
    for (int k = 0; k < i; k++) t -= IKW(c, A + i * m + k) * IKW(c, y + k);
    IKW(c, y + i) = t / IKW(c, A + i * m + i);
  }
  for (int i = m - 1; i >= 0; i--) {
    double t = IKW(c, y + i);
    for (int k = i + 1; k < m; k++) t -= IKW(c, A + k * m + i) * IKW(c, y + k);
    IKW(c, y + i) = t / IKW(c, A + i * m + i);
  }
}

// delta of IKSolver.cpp:442-477 from the J and diff of the last ikEval: J^T diff in transpose mode, else the damped-least-squares step.
DEV void ikDelta(const IkCtx& c, bool useTranspose, double lambda) {
  const int n = c.L.n, P = c.L.P, J = c.L.J, m = c.L.m;
  if (useTranspose) {
    for (int d = 0; d < n; d++) {
      double s = 0.0;
      for (int p = 0; p < P; p++) s += IKW(c, J + p * n + d) * IKW(c, c.L.diff + p);
      IKW(c, c.L.delta + d) = s;
    }
    return;
  }
  if (P < n) {   // delta = J^T (J J^T + lambda I)^-1 diff
    for (int i = 0; i < P; i++) {
      for (int j = 0; j <= i; j++) {
        double s = 0.0;
        for (int d = 0; d < n; d++) s += IKW(c, J + i * n + d) * IKW(c, J + j * n + d);
        IKW(c, c.L.A + i * m + j) = i == j ? s + lambda : s;
      }
      IKW(c, c.L.y + i) = IKW(c, c.L.diff + i);
    }
    ikCholSolve(c);
    for (int d = 0; d < n; d++) {
      double s = 0.0;
      for (int p = 0; p < P; p++) s += IKW(c, J + p * n + d) * IKW(c, c.L.y + p);
      IKW(c, c.L.delta + d) = s;
    }
  } else {       // delta = (J^T J + lambda I)^-1 J^T diff
    for (int i = 0; i < n; i++) {
      for (int j = 0; j <= i; j++) {
        double s = 0.0;
        for (int p = 0; p < P; p++) s += IKW(c, J + p * n + i) * IKW(c, J + p * n + j);
        IKW(c, c.L.A + i * m + j) = i == j ? s + lambda : s;
      }
      double s = 0.0;
      for (int p = 0; p < P; p++) s += IKW(c, J + p * n + i) * IKW(c, c.L.diff + p);
      IKW(c, c.L.y + i) = s;
    }
    ikCholSolve(c);
    for (int d = 0; d < n; d++) IKW(c, c.L.delta + d) = IKW(c, c.L.y + d);
  }
}

// math::solveIK with maxRestarts = 1 for world b.  q_init [n][B] (null: zeros), q_out [n][B]; loss [B] and steps [B] may be null.
DEV void ikSolveWorld(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs, const DevKinEntry* __restrict__ entries,
                      const int32_t* __restrict__ path, int count, int nb, int n, int P, int64_t B, int64_t b, const double* __restrict__ target,
                      const double* __restrict__ q_init, IkConfig cfg, double* __restrict__ q_out, double* __restrict__ loss,
                      int32_t* __restrict__ steps, double* __restrict__ ws) {
  IkCtx c;
  c.bodies = bodies; c.dofs = dofs; c.entries = entries; c.path = path; c.count = count; c.nb = nb; c.B = B; c.b = b;
  c.target = target; c.ws = ws; c.L = ikLayout(n, P);
  const IkLayout& L = c.L;
  const double inf = __builtin_huge_val();
  for (int d = 0; d < n; d++) IKW(c, L.pos + d) = q_init ? q_init[(int64_t)d * B + b] : 0.0;
  for (int k = 0; k < P * n; k++) IKW(c, L.J + k) = 0.0;
  if (cfg.startClamped) ikClamp(c, L.pos);                         // IKSolver.cpp:225
  int evals = 0;
  for (int phase = 0; phase < 2; phase++) {
    const int maxSteps = phase == 0 ? IK_RESTART_STEPS : cfg.maxStepCount;
    // ---- refineIK (IKSolver.cpp:291-493) ----
    double lastError = inf, lr = 1.0;
    bool useTranspose = false, clamp = cfg.startClamped != 0;
    if (clamp) ikClamp(c, L.pos);
    for (int d = 0; d < n; d++) IKW(c, L.last + d) = IKW(c, L.pos + d);
    for (int i = 0; i < maxSteps; i++) {
      if (i > maxSteps - 5) clamp = true;
      const double currentError = ikEval<true>(c, L.pos);
      evals++;
      if (i > 0) {
        const double errorChange = currentError - lastError;
        if (currentError < 1e-21) { lastError = currentError; break; }
        if (errorChange > 0) {
          lr *= 0.5;
          if (lr < 1e-4) useTranspose = true;
          else if (!cfg.dontExitTranspose) useTranspose = false;
          if (cfg.lineSearch) {
            for (int d = 0; d < n; d++) IKW(c, L.pos + d) = IKW(c, L.last + d);
            if (clamp) ikClamp(c, L.pos);
          }
          if (lr < 1e-10) { lastError = currentError; break; }
        } else if (errorChange > -cfg.convergenceThreshold) {
          if (!useTranspose) {
            if (lr > 5e-5) lr = 5e-5;
            useTranspose = true;
          } else if (!clamp) {
            clamp = true;
          } else {
            break;
          }
        } else {
          lr *= 1.1;
          lastError = currentError;
        }
      }
      ikDelta(c, useTranspose, cfg.damping);
      for (int d = 0; d < n; d++) {
        const double p = IKW(c, L.pos + d);
        IKW(c, L.last + d) = p;
        IKW(c, L.pos + d) = p - lr * IKW(c, L.delta + d);
      }
      if (clamp) ikClamp(c, L.pos);
    }
    // solveIK keeps the restart's result unless its loss is not below infinity (:251-254): then it goes on from initialPos as it was given
    if (phase == 0 && !(lastError < inf))
      for (int d = 0; d < n; d++) IKW(c, L.pos + d) = q_init ? q_init[(int64_t)d * B + b] : 0.0;
  }
  const double finalError = ikEval<false>(c, L.pos);
  for (int d = 0; d < n; d++) q_out[(int64_t)d * B + b] = IKW(c, L.pos + d);
  if (loss) loss[b] = finalError;
  if (steps) steps[b] = evals;
}

}  // namespace NBL_NS
