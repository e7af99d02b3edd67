// ik_grad_dev.hpp — the vector-Jacobian product of one world's inverse-kinematics solve (nbl_ik_solve_vjp): the gradient of a loss with
// respect to the TARGET, given its gradient with respect to the positions q* the solve returned.  The reference has no such gradient;
// nothing here restates it.
//
// Plain C++ like ik_dev.hpp (the tests compile this header for the host: tests/host_shim/ik_grad_shim.cpp).  It reuses ik_dev.hpp's
// Jacobian builder (ikEval<true>) and Cholesky (ikCholSolve) as they are, on the same [slot][B] workspace (IkLayout): ONE WORLD PER LANE,
// every index computed, no private arrays of its own, no atomics, no cross-lane operations.
//
// The convention (include/nimble_amd.h states it for callers): with J = IKMapping::getPosJacobian at q* and F the FREE coordinates - a
// coordinate is clamped when q*_i equals a finite pos_lo_i or pos_hi_i bit for bit, which is what ikClamp leaves behind -,
//     grad_t = J_F (J_F^T J_F + mu I)^-1 (grad_q)_F  =  (J_F J_F^T + mu I)^-1 J_F (grad_q)_F,
// the Gauss-Newton sensitivity of min |rows(q) - t|^2 over the free coordinates; the second-order term sum_k (r - t)_k grad^2 r_k is left
// out (it vanishes where the target is met).  The SMALLER of the two forms is factored, min(P, |F|) on a side (for P = |F| the second,
// as ikDelta does for P = n).  mu > 0 is the caller's Tikhonov term, not the solver's damping.
#pragma once
#include "ik_dev.hpp"

namespace NBL_NS {

// q, grad_q [n][B]; grad_target [P][B] (accumulate: added to); free_count [B] or null; ws: IkLayout(n, P).total slots, [slot][B].
// Slots: pos = q, then J's columns and grad_q are compacted IN PLACE onto the free coordinates (J keeps its row stride n, its first
// |F| columns count; (grad_q)_F goes to `last`), A and y take the normal matrix and the right-hand side.
DEV void ikVjpWorld(const DevBody* __restrict__ bodies, const DevDof* __restrict__ dofs, const DevKinEntry* __restrict__ entries,
                    const int32_t* __restrict__ path, int count, int nb, int n, int P, int64_t B, int64_t b, const double* __restrict__ q,
                    const double* __restrict__ grad_q, double mu, double* __restrict__ grad_target, int accumulate,
                    int32_t* __restrict__ free_count, double* __restrict__ ws) {
  IkCtx c;
  c.bodies = bodies; c.dofs = dofs; c.entries = entries; c.path = path; c.count = count; c.nb = nb; c.B = B; c.b = b;
  c.ws = ws; c.L = ikLayout(n, P);
  const IkLayout L = c.L;
  // ikEval subtracts a target from every row before it stores it: the zeroed diff slots stand in for one (it reads a row's slot before
  // it writes it), so no target is needed here
  c.target = ws + (int64_t)L.diff * B;
  for (int d = 0; d < n; d++) IKW(c, L.pos + d) = q[(int64_t)d * B + b];
  for (int p = 0; p < P; p++) IKW(c, L.diff + p) = 0.0;
  for (int k = 0; k < P * n; k++) IKW(c, L.J + k) = 0.0;
  ikEval<true>(c, L.pos);

  const double inf = __builtin_huge_val();
  int nf = 0;
  for (int d = 0; d < n; d++) {
    const double p = IKW(c, L.pos + d), lo = dofs[d].posLo, hi = dofs[d].posHi;
    if ((p == lo && lo != -inf) || (p == hi && hi != inf)) continue;   // clamped: no gradient passes through it
    IKW(c, L.last + nf) = grad_q[(int64_t)d * B + b];
    if (nf != d)
      for (int r = 0; r < P; r++) IKW(c, L.J + r * n + nf) = IKW(c, L.J + r * n + d);
    nf++;
  }
  if (free_count) free_count[b] = nf;
  if (nf == 0) {
    if (!accumulate)
      for (int r = 0; r < P; r++) grad_target[(int64_t)r * B + b] = 0.0;
    return;
  }
  const int m = P < nf ? P : nf;
  c.L.m = m;   // ikCholSolve's side and row stride
  if (P < nf) {   // (J_F J_F^T + mu I)^-1 J_F g_F
    for (int i = 0; i < P; i++) {
      for (int j = 0; j <= i; j++) {
        double s = 0.0;
        for (int d = 0; d < nf; d++) s += IKW(c, L.J + i * n + d) * IKW(c, L.J + j * n + d);
        IKW(c, L.A + i * m + j) = i == j ? s + mu : s;
      }
      double s = 0.0;
      for (int d = 0; d < nf; d++) s += IKW(c, L.J + i * n + d) * IKW(c, L.last + d);
      IKW(c, L.y + i) = s;
    }
    ikCholSolve(c);
    for (int r = 0; r < P; r++) {
      const double g = IKW(c, L.y + r);
      double* const out = grad_target + (int64_t)r * B + b;
      *out = accumulate ? *out + g : g;
    }
  } else {        // J_F (J_F^T J_F + mu I)^-1 g_F
    for (int i = 0; i < nf; i++) {
      for (int j = 0; j <= i; j++) {
        double s = 0.0;
        for (int r = 0; r < P; r++) s += IKW(c, L.J + r * n + i) * IKW(c, L.J + r * n + j);
        IKW(c, L.A + i * m + j) = i == j ? s + mu : s;
      }
      IKW(c, L.y + i) = IKW(c, L.last + i);
    }
    ikCholSolve(c);
    for (int r = 0; r < P; r++) {
      double g = 0.0;
      for (int d = 0; d < nf; d++) g += IKW(c, L.J + r * n + d) * IKW(c, L.y + d);
      double* const out = grad_target + (int64_t)r * B + b;
      *out = accumulate ? *out + g : g;
    }
  }
}

}  // namespace NBL_NS
