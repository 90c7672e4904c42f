// krcn_cgn_state.hpp — the state rule of krcn_cubic_cg (krcn_cubic_cg.hip,
// kernels: krcn_cgn.hpp): scipy's scalar Newton on phi(lam) = lam^2 - M^2
// ||s(lam)||^2 (cubic_newton's loop, krcn_cubic.hpp) with every (H + lam I)^{-1}
// applied by conjugate gradients, as one chain of ticks.  Plain C++17, no HIP
// header: the kernels call these functions, the host reads the record through
// them, and tests/native/cgn_state_check.cpp walks them with g++ under the
// host sanitizers.
//
// A tick is one CG iteration and a turn.  The turn (cgn_turn) is the only
// writer of the state; it sees the iteration's p.q and r.r, and, when the
// solve has ended (cgn_solve_ended: converged, cg_maxiter reached, or nothing
// to iterate on), the sums the direction kernel formed in its ended branch.
// One phase says which solve is running:
//   solve_g  y = (H + lam I)^{-1} g into the caller's s; ends with y.y
//   solve_y  z = (H + lam I)^{-1} y; ends with y.z
//   close    y at the root; ends with y.y and g.y, s = -y
//   fail     a status 1, 2 or 4 was met: the next tick zeroes s
//   done     every later launch returns at once
// The vector part of a turn does not wait for the decision: solve_g always
// hands y to solve_y (z = 0, r = p = y) and solve_y always restarts from g
// (s = 0, r = p = g).  The two decisions that do not fit — phi(lam) == 0 after
// solve_g, where the closing solve starts from g, and a failure — go through
// one tick whose solve is skipped (skip = 1): its direction kernel does the
// vector part of the phase the turn chose, and the next turn moves on.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef KRCN_HD
#ifdef __HIPCC__
#define KRCN_HD __host__ __device__
#else
#define KRCN_HD
#endif
#endif

namespace krcn {

enum { kCgnSolveG = 0, kCgnSolveY = 1, kCgnClose = 2, kCgnFail = 3, kCgnDone = 4 };

// solver_status (the kCubic* values of krcn_cubic.hpp, which static_asserts them equal)
enum { kCgnOk = 0, kCgnNotPd = 1, kCgnDerZero = 2, kCgnItMax = 3, kCgnNonFinite = 4 };

// The call's scalars, passed to the kernels by value.
struct CgnParams {
  double M, l2, r0, eps, cg_rtol;
  int it_max, cg_maxiter;
};

// Device state, and the mapped host record the turn that ends the chain writes.
struct CgnState {
  int done;             // shares its offset with LanczosState::done (SrcGuard reads it)
  int phase;            // kCgn*
  int skip;             // the current solve has nothing to iterate on: the tick's update is skipped and its
                        //   direction kernel takes the ended branch
  int found;            // the root is fixed (phi == 0): solve_y passes through to close
  int k;                // updates of x in the current solve
  int itr;              // Newton iterations completed
  int solver_it;
  int solver_status;    // kCgn*
  int cg_solves;        // solves started
  int cg_unconverged;   // solves that ended at cg_maxiter
  int64_t cg_iterations;   // updates of x over all solves
  int64_t ticks;        // turns taken
  double lam;           // the Newton iterate the current solve is shifted by; after the end: the root
  double shift;         // l2 + lam (EpiCgnQ reads it)
  double rho;           // r.r of the current solve's iterate
  double atol;          // cg_rtol ||rhs||
  double gg;            // g.g, formed once
  double fval;          // phi(lam), between solve_g's turn and solve_y's
  double pq;            // p.q of the tick (k_cgn_update's lead thread writes it, the turn reads it)
  double model_decrease;
  double s_norm;
};
static_assert(sizeof(CgnState) % sizeof(double) == 0, "the state heads a block of doubles");

KRCN_HD inline bool cgn_finite(double v) { return v - v == 0.0; }

// x = 0, r = p = rhs is in place (or queued in the same tick): rho_0 = rhs.rhs,
// atol = cg_rtol ||rhs|| (k_cg_init's expressions); a zero rhs ends at once with x = 0.
KRCN_HD inline void cgn_begin_solve(CgnState& s, const CgnParams& a, int phase, double lam, double rr) {
  s.phase = phase;
  s.lam = lam;
  s.shift = a.l2 + lam;
  s.k = 0;
  s.rho = rr;
  s.atol = a.cg_rtol * sqrt(rr);
  s.skip = rr == 0.0 ? 1 : 0;
  s.cg_solves += 1;
}

KRCN_HD inline void cgn_fail(CgnState& s, int status) {
  s.phase = kCgnFail;
  s.solver_status = status;
  s.skip = 1;
}

// The state after k_cg_begin on g (s = 0, r = p = g) and the sum of its partials.
KRCN_HD inline CgnState cgn_start(const CgnParams& a, double gg) {
  CgnState s{};
  s.gg = gg;
  s.lam = a.r0;
  if (!cgn_finite(gg)) cgn_fail(s, kCgnNonFinite);
  else cgn_begin_solve(s, a, kCgnSolveG, a.r0, gg);
  return s;
}

// Has the current solve ended with this tick?  rho_new is r.r after the
// tick's update (unused under skip).  The direction kernel and the turn both
// ask, with the same arguments.
KRCN_HD inline bool cgn_solve_ended(int skip, int k, int cg_maxiter, double atol, double rho_new) {
  return skip || sqrt(rho_new) < atol || k + 1 >= cg_maxiter;
}

// One turn.  rho_new: r.r after the tick's update; sum_a, sum_b: what the
// direction kernel's ended branch formed for s.phase (solve_g: y.y, -;
// solve_y: y.z, -; close: y.y, g.y), read only when the solve has ended.
KRCN_HD inline CgnState cgn_turn(const CgnState& s, const CgnParams& a, double rho_new, double sum_a, double sum_b) {
  CgnState n = s;
  if (s.phase == kCgnDone) return n;
  n.ticks = s.ticks + 1;
  if (s.phase == kCgnFail) {   // this tick's direction kernel zeroed s
    n.phase = kCgnDone;
    n.done = 1;
    return n;
  }
  if (!s.skip) {
    if (!cgn_finite(s.pq)) return cgn_fail(n, kCgnNonFinite), n;
    if (s.pq <= 0.0 && s.rho > 0.0) return cgn_fail(n, kCgnNotPd), n;
    if (!cgn_finite(rho_new)) return cgn_fail(n, kCgnNonFinite), n;
    n.k = s.k + 1;
    n.cg_iterations = s.cg_iterations + 1;
    n.rho = rho_new;
    if (!cgn_solve_ended(0, s.k, a.cg_maxiter, s.atol, rho_new)) return n;
    if (!(sqrt(rho_new) < s.atol)) n.cg_unconverged = s.cg_unconverged + 1;
  }
  const double M2 = a.M * a.M;
  const double p0 = s.lam;
  if (s.phase == kCgnSolveG) {
    const double nrm = sqrt(sum_a);
    const double fval = p0 * p0 - M2 * (nrm * nrm);
    if (!cgn_finite(fval)) return cgn_fail(n, kCgnNonFinite), n;
    n.fval = fval;
    if (fval == 0.0) {          // newton() returns p0: the closing solve restarts from g, through solve_y's vector part
      n.solver_it = s.itr;
      n.found = 1;
      n.phase = kCgnSolveY;
      n.skip = 1;
    } else {
      cgn_begin_solve(n, a, kCgnSolveY, p0, sum_a);
    }
    return n;
  }
  if (s.phase == kCgnSolveY) {
    if (s.found) return cgn_begin_solve(n, a, kCgnClose, p0, s.gg), n;
    const double dnorm2 = -2.0 * sum_a;
    const double fder = 2.0 * p0 - M2 * dnorm2;
    n.solver_it = s.itr + 1;
    if (fder == 0.0) return cgn_fail(n, kCgnDerZero), n;
    const double p = p0 - s.fval / fder;
    if (!cgn_finite(p)) return cgn_fail(n, kCgnNonFinite), n;
    if (p == p0 || fabs(p - p0) <= a.eps) {
      n.found = 1;
      cgn_begin_solve(n, a, kCgnClose, p, s.gg);
    } else if (s.itr + 1 >= a.it_max) {   // the last p is the root, as root_scalar returns it
      n.solver_status = kCgnItMax;
      cgn_begin_solve(n, a, kCgnClose, p, s.gg);
    } else {
      n.itr = s.itr + 1;
      cgn_begin_solve(n, a, kCgnSolveG, p, s.gg);
    }
    return n;
  }
  // close: the host's closing expressions, with g.s = -(g.y) (negation is exact)
  const double ns = sqrt(sum_a);
  const double gs = -sum_b;
  n.s_norm = ns;
  n.model_decrease = p0 / 2.0 * (ns * ns) - a.M / 3.0 * (ns * ns * ns) - gs / 2.0;
  n.phase = kCgnDone;
  n.done = 1;
  return n;
}

// Ticks a chain can need: at most 2 it_max + 1 solves of at most cg_maxiter
// ticks each (a skipped solve takes one), and the two pass-through ticks.
KRCN_HD inline int64_t cgn_tick_bound(int it_max, int cg_maxiter) {
  return (2 * int64_t(it_max) + 1) * (int64_t(cg_maxiter) + 1);
}

}  // namespace krcn
