// krcn_cgn.hpp — the kernels of krcn_cubic_cg (krcn_cubic_cg.hip): the cubic
// subproblem of the full-space CRN with every (H + lam I)^{-1} applied by
// conjugate gradients, Newton iteration included, as one chain of ticks
// (optimizer/cubic.py Cubic_LS.cubic_solver_root_CG; reference cubic.py:152-182).
// The state rule is krcn_cgn_state.hpp.
//
// A tick is krcn_cg_solve's iteration with the state read from the device —
//   pass 1 (EpiWeighted), pass 2 (EpiCgnQ: EpiCgQ with the shift T(st->shift))
//   k_cgn_update   k_cg_update's expressions on the current solve's x (s or z)
//   k_cgn_dir      k_cg_dir's, and in the ended branch the vector part of the turn
// — and one added single-workgroup launch:
//   k_cgn_turn     the sums of the ended branch, the scalar decision, the next solve
// so a CG iteration of the chain has the bits of krcn_cg_solve's, and the sums
// those of krcn_dot / krcn_diff_norm (k_reduce2's loop on vec_grid(d) blocks,
// sum_partials' fixed order).
//
// The flag rule.  k_cgn_turn is the only kernel that writes what another
// kernel branches on (done, skip, phase, k, rho, atol, shift), and it is a
// launch of its own at the end of the tick: every flag written during launch L
// is read from launch L + 1 onwards, never by a workgroup of L.  The one other
// state write, p.q by k_cgn_update's lead thread, is read by k_cgn_turn only.
// k_cgn_dir's workgroups agree on "ended" without a flag: each re-sums the r.r
// partials in the same order and asks cgn_solve_ended.
// Every loop is bounded by d or the partial count; no kernel waits on another
// workgroup; no atomics.
#pragma once
#include <cstddef>

#include "krcn_cg.hpp"
#include "krcn_cgn_state.hpp"
#include "krcn_cubic.hpp"

namespace krcn {

static_assert(offsetof(CgnState, done) == offsetof(LanczosState, done), "SrcGuard reads done");
static_assert(kCgnOk == kCubicOk && kCgnNotPd == kCubicNotPd && kCgnDerZero == kCubicDerZero &&
                  kCgnItMax == kCubicItMax && kCgnNonFinite == kCubicNonFinite,
              "krcn_cubic_cg_info.solver_status has krcn_crn_info's values");

constexpr int kCgnMaxGrid = 1024;   // vec_grid's cap: the ended branch's two partial arrays hold this many each

// EpiCgQ with the shift of the current solve, read once per workgroup.
template <typename T> struct EpiCgnQ {
  const T* p; T* q; T n; const CgnState* st; T shift;
  static constexpr bool kReduce = true;
  struct Pre { T pr; };
  template <class S> __device__ __forceinline__ void init(const S&) { shift = T(st->shift); }
  __device__ __forceinline__ Pre pre(int r) const { return Pre{p[r]}; }
  __device__ __forceinline__ double row(int r, T s, int, const Pre& a) const {
    const T v = s / n + shift * a.pr;
    q[r] = v;
    return double(a.pr) * double(v);
  }
};

// After k_cg_begin on g: g.g and the first solve's state.
[[maybe_unused]] static __global__ __launch_bounds__(kNT) void k_cgn_init(const double* __restrict__ partials, int P,
                                                                         CgnParams a, CgnState* st) {
  __shared__ double sm[kNT / 64];
  const double gg = sum_partials(partials, P, sm);
  if (threadIdx.x == 0) *st = cgn_start(a, gg);
}

// alpha = rho_k / p.q; x += alpha p; r -= alpha q; partials of r.r (k_cg_update).
template <typename T>
__global__ __launch_bounds__(kNT) void k_cgn_update(int64_t d, const double* __restrict__ pq_part, int P, CgnState* st,
                                                    T* __restrict__ s, T* __restrict__ z, T* __restrict__ r,
                                                    const T* __restrict__ p, const T* __restrict__ q,
                                                    double* __restrict__ rr_part) {
  if (st->done || st->skip) return;
  T* __restrict__ x = st->phase == kCgnSolveY ? z : s;
  __shared__ double sm[kNT / 64];
  const double pq = sum_partials(pq_part, P, sm);
  const T alpha = T(st->rho / pq);
  double acc = 0.0;
  for (int64_t i = int64_t(blockIdx.x) * kNT + threadIdx.x; i < d; i += int64_t(gridDim.x) * kNT) {
    x[i] = x[i] + alpha * p[i];
    const T ri = r[i] - alpha * q[i];
    r[i] = ri;
    acc += double(ri) * double(ri);
  }
  const double t = block_sum(acc, sm);
  if (threadIdx.x == 0) rr_part[blockIdx.x] = t;
  if (blockIdx.x == 0 && threadIdx.x == 0) st->pq = pq;
}

// rho_{k+1} = r.r; the solve goes on: p = p beta + r (k_cg_dir).  It has ended:
// the sums its turn needs and the next solve's vectors, by phase —
//   solve_g  partials of y.y;           z = 0, r = p = y      (y is s)
//   solve_y  partials of y.z;           s = 0, r = p = g
//   close    partials of y.y and g.y;   s = -y
//   fail     s = 0
template <typename T>
__global__ __launch_bounds__(kNT) void k_cgn_dir(int64_t d, int cg_maxiter, const double* __restrict__ rr_part, int P,
                                                 const CgnState* st, const T* __restrict__ g, T* __restrict__ s,
                                                 T* __restrict__ z, T* __restrict__ r, T* __restrict__ p,
                                                 double* __restrict__ pt) {
  if (st->done) return;
  const int skip = st->skip, phase = st->phase;
  __shared__ double sm[kNT / 64];
  const double rho = skip ? 0.0 : sum_partials(rr_part, P, sm);
  const int64_t i0 = int64_t(blockIdx.x) * kNT + threadIdx.x, step = int64_t(gridDim.x) * kNT;
  if (!cgn_solve_ended(skip, st->k, cg_maxiter, st->atol, rho)) {
    const T beta = T(rho / st->rho);
    for (int64_t i = i0; i < d; i += step) p[i] = p[i] * beta + r[i];
    return;
  }
  double a = 0.0, b = 0.0;
  if (phase == kCgnSolveG) {
    for (int64_t i = i0; i < d; i += step) {
      const T y = s[i];
      const double t = y;
      a += t * t;
      z[i] = T(0);
      r[i] = y;
      p[i] = y;
    }
  } else if (phase == kCgnSolveY) {
    for (int64_t i = i0; i < d; i += step) {
      const T gi = g[i];
      a += double(s[i]) * double(z[i]);
      s[i] = T(0);
      r[i] = gi;
      p[i] = gi;
    }
  } else if (phase == kCgnClose) {
    for (int64_t i = i0; i < d; i += step) {
      const T y = s[i];
      const double t = y;
      a += t * t;
      b += double(g[i]) * double(y);
      s[i] = -y;
    }
  } else {
    for (int64_t i = i0; i < d; i += step) s[i] = T(0);
  }
  const double ta = block_sum(a, sm);
  const double tb = block_sum(b, sm);
  if (threadIdx.x == 0) {
    pt[blockIdx.x] = ta;
    pt[kCgnMaxGrid + blockIdx.x] = tb;
  }
}

// The turn: one workgroup re-sums what the tick left, thread 0 applies the
// state rule; the turn that ends the chain also writes the mapped host record.
[[maybe_unused]] static __global__ __launch_bounds__(kNT) void k_cgn_turn(CgnParams par,
                                                                         const double* __restrict__ rr_part, int P,
                                                                         const double* __restrict__ pt, CgnState* st,
                                                                         CgnState* res) {
  const CgnState s = *st;
  if (s.done) return;
  __shared__ double sm[kNT / 64];
  const double rho = s.skip ? 0.0 : sum_partials(rr_part, P, sm);
  double a = 0.0, b = 0.0;
  if (cgn_solve_ended(s.skip, s.k, par.cg_maxiter, s.atol, rho)) {
    a = sum_partials(pt, P, sm);
    if (s.phase == kCgnClose) b = sum_partials(pt + kCgnMaxGrid, P, sm);
  }
  if (threadIdx.x == 0) {
    const CgnState n = cgn_turn(s, par, rho, a, b);
    *st = n;
    if (n.done) *res = n;
  }
}

}  // namespace krcn
