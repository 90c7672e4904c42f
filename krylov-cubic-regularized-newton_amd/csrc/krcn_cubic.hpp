// krcn_cubic.hpp — the device side of a one-call Krylov-CRN step: the m x m
// tridiagonal cubic subproblem in one workgroup, and the guarded kernels of a
// backtracking trial (optimizer/cubic.py: cubic_solver_root_tridiag :76-123,
// Cubic_Krylov_LS.step :239-270; reference cubic.py:40-75, :265-309).
//
// Control stays on the device, as in krcn_cg.hpp: CrnState.done is set by the
// judge kernel of the trial that ends the line search (or by the subproblem
// kernel when its solve fails), and every later launch of the chain returns at
// once, so the host enqueues trials in batches and reads the state once per
// batch (krcn_crn_chain.hpp: the host side of every such chain).  The arithmetic of the subproblem is fp64 whatever the handle's dtype.
#pragma once
#include <cstddef>

#include "krcn.h"
#include "krcn_kernels.hpp"

namespace krcn {

constexpr int kCubicMaxM = 2044;   // = kLzMaxM (krcn_internal.hpp static_asserts it)

// Solver status of the subproblem (krcn_crn_info.solver_status); kCubicNonFinite
// is krcn_cubic_cg's alone (a non-finite lam, rho or p.q: krcn_cgn_state.hpp).
enum { kCubicOk = 0, kCubicNotPd = 1, kCubicDerZero = 2, kCubicItMax = 3, kCubicNonFinite = 4 };

struct CrnState {
  int done;            // shares its offset with LanczosState::done (SrcGuard reads it)
  int accepted;        // the trial that set done met value_new <= value - model_decrease
  int trials;          // backtracking trials after the first solve
  int solver_it;       // Newton iterations of the last solve
  int solver_status;   // kCubic*
  int m_eff;           // basis vectors kept by the recurrence (cubic.py:105-108)
  int pad0, pad1;
  double M;            // regularisation of the next (after done: the last) solve
  double lam;          // its root
  double model_decrease;
  double value_new;
  double gnorm;        // ||g||: the subproblem's g is gnorm e1
  double dx2;          // ||x_new - x||^2 (k_crn_dx_finish, after done)
};
static_assert(offsetof(CrnState, done) == offsetof(LanczosState, done), "SrcGuard reads done");
static_assert(sizeof(CrnState) % sizeof(double) == 0, "the state heads a block of doubles");

// Trials per submission of a chain (crn_run_chain, krcn_crn_chain.hpp): the
// first holds trials 0 and 1, every later one kCrnBatch (a
// guarded trial that finds done set costs its launches only, a host round trip
// costs a synchronisation).
constexpr int kCrnFirstBatch = 2;
constexpr int kCrnBatch = 4;

// Start of a chain.  lz != nullptr: the block k_lz_final packed (state,
// alphas[0..m), betas[0..m-1)) becomes the subproblem's input, with the
// reference's truncation rule (cubic.py:105-108: a breakdown before j = m - 2
// keeps j_break + 1 vectors).  lz == nullptr: alphas / betas were staged by
// the caller, m_eff = m and ||g|| = gnorm.
[[maybe_unused]] static __global__ __launch_bounds__(kNT) void k_crn_begin(const double* __restrict__ lz, int m,
                                                                          double gnorm, double M0, CrnState* st,
                                                                          double* __restrict__ al,
                                                                          double* __restrict__ be) {
  int m_eff = m;
  if (lz) {
    const LanczosState ls = *reinterpret_cast<const LanczosState*>(lz);
    if (ls.done && ls.j_break < m - 2) m_eff = ls.j_break + 1;
    gnorm = ls.gnorm;
    for (int i = threadIdx.x; i < m_eff; i += kNT) al[i] = lz[4 + i];
    for (int i = threadIdx.x; i + 1 < m_eff; i += kNT) be[i] = lz[4 + m + i];
  }
  if (threadIdx.x == 0) {
    CrnState s{};
    s.m_eff = m_eff;
    s.M = M0;
    s.gnorm = gnorm;
    *st = s;
  }
}

// The serial sweeps below run on one thread over LDS.  Each walks its vectors
// in chunks of kCubicChunk elements: the chunk's operands are loaded into
// registers first (independent LDS loads, one wait), the dependent chain then
// runs register to register, and the results are stored together — the same
// operations in the same order as the element-at-a-time loop, without an LDS
// round trip inside the chain.
constexpr int kCubicChunk = 8;

// (T + lam I) = L D L^T by dpttrf's recurrence, left to right, on d = alphas +
// lam and e = betas (thread 0; both in LDS).  A pivot <= 0 or non-finite:
// false (the host raises LinAlgError on dpttrf's info != 0).
__device__ __forceinline__ bool cubic_factor(int m, double* d, double* e) {
  constexpr int C = kCubicChunk;
  double di = d[0];
  int i = 0;
  for (; i + C < m; i += C) {
    double ev[C], dv[C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
      ev[k] = e[i + k];
      dv[k] = d[i + 1 + k];
    }
#pragma unroll
    for (int k = 0; k < C; ++k) {
      if (!(di > 0.0) || isinf(di)) return false;
      const double ei = ev[k];
      const double li = ei / di;
      ev[k] = li;
      di = dv[k] - li * ei;
      dv[k] = di;
    }
#pragma unroll
    for (int k = 0; k < C; ++k) {
      e[i + k] = ev[k];
      d[i + 1 + k] = dv[k];
    }
  }
  for (; i + 1 < m; ++i) {
    if (!(di > 0.0) || isinf(di)) return false;
    const double ei = e[i];
    const double li = ei / di;
    e[i] = li;
    di = d[i + 1] - li * ei;
    d[i + 1] = di;
  }
  return di > 0.0 && !isinf(di);
}

// dptts2's forward substitution b[i] -= b[i-1] e[i-1] (thread 0).
__device__ __forceinline__ void cubic_forward(int m, const double* e, double* b) {
  constexpr int C = kCubicChunk;
  double prev = b[0];
  int i = 1;
  for (; i + C <= m; i += C) {
    double ev[C], bv[C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
      ev[k] = e[i - 1 + k];
      bv[k] = b[i + k];
    }
#pragma unroll
    for (int k = 0; k < C; ++k) {
      prev = bv[k] - prev * ev[k];
      bv[k] = prev;
    }
#pragma unroll
    for (int k = 0; k < C; ++k) b[i + k] = bv[k];
  }
  for (; i < m; ++i) {
    prev = b[i] - prev * e[i - 1];
    b[i] = prev;
  }
}

// dptts2's backward substitution on q[i] = b[i] / d[i] (formed by all
// threads): b[m-1] = q[m-1], b[i] = q[i] - b[i+1] e[i] (thread 0).
__device__ __forceinline__ void cubic_backward(int m, const double* e, double* b) {
  constexpr int C = kCubicChunk;
  double next = b[m - 1];
  int i = m - 2;
  for (; i - (C - 1) >= 0; i -= C) {
    double ev[C], bv[C];
#pragma unroll
    for (int k = 0; k < C; ++k) {
      ev[k] = e[i - k];
      bv[k] = b[i - k];
    }
#pragma unroll
    for (int k = 0; k < C; ++k) {
      next = bv[k] - next * ev[k];
      bv[k] = next;
    }
#pragma unroll
    for (int k = 0; k < C; ++k) b[i - k] = bv[k];
  }
  for (; i >= 0; --i) {
    next = b[i] - next * e[i];
    b[i] = next;
  }
}

struct CubicSolve {
  int its, status;
  double root, dec;
  double ns;   // ||s|| of the closing solve (0 when it failed)
};

// The scalar Newton loop of the cubic subproblem, shared by the tridiagonal
// kernels (cubic_tridiag_solve) and the dense one (krcn_cubic_dense.hpp):
// scipy's newton() on phi(lam) = lam^2 - M^2 ||s(lam)||^2 from r0 (fval == 0
// returns p0, fder == 0 is an error, p = p0 - fval / fder, converged when
// |p - p0| <= eps, at most it_max iterations and then the last p with "not
// converged"), and the host's closing expressions.  The caller supplies the
// linear algebra over y = (H + lam I)^{-1} g = -s(lam) (negation is exact and
// the solves are odd, so phi, dphi and s have the host expressions' values):
//   solve_g(lam)  factor H + lam I and solve for y; false: not positive definite
//   solve_y()     z = (H + lam I)^{-1} y with the factorisation solve_g left
//   dot_yy / dot_yz   the block's fixed-order sums
//   g_dot_s()     np.dot(g, s) of the closing solve
//   store_s()     writes s = -y out
// Every thread of the workgroup calls it with the same arguments and gets the
// same result; the loop is bounded by it_max.
template <class SolveG, class SolveY, class DotYY, class DotYZ, class GDotS, class StoreS>
__device__ __forceinline__ CubicSolve cubic_newton(double M, double r0, double eps, int it_max, SolveG&& solve_g,
                                                   SolveY&& solve_y, DotYY&& dot_yy, DotYZ&& dot_yz,
                                                   GDotS&& g_dot_s, StoreS&& store_s) {
  int status = kCubicOk, its = 0;
  double p0 = r0, root = r0;
  bool found = false;
  const double M2 = M * M;
  for (int itr = 0; itr < it_max; ++itr) {
    if (!solve_g(p0)) {
      status = kCubicNotPd;
      break;
    }
    const double nrm = sqrt(dot_yy());
    const double fval = p0 * p0 - M2 * (nrm * nrm);
    if (fval == 0.0) {
      root = p0;
      its = itr;
      found = true;
      break;
    }
    solve_y();
    const double dnorm2 = -2.0 * dot_yz();
    const double fder = 2.0 * p0 - M2 * dnorm2;
    if (fder == 0.0) {
      root = p0;
      its = itr + 1;
      status = kCubicDerZero;
      break;
    }
    const double p = p0 - fval / fder;
    its = itr + 1;
    root = p;
    if (p == p0 || fabs(p - p0) <= eps) {
      found = true;
      break;
    }
    p0 = p;
  }
  if (status == kCubicOk && !found) status = kCubicItMax;   // the last p is the root, as root_scalar returns it

  double dec = 0.0, ns = 0.0;
  if (status == kCubicOk || status == kCubicItMax) {
    if (!solve_g(root)) {
      status = kCubicNotPd;
    } else {
      ns = sqrt(dot_yy());
      const double gs = g_dot_s();
      dec = root / 2.0 * (ns * ns) - M / 3.0 * (ns * ns * ns) - gs / 2.0;
      store_s();
    }
  }
  return CubicSolve{its, status, root, dec, ns};
}

// The tridiagonal cubic subproblem argmin_s <g,s> + 1/2 s^T T s + M/3 ||s||^3,
// T = tridiag(be, al, be), g = gnorm e1 (cubic_solver_root_tridiag): scipy's
// scalar Newton on phi(lam) = lam^2 - M^2 ||s(lam)||^2 from r0 (cubic_newton
// above), one LDL^T per lam shared by phi and dphi, and the host's closing
// expressions.  One workgroup; the recurrences run on thread 0 over
// LDS, the elementwise divisions and the sums on all threads.  Works with
// y = (T + lam I)^{-1} g = -s(lam): negation is exact and the solves are odd,
// so phi, dphi and s have the host expressions' values.
// Every loop is bounded by it_max or m; no other workgroup is waited on.
// The body is a device function of one workgroup (every thread calls it with
// the same arguments and gets the same result): k_cubic_tridiag runs it on the
// single chain's state, k_crnb_solve (krcn_crnb.hpp) on one column per
// workgroup.  s_g receives the m entries of s when the solve succeeded.
__device__ __forceinline__ CubicSolve cubic_tridiag_solve(int m, double M, double gnorm,
                                                          const double* __restrict__ al_g,
                                                          const double* __restrict__ be_g,
                                                          double* __restrict__ s_g, double r0, double eps,
                                                          int it_max) {
  __shared__ double al[kCubicMaxM], be[kCubicMaxM], dd[kCubicMaxM], ee[kCubicMaxM], y[kCubicMaxM], z[kCubicMaxM];
  __shared__ double sm[kNT / 64];
  __shared__ int ok_sm;
  const int tid = threadIdx.x;
  for (int i = tid; i < m; i += kNT) al[i] = al_g[i];
  for (int i = tid; i + 1 < m; i += kNT) be[i] = be_g[i];
  __syncthreads();

  // y = (T + lam I)^{-1} (gnorm e1); false when T + lam I is not positive definite
  auto solve_g = [&](double lam) -> bool {
    for (int i = tid; i < m; i += kNT) {
      dd[i] = al[i] + lam;
      if (i + 1 < m) ee[i] = be[i];
      y[i] = i == 0 ? gnorm : 0.0;   // the right-hand side gnorm e1
    }
    __syncthreads();
    if (tid == 0) {
      const bool ok = cubic_factor(m, dd, ee);
      ok_sm = ok;
      if (ok) cubic_forward(m, ee, y);
    }
    __syncthreads();
    const bool ok = ok_sm != 0;
    if (!ok) return false;
    for (int i = tid; i < m; i += kNT) y[i] = y[i] / dd[i];
    __syncthreads();
    if (tid == 0) cubic_backward(m, ee, y);
    __syncthreads();
    return true;
  };
  // z = (T + lam I)^{-1} y with the factorisation solve_g left in dd / ee
  auto solve_y = [&]() {
    for (int i = tid; i < m; i += kNT) z[i] = y[i];
    __syncthreads();
    if (tid == 0) cubic_forward(m, ee, z);
    __syncthreads();
    for (int i = tid; i < m; i += kNT) z[i] = z[i] / dd[i];
    __syncthreads();
    if (tid == 0) cubic_backward(m, ee, z);
    __syncthreads();
  };
  auto dot = [&](const double* a, const double* b) -> double {
    double acc = 0.0;
    for (int i = tid; i < m; i += kNT) acc += a[i] * b[i];
    return block_sum(acc, sm);
  };

  return cubic_newton(
      M, r0, eps, it_max, solve_g, solve_y, [&]() { return dot(y, y); }, [&]() { return dot(y, z); },
      [&]() { return gnorm * (0.0 - y[0]); },   // np.dot(g, s): g = gnorm e1, s = -y
      [&]() {
        for (int i = tid; i < m; i += kNT) s_g[i] = 0.0 - y[i];
      });
}

[[maybe_unused]] static __global__ __launch_bounds__(kNT) void k_cubic_tridiag(CrnState* st,
                                                                              const double* __restrict__ al_g,
                                                                              const double* __restrict__ be_g,
                                                                              double* __restrict__ s_g, double r0,
                                                                              double eps, int it_max, CrnState* res) {
  if (st->done) return;
  const CubicSolve r = cubic_tridiag_solve(st->m_eff, st->M, st->gnorm, al_g, be_g, s_g, r0, eps, it_max);
  if (threadIdx.x == 0) {
    st->solver_it = r.its;
    st->solver_status = r.status;
    st->lam = r.root;
    st->model_decrease = r.dec;
    if (r.status == kCubicNotPd || r.status == kCubicDerZero) st->done = 1;   // nothing to try: the chain ends here
    *res = *st;
  }
}

// x_new = x + V^T s over the state's m_eff basis rows with s in device memory:
// k_basis_combine's sums in its order, skipped once the chain has ended.
template <typename T>
__global__ __launch_bounds__(kNT) void k_basis_combine_dev(int64_t d, const CrnState* st, const T* __restrict__ V,
                                                           const double* __restrict__ s, const T* __restrict__ x,
                                                           T* __restrict__ xn) {
  if (st->done) return;
  const int m = st->m_eff;
  __shared__ T ss[kBasisMaxM];
  for (int j = threadIdx.x; j < m; j += kNT) ss[j] = T(s[j]);
  __syncthreads();
  for (int64_t i = int64_t(blockIdx.x) * kNT + threadIdx.x; i < d; i += int64_t(gridDim.x) * kNT) {
    T acc = T(0);
    int j = 0;
    for (; j + kBasisU <= m; j += kBasisU) {
      T v[kBasisU];
#pragma unroll
      for (int u = 0; u < kBasisU; ++u) v[u] = V[int64_t(j + u) * d + i];
#pragma unroll
      for (int u = 0; u < kBasisU; ++u) acc += v[u] * ss[j + u];
    }
    for (; j < m; ++j) acc += V[int64_t(j) * d + i] * ss[j];
    xn[i] = x[i] + acc;
  }
}

// k_loss_terms, skipped once the chain has ended.
template <typename T>
__global__ __launch_bounds__(kNT) void k_loss_terms_guard(int64_t n, const T* __restrict__ Ax,
                                                          const T* __restrict__ b, double* __restrict__ partials,
                                                          const CrnState* st) {
  if (st->done) return;
  double acc = 0.0;
  for (int64_t i = int64_t(blockIdx.x) * kNT + threadIdx.x; i < n; i += int64_t(gridDim.x) * kNT) {
    const T a = Ax[i];
    const T t = (T(1) - b[i]) * a - logsig(a);
    acc += double(t);
  }
  __shared__ double sm[kNT / 64];
  const double t = block_sum(acc, sm);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// k_reduce2's partials of ||a||^2 (b == nullptr) or ||a - b||^2, run while the
// chain's done flag equals `when` (0: inside a trial; 1: the step length after it).
template <typename T>
__global__ __launch_bounds__(kNT) void k_sqnorm_guard(int64_t n, const T* __restrict__ a, const T* __restrict__ b,
                                                      double* __restrict__ partials, const CrnState* st, int when) {
  if ((st->done != 0) != (when != 0)) return;
  double acc = 0.0;
  for (int64_t i = int64_t(blockIdx.x) * kNT + threadIdx.x; i < n; i += int64_t(gridDim.x) * kNT) {
    if (b) {
      const T t = a[i] - b[i];
      acc += double(t) * double(t);
    } else {
      const double t = a[i];
      acc += t * t;
    }
  }
  __shared__ double sm[kNT / 64];
  const double t = block_sum(acc, sm);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

// The judge of a trial (one block): value_new = mean + l2 / 2 * norm ** 2 as
// LogisticRegression._value forms it (krcn_loss_mean's and krcn_diff_norm's
// partial sums in their order), then the line search's test (cubic.py:293-303):
// accept, stop at the cap, or divide M by beta for the next trial.
[[maybe_unused]] static __global__ __launch_bounds__(kNT) void k_crn_judge(const double* __restrict__ pl, int Pl,
                                                                          const double* __restrict__ pn, int Pn,
                                                                          double n_global, double l2, double value,
                                                                          double ls_beta, int max_trials, CrnState* st,
                                                                          CrnState* res) {
  if (st->done) return;
  __shared__ double sm[kNT / 64];
  double vnew = sum_partials(pl, Pl, sm) / n_global;
  if (l2 != 0.0) {
    const double nrm = sqrt(sum_partials(pn, Pn, sm));
    vnew = vnew + l2 / 2.0 * (nrm * nrm);
  }
  if (threadIdx.x != 0) return;
  st->value_new = vnew;
  if (!(vnew > value - st->model_decrease)) {
    st->accepted = 1;
    st->done = 1;
  } else if (st->trials >= max_trials) {
    st->done = 1;
  } else {
    st->M = st->M / ls_beta;
    st->trials = st->trials + 1;
  }
  *res = *st;
}

// ||x_new - x||^2 from k_sqnorm_guard's partials once the chain has ended.
[[maybe_unused]] static __global__ __launch_bounds__(kNT) void k_crn_dx_finish(const double* __restrict__ partials,
                                                                              int P, CrnState* st, CrnState* res) {
  if (!st->done) return;
  __shared__ double sm[kNT / 64];
  const double s = sum_partials(partials, P, sm);
  if (threadIdx.x == 0) {
    st->dx2 = s;
    res->dx2 = s;
  }
}

}  // namespace krcn
