// krcn_crnb.hpp — the kernels of the batched Krylov-CRN step
// (krcn_crn_block.hip): k problems over one X advance one step of
// Cubic_Krylov_LS.step (optimizer/cubic.py:265-309) behind one call, the line
// search decided per column on the device.  The block forms of krcn_cubic.hpp's
// guarded trial kernels, over krcn_blz.hpp's (L, k) blocks.
//
// Lane mapping and reductions are krcn_blz.hpp's: K = the next power of two
// >= k, a lane group of K consecutive lanes owns a row of the block and its
// member c < k the column c, kBlzU rows a round on at most kBlzMaxGrid
// workgroups; per-column two-stage sums (blz_col_sum / blz_sum_partials), one
// partial per workgroup and column at p[b * K + c], no atomics.
//
// State: one double block, a CrnbHead followed by k CrnbCol records
// (krcn_crnb_state.hpp gives the transition).  Every launch of a trial returns
// at once in every workgroup when head.all_done is set; within a live chain a
// column that is no longer live is neither read for a decision nor stored.
// Per-column scalars (value, l2, r0, M) are read from the records in global
// memory by the lane that owns the column: no runtime-indexed private array.
#pragma once
#include "krcn_blz.hpp"
#include "krcn_crnb_state.hpp"
#include "krcn_cubic.hpp"

namespace krcn {

// The parameter block the host stages per call: kCrnbPar doubles a column.
enum { kCrnbParValue = 0, kCrnbParL2, kCrnbParM0, kCrnbParR0, kCrnbParActive, kCrnbParMeff, kCrnbParGnorm, kCrnbPar = 8 };

constexpr size_t kCrnbHeadDoubles = sizeof(CrnbHead) / sizeof(double);
constexpr size_t kCrnbColDoubles = sizeof(CrnbCol) / sizeof(double);
static_assert(sizeof(CrnbHead) == sizeof(double), "the head is the first double of the state block");

__device__ __forceinline__ const CrnbHead* crnb_head(const double* st) {
  return reinterpret_cast<const CrnbHead*>(st);
}
__device__ __forceinline__ const CrnbCol* crnb_cols(const double* st) {
  return reinterpret_cast<const CrnbCol*>(st + kCrnbHeadDoubles);
}

#define KRCN_CRNB_ROWS(len)                                                                       \
  constexpr int G = kNT / K;                                                                      \
  const int g = int(threadIdx.x) / K, c = int(threadIdx.x) % K;                                   \
  const bool own = c < k;                                                                         \
  for (int64_t i0 = int64_t(blockIdx.x) * (G * kBlzU) + g; i0 < (len); i0 += int64_t(gridDim.x) * (G * kBlzU))

// R[i, c] = expit(AX[i, c]) - b_c[i], k_residual's expression per entry.
// bk = 0: one label vector for every column; bk = k: an (n, k) block.
template <typename T, int K>
__global__ __launch_bounds__(kNT) void k_crnb_residual(int64_t n, int k, const T* __restrict__ AX,
                                                       const T* __restrict__ b, int bk, T* __restrict__ R) {
  KRCN_CRNB_ROWS(n) {
    T a[kBlzU], bv[kBlzU];
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      const bool on = own && i < n;
      a[u] = on ? AX[i * k + c] : T(0);
      bv[u] = on ? (bk ? b[i * bk + c] : b[i]) : T(0);
    }
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      if (own && i < n) R[i * k + c] = expit(a[u]) - bv[u];
    }
  }
}

// Start of a chain (one workgroup): the records from the staged parameters.
// blz != nullptr: m_eff and ||g|| come from the batched Lanczos' states on the
// device (blz_m_eff: the reference's truncation rule); else from the parameters.
[[maybe_unused]] static __global__ __launch_bounds__(kNT) void k_crnb_begin(int k, int m,
                                                                           const double* __restrict__ par,
                                                                           const BlzCol* __restrict__ blz,
                                                                           double* st) {
  const int c = threadIdx.x;
  if (c < k) {
    const double* p = par + c * kCrnbPar;
    CrnbCol s{};
    s.phase = crnb_start(p[kCrnbParActive] != 0.0);
    s.m_eff = blz ? blz_m_eff(blz[c].j_break, m) : int(p[kCrnbParMeff]);
    s.gnorm = blz ? blz[c].gnorm : p[kCrnbParGnorm];
    s.M = p[kCrnbParM0];
    s.value = p[kCrnbParValue];
    s.l2 = p[kCrnbParL2];
    s.r0 = p[kCrnbParR0];
    reinterpret_cast<CrnbCol*>(st + kCrnbHeadDoubles)[c] = s;
  }
  if (c == 0) *reinterpret_cast<CrnbHead*>(st) = CrnbHead{0, 0};
}

// X_new / AX_new of a column that starts as done: byte copies of the inputs.
template <typename T, int K>
__global__ __launch_bounds__(kNT) void k_crnb_copy_inactive(int64_t len, int k, const T* __restrict__ src,
                                                            T* __restrict__ dst, const double* __restrict__ st) {
  const int cc = int(threadIdx.x) % K;
  const bool copy = cc < k && crnb_cols(st)[cc].phase == kCrnbInactive;
  KRCN_CRNB_ROWS(len) {
    T x[kBlzU];
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      x[u] = (own && copy && i < len) ? src[i * k + c] : T(0);
    }
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      if (own && copy && i < len) dst[i * k + c] = x[u];
    }
  }
}

// The batched subproblem: workgroup c runs k_cubic_tridiag's solve over column
// c's m_eff entries (alphas row c at al + c * als, betas at be + c * bes) from
// the column's r0 and writes s row c at s + c * ss, zero past m_eff.  A failed
// solve (status 1 or 2) ends the column's chain only.
[[maybe_unused]] static __global__ __launch_bounds__(kNT) void k_crnb_solve(double* st, int m,
                                                                           const double* __restrict__ al, int als,
                                                                           const double* __restrict__ be, int bes,
                                                                           double* __restrict__ s, int ss, double eps,
                                                                           int it_max) {
  if (crnb_head(st)->all_done) return;
  CrnbCol* col = reinterpret_cast<CrnbCol*>(st + kCrnbHeadDoubles) + blockIdx.x;
  if (!crnb_live(col->phase)) return;
  const int me = col->m_eff;
  double* sc = s + int64_t(blockIdx.x) * ss;
  const CubicSolve r = cubic_tridiag_solve(me, col->M, col->gnorm, al + int64_t(blockIdx.x) * als,
                                           be + int64_t(blockIdx.x) * bes, sc, col->r0, eps, it_max);
  const bool solved = r.status == kCubicOk || r.status == kCubicItMax;
  for (int i = (solved ? me : 0) + int(threadIdx.x); i < m; i += kNT) sc[i] = 0.0;
  if (threadIdx.x == 0) {
    col->solver_it = r.its;
    col->solver_status = r.status;
    col->lam = r.root;
    col->model_decrease = r.dec;
    col->phase = crnb_after_solve(col->phase, r.status);
  }
}

// X_new[i, c] = X[i, c] + sum_j V[j, i, c] * s_c[j], j ascending over the m
// slabs with s zero past m_eff_c, product and sum rounded separately:
// k_blz_combine's sum per column.  A column that is not live is not stored.
template <typename T, int K>
__global__ __launch_bounds__(kNT) void k_crnb_combine(int64_t d, int k, int m, const T* __restrict__ V,
                                                      const double* __restrict__ s, int ss, const T* __restrict__ X,
                                                      T* __restrict__ Xn, const double* __restrict__ st) {
  if (crnb_head(st)->all_done) return;
  const int cc = int(threadIdx.x) % K;
  const bool live = cc < k && crnb_live(crnb_cols(st)[cc].phase);
  const double* sc = s + int64_t(cc < k ? cc : 0) * ss;
  const int64_t slab = d * k;
  KRCN_CRNB_ROWS(d) {
    T acc[kBlzU], x0[kBlzU];
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      acc[u] = T(0);
      x0[u] = (own && live && i < d) ? X[i * k + c] : T(0);
    }
    for (int j = 0; j < m; ++j) {
      const T sv = T(sc[j]);
      T v[kBlzU];
#pragma unroll
      for (int u = 0; u < kBlzU; ++u) {
        const int64_t i = i0 + int64_t(u) * G;
        v[u] = (own && live && i < d) ? V[int64_t(j) * slab + i * k + c] : T(0);
      }
#pragma unroll
      for (int u = 0; u < kBlzU; ++u) acc[u] += v[u] * sv;
    }
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      if (own && live && i < d) Xn[i * k + c] = x0[u] + acc[u];
    }
  }
}

// Per-column partials of the loss terms (1 - b) a - logsig(a) over an (n, k)
// block, k_loss_terms' expression per entry.  st != nullptr: a trial's launch
// (guarded; the columns that are not live give zero partials).
template <typename T, int K>
__global__ __launch_bounds__(kNT) void k_crnb_loss(int64_t n, int k, const T* __restrict__ AX,
                                                   const T* __restrict__ b, int bk, double* __restrict__ pl,
                                                   const double* __restrict__ st) {
  if (st && crnb_head(st)->all_done) return;
  __shared__ double sm[4 * K];
  const int cc = int(threadIdx.x) % K;
  const bool live = cc < k && (!st || crnb_live(crnb_cols(st)[cc].phase));
  double acc = 0.0;
  KRCN_CRNB_ROWS(n) {
    T a[kBlzU], bv[kBlzU];
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      const bool on = own && live && i < n;
      a[u] = on ? AX[i * k + c] : T(0);
      bv[u] = on ? (bk ? b[i * bk + c] : b[i]) : T(0);
    }
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      if (own && live && i < n) {
        const T t = (T(1) - bv[u]) * a[u] - logsig(a[u]);
        acc += double(t);
      }
    }
  }
  const double t = blz_col_sum<K>(acc, sm);
  if (g == 0 && own) pl[int64_t(blockIdx.x) * K + c] = t;
}

// Per-column partials of ||A_c||^2 (B == nullptr) or ||A_c - B_c||^2 over
// (len, k) blocks, k_sqnorm_guard's expressions.  when = 0: inside a trial
// (the live columns, while the chain runs); 1: the step length (every column,
// once the chain has ended); st == nullptr: unguarded, every column.
template <typename T, int K>
__global__ __launch_bounds__(kNT) void k_crnb_sq(int64_t len, int k, const T* __restrict__ A,
                                                 const T* __restrict__ B, double* __restrict__ pn,
                                                 const double* __restrict__ st, int when) {
  if (st && (crnb_head(st)->all_done != 0) != (when != 0)) return;
  __shared__ double sm[4 * K];
  const int cc = int(threadIdx.x) % K;
  const bool live = cc < k && (!st || when != 0 || crnb_live(crnb_cols(st)[cc].phase));
  double acc = 0.0;
  KRCN_CRNB_ROWS(len) {
    T a[kBlzU], bv[kBlzU];
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      const bool on = own && live && i < len;
      a[u] = on ? A[i * k + c] : T(0);
      bv[u] = (on && B) ? B[i * k + c] : T(0);
    }
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      if (B) {
        const T t = a[u] - bv[u];
        acc += double(t) * double(t);
      } else {
        const double t = a[u];
        acc += t * t;
      }
    }
  }
  const double t = blz_col_sum<K>(acc, sm);
  if (g == 0 && own) pn[int64_t(blockIdx.x) * K + c] = t;
}

// The state block (head and k records) to the mapped host block.
__device__ __forceinline__ void crnb_publish(int k, const double* st, double* __restrict__ out) {
  const int nd = int(kCrnbHeadDoubles + size_t(k) * kCrnbColDoubles);
  for (int i = threadIdx.x; i < nd; i += kNT) out[i] = st[i];
}
[[maybe_unused]] static __global__ __launch_bounds__(kNT) void k_crnb_publish(int k, const double* st,
                                                                             double* __restrict__ out) {
  crnb_publish(k, st, out);
}

// The judge of a trial (one workgroup).  Per live column: value_new = mean +
// l2 / 2 * norm ** 2 as LogisticRegression._value forms it, then the line
// search's test through crnb_judge (cubic.py:293-303).  Sets all_done when no
// column is live — the only writer of the flag after k_crnb_begin's reset —
// and copies the records to the mapped host block.
template <int K>
__global__ __launch_bounds__(kNT) void k_crnb_judge(int k, const double* __restrict__ pl, int Pl,
                                                    const double* __restrict__ pn, int Pn, int any_l2,
                                                    double n_global, double ls_beta, int max_trials, double* st,
                                                    double* __restrict__ out) {
  if (crnb_head(st)->all_done) return;
  __shared__ double sm[4 * K];
  const double sl = blz_sum_partials<K>(pl, Pl, K, sm);
  const double sn = any_l2 ? blz_sum_partials<K>(pn, Pn, K, sm) : 0.0;
  int live_after = 0;
  if (int(threadIdx.x) < k) {   // lane group 0: one lane per column
    CrnbCol* col = reinterpret_cast<CrnbCol*>(st + kCrnbHeadDoubles) + threadIdx.x;
    if (crnb_live(col->phase)) {
      double vnew = sl / n_global;
      const double l2 = col->l2;
      if (l2 != 0.0) {
        const double nrm = sqrt(sn);
        vnew = vnew + l2 / 2.0 * (nrm * nrm);
      }
      const CrnbVerdict v = crnb_judge(col->phase, col->trials, col->M, col->value, col->model_decrease, vnew,
                                       ls_beta, max_trials);
      col->value_new = vnew;
      col->phase = v.phase;
      col->trials = v.trials;
      col->M = v.M;
      live_after = crnb_live(v.phase);
    }
  }
  const unsigned long long any = __ballot(live_after);   // k <= 16: every column's lane is in wave 0
  if (threadIdx.x == 0) reinterpret_cast<CrnbHead*>(st)->all_done = any == 0ull;
  __syncthreads();
  crnb_publish(k, st, out);
}

// ||x_new,c - x_c||^2 from k_crnb_sq's partials once the chain has ended.
template <int K>
__global__ __launch_bounds__(kNT) void k_crnb_dx_finish(int k, const double* __restrict__ pn, int Pn, double* st,
                                                        double* __restrict__ out) {
  if (!crnb_head(st)->all_done) return;
  __shared__ double sm[4 * K];
  const double s = blz_sum_partials<K>(pn, Pn, K, sm);
  if (int(threadIdx.x) < k) reinterpret_cast<CrnbCol*>(st + kCrnbHeadDoubles)[threadIdx.x].dx2 = s;
  __syncthreads();
  crnb_publish(k, st, out);
}

// krcn_value_block's closing launch: f_c = sum / n + l2_c / 2 * norm ** 2 to the mapped host block.
template <int K>
__global__ __launch_bounds__(kNT) void k_crnb_value_finish(int k, const double* __restrict__ pl, int Pl,
                                                           const double* __restrict__ pn, int Pn, int any_l2,
                                                           double n_global, const double* __restrict__ par,
                                                           double* __restrict__ out) {
  __shared__ double sm[4 * K];
  const double sl = blz_sum_partials<K>(pl, Pl, K, sm);
  const double sn = any_l2 ? blz_sum_partials<K>(pn, Pn, K, sm) : 0.0;
  if (int(threadIdx.x) < k) {
    const double l2 = par[threadIdx.x * kCrnbPar + kCrnbParL2];
    double v = sl / n_global;
    if (l2 != 0.0) {
      const double nrm = sqrt(sn);
      v = v + l2 / 2.0 * (nrm * nrm);
    }
    out[threadIdx.x] = v;
  }
}

#undef KRCN_CRNB_ROWS
}  // namespace krcn
