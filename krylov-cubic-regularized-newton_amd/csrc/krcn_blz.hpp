// krcn_blz.hpp — the vector kernels of the batched Lanczos (krcn_lanczos_block.hip):
// k independent three-term recurrences of cubic.py:77-111 in lockstep over
// (d, k) blocks, element (i, c) at i * k + c; m slabs of them make the basis.
//
// Lane mapping (k_block_pass's): K = the next power of two >= k, a 256-thread
// workgroup holds 256 / K lane groups of K consecutive lanes, a group owns a
// row i of the block and its member c < k owns column c: adjacent lanes touch
// adjacent addresses and a thread's column is fixed.  A workgroup covers
// kBlzU * 256 / K rows a round (kBlzU independent loads per array and thread in
// flight) on at most kBlzMaxGrid workgroups, grid-stride beyond.
//
// Reductions are per column and two-stage.  Within a workgroup the lanes of a
// column are summed by an xor butterfly over the lane bits above K, then the
// four wave sums are added as (w0 + w1) + (w2 + w3); the workgroup stores one
// partial per column, p[b * stride + c].  The consumer launch re-sums them:
// lane group g adds partials g, g + 256 / K, .. in that order and the groups
// are combined by the same workgroup sum, so every workgroup of the consumer
// holds the same bits.  No atomics; a column's sums never see another
// column's values.
//
// The control state is one BlzCol per column (krcn_blz_state.hpp gives its
// meaning); alphas[c * m + j], betas[c * max(m - 1, 1) + j].  A launch that
// settles a step reads the state of the launches before it; its block 0
// writes the new one.
#pragma once
#include "krcn_blz_state.hpp"
#include "krcn_block_rows.hpp"
#include "krcn_kernels.hpp"

namespace krcn {

constexpr int kBlzU = 4;            // rows a lane group works on per round
constexpr int kBlzMaxGrid = 1024;   // workgroups of a vector launch (the partials buffers hold this many per column)

struct BlzCol {
  int j_break;     // kBlzLive, or the loop index of the breakdown
  int pad;
  double gnorm;    // ||g_c|| (cubic.py:85)
  double beta_last;   // the reference's 4th return value
  double pad1;
};
static_assert(sizeof(BlzCol) == 4 * sizeof(double), "a BlzCol is four doubles of the results block");

inline int blz_grid(int64_t rows, int K) {
  const int64_t per = int64_t(kBlzU) * (kNT / K);
  const int64_t b = (rows + per - 1) / per;
  return int(b < 1 ? 1 : (b > kBlzMaxGrid ? kBlzMaxGrid : b));
}

// Sum over the workgroup's lanes of one column (threadIdx.x % K); every lane
// returns its column's sum.  sm: 4 * K doubles.
template <int K>
__device__ __forceinline__ double blz_col_sum(double v, double* sm) {
#pragma unroll
  for (int off = 32; off >= K; off >>= 1) v += __shfl_xor(v, off, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = threadIdx.x % K;
  if (lane < K) sm[w * K + lane] = v;
  __syncthreads();
  const double r = (sm[c] + sm[K + c]) + (sm[2 * K + c] + sm[3 * K + c]);
  __syncthreads();
  return r;
}

// Sum of P per-workgroup partials of the lane's column, p[i * stride + c].
template <int K>
__device__ __forceinline__ double blz_sum_partials(const double* __restrict__ p, int P, int stride, double* sm) {
  constexpr int G = kNT / K;
  const int g = threadIdx.x / K, c = threadIdx.x % K;
  double v = 0.0;
  for (int i = g; i < P; i += G) v += p[int64_t(i) * stride + c];
  return blz_col_sum<K>(v, sm);
}

// Rows of a round: lane group g of block b takes rows i0 + u * G, u < kBlzU.
#define KRCN_BLZ_ROWS(d)                                                                          \
  constexpr int G = kNT / K;                                                                      \
  const int g = int(threadIdx.x) / K, c = int(threadIdx.x) % K;                                   \
  const bool own = c < k;                                                                         \
  for (int64_t i0 = int64_t(blockIdx.x) * (G * kBlzU) + g; i0 < (d); i0 += int64_t(gridDim.x) * (G * kBlzU))

// Start of a call: zero alphas and betas (block 0), partials of ||g_c||^2.
template <typename T, int K>
__global__ __launch_bounds__(kNT) void k_blz_begin(int64_t d, int k, int m, const T* __restrict__ Gm,
                                                   double* __restrict__ alphas, double* __restrict__ betas,
                                                   double* __restrict__ pn) {
  __shared__ double sm[4 * K];
  if (blockIdx.x == 0) {
    const int mb = m > 1 ? m - 1 : 1;
    for (int i = threadIdx.x; i < k * m; i += kNT) alphas[i] = 0.0;
    for (int i = threadIdx.x; i < k * mb; i += kNT) betas[i] = 0.0;
  }
  double acc = 0.0;
  KRCN_BLZ_ROWS(d) {
    T gv[kBlzU];
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      gv[u] = (own && i < d) ? Gm[i * k + c] : T(0);
    }
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) acc += double(gv[u]) * double(gv[u]);
  }
  const double t = blz_col_sum<K>(acc, sm);
  if (g == 0 && own) pn[int64_t(blockIdx.x) * K + c] = t;
}

// Settles a norm and normalises.  j < 0, the start (cubic.py:85): dst = V[0]
// = G / ||g||, the state is reset.  Loop step j (cubic.py:97-103): beta = the
// norm of the unnormalised z in src = dst = V[j + 1]; a live column that does
// not break gets v = z / beta in place, every other column zeros (a frozen
// column's v is never divided by its tiny beta, and whatever V held is gone).
template <typename T, int K>
__global__ __launch_bounds__(kNT) void k_blz_norm(int64_t d, int k, int m, int j, const T* src, T* dst,
                                                  const double* __restrict__ pn, int P, double tol, BlzCol* st,
                                                  double* __restrict__ betas) {
  __shared__ double sm[4 * K];
  const double nrm = sqrt(blz_sum_partials<K>(pn, P, K, sm));
  const int cc = int(threadIdx.x) % K;
  int jb = kBlzLive;
  if (j >= 0 && cc < k) jb = __hip_atomic_load(&st[cc].j_break, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const BlzStep s = j < 0 ? BlzStep{true, false, kBlzLive} : blz_step(jb, j, nrm, tol);
  const bool divide = s.live && !s.breaks;
  const T div = T(nrm);
  KRCN_BLZ_ROWS(d) {
    T z[kBlzU];
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      z[u] = (own && divide && i < d) ? src[i * k + c] : T(0);
    }
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      if (own && i < d) dst[i * k + c] = divide ? z[u] / div : T(0);
    }
  }
  if (blockIdx.x == 0 && int(threadIdx.x) < k) {   // lane group 0: one lane per column
    const int c0 = threadIdx.x;
    if (j < 0) {
      st[c0].gnorm = nrm;
      st[c0].beta_last = 0.0;
      __hip_atomic_store(&st[c0].j_break, kBlzLive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (s.live) {
      const int mb = m > 1 ? m - 1 : 1;
      st[c0].beta_last = nrm;
      if (s.breaks) __hip_atomic_store(&st[c0].j_break, j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else betas[c0 * mb + j] = nrm;
    }
  }
}

// Partials of v.y and v.v_prev per column (vp == nullptr: of v.y alone, the
// second is zero): alpha_j = v.(y - beta v_prev) = v.y - beta (v.v_prev),
// settled by the consumer.  pa[(b * 2 + q) * K + c].
template <typename T, int K>
__global__ __launch_bounds__(kNT) void k_blz_dots(int64_t d, int k, const T* __restrict__ v, const T* __restrict__ vp,
                                                  const T* __restrict__ y, double* __restrict__ pa) {
  __shared__ double sm[4 * K];
  double a1 = 0.0, a2 = 0.0;
  KRCN_BLZ_ROWS(d) {
    T vv[kBlzU], yv[kBlzU], pv[kBlzU];
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      const bool on = own && i < d;
      vv[u] = on ? v[i * k + c] : T(0);
      yv[u] = on ? y[i * k + c] : T(0);
      pv[u] = (on && vp) ? vp[i * k + c] : T(0);
    }
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      a1 += double(vv[u]) * double(yv[u]);
      a2 += double(vv[u]) * double(pv[u]);
    }
  }
  const double t1 = blz_col_sum<K>(a1, sm);
  const double t2 = blz_col_sum<K>(a2, sm);
  if (g == 0 && own) {
    pa[(int64_t(blockIdx.x) * 2 + 0) * K + c] = t1;
    pa[(int64_t(blockIdx.x) * 2 + 1) * K + c] = t2;
  }
}

// Loop step j (cubic.py:93-97) of every live column: alpha from k_blz_dots'
// partials, w = y - beta_{j-1} v_{j-1} re-formed (w = y at j = 0), z = w - alpha v
// stored unnormalised in V[j + 1], partials of ||z||^2.  Block 0 stores
// alphas[j].  A broken column is left alone (its partial is zero).
template <typename T, int K>
__global__ __launch_bounds__(kNT) void k_blz_form(int64_t d, int k, int m, int j, const T* __restrict__ v,
                                                  const T* __restrict__ vp, const T* __restrict__ y, T* __restrict__ z,
                                                  const double* __restrict__ pa, int P, const BlzCol* __restrict__ st,
                                                  const double* __restrict__ betas, double* __restrict__ alphas,
                                                  double* __restrict__ pn) {
  __shared__ double sm[4 * K];
  const double a1 = blz_sum_partials<K>(pa, P, 2 * K, sm);
  const double a2 = blz_sum_partials<K>(pa + K, P, 2 * K, sm);
  const int cc = int(threadIdx.x) % K;
  const int mb = m > 1 ? m - 1 : 1;
  const bool live = cc < k && st[cc].j_break == kBlzLive;
  const double bprev = (j > 0 && cc < k) ? betas[cc * mb + j - 1] : 0.0;
  const double alpha = j > 0 ? a1 - bprev * a2 : a1;
  const T tb = T(bprev), ta = T(alpha);
  double acc = 0.0;
  KRCN_BLZ_ROWS(d) {
    T vv[kBlzU], yv[kBlzU], pv[kBlzU];
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      const bool on = own && live && i < d;
      vv[u] = on ? v[i * k + c] : T(0);
      yv[u] = on ? y[i * k + c] : T(0);
      pv[u] = (on && j > 0) ? vp[i * k + c] : T(0);
    }
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      if (own && live && i < d) {
        const T w = j > 0 ? yv[u] - tb * pv[u] : yv[u];
        const T zi = w - ta * vv[u];
        z[i * k + c] = zi;
        acc += double(zi) * double(zi);
      }
    }
  }
  const double t = blz_col_sum<K>(acc, sm);
  if (g == 0 && own) pn[int64_t(blockIdx.x) * K + c] = t;
  if (blockIdx.x == 0 && g == 0 && live) alphas[c * m + j] = alpha;
}

// The final quotient's operand: each column's current v (slab j_break of a
// broken column, slab m - 1 of the others).
template <typename T, int K>
__global__ __launch_bounds__(kNT) void k_blz_pick(int64_t d, int k, int m, const T* __restrict__ V,
                                                  const BlzCol* __restrict__ st, T* __restrict__ op) {
  const int cc = int(threadIdx.x) % K;
  const int cur = cc < k ? blz_current(st[cc].j_break, m) : 0;
  const T* src = V + int64_t(cur) * d * k;
  KRCN_BLZ_ROWS(d) {
    T x[kBlzU];
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      x[u] = (own && i < d) ? src[i * k + c] : T(0);
    }
#pragma unroll
    for (int u = 0; u < kBlzU; ++u) {
      const int64_t i = i0 + int64_t(u) * G;
      if (own && i < d) op[i * k + c] = x[u];
    }
  }
}

// One workgroup: alphas[final slot] = v.A(v) (cubic.py:109) from k_blz_dots'
// partials, then the results block (k BlzCol | alphas | betas: res, nres
// doubles) is copied to the mapped host block.
template <int K>
__global__ __launch_bounds__(kNT) void k_blz_finish(int k, int m, const double* __restrict__ pa, int P, double* res,
                                                    int nres, double* __restrict__ out) {
  __shared__ double sm[4 * K];
  __shared__ double fa[K];
  __shared__ int fs[K];
  const double a = blz_sum_partials<K>(pa, P, 2 * K, sm);
  const BlzCol* st = reinterpret_cast<const BlzCol*>(res);
  if (int(threadIdx.x) < K) {
    fa[threadIdx.x] = a;
    fs[threadIdx.x] = int(threadIdx.x) < k ? blz_final_slot(st[threadIdx.x].j_break, m) : 0;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nres; i += kNT) {
    const int q = i - 4 * k;   // position in alphas when 0 <= q < k * m
    const bool fin = q >= 0 && q < k * m && q % m == fs[q / m];
    const double x = fin ? fa[q / m] : res[i];
    if (fin) res[i] = x;
    out[i] = x;
  }
}

// X_new[i, c] = X0[i, c] + sum_j V[j, i, c] * s[j, c], j ascending, product and
// sum rounded separately: k_basis_combine's sum per column.
constexpr int kBlzCombU = 8;
template <typename T>
__global__ __launch_bounds__(kNT) void k_blz_combine(int64_t len, int k, int m, const T* __restrict__ V,
                                                     const double* __restrict__ s, const T* __restrict__ x0,
                                                     T* __restrict__ xn) {
  for (int64_t e = int64_t(blockIdx.x) * kNT + threadIdx.x; e < len; e += int64_t(gridDim.x) * kNT) {
    const int c = int(e % k);
    T acc = T(0);
    int j = 0;
    for (; j + kBlzCombU <= m; j += kBlzCombU) {
      T v[kBlzCombU], sv[kBlzCombU];
#pragma unroll
      for (int u = 0; u < kBlzCombU; ++u) {
        v[u] = V[int64_t(j + u) * len + e];
        sv[u] = T(s[(j + u) * k + c]);
      }
#pragma unroll
      for (int u = 0; u < kBlzCombU; ++u) acc += v[u] * sv[u];
    }
    for (; j < m; ++j) acc += V[int64_t(j) * len + e] * T(s[j * k + c]);
    xn[e] = x0[e] + acc;
  }
}

#undef KRCN_BLZ_ROWS
}  // namespace krcn
