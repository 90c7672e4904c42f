// krcn_coord.hpp — coordinate-block kernels of SSCN: the gradient, the Hessian
// block and the incremental Ax update over a selection of k columns of X.
//
// All three read the handle's transposed CSR (tptr / tidx / tval): column c of X
// is the contiguous, row-sorted list tidx / tval[tptr[c] .. tptr[c + 1]) with
// distinct rows.  Sums are fp64 in a fixed order (no atomics), whatever the
// handle's dtype; the logistic pieces are evaluated inline in the handle's
// dtype with the arithmetic of k_residual / k_weights.
//
//   k_coord_grad    one 256-thread block per selected column: threads stride
//                   over the column's entries, fixed-order block sum.  A
//                   column's value depends on that column alone.
//   k_coord_hess    one 1024-thread block per DISTINCT selected column a (the
//                   host removes duplicates and expands the result): per row
//                   window the block scatters u_r = w_r X[r, c_a] into a dense
//                   fp64 LDS window, its waves take the partner columns b,
//                   find their entries inside the window (wave-wide 64-ary
//                   search) and sum X[r, c_b] * win[r - r0]; the window is
//                   cleared by un-scattering column a.  Partners are the
//                   cyclic half (a + j) mod ku, j <= ku / 2, so every block
//                   owns about ku / 2 pairs and each unordered pair has one
//                   owner; the owner writes H[a][b] and its mirror H[b][a].
//   k_coord_update  every wave owns a window of rows in LDS (t = 0), walks the
//                   selected columns in the order given (duplicates included)
//                   and adds tval * delta[a] at the column's rows inside its
//                   window — scipy's csc_matvec order per row, multiply and add
//                   kept apart — then stores Ax_in + t.  A wave's LDS
//                   operations execute in program order, so no barrier sits
//                   between columns and the loads of U columns are in flight
//                   together.
#pragma once
#include "krcn_kernels.hpp"

namespace krcn {

constexpr int kCoordGradNT = kNT;
constexpr int kCoordHessNT = 1024;
constexpr int kCoordHessWaves = kCoordHessNT / 64;
// rows of the Hessian's fp64 LDS window: the 160 KiB of a CU less the 256 B
// the project's kernels keep back, in whole waves of rows
constexpr int kCoordWinMax = ((163840 - 256) / 8) / 64 * 64;   // 20,416
constexpr int kCoordUpdNT = kNT;
constexpr int kCoordUpdWaves = kCoordUpdNT / 64;
constexpr int kCoordUpdAuto = 256;    // rows a wave of the update owns (auto)
constexpr int kCoordUpdMax = 1024;    //   and at most (a set window above it is clamped)
constexpr int kCoordUpdU = 8;         // columns whose loads the update keeps in flight

// Orders a wave's LDS stores before its later LDS loads (another lane's
// address): LDS operations of one wave execute in program order, so this only
// keeps the compiler from moving them (the idiom of krcn_tiled.hpp).
__device__ __forceinline__ void coord_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// First position p in [lo, hi) with idx[p] >= key (idx ascending), searched by
// the whole wave: 64 probes per round.  Every lane returns the same value.
__device__ __forceinline__ int wave_lower_bound(const int* __restrict__ idx, int lo, int hi, int key) {
  const int lane = threadIdx.x & 63;
  while (hi - lo > 64) {
    const int step = (hi - lo + 63) / 64;
    const int p = lo + lane * step;
    const bool below = p < hi && idx[p] < key;
    const int cnt = __popcll(__ballot(below));   // probes are ascending: the lanes below form a prefix
    if (cnt == 0) return lo;
    const int nlo = lo + (cnt - 1) * step + 1;   // idx[lo + (cnt - 1) step] < key
    const int nhi = lo + cnt * step;             // idx[lo + cnt step] >= key (or past the end)
    lo = nlo;
    hi = nhi < hi ? nhi : hi;
  }
  const int p = lo + lane;
  const bool below = p < hi && idx[p] < key;
  return lo + __popcll(__ballot(below));
}

// g[a] = sum_r X[r, c_a] (expit(Ax_r) - b_r) / n (+ l2 x[c_a])
template <typename T>
__global__ __launch_bounds__(kCoordGradNT) void k_coord_grad(const int* __restrict__ cols,
                                                             const int* __restrict__ tptr,
                                                             const int* __restrict__ tidx,
                                                             const T* __restrict__ tval, const T* __restrict__ Ax,
                                                             const T* __restrict__ b, const T* __restrict__ x,
                                                             double n, double l2, int has_l2,
                                                             double* __restrict__ g) {
  __shared__ double sm[kCoordGradNT / 64];
  const int c = cols[blockIdx.x];
  const int p0 = tptr[c], p1 = tptr[c + 1];
  double acc = 0.0;
  for (int e = p0 + int(threadIdx.x); e < p1; e += kCoordGradNT) {
    const int r = tidx[e];
    const T res = expit(Ax[r]) - b[r];
    acc += double(tval[e]) * double(res);
  }
  const double s = block_sum(acc, sm);
  if (threadIdx.x == 0) {
    const double q = s / n;
    g[blockIdx.x] = has_l2 ? q + l2 * double(x[c]) : q;
  }
}

// g[a] = l2 x[c_a]: the gradient of a matrix without rows or nonzeros.
template <typename T>
__global__ __launch_bounds__(kNT) void k_coord_l2x(int k, const int* __restrict__ cols, const T* __restrict__ x,
                                                   double l2, double* __restrict__ g) {
  const int a = blockIdx.x * kNT + threadIdx.x;
  if (a < k) g[a] = l2 * double(x[cols[a]]);
}

// H[a][b] = H[b][a] = sum_r w_r X[r, c_a] X[r, c_b] / n over ku distinct columns.
template <typename T>
__global__ __launch_bounds__(kCoordHessNT) void k_coord_hess(int nrows, int R, int ku, const int* __restrict__ cols,
                                                             const int* __restrict__ tptr,
                                                             const int* __restrict__ tidx,
                                                             const T* __restrict__ tval, const T* __restrict__ Ax,
                                                             double n, double* __restrict__ H) {
  __shared__ double win[kCoordWinMax];
  const int a = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // partners (a + j) mod ku, j = 0 .. J - 1: the cyclic half; for even ku the
  // opposite column (j = ku / 2) belongs to the lower index of the two
  const int half = ku / 2;
  const int J = (ku & 1) ? half + 1 : (a < half ? half + 1 : half);
  // this wave's partners j = wave + 16 i: lane i keeps partner i's column
  // range and its running sum
  int q0 = 0, q1 = 0;
  double acc = 0.0;
  const int nj = J > wave ? (J - wave + kCoordHessWaves - 1) / kCoordHessWaves : 0;
  if (lane < nj) {
    const int cb = cols[(a + wave + kCoordHessWaves * lane) % ku];
    q0 = tptr[cb];
    q1 = tptr[cb + 1];
  }
  for (int i = threadIdx.x; i < R; i += kCoordHessNT) win[i] = 0.0;
  const int ca = cols[a];
  const int p0 = tptr[ca], p1 = tptr[ca + 1];
  __syncthreads();
  int pa = p0;
  while (pa < p1) {                       // windows that hold entries of column a, ascending
    const int r0 = (tidx[pa] / R) * R;
    const int r1 = nrows - r0 < R ? nrows : r0 + R;   // (no overflow for nrows near 2^31)
    const int pe = wave_lower_bound(tidx, pa, p1, r1);
    for (int e = pa + int(threadIdx.x); e < pe; e += kCoordHessNT) {
      const int r = tidx[e];
      const T s = expit(Ax[r]);
      const T w = s * (T(1) - s);
      win[r - r0] = double(w) * double(tval[e]);
    }
    __syncthreads();
    for (int i = 0; i < nj; ++i) {
      const int b0 = __shfl(q0, i, 64), b1 = __shfl(q1, i, 64);
      double s = 0.0;
      for (int e = wave_lower_bound(tidx, b0, b1, r0) + lane; e < b1; e += 64) {
        const int r = tidx[e];
        if (r >= r1) break;
        s += double(tval[e]) * win[r - r0];
      }
      s = wave_sum(s);
      if (lane == i) acc += s;
    }
    __syncthreads();
    for (int e = pa + int(threadIdx.x); e < pe; e += kCoordHessNT) win[tidx[e] - r0] = 0.0;
    __syncthreads();
    pa = pe;
  }
  if (lane < nj) {
    const int bb = (a + wave + kCoordHessWaves * lane) % ku;
    const double v = acc / n;
    H[size_t(a) * ku + bb] = v;
    H[size_t(bb) * ku + a] = v;
  }
}

// Ax_out = Ax_in + X[:, cols] delta, column by column in the order of cols.
// Dynamic LDS per wave: Rw doubles (the window), then k column starts and k
// column counts inside the window.
// kGuard (the SSCN step's trials, krcn_sscn.hip): the launch returns at once
// when *done is set, and delta was written by the launch before it.
template <typename T, bool kGuard = false>
__global__ __launch_bounds__(kCoordUpdNT) void k_coord_update(int n, int Rw, int k, const int* __restrict__ cols,
                                                              const double* __restrict__ delta,
                                                              const int* __restrict__ tptr,
                                                              const int* __restrict__ tidx,
                                                              const T* __restrict__ tval, const T* Ax_in,
                                                              T* Ax_out, const int* __restrict__ done) {
  if constexpr (kGuard) {
    if (*done) return;
  }
  extern __shared__ double coord_dyn[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0l = (int64_t(blockIdx.x) * kCoordUpdWaves + wave) * Rw;
  if (r0l >= n) return;                  // (no block barrier below: waves are independent)
  const int r0 = int(r0l);
  const int r1 = n - r0 < Rw ? n : r0 + Rw;
  const size_t per_wave = size_t(Rw) + size_t(k);   // doubles: window | k x (int start, int count)
  double* t = coord_dyn + size_t(wave) * per_wave;
  int* start = reinterpret_cast<int*>(t + Rw);
  int* count = start + k;
  for (int i = lane; i < Rw; i += 64) t[i] = 0.0;
  for (int a = lane; a < k; a += 64) {
    const int c = cols[a];
    const int p0 = tptr[c], p1 = tptr[c + 1];
    int lo = p0, hi = p1;
    while (lo < hi) {                    // first entry with row >= r0
      const int mid = lo + ((hi - lo) >> 1);
      if (tidx[mid] < r0) lo = mid + 1; else hi = mid;
    }
    const int first = lo;
    hi = p1;
    while (lo < hi) {                    // first entry with row >= r1
      const int mid = lo + ((hi - lo) >> 1);
      if (tidx[mid] < r1) lo = mid + 1; else hi = mid;
    }
    start[a] = first;
    count[a] = lo - first;
  }
  coord_wave_sync();
  for (int a0 = 0; a0 < k; a0 += kCoordUpdU) {
    int st[kCoordUpdU], cn[kCoordUpdU], rr[kCoordUpdU];
    double vv[kCoordUpdU], dl[kCoordUpdU];
#pragma unroll
    for (int u = 0; u < kCoordUpdU; ++u) {
      const int a = a0 + u;
      st[u] = a < k ? start[a] : 0;
      cn[u] = a < k ? count[a] : 0;
      dl[u] = a < k ? delta[a] : 0.0;
      rr[u] = 0;
      vv[u] = 0.0;
      if (lane < cn[u]) {
        rr[u] = tidx[st[u] + lane];
        vv[u] = double(tval[st[u] + lane]);
      }
    }
#pragma unroll
    for (int u = 0; u < kCoordUpdU; ++u) {
      if (lane < cn[u]) {
        const double p = vv[u] * dl[u];
        t[rr[u] - r0] = t[rr[u] - r0] + p;
      }
      for (int e = lane + 64; e < cn[u]; e += 64) {   // more than a wave of entries in the window
        const int r = tidx[st[u] + e];
        const double p = double(tval[st[u] + e]) * dl[u];
        t[r - r0] = t[r - r0] + p;
      }
      coord_wave_sync();
    }
  }
  for (int i = lane; r0 + i < r1; i += 64) {
    const double s = Ax_in ? double(Ax_in[r0 + i]) + t[i] : t[i];
    Ax_out[r0 + i] = T(s);
  }
}

}  // namespace krcn
