// krcn_block.hpp — block products: k vectors per pass over the matrix.
//
// A block of k vectors over a space of length L is an (L, k) row-major array,
// element (i, j) at i * k + j (64-bit offsets), 1 <= k <= KRCN_BLOCK_MAX.  One
// kernel template serves both passes: pass 1 walks the caller's CSR of X and
// gathers rows of V (d, k), pass 2 walks the handle's transposed CSR and gathers
// rows of U (n, k).  A gather of column c fetches the k contiguous values
// V[c, 0..k): one 64-byte segment at k = 8 in fp64.
//
// Lane mapping.  K = the next power of two >= k.  A 256-thread block holds
// 256 / K lane groups of K consecutive lanes; group g of block b owns row
// b * (256 / K) + g and member j < k of the group owns vector j of that row
// (no grid cap: ceil(rows / (256 / K)) blocks).
// Members j >= k take part in staging the matrix stream but neither gather
// nor store.
//
// Matrix stream.  A group reads its row in stages of S = max(K, 8) elements:
// member m loads elements m, m + K, .. of the stage (index and value, adjacent
// lanes adjacent addresses, so one wave instruction fetches the stages of all
// its rows), the next stage is loaded before the current one is consumed, and
// the members hand the elements round by width-K shuffles.  All S gathers of a
// stage are issued before the first add; the adds then run left to right,
// product and sum rounded separately (-ffp-contract=off): entry (r, j) is
// scipy's csr_matvecs / csc_matvecs sum, bit for bit, for every row of at most
// KRCN_BLOCK_LONG_ROW elements.
//
// Long rows.  The short-row kernel skips a row above the threshold; the host
// lists those rows once per handle (krcn_block_rows.hpp) and a second kernel
// gives each of them a 1024-thread workgroup: the row is cut into 1024 / K
// contiguous segments of ceil(len / (1024 / K)) elements, group g sums segment
// g left to right as above, the partials go to LDS and lane group 0 adds them
// in segment order.  The order depends on the row's length and on K alone: no
// atomics, bitwise equal from run to run and whatever rows surround it.
//
// Epilogues are functors called once per (row, vector) by the owning lane.
#pragma once
#include "krcn_block_rows.hpp"
#include "krcn_crnb_state.hpp"
#include "krcn_kernels.hpp"

namespace krcn {

// T[r, j] = s                                (X V, one krcn_matvec per column)
template <typename T> struct BlkStore {
  T* out;
  __device__ __forceinline__ void row(int64_t r, int j, int k, T s) const { out[r * k + j] = s; }
};

// U[r, j] = w * s, w = w[r] (wk = 0) or w[r, j] (wk = k)     (EpiWeighted per column)
template <typename T> struct BlkWeighted {
  const T* w; T* u; int wk;
  __device__ __forceinline__ void row(int64_t r, int j, int k, T s) const {
    const T wr = wk ? w[r * wk + j] : w[r];
    u[r * k + j] = wr * s;
  }
};

// Y[r, j] = s / n (+ l2_j * V[r, j] when l2_j != 0)           (EpiHvpOut per column:
// a column with l2_j == 0 never reads v, which may then be null)
template <typename T> struct BlkHvpOut {
  const T* v; T* y; T n;
  T l2[KRCN_BLOCK_MAX];
  __device__ __forceinline__ void row(int64_t r, int j, int k, T s) const {
    T l = T(0);
#pragma unroll
    for (int q = 0; q < KRCN_BLOCK_MAX; ++q) l = q == j ? l2[q] : l;   // (no runtime-indexed argument array)
    const T q = s / n;
    y[r * k + j] = l != T(0) ? q + l * v[r * k + j] : q;
  }
};

// T[r, j] = s for the live columns of a batched Krylov-CRN trial (krcn_crn_block.hip):
// the launch returns at once when the chain has ended and a column that is no
// longer live keeps its bytes.  An epilogue with a member type Guarded makes
// k_block_pass / k_block_long ask stop() first; the other epilogues' kernels
// are compiled without the question.
template <typename T> struct BlkStoreLive {
  using Guarded = void;
  T* out;
  const CrnbHead* head;
  const CrnbCol* cols;
  __device__ __forceinline__ bool stop() const { return head->all_done != 0; }
  __device__ __forceinline__ void row(int64_t r, int j, int k, T s) const {
    if (crnb_live(cols[j].phase)) out[r * k + j] = s;
  }
};
template <class E, class = void> struct BlkGuarded : std::false_type {};
template <class E> struct BlkGuarded<E, std::void_t<typename E::Guarded>> : std::true_type {};

// Left-to-right sum over elements [b, e) of a_e * V[col_e, j] by one lane group
// (m: the lane's position in its group, j == m; gathers only when j < k).
// Every lane of the group must call it with the same b and e.
template <typename T, int K>
__device__ __forceinline__ T block_row_sum(const int* __restrict__ idx, const T* __restrict__ val,
                                           const T* __restrict__ V, int k, int m, int b, int e) {
  constexpr int S = K < 8 ? 8 : K;   // elements per stage
  constexpr int R = S / K;           // of them per member
  const bool gathers = m < k;
  int ci[R];
  T cv[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int p = b + r * K + m;
    ci[r] = p < e ? idx[p] : 0;
    cv[r] = p < e ? val[p] : T(0);
  }
  T s = T(0);
  for (int p0 = b; p0 < e; p0 += S) {
    int ni[R];
    T nv[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int p = p0 + S + r * K + m;
      ni[r] = p < e ? idx[p] : 0;
      nv[r] = p < e ? val[p] : T(0);
    }
    T g[S], a[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
      int col;
      if constexpr (K == 1) {
        col = ci[i];
        a[i] = cv[i];
      } else {
        col = __shfl(ci[i / K], i % K, K);
        a[i] = __shfl(cv[i / K], i % K, K);
      }
      g[i] = (gathers && p0 + i < e) ? V[int64_t(col) * k + m] : T(0);
    }
#pragma unroll
    for (int i = 0; i < S; ++i)
      if (p0 + i < e) s = s + a[i] * g[i];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      ci[r] = ni[r];
      cv[r] = nv[r];
    }
  }
  return s;
}

// The short rows of a CSR of `rows` rows: out(r, j) = epi(sum_e val_e V[idx_e, j]).
template <typename T, int K, class Epi>
__global__ __launch_bounds__(kBlockNT) void k_block_pass(int rows, const int* __restrict__ ptr,
                                                         const int* __restrict__ idx, const T* __restrict__ val,
                                                         const T* __restrict__ V, int k, Epi epi) {
  if constexpr (BlkGuarded<Epi>::value)
    if (epi.stop()) return;
  constexpr int G = kBlockNT / K;
  const int g = int(threadIdx.x) / K, m = int(threadIdx.x) % K;
  const int64_t r = int64_t(blockIdx.x) * G + g;
  if (r >= rows) return;
  const int b = ptr[r], e = ptr[r + 1];
  if (e - b > kBlockLongRow) return;   // k_block_long's
  const T s = block_row_sum<T, K>(idx, val, V, k, m, b, e);
  if (m < k) epi.row(r, m, k, s);
}

// The long rows: workgroup b sums row longrows[b] by segments.
template <typename T, int K, class Epi>
__global__ __launch_bounds__(kBlockLongNT) void k_block_long(const int* __restrict__ longrows,
                                                             const int* __restrict__ ptr,
                                                             const int* __restrict__ idx, const T* __restrict__ val,
                                                             const T* __restrict__ V, int k, Epi epi) {
  if constexpr (BlkGuarded<Epi>::value)
    if (epi.stop()) return;
  constexpr int G = kBlockLongNT / K;
  __shared__ T part[kBlockLongNT];
  const int g = int(threadIdx.x) / K, m = int(threadIdx.x) % K;
  const int r = longrows[blockIdx.x];
  const int lb = ptr[r], le = ptr[r + 1];
  const int seg = (le - lb + G - 1) / G;           // block_segment(len, K)
  const int64_t sb64 = int64_t(lb) + int64_t(g) * seg;
  const int sb = sb64 < le ? int(sb64) : le;
  const int se = sb64 + seg < le ? int(sb64 + seg) : le;
  part[threadIdx.x] = block_row_sum<T, K>(idx, val, V, k, m, sb, se);
  __syncthreads();
  if (g == 0 && m < k) {
    T s = part[m];
#pragma unroll 4
    for (int c = 1; c < G; ++c) s = s + part[c * K + m];
    epi.row(r, m, k, s);
  }
}

// Y[i, j] = l2_j * V[i, j] (0 where l2_j == 0, without reading V): the HVP of a
// matrix without nonzeros.
template <typename T>
__global__ void k_block_l2v(int64_t len, int k, BlkHvpOut<T> epi) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < len * k; i += int64_t(gridDim.x) * blockDim.x)
    epi.row(i / k, int(i % k), k, T(0));
}

}  // namespace krcn
