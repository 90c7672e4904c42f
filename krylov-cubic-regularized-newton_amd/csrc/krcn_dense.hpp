// krcn_dense.hpp — the dense pass format (KRCN_FORMAT_DENSE): geometry and kernels.
//
// A dense pass owns a row-major image of its matrix (X for pass 1, X^T for
// pass 2): `rows` rows of `ld` entries, ld the column count rounded up to whole
// 16-byte vectors, entries absent from the CSR stored as exact zeros.  No
// index bytes, row pointers or tiles: a row is a contiguous run of vectors.
//
//  * Lanes.  A row is summed by L lanes (a power of two, 1..64), a wave holds
//    64 / L rows and a 256-thread block 256 / L (one "row group").  Lane `sub`
//    of a row loads the 16-byte vectors sub, sub + L, ... of the row's slice,
//    so neighbouring lanes read neighbouring 16 bytes, kDenseU of them in
//    flight per lane before the first multiply.
//  * Slices.  A pass with few long rows is cut into S column slices of whole
//    vectors (slice k holds vectors [nvec k / S, nvec (k + 1) / S)); block b
//    runs slice b % S of row groups b / S, b / S + grid / S, ...  Slices store
//    per-slice row sums (EpiSlicePart), which the slice combine of the other
//    formats adds in slice order before the epilogue.
//
// Row-sum order (deterministic, independent of the grid): lane `sub` adds the
// products of its vectors left to right, entry by entry; the L lane sums go
// through the xor butterfly of k_tiled_pass; slice sums are added in slice
// order.  L = 1 with S = 1 is one left-to-right sum per row: scipy's
// csr_matvec order for finite vectors (the stored zeros add +-0, which changes
// no sum that starts from +0).
//
// Stored width (krcn_csr_set_value_storage).  The image's values have a stored
// type TS of their own: the arithmetic type T, or float under T = double
// (KRCN_VALUES_F32).  A narrowed image holds static_cast<float>(v) and has the
// geometry of an fp32 image (four entries per 16-byte vector); the kernel
// widens each stored value to double, which is exact, so vectors, products and
// sums stay fp64 and the pass computes with double(float(A)).  The order above
// holds with four entries per vector.
#pragma once
#include <cstddef>
#include <cstdint>

#include "krcn.h"

namespace krcn {

constexpr int kDenseNT = 256;        // threads per block (= kNT)
constexpr int kDenseU = 8;           // 16-byte matrix loads in flight per lane: a wave holds 8 KiB, and the
                                     // >= 4 waves a CU runs reach the ~32 KiB that keep HBM streaming
// ... under fp32 values and fp64 arithmetic (KRCN_VALUES_F32), where a matrix vector brings two 16-byte
// loads of the gathered vector with it: 12 loads in flight per lane.  gisette, us per HVP / Lanczos call:
// 41.3 / 517 at 4, 45.1 / 621 at 5, 52.8 / 661 at 8 (-DKRCN_DENSE_U_NARROW=...: the A/B of DESIGN.md §11)
#ifndef KRCN_DENSE_U_NARROW
#define KRCN_DENSE_U_NARROW 4
#endif
constexpr int kDenseUNarrow = KRCN_DENSE_U_NARROW;
constexpr int kDenseLaneVecs = 4;    // AUTO lanes: the smallest L that leaves a lane <= this many vectors
#if defined(KRCN_DENSE_LDS) && KRCN_DENSE_LDS
constexpr int kDenseMaxGrid = 768;   // LDS-staging A/B build: 3 blocks per CU, each stages its slice of x once
#else
constexpr int kDenseMaxGrid = 2048;  // blocks of a launch (<= kMaxPartials); further row groups are strided
#endif
constexpr int kDenseFewGroups = 128; // AUTO slices: passes with fewer row groups than this are sliced ...
constexpr int kDenseWantBlocks = 256;   // ... towards one block per CU ...
constexpr int64_t kDenseSliceVecs = 256;  // ... while a slice keeps >= 4 KiB of every row

// Geometry of one dense pass over a rows x cols matrix.
struct DenseGeom {
  int64_t ld = 0;      // entries per image row (a multiple of 16 / vs, vs the stored bytes per value; >= cols)
  int64_t nvec = 0;    // 16-byte vectors per row
  int L = 1, S = 1;    // lanes per row, column slices
  int64_t width = 0;   // entries of the widest slice (whole vectors; S * width >= cols)
  int64_t groups = 1;  // row groups (256 / L rows each)
  int grid = 1;        // blocks of the main launch (a multiple of S)
  int64_t bytes = 0;   // device bytes of the image (saturates at INT64_MAX)
};

inline int dense_auto_lanes(int64_t vecs) {
  int L = 1;
  while (L < 64 && int64_t(L) * kDenseLaneVecs < vecs) L *= 2;
  return L;
}

// lanes: KRCN_LANES_AUTO / _SEQUENTIAL or an explicit power of two 2..64;
// slicing: KRCN_SLICING_AUTO / _OFF or a forced slice count.  Pure host
// arithmetic (exported as krcn_dense_geometry).
inline DenseGeom dense_geometry(int64_t rows, int64_t cols, size_t vs, int lanes, int slicing) {
  DenseGeom g;
  const int64_t vw = int64_t(16 / vs);
  g.nvec = (cols + vw - 1) / vw;
  g.ld = (g.nvec > 0 ? g.nvec : 1) * vw;
  const bool seq = lanes == KRCN_LANES_SEQUENTIAL;
  auto groups_of = [&](int L) {
    const int64_t rpb = kDenseNT / L;
    const int64_t q = (rows + rpb - 1) / rpb;
    return q < 1 ? int64_t(1) : q;
  };
  int64_t S = 1;
  if (seq || slicing == KRCN_SLICING_OFF) {
    S = 1;
  } else if (slicing != KRCN_SLICING_AUTO) {
    S = slicing;                                   // forced: every slice keeps at least one vector
  } else {
    const int L0 = lanes == KRCN_LANES_AUTO ? dense_auto_lanes(g.nvec) : lanes;
    const int64_t q = groups_of(L0);
    if (q < kDenseFewGroups) S = (kDenseWantBlocks + q - 1) / q;
    if (S > g.nvec / kDenseSliceVecs) S = g.nvec / kDenseSliceVecs;
  }
  if (S > g.nvec) S = g.nvec;
  if (S < 1) S = 1;
  g.S = int(S);
  const int64_t wv = (g.nvec + S - 1) / S;         // vectors of the widest slice
  g.width = (wv > 0 ? wv : 1) * vw;
  g.L = seq ? 1 : (lanes == KRCN_LANES_AUTO ? dense_auto_lanes(wv) : lanes);
  g.groups = groups_of(g.L);
  // blocks per slice: at most kDenseMaxGrid / S, every block the same number of row groups (+- 1)
  const int64_t cap = kDenseMaxGrid / S > 1 ? kDenseMaxGrid / S : 1;
  const int64_t rounds = (g.groups + cap - 1) / cap;
  g.grid = int(((g.groups + rounds - 1) / rounds) * S);
  const int64_t r1 = rows > 0 ? rows : 1;
  const int64_t row_bytes = g.ld * int64_t(vs);
  g.bytes = r1 > INT64_MAX / row_bytes ? INT64_MAX : r1 * row_bytes;
  return g;
}

}  // namespace krcn

#ifdef __HIPCC__
#include "krcn_tiled.hpp"

namespace krcn {

// Matrix stream: plain loads (-DKRCN_DENSE_NT=1: nontemporal, the A/B of DESIGN.md §11).
#ifndef KRCN_DENSE_NT
#define KRCN_DENSE_NT 0
#endif
#if KRCN_DENSE_NT
#define KRCN_DENSE_LOAD(p) __builtin_nontemporal_load(p)
#else
#define KRCN_DENSE_LOAD(p) (*(p))
#endif
// Gathered vector: read through L1 / L2 with the matrix's own vector indices
// (-DKRCN_DENSE_LDS=1: the slice is staged in LDS first, the other A/B).
#ifndef KRCN_DENSE_LDS
#define KRCN_DENSE_LDS 0
#endif
constexpr int kDenseLdsBytes = 48 * 1024;   // KRCN_DENSE_LDS: the largest slice staged (wider ones read L1 / L2)

template <typename T> struct DenseVec;
template <> struct DenseVec<double> {
  static constexpr int VW = 2;
  using V = f64x2;
  __device__ __forceinline__ static void unpack(const V& q, double (&o)[2]) { o[0] = q.x; o[1] = q.y; }
};
template <> struct DenseVec<float> {
  static constexpr int VW = 4;
  using V = f32x4;
  __device__ __forceinline__ static void unpack(const V& q, float (&o)[4]) {
    o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
  }
};

struct DenseArgs {
  int rows, S, groups;
  int64_t cols, ld, nvec;
  const void* mat;
};

// Entries [c, c + VW) of the gathered vector x (cols entries, any alignment),
// VW the entries of one 16-byte vector of the stored type TS: 16-byte loads
// (one when TS = T, two for fp32 values under fp64 arithmetic) where the vector
// is whole and x is 16-byte aligned (c is a multiple of VW), guarded scalar
// loads otherwise — x is never read at or past cols (the image's padding
// multiplies zeros).
template <typename T, typename TS>
__device__ __forceinline__ void dense_x(const T* __restrict__ x, int64_t c, int64_t cols, bool aligned,
                                        T (&o)[DenseVec<TS>::VW]) {
  using DV = DenseVec<T>;
  constexpr int VW = DenseVec<TS>::VW;
  if (aligned && c + VW <= cols) {
#pragma unroll
    for (int q = 0; q < VW / DV::VW; ++q) {
      T part[DV::VW];
      DV::unpack(*reinterpret_cast<const typename DV::V*>(x + c + q * DV::VW), part);
#pragma unroll
      for (int e = 0; e < DV::VW; ++e) o[q * DV::VW + e] = part[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < VW; ++e) o[e] = c + e < cols ? x[c + e] : T(0);
  }
}

// T: the arithmetic type (vectors, products, sums); TS: the stored type of the
// image (T itself, or float under T = double: KRCN_VALUES_F32, each stored
// value widened to double, which is exact, before its fp64 product).
template <typename T, typename TS, int L, class Src, class Epi>
__global__ __launch_bounds__(kDenseNT) void k_dense_pass(DenseArgs a, Src src, Epi epi,
                                                         double* __restrict__ partials) {
  using DV = DenseVec<TS>;
  using V = typename DV::V;
  constexpr int VW = DV::VW;
  constexpr int kU = sizeof(TS) == sizeof(T) ? kDenseU : kDenseUNarrow;
  constexpr int kRowsPerWave = 64 / L, kRowsPerBlock = kDenseNT / L;
  __shared__ double sm[kDenseNT / 64];
  if constexpr (HasPreload<Src>::value) src.preload();
  if (src.begin(sm)) return;
  const T* __restrict__ x = src.get();
  epi.init(src);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int sub = lane & (L - 1), grp = lane / L;
  const int slice = blockIdx.x % a.S;
  const int64_t v0 = a.nvec * slice / a.S, v1 = a.nvec * (slice + 1) / a.S;
  const int nv = int(v1 - v0);
  const int64_t c0 = v0 * VW;
  const bool aligned = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
#if KRCN_DENSE_LDS
  // the slice of x as whole vectors in LDS (zeros past cols), read back with the matrix's vector indices
  __shared__ __attribute__((aligned(16))) T xs[kDenseLdsBytes / sizeof(T)];
  const bool staged = int64_t(nv) * VW * int64_t(sizeof(T)) <= kDenseLdsBytes;
  if (staged) {
    for (int i = threadIdx.x; i < nv * VW; i += kDenseNT) xs[i] = c0 + i < a.cols ? x[c0 + i] : T(0);
    __syncthreads();
  }
#endif
  const TS* __restrict__ mat = static_cast<const TS*>(a.mat);
  typename RedOf<Epi>::type acc{};
  const int gstride = gridDim.x / a.S;
  for (int rg = blockIdx.x / a.S; rg < a.groups; rg += gstride) {
    const int64_t r64 = int64_t(rg) * kRowsPerBlock + wave * kRowsPerWave + grp;
    const bool live = r64 < a.rows;
    const int r = int(r64);
    typename Epi::Pre pf{};
    if (sub == 0 && live) pf = epi.pre(r);
    T s = T(0);
    if (live) {
      const V* __restrict__ row = reinterpret_cast<const V*>(mat + r64 * a.ld + c0);
      for (int k = sub; k < nv; k += L * kU) {
        V m[kU];
        T xv[kU][VW];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int i = k + u * L;
          m[u] = KRCN_DENSE_LOAD(row + (i < nv ? i : k));
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          const int i = k + u * L;
          if (i < nv) {
#if KRCN_DENSE_LDS
            if (staged) dense_x<T, TS>(xs, int64_t(i) * VW, int64_t(nv) * VW, true, xv[u]);
            else
#endif
            dense_x<T, TS>(x, c0 + int64_t(i) * VW, a.cols, aligned, xv[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          if (k + u * L < nv) {
            TS mv[VW];
            DV::unpack(m[u], mv);
#pragma unroll
            for (int e = 0; e < VW; ++e) s += T(mv[e]) * xv[u][e];
          }
        }
      }
    }
    if constexpr (L > 1) {
#pragma unroll
      for (int off = L / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, L);
    }
    if (sub == 0 && live) acc += epi.row(r, s, slice, pf);
  }
  if constexpr (Epi::kReduce) {
    store_block_red<kDenseNT>(acc, sm, partials, epi);
  }
}

// Image build: img[r * ld + idx[e]] = val[e] over the CSR's nonzeros, one wave
// per row (the image is zero-filled first; a repeated entry would keep one of
// its values, not their sum — unsupported, as elsewhere in the library).
// TS: the stored type (a narrowed image rounds each value to nearest even).
template <typename T, typename TS>
__global__ __launch_bounds__(kDenseNT) void k_dense_scatter(int rows, const int* __restrict__ ptr,
                                                            const int* __restrict__ idx, const T* __restrict__ val,
                                                            int64_t ld, TS* __restrict__ img) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = int64_t(blockIdx.x) * (kDenseNT / 64) + (threadIdx.x >> 6);
  const int64_t nw = int64_t(gridDim.x) * (kDenseNT / 64);
  for (int64_t r = w0; r < rows; r += nw) {
    const int b = ptr[r], e = ptr[r + 1];
    for (int p = b + lane; p < e; p += 64) img[r * ld + idx[p]] = static_cast<TS>(val[p]);
  }
}

}  // namespace krcn
#endif  // __HIPCC__
