// krcn_gram.hpp — the dense Hessian as one weighted Gram product over the dense
// image of X^T (krcn_dense.hpp): H = X^T diag(w) X / n + l2 I, with
// v_mfma_f64_16x16x4_f64.  Geometry and its reasons: krcn_gram_geom.hpp;
// DESIGN.md §18.
//
// One 256-thread workgroup owns the 64 x 64 output tile (ta, tb), tb >= ta, over
// the slabs of its split.  Both operand panels are rows of the same image
// (rows a0 .. a0 + 63 and b0 .. b0 + 63, entries r0 .. r0 + 31 of each): lane
// t % VPR of row t / VPR (+ 256 / VPR per further vector) loads one 16-byte
// vector, so neighbouring lanes read neighbouring 16 bytes of a row.  The
// vectors are widened to double, the b panel is multiplied by w_r (one rounding,
// as the reference's A.T * weights) and both go to LDS rows of 34 doubles.  The
// loads of slab s + 1 are issued before slab s is multiplied and stored to the
// other buffer after it: one barrier per slab.
//
// Lane maps of v_mfma_f64_16x16x4_f64 (they differ from every f32 form): lane l
// holds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15], one double each; its
// four results are D[(l >> 4) + 4 reg][l & 15].  Wave v of the workgroup owns
// the quadrant (v >> 1, v & 1) of the tile as 2 x 2 such products.
//
// Sum order of one entry (fixed by the shape and the split alone): the slabs of
// a split ascending, inside a slab k ascending, every term one fused
// multiply-add of x_ra and the rounded w_r x_rb into the running sum; split
// sums are added in split order by k_gram_reduce.  No atomics.
//
// Edges: image rows at or past d and entries at or past ld are not read (zeros
// stand in); w is not read at or past n (zero stands in, so nothing stale beyond
// w meets the image's zero padding between n and ld, which may be read).
#pragma once
#include "krcn_dense.hpp"
#include "krcn_gram_geom.hpp"

namespace krcn {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kGramNT = 256;
constexpr int kGramPanel = kGramT * kGramLd;          // doubles of one staged panel
constexpr int kGramCtLd = kGramT + 1;                 // the finished tile in LDS: the mirror reads columns
constexpr int kGramLds = 4 * kGramPanel;              // a | b panels, two buffers (the tile reuses them)
static_assert(kGramT * kGramCtLd <= kGramLds, "the finished tile fits the staging buffers");
static_assert(kGramT == 64 && kGramNT == 256, "four waves, one 32 x 32 quadrant each");

struct GramArgs {
  const void* img;      // d rows of ld stored values
  int64_t d, n, ld;
  int64_t slabs;
  int split;
  double n_global, l2;
  double* H;            // d x d
  double* ws;           // split > 1: raw tiles, (tile * split + s) * T * T
};

// Writes tile (ta, tb) from its finished sums ct (LDS, kGramCtLd doubles per
// row): H[a][b] = s / n + l2 [a == b] for the tile's entries with b >= a, then
// the mirrors H[b][a] from the same sums, with the column of ct on the lanes so
// that both passes store along a row of H.  Every entry of the tile and of its
// mirror is written exactly once.
__device__ __forceinline__ void gram_store(const double* ct, int64_t ta, int64_t tb, const GramArgs& g) {
  const int64_t a0 = ta * kGramT, b0 = tb * kGramT;
  const bool diag = ta == tb;
  for (int idx = threadIdx.x; idx < kGramT * kGramT; idx += kGramNT) {
    const int i = idx >> 6, j = idx & 63;
    const int64_t a = a0 + i, b = b0 + j;
    if (a < g.d && b < g.d && (!diag || b >= a)) {
      double v = ct[i * kGramCtLd + j] / g.n_global;
      if (a == b) v += g.l2;
      g.H[a * g.d + b] = v;
    }
  }
  for (int idx = threadIdx.x; idx < kGramT * kGramT; idx += kGramNT) {
    const int j = idx >> 6, i = idx & 63;
    const int64_t a = a0 + i, b = b0 + j;
    if (a < g.d && b < g.d && (!diag || b > a)) g.H[b * g.d + a] = ct[i * kGramCtLd + j] / g.n_global;
  }
}

template <typename TS, typename TW>
__global__ __launch_bounds__(kGramNT) void k_gram(GramArgs g, const TW* __restrict__ w) {
  using DV = DenseVec<TS>;
  using V = typename DV::V;
  constexpr int VW = DV::VW;
  constexpr int VPR = kGramKS / VW;                 // 16-byte vectors of a row per slab
  constexpr int RSTEP = kGramNT / VPR;              // rows between a thread's vectors
  constexpr int NV = kGramT / RSTEP;                // vectors per thread and panel
  __shared__ __attribute__((aligned(16))) double lds[kGramLds];

  const int64_t id = blockIdx.x;
  const int64_t tile = id / g.split;
  const int sp = int(id % g.split);
  int64_t ta, tb;
  gram_tile_of(tile, ta, tb);
  const int64_t a0 = ta * kGramT, b0 = tb * kGramT;
  int64_t s0, s1;
  gram_split_range(g.slabs, g.split, sp, s0, s1);

  const int tid = threadIdx.x;
  const int vcol = tid % VPR, vrow = tid / VPR;
  const TS* img = static_cast<const TS*>(g.img);

  V ra[NV], rb[NV];
  double wq[VW];
  auto fetch = [&](int64_t slab) {
    const int64_t e = slab * kGramKS + int64_t(vcol) * VW;
    const bool in = e < g.ld;                       // ld is a whole number of vectors
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int64_t a = a0 + vrow + i * RSTEP, b = b0 + vrow + i * RSTEP;
      ra[i] = in && a < g.d ? *reinterpret_cast<const V*>(img + a * g.ld + e) : V(0);
      rb[i] = in && b < g.d ? *reinterpret_cast<const V*>(img + b * g.ld + e) : V(0);
    }
#pragma unroll
    for (int q = 0; q < VW; ++q) wq[q] = e + q < g.n ? double(w[e + q]) : 0.0;
  };
  auto stage = [&](int buf) {
    double* pa = lds + buf * 2 * kGramPanel;
    double* pb = pa + kGramPanel;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      TS xa[VW], xb[VW];
      DV::unpack(ra[i], xa);
      DV::unpack(rb[i], xb);
      const int o = (vrow + i * RSTEP) * kGramLd + vcol * VW;
#pragma unroll
      for (int q = 0; q < VW; q += 2) {
        f64x2 va, vb;
        va.x = double(xa[q]);
        va.y = double(xa[q + 1]);
        vb.x = double(xb[q]) * wq[q];
        vb.y = double(xb[q + 1]) * wq[q + 1];
        if constexpr (kGramLd % 2 == 0) {   // rows start on 16 bytes: one store per pair
          *reinterpret_cast<f64x2*>(pa + o + q) = va;
          *reinterpret_cast<f64x2*>(pb + o + q) = vb;
        } else {
          pa[o + q] = va.x;
          pa[o + q + 1] = va.y;
          pb[o + q] = vb.x;
          pb[o + q + 1] = vb.y;
        }
      }
    }
  };

  const int lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int li = lane & 15, lk = lane >> 4;
  f64x4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f64x4(0.0);

  if (s0 < s1) {
    fetch(s0);
    stage(0);
  }
  __syncthreads();
  for (int64_t s = s0; s < s1; ++s) {
    const int cur = int((s - s0) & 1);
    const bool more = s + 1 < s1;
    if (more) fetch(s + 1);
    const double* pa = lds + cur * 2 * kGramPanel + (wr * 32 + li) * kGramLd + lk;
    const double* pb = lds + cur * 2 * kGramPanel + kGramPanel + (wc * 32 + li) * kGramLd + lk;
#pragma unroll
    for (int kk = 0; kk < kGramKS / 4; ++kk) {
      double fa[2], fb[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        fa[m] = pa[m * 16 * kGramLd + kk * 4];
        fb[m] = pb[m * 16 * kGramLd + kk * 4];
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[mi], fb[ni], acc[mi][ni], 0, 0, 0);
    }
    if (more) stage(cur ^ 1);
    __syncthreads();
  }

  // the finished sums to LDS (every wave has passed its last fragment read)
  double* ct = lds;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        ct[(wr * 32 + mi * 16 + lk + 4 * reg) * kGramCtLd + wc * 32 + ni * 16 + li] = acc[mi][ni][reg];
  __syncthreads();
  if (g.split == 1) {
    gram_store(ct, ta, tb, g);
  } else {
    double* out = g.ws + id * (kGramT * kGramT);
    for (int idx = tid; idx < kGramT * kGramT; idx += kGramNT) out[idx] = ct[(idx >> 6) * kGramCtLd + (idx & 63)];
  }
}

// split > 1: one workgroup per tile adds the split partials in split order and
// writes the tile as k_gram does at split 1.
__global__ __launch_bounds__(kGramNT) void k_gram_reduce(GramArgs g) {
  __shared__ double ct[kGramT * kGramCtLd];
  const int64_t tile = blockIdx.x;
  int64_t ta, tb;
  gram_tile_of(tile, ta, tb);
  const double* p = g.ws + tile * g.split * (kGramT * kGramT);
  for (int idx = threadIdx.x; idx < kGramT * kGramT; idx += kGramNT) {
    double s = p[idx];
    for (int k = 1; k < g.split; ++k) s += p[int64_t(k) * (kGramT * kGramT) + idx];
    ct[(idx >> 6) * kGramCtLd + (idx & 63)] = s;
  }
  __syncthreads();
  gram_store(ct, ta, tb, g);
}

// n == 0 or nnz == 0: H = l2 I without reading the image.
__global__ __launch_bounds__(kGramNT) void k_gram_l2(int64_t d, double l2, double* __restrict__ H) {
  const int64_t total = d * d;
  for (int64_t i = int64_t(blockIdx.x) * kGramNT + threadIdx.x; i < total; i += int64_t(gridDim.x) * kGramNT)
    H[i] = i / d == i % d ? l2 : 0.0;
}

}  // namespace krcn
