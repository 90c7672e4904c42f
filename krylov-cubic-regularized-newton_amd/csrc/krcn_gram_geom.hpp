// krcn_gram_geom.hpp — how the dense Hessian's Gram product is cut (krcn_gram.hpp,
// krcn_gram.hip): output tiles, K slabs, K splits, the grid and the workspace of
// the split partials.  Plain C++17, no HIP header: it also builds with g++ under
// the host sanitizers (tests/native/gram_geom_check.cpp).
//
// H = X^T diag(w) X / n + l2 I over the d x ld image of X^T.  H is symmetric, so
// only the nt (nt + 1) / 2 tiles (ta, tb) with tb >= ta are computed; a tile
// writes its mirror too.  The summed index r in [0, n) is walked in slabs of
// kGramKS entries; with `split` > 1 the slabs are dealt to `split` workgroups
// per tile, whose raw sums a second kernel adds in split order.
#pragma once
#include <cstdint>

#include "krcn_geom.hpp"

namespace krcn {

// Output tile edge.  64 x 64 per 256-thread workgroup: each of the four waves
// owns a 32 x 32 quadrant = 2 x 2 MFMA tiles of 16 x 16, i.e. 16 accumulator
// doubles (32 registers) per lane, and every fragment read from LDS feeds two
// MFMAs.  A wider tile would halve the LDS reads per MFMA again, but the
// instruction is the bottleneck long before LDS is (one ds_read_b64 per
// v_mfma_f64_16x16x4_f64), and 64 keeps the tile count of mid-sized d
// (d = 1,100: 171 tiles) close to the CU count.
constexpr int kGramT = 64;
// Entries of r staged per step.  32 doubles = 256 bytes of every row: 16 lanes
// of a 16-byte load cover it (fp64), and a padded LDS row of KS + 2 doubles
// puts the 32 fragment reads of a half-wave (16 rows x 2 values of k) on 32
// different 8-byte banks.  Two panels x two buffers x 64 x 34 x 8 B = 69,632 B
// of LDS: two workgroups fit a CU's 160 KiB.
constexpr int kGramKS = 32;
#ifndef KRCN_GRAM_LD
#define KRCN_GRAM_LD (kGramKS + 2)   // A/B: variant builds with -DKRCN_GRAM_LD=33
#endif
constexpr int kGramLd = KRCN_GRAM_LD;   // doubles per LDS row
// A split keeps at least this many slabs (256 summed entries): below that the
// prologue, the partial's store (32 KiB) and the second kernel's reload cost
// more than the slabs they spread.  Reasoned, not measured.
constexpr int kGramMinSlabs = 8;
// Auto splits keep the partials at or under 256 MiB, the Infinity Cache size:
// the second kernel then reads what the first just wrote without a trip to
// HBM.  A forced split is honoured whatever it costs.
constexpr int64_t kGramWsCap = int64_t(256) << 20;
// Largest split: one workgroup per CU from a single tile.
constexpr int kGramMaxSplit = kNumCUs;

struct GramGeom {
  int T = kGramT, KS = kGramKS;
  int64_t nt = 0;        // tiles per side, ceil(d / T)
  int64_t tiles = 0;     // upper-triangle tiles, nt (nt + 1) / 2
  int64_t slabs = 0;     // ceil(n / KS)
  int split = 1;         // workgroups per tile
  int64_t grid = 0;      // tiles * split workgroups; workgroup g runs tile g / split, split g % split
  int64_t ws_bytes = 0;  // split > 1: tiles * split raw T x T tiles of doubles
};

// Linear tile id -> (ta, tb), tb >= ta, columns of the upper triangle one after
// the other: id = tb (tb + 1) / 2 + ta.  Needs no nt.
KRCN_HD inline int64_t gram_tile_id(int64_t ta, int64_t tb) { return tb * (tb + 1) / 2 + ta; }
KRCN_HD inline void gram_tile_of(int64_t id, int64_t& ta, int64_t& tb) {
  // the root of tb (tb + 1) / 2 <= id in floating point (exact to within one for
  // id < 2^52), then at most two corrections each way
  int64_t t = int64_t((__builtin_sqrt(8.0 * double(id) + 1.0) - 1.0) * 0.5);
  for (int i = 0; i < 2 && t * (t + 1) / 2 > id; ++i) --t;
  for (int i = 0; i < 2 && (t + 1) * (t + 2) / 2 <= id; ++i) ++t;
  tb = t;
  ta = id - t * (t + 1) / 2;
}

// Slabs [s0, s1) of split s of `split`: consecutive ranges that partition
// [0, slabs); a split beyond the slab count gets an empty range.
KRCN_HD inline void gram_split_range(int64_t slabs, int split, int s, int64_t& s0, int64_t& s1) {
  s0 = slabs * s / split;
  s1 = slabs * (s + 1) / split;
}

// The split the rule picks: 1 when the tiles already give every CU a workgroup,
// else the smallest split that does, while every split keeps kGramMinSlabs
// slabs and the partials stay under kGramWsCap.
inline int gram_auto_split(int64_t tiles, int64_t slabs) {
  if (tiles <= 0 || tiles >= kNumCUs) return 1;
  int64_t s = (kNumCUs + tiles - 1) / tiles;
  const int64_t by_slabs = slabs / kGramMinSlabs;
  if (s > by_slabs) s = by_slabs;
  const int64_t tile_bytes = int64_t(kGramT) * kGramT * 8;
  const int64_t by_bytes = kGramWsCap / (tiles * tile_bytes);
  if (s > by_bytes) s = by_bytes;
  if (s > kGramMaxSplit) s = kGramMaxSplit;
  return s < 1 ? 1 : int(s);
}

// forced_split: 0 = the rule, else 1..kGramMaxSplit taken as it is.
// 0 <= d <= 2^20 keeps every product below far from 2^63; n >= 0.
inline GramGeom gram_geometry(int64_t d, int64_t n, int forced_split) {
  GramGeom g;
  g.nt = (d + kGramT - 1) / kGramT;
  g.tiles = g.nt * (g.nt + 1) / 2;
  g.slabs = (n + kGramKS - 1) / kGramKS;
  g.split = forced_split > 0 ? forced_split : gram_auto_split(g.tiles, g.slabs);
  g.grid = g.tiles * g.split;
  g.ws_bytes = g.split > 1 ? g.grid * int64_t(kGramT) * kGramT * 8 : 0;
  return g;
}

}  // namespace krcn
