// krcn_geom.hpp — the constants and small structs that host and device agree
// through: block shapes, tile caps, the LDS geometry of the window and jagged
// formats, the records a plan hands its kernels (TileDesc, WinSeg), the lane
// rule and the tuning-knob readers.  Host-only C++17 (it also builds with g++
// alone: krcn_layout.hpp and tests/native/layout_check.cpp); the kernel
// headers include it and keep everything that runs on the device.
#pragma once
#include <stdint.h>

#include <cstdlib>
#include <cstring>

#include "krcn.h"

// Functions that device code calls too.
#ifdef __HIPCC__
#define KRCN_HD __host__ __device__
#else
#define KRCN_HD
#endif

namespace krcn {

constexpr int kNumCUs = 256;   // MI355X: 8 XCDs x 32 CUs
constexpr int kNT = 256;           // threads per block for every kernel here
constexpr int kMaxPartials = 2048;  // upper bound on blocks of a reducing launch

// k_rows_apply (krcn_tiled.hpp): kApplyU rows a thread per round, on
// apply_grid(rows) blocks.
constexpr int kApplyU = 4;
inline int apply_grid(int64_t rows) {
  int64_t b = (rows + int64_t(kNT) * kApplyU - 1) / (int64_t(kNT) * kApplyU);
  return int(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

// A/B tuning knobs (the variants of DESIGN.md's measurements) are read from
// the environment only in tuning builds (make variant EXTRA_FLAGS=-DKRCN_TUNING);
// the product library runs the measured defaults whatever the environment holds.
inline const char* tuning_env(const char* name) {
#ifdef KRCN_TUNING
  return getenv(name);
#else
  (void)name;
  return nullptr;
#endif
}
// The three readings of a knob: a number (dflt when unset; V is int, int64_t
// or double; field f of a comma-separated list), a switch that is on unless
// set to 0, one that is off unless set to 1.  A site keeps the value in a
// function-local static and checks its range.
template <typename V>
inline V tuning_value(const char* name, V dflt, int field = 0) {
  const char* e = tuning_env(name);
  for (; e && field > 0; --field)
    if ((e = std::strchr(e, ',')) != nullptr) ++e;
  return e ? V(std::atof(e)) : dflt;
}
inline bool tuning_on(const char* name) {
  const char* e = tuning_env(name);
  return !(e && e[0] == '0');
}
inline bool tuning_off(const char* name) {
  const char* e = tuning_env(name);
  return e && e[0] == '1';
}

// Lanes per row: the largest power of two <= mean row length / 8, in [1, 64]
// (measured on news20 / rcv1 shapes: 6.7 nnz/row -> 1, 57 -> 4, 74 -> 8).
inline int auto_lanes(int64_t rows, int64_t nnz) {
  const double mean = rows > 0 ? double(nnz) / double(rows) : 0.0;
  int L = 1;
  while (L < 64 && double(L * 2) * 8.0 <= mean) L *= 2;
  return L;
}

inline int resolve_lanes(int policy, int64_t rows, int64_t nnz) {
  if (policy == KRCN_LANES_AUTO) return auto_lanes(rows, nnz);
  if (policy == KRCN_LANES_SEQUENTIAL) return 1;
  return policy;
}

// ------------------------------------------------------------ tiles (krcn_tiled.hpp)
// One tile: rows [row0, row1) of slice `slice`, nonzeros [p0, p1) of the
// pass's CSR arrays; long_row != 0 marks a single row with more than
// kWaveTileNnz nonzeros.  32 bytes: one scalar load per tile.
struct __attribute__((aligned(32))) TileDesc {
  int slice, long_row, row0, row1, p0, p1, pad0, pad1;
};

constexpr int kWaveTileNnz = 512;                    // nonzeros per wave tile
constexpr int kWaveTileRows = 128;                   // rows per wave tile (cap)
constexpr int kWavesPerBlock = kNT / 64;

constexpr int kCombineRows = 128;
constexpr int kCombineSpread = 256;   // one row range per CU (MI355X: 256 CUs)
inline int combine_rows(int rows) {
  const int R = (rows + kCombineSpread - 1) / kCombineSpread;
  return R < 1 ? 1 : (R > kCombineRows ? kCombineRows : R);
}
// at most one block per CU: past 256 x 128 rows a block walks several ranges
// (each block runs the source prologue, e.g. the beta reduction, once)
inline int combine_grid(int rows) {
  const int R = combine_rows(rows);
  const int g = (rows + R - 1) / R;
  return g < 1 ? 1 : (g > kCombineSpread ? kCombineSpread : g);
}

constexpr int kSortPerThread = 8;
constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v / 2); }
template <int NT> struct SortGeom {
  static constexpr int kTile = NT * kSortPerThread;   // nonzeros per block tile / sort segment
  static constexpr int kRows = kTile / 4;             // rows per block tile (cap)
  static constexpr int kRowRegs = (kRows + 1 + NT - 1) / NT;   // row pointers per thread
  static constexpr int kSlotBits = ilog2(kTile);
  static_assert((1 << kSlotBits) == kTile, "slot field must address a whole tile");
  // packed word: (column - tile's column base) << kSlotBits | slot
  static constexpr int64_t kMaxWindow = int64_t(1) << (32 - kSlotBits);
};

// ------------------------------------------------------------ LDS windows (krcn_window.hpp)
struct __attribute__((aligned(16))) WinSeg {
  int slice, t0, t1, flags;   // flags: kSegLoad | kSegFlush | (segments of the block << 8, first entry only)
};
enum { kSegLoad = 1, kSegFlush = 2 };

constexpr int kWinNT = 1024;                 // one block per CU (the window takes the LDS)
constexpr int kWinWaves = kWinNT / 64;
constexpr int kWinChunk = 256;               // nonzeros per staging step (4 per lane)
constexpr int kWinTMax = 6;                  // accumulate mode: tiles per wave (register sums)
constexpr int kWinPad = kWinChunk + 8;       // array padding: unconditional chunk loads stay in bounds
constexpr int kWinRing = 3;                  // chunk slots in flight per wave (slices mode)
#ifndef KRCN_WIN_CLAIM
#define KRCN_WIN_CLAIM 1
#endif
constexpr int kWinClaimRun = KRCN_WIN_CLAIM; // slices mode: consecutive tiles a wave takes per claim (win_claim_run)
// LDS: window + 16 slabs of kWinChunk + the reduction scratch must fit 160 KiB
template <typename T> struct WinGeom {
  static constexpr int kSlabBytes = kWinWaves * kWinChunk * int(sizeof(T));
  static constexpr int kBytes = 163840 - kSlabBytes - 256;
  static constexpr int kW = kBytes / int(sizeof(T));      // max window (fp64 16,352; fp32 36,800)
  static constexpr int kPer = (kW + kWinNT - 1) / kWinNT;  // window entries per thread
  static_assert(kW <= 65536, "16-bit slice-local offsets");
};

// Slices mode: block b's slice and row chunk.  kpb == 0: b = slice + S chunk
// (S a multiple of 8 and kpb a power of two: the slice's blocks share an XCD,
// b % 8).  Else (round 5: 85 slices x 3 blocks) the blocks of XCD b % 8 take
// consecutive slots of a slice-major numbering (slot = kpb slice + chunk):
// slot = (slots of the XCDs before b's) + b / 8, so a slice's blocks share
// an XCD except where its slots straddle two XCDs.  G = the grid.
KRCN_HD inline void win_block_slice(int b, int G, int S, int kpb, int& slice, int& chunk) {
  if (kpb == 0) {
    slice = b % S;
    chunk = b / S;
    return;
  }
  const int x = b % 8, q = G / 8, r = G % 8;
  const int slot = x * q + (x < r ? x : r) + b / 8;
  slice = slot / kpb;
  chunk = slot % kpb;
}

// Slices mode: how a block's waves share the tiles [t0, t1) of its segment
// (win_stream).  The first ring fill is dealt statically — wave w takes tiles
// t0 + w + kWinWaves k, k < kWinRing, those below t1 — and the rest, the pool
// [win_claim_start, t1), is handed out by one LDS counter per block that
// counts the claims drawn: claim c = 0, 1, ... (whichever wave draws it) takes
// win_claim_run's tiles, `run` consecutive ones.  A wave goes on claiming
// until a claim reaches t1 (and a few claims further: its look-ahead), so
// claims past the pool are drawn; they denote no tiles.
KRCN_HD inline int win_claim_start(int t0, int t1) {
  const int n = t1 - t0, p = kWinWaves * kWinRing;
  return t0 + (n < p ? (n > 0 ? n : 0) : p);
}
// Tile k < kWinRing of wave w's static deal, or -1 where the segment ends before it.
KRCN_HD inline int win_static_tile(int t0, int t1, int w, int k) {
  const int t = t0 + w + kWinWaves * k;
  return t < t1 ? t : -1;
}
struct WinRun {
  int first, n;   // tiles [first, first + n); n == 0: none (first is then the pool's end)
};
KRCN_HD inline WinRun win_claim_run(int t0, int t1, int c, int run = kWinClaimRun) {
  const int start = win_claim_start(t0, t1);
  const int pool = t1 > start ? t1 - start : 0;
  const int before = c <= pool / run ? c * run : pool;   // tiles of the claims before c, clamped (no overflow)
  const int taken = before < pool ? before : pool;
  const int left = pool - taken;
  return WinRun{start + taken, left < run ? left : run};
}
// The tile whose bounds a wave reads for tile t: t itself below t1, else the
// segment's last tile (at least 0), whose bounds are loaded and not used.
KRCN_HD inline int win_tile_clamp(int t, int t1) {
  t = t < t1 ? t : t1 - 1;
  return t > 0 ? t : 0;
}

// The per-block X^T copies of one-piece window-accum plans (EpiLz1X).
constexpr int kXtChunk = 4;
constexpr int kXtRowCap = kWinWaves * kWinTMax * 64;   // rows of one accumulate block (<= 96 tiles of <= 64)
constexpr unsigned short kXtPad = 0xFFFF;
template <typename T> struct XtGeom {
  static constexpr int kChunks = WinGeom<T>::kW - kWinNT - kXtRowCap;   // chunk sums in LDS past lu
};

// ------------------------------------------------------------ jagged format (krcn_jag.hpp)
constexpr int kJagNT = 1024;                     // one block per CU: the window takes the LDS
constexpr int kJagWaves = kJagNT / 64;
constexpr int kJagLdsBytes = 163840 - 256;       // window(s); 256 B stay for the block reduction
constexpr int kJagPieces = kJagLdsBytes / 16;    // 16-byte pieces of window: 10,224
constexpr int kJagSlab = 128;                    // accumulate mode: elements per unit (products slab)
constexpr int kJagPad = 2 * kJagSlab;            // element arrays' padding (unit loads past the end)

// Variants (host and device agree through these):
//   single window (k_jag_pass): K <= 6 groups per wave, 2 chunks of 8 levels,
//                               8-bit counts
//   accumulate (k_jag_acc):     K = 4 or 8 groups per wave, <= 128 elements
//                               per unit, 8-bit counts
#ifndef KRCN_JAG_CPG
#define KRCN_JAG_CPG 2   // static chunks per unit of K >= 3 plans (A/B: variant builds)
#endif
constexpr int kJagK1 = 6, kJagCPG1 = KRCN_JAG_CPG, kJagLC = 8;
// the first kJagCPGU chunks of a unit are loaded whatever its counts; later
// static chunks only when some lane of the wave has levels there (a wave-
// uniform test).  Measured (round 6, -DKRCN_JAG_CPG=3): news20's X^T rows
// (Poisson, mean 6.7) pass 16 levels in 3.9 % of the 64-row groups, so most
// blocks wait for one synchronous overflow round trip — but a third static
// chunk makes the fused Lanczos pass 2 spill 44 B and run 27.9 -> 38.9 us
// (profiles/r06ag_news20_cpg3_ab.txt); the default stays 2
constexpr int kJagCPGU = 2;
// K <= 2 plans (rcv1's X^T: rows to 60 levels) keep 2 static chunks and run
// the overflow one chunk ahead instead (a third static chunk would spill)
constexpr int jag_cpg(int K) { return K <= 2 ? 2 : kJagCPG1; }
constexpr int kJagK2 = 8;                        // largest accumulate K (4 when the groups allow)
// Single window, long rows: rows with more than kJagLong elements leave the
// lane-per-row units (a 64-row group would wait for its longest row) and are
// summed by whole waves in tasks of kJagTask elements, <= kJagLongTasks tasks a
// block (their partials sit in LDS past the window).
constexpr int kJagLong = 32, kJagTask = 128, kJagLongTasks = 256;

template <typename T> struct JagGeom {
  static constexpr int kE = 16 / int(sizeof(T));                       // entries per piece
  static constexpr int kW1 = kJagPieces * kE;                          // single window (fp64 20,448)
  static constexpr int kR1 = (kJagPieces + kJagNT - 1) / kJagNT;       // piece loads per thread
  // accumulate: two windows beside the 16 per-wave product slabs
  static constexpr int kPieces2 = (kJagLdsBytes - kJagWaves * (kJagSlab + 2) * int(sizeof(T))) / 32;
  static constexpr int kW2 = kPieces2 * kE;                            // fp64 9,200; fp32 19,424
  static constexpr int kR2 = (kPieces2 + kJagNT - 1) / kJagNT;
  static_assert(kW1 <= 65536, "16-bit slice-local offsets");
};

}   // namespace krcn
