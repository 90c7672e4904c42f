// krcn_layout.hpp — the layout of the pass plans: the format policy and, per
// format, one function from the shape, the policy inputs and host row pointers
// to a plain struct of scalars and vectors (slices, cuts, tiles, segments,
// tasks, grids), or to a refusal (fail(KRCN_ERR_UNSUPPORTED, ..), kept in the
// struct's `refused`).  Integer arithmetic on the host only: nothing here
// touches a device, and the file builds with g++ alone
// (tests/native/layout_check.cpp runs it under ASan + UBSan).  The plan
// builders materialise what these functions return.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

#include "krcn_geom.hpp"
#include "krcn_host.hpp"

namespace krcn {

// ----------------------------------------------------------- pass plans
constexpr int64_t kSliceThresholdBytes = 3 << 20;   // gathered vector above this: slice
constexpr int64_t kSliceTargetBytes = 2 << 20;      // x window per slice
constexpr int kBlocksPerGroup = 256;                // sliced: 8 groups x 256 = 2048 blocks (8 per CU)
constexpr int kMaxGrid = 2048;

// Cut [0, n) into B ranges of equal weight by the prefix sums pre[0 .. n]:
// cut[b] is the first i with pre[i] >= pre[n] b / B (cut[0] = 0, cut[B] = n).
template <class Pre>
inline void balanced_cuts(const Pre& pre, int n, int B, int* cut) {
  cut[0] = 0;
  int i = 0;
  for (int b = 1; b < B; ++b) {
    const int64_t target = int64_t(pre[n]) * b / B;
    while (i < n && pre[i] < target) ++i;
    cut[b] = i;
  }
  cut[B] = n;
}

inline int slices_for(int64_t bytes) {
  if (bytes <= kSliceThresholdBytes) return 1;
  const int64_t per8 = 8 * kSliceTargetBytes;
  return int(8 * ((bytes + per8 - 1) / per8));
}

// Column bounds of S equal slices (build_slices' default; sorted tiles gather
// relative to their slice's first column).
inline int slice_base(int64_t cols, int sl, int S) { return int((cols * sl) / S); }

// Sorted tiles pay when the gathered window per slice is dense enough for a
// 2 K-nonzero tile to put several lanes on one cache line: at most
// kSortWindow entries per slice, and the slice partials (S x rows, written
// and re-read) cheap next to the matrix stream.
constexpr int64_t kSortWindowDefault = 24576;

inline int64_t sort_window() {
  static const int64_t w = [] {
    const int64_t v = tuning_value("KRCN_SORT_WINDOW", int64_t(0));   // tuning knob
    return v >= 1024 ? v : kSortWindowDefault;
  }();
  return w;
}

inline int sorted_slices(int64_t cols) {
  const int64_t kSortWindow = sort_window();
  if (cols <= kSortWindow) return 1;
  const int64_t per8 = 8 * kSortWindow;
  return int(8 * ((cols + per8 - 1) / per8));
}

// The wave / sorted tile formats of one pass: which of the two, its slices,
// XCD groups, lanes and block size.
struct TilePolicyIn {
  int fmt, pass, lanes, slicing;   // the pass's KRCN_FORMAT_*, 1 / 2, the handle's lane and slicing policies
  int sort_nt;                     // the handle's sorted block size (0: by the nonzero count)
  bool sharded, p1_unsliced;
  size_t vs;                       // the handle's value size
};
struct TilePolicy {
  bool sorted = false;
  int S = 1, groups = 1, L = 1, sort_nt = 256;
};
// hp: the pass's CSR row pointers (rows + 1), read by the skew-aware lane rule.
inline TilePolicy tile_policy(int rows, int64_t cols, int64_t nnz, const TilePolicyIn& in, const int* hp) {
  const bool seq = in.lanes == KRCN_LANES_SEQUENTIAL;
  const int fmt = in.fmt, pass = in.pass;
  TilePolicy P;
  bool sorted = false;
  int S_sorted = sorted_slices(cols);
  // sharded passes run without the fused step B, so the slices' combine is
  // pure overhead while the gathered vector is L2-sized: a news20 rank of 8
  // (170 K columns, 1.36 MB) ran 27.4 k HVP/s unsliced against 25.3 k sliced;
  // a rank of 4 (2.7 MB) 20.4 k against 23.8 k
  if (in.sharded && cols * int64_t(in.vs) <= int64_t(3) << 19) S_sorted = 1;
  // pass 1 beside a single-window jagged pass 2: unsliced sorted tiles (no
  // slice partials, no combine launch: the two-launch Lanczos step)
  if (pass == 1 && in.p1_unsliced) S_sorted = 1;
  if (in.slicing >= 8) S_sorted = in.slicing;
  // largest block tile that still leaves >= one tile per CU
  int sort_nt = in.sort_nt;
  if (sort_nt == 0)
    sort_nt = nnz >= int64_t(kNumCUs) * 1024 * kSortPerThread ? 1024
              : nnz >= int64_t(kNumCUs) * 512 * kSortPerThread ? 512 : 256;
  const int64_t max_window = sort_nt == 256 ? SortGeom<256>::kMaxWindow
                             : sort_nt == 512 ? SortGeom<512>::kMaxWindow : SortGeom<1024>::kMaxWindow;
  const bool one_slice = in.slicing == KRCN_SLICING_OFF || seq;
  if (one_slice) S_sorted = 1;
  // the packed gather word addresses kSortMaxWindow columns past a slice's base
  while (!one_slice && (cols + S_sorted - 1) / S_sorted >= max_window) S_sorted = S_sorted < 8 ? 8 : S_sorted + 8;
  const bool sortable = (cols + S_sorted - 1) / S_sorted < max_window;
  const bool unsliced_pick = pass == 1 && in.p1_unsliced && S_sorted == 1;
  if (fmt == KRCN_FORMAT_SORTED && sortable) {
    sorted = true;
  } else if (fmt == KRCN_FORMAT_AUTO && !seq && nnz > 0) {
    const double part_bytes = S_sorted > 1 ? 16.0 * double(S_sorted) * double(rows) : 0.0;
    const double mat_bytes = double(nnz) * (in.vs + sizeof(int));
    const int64_t window = (cols + S_sorted - 1) / S_sorted;
    sorted = (window <= sort_window() || unsliced_pick) && part_bytes <= 0.25 * mat_bytes;
  }
  if (sorted) {
    P.S = S_sorted;
  } else if (seq || in.slicing == KRCN_SLICING_OFF) {
    P.S = 1;
  } else if (in.slicing >= 8) {
    P.S = in.slicing;
  } else {
    P.S = slices_for(cols * int64_t(in.vs));
  }
  if (P.S > 1 && cols < P.S) P.S = 1;
  P.sorted = sorted;
  P.sort_nt = sort_nt;
  P.groups = P.S > 1 ? 8 : 1;
  // a sliced row holds ~1/S of its nonzeros: pick lanes from the slice-local mean
  P.L = resolve_lanes(in.lanes, int64_t(rows) * P.S, nnz);
  if (sorted && in.lanes == KRCN_LANES_AUTO && pass == 1 && rows > 0 && nnz > 0) {
    // skewed rows: a row's lane group walks ceil(len / L) staged products,
    // so a wave waits on the longest of its rows, not on the mean one. When
    // the nonzero-weighted mean row (sum len^2 / nnz) is >= 2x the plain
    // mean, lanes come from 4x the weighted slice-local mean (auto_lanes: the
    // largest L with 8 L <= that): rcv1 with a power-law row tail (max 2160,
    // mean 71, weighted 189, 8 slices: 94) takes L = 8, 37.0 -> 28.4 us per
    // HVP, best of L = 1..32 on two boxes (L = 4 29.4, L = 16 30.8; calibrated
    // on this one tail shape;
    // profiles/r06aa_rcv1skew_lanes.txt); uniform rows (ratio 1.0) keep the
    // plain mean (rcv1: L = 1 18.0 us, L = 4 19.0 us)
    double sq = 0.0;
    for (int r = 0; r < rows; ++r) {
      const double len = double(hp[r + 1] - hp[r]);
      sq += len * len;
    }
    const double mean = double(nnz) / double(rows);
    const double wmean = sq / double(nnz);
    if (wmean >= 2.0 * mean) P.L = std::max(P.L, auto_lanes(int64_t(P.S), int64_t(4.0 * wmean)));
  }
  return P;
}

// Tile list (host greedy over the row pointers), grouped by XCD group.
// Wave tiles: <= kWaveTileNnz nonzeros in the 4-aligned window, <= kWaveTileRows
// rows.  Sorted block tiles: <= kSortTile nonzeros, <= kSortTileRows rows, and
// `segs` receives the sort segments (a normal tile, or kSortTile chunks of a
// long row) as nonzero offsets, `segbase` their slice's first column.
struct TileLayout {
  std::vector<TileDesc> tiles;     // group by group
  std::vector<int> tbeg, tmid;     // groups + 1 tile offsets; sorted: first single-long-row tile of each group
  std::vector<int> segs, segbase;  // sorted only
  int ntiles = 0, grid = 1;
};
// hp: the slice-major row pointers (S * rows + 1).
inline TileLayout tile_layout(int rows, int64_t cols, const TilePolicy& tp, const int* hp) {
  const int S = tp.S, groups = tp.groups;
  const bool sorted = tp.sorted;
  const int sort_tile = tp.sort_nt * kSortPerThread;
  const int cap_nnz = sorted ? sort_tile : kWaveTileNnz;
  const int cap_rows = sorted ? sort_tile / 4 : kWaveTileRows;
  const int per_block = sorted ? 1 : kWavesPerBlock;
  const size_t nptr = size_t(S) * rows + 1;
  TileLayout out;
  auto win = [&](const int* rp, int a, int b) { return sorted ? rp[b] - rp[a] : rp[b] - (rp[a] & ~3); };
  // Greedy tiling of one slice with nonzero cap `cap`; emit(long, r0, r1).
  auto walk = [&](int sl, int cap, auto&& emit) {
    const int* rp = hp + size_t(sl) * rows;
    int r = 0;
    while (r < rows) {
      // a tile's nonzero window must fit one wave slab / block tile
      if (win(rp, r, r + 1) > cap) {
        emit(1, r, r + 1);
        ++r;
        continue;
      }
      int r1 = r + 1;
      while (r1 < rows && r1 - r < cap_rows && win(rp, r, r1 + 1) <= cap) ++r1;
      emit(0, r, r1);
      r = r1;
    }
  };
  // Sorted tiles run one resident wave of B blocks per XCD group: shrink
  // the tiles of a group until its tile count fills whole rounds of B blocks
  // (smallest cap with count(cap) <= R * B, R = rounds at the full tile), so
  // no block runs a last round alone.
  // sorted tiles: one resident wave of blocks (8 waves per SIMD)
  const int per_group = sorted ? kBlocksPerGroup * kNT / tp.sort_nt : kBlocksPerGroup;
  const int max_grid = sorted ? kMaxGrid * kNT / tp.sort_nt : kMaxGrid;
  std::vector<int> gcap(groups, cap_nnz);
  if (sorted) {
    const int B = groups > 1 ? per_group : max_grid;
    for (int g = 0; g < groups; ++g) {
      auto count = [&](int cap) {
        int64_t c = 0;
        for (int sl = g; sl < S; sl += groups) walk(sl, cap, [&](int, int, int) { ++c; });
        return c;
      };
      const int64_t n0 = count(cap_nnz);
      if (n0 == 0) continue;
      const int64_t R = (n0 + B - 1) / B;
      if (R < 2) continue;   // a single partial round: keep the tiles whole
      int lo = std::max(64, cap_nnz / 16), hi = cap_nnz;   // count(hi) <= R * B
      if (count(lo) <= R * B) { gcap[g] = lo; continue; }
      while (hi - lo > 32) {
        const int mid = (lo + hi) / 2;
        if (count(mid) <= R * B) hi = mid; else lo = mid;
      }
      gcap[g] = hi;
    }
  }
  std::vector<std::vector<TileDesc>> per(groups);
  for (int sl = 0; sl < S; ++sl) {
    const int* rp = hp + size_t(sl) * rows;
    const int g = sl % groups;
    // sorted tiles gather relative to their slice's first column (slice_bounds)
    const int base = sorted ? slice_base(cols, sl, S) : 0;
    auto seg = [&](int c) {
      out.segs.push_back(c);
      out.segbase.push_back(base);
    };
    walk(sl, gcap[g], [&](int lng, int r0, int r1) {
      per[g].push_back(TileDesc{sl, lng, r0, r1, rp[r0], rp[r1], base, 0});
      if (!sorted) return;
      if (lng) {
        for (int c = rp[r0]; c < rp[r1]; c += sort_tile) seg(c);
      } else if (rp[r1] > rp[r0]) {
        seg(rp[r0]);
      }
    });
  }
  if (sorted) out.segs.push_back(hp[nptr - 1]);
  out.tbeg.assign(groups + 1, 0);
  out.tmid.assign(groups, 0);
  int maxg = 0;
  for (int g = 0; g < groups; ++g) {
    out.tbeg[g] = int(out.tiles.size());
    // sorted tiles: ordinary tiles first, single long rows after tmid[g]
    if (sorted)
      std::stable_partition(per[g].begin(), per[g].end(), [](const TileDesc& d) { return d.long_row == 0; });
    int nshort = 0;
    for (const TileDesc& d : per[g]) nshort += d.long_row == 0;
    out.tmid[g] = out.tbeg[g] + nshort;
    out.tiles.insert(out.tiles.end(), per[g].begin(), per[g].end());
    maxg = std::max<int>(maxg, int(per[g].size()));
  }
  out.tbeg[groups] = int(out.tiles.size());
  out.ntiles = int(out.tiles.size());
  const int units = (maxg + per_block - 1) / per_block;
  if (groups > 1)
    out.grid = groups * std::max(1, std::min(units, per_group));
  else
    out.grid = std::max(1, std::min((out.ntiles + per_block - 1) / per_block, max_grid));
  return out;
}

// ------------------------------------------------------ LDS-window plans
// (krcn_window.hpp.)  Slices of W columns, 16-bit slice-local offsets, tiles
// of R rows, and per-block segment lists.
//   accum:  S = ceil(cols / Wmax) slices of equal width; blocks own contiguous
//           tile ranges of equal nonzero count and walk every slice over them
//           (row sums carry across slices: no partials).
//   slices: S = the smallest divisor of 256 >= ceil(cols / Wmax) (or, past
//           256, a multiple of 8), k = 256 / S blocks per slice, each owning a
//           nonzero-balanced row range of it; block s + S c holds chunk c of
//           slice s, so a slice's blocks share an XCD (b % 8) and its window
//           is fetched from HBM once per XCD.  Per-slice partial row sums,
//           combined in slice order by k_slice_combine.
constexpr int kWinTileCost = 24;   // fixed per-tile work, in nonzero equivalents

inline int win_slices_mode(int64_t cols, int64_t Wmax, int* k_out) {
  const int64_t smin = (cols + Wmax - 1) / Wmax;
  // A/B knob: blocks per slice (S = 256 / k slices, e.g. k = 3: 85)
  static const int k_env = tuning_value("KRCN_WIN_KPB", 0);
  if (k_env >= 2 && k_env <= 8 && kNumCUs / k_env >= smin) {
    *k_out = k_env;
    return kNumCUs / k_env;
  }
  // 65-85 slices needed (news20: 83): 85 slices x 3 blocks (255 blocks,
  // XCD-packed, win_block_slice) instead of 128 x 2 — a third fewer slice
  // partials (20.5 -> 13.6 MB written and re-read per pass on news20) for a
  // 50 % larger window per block; interleaved on one box 16.6-17.3 k against
  // 16.5-17.1 k HVP/s, the combine 6.6-6.8 us against 7.7-7.8
  // (profiles/r05h_news20_kpb_ab.txt; KRCN_WIN_KPB=2 restores 128 x 2)
  if (k_env == 0 && smin > kNumCUs / 4 && smin <= kNumCUs / 3) {
    *k_out = 3;
    return kNumCUs / 3;
  }
  static const int s_env = tuning_value("KRCN_WIN_MIN_SLICES", 0);   // A/B knob: minimum slice count (a power of two)
  for (int S = 8; S <= kNumCUs; S *= 2)
    if (S >= smin && S >= s_env) { *k_out = kNumCUs / S; return S; }
  for (int S = 8; S <= kNumCUs; S *= 2)
    if (S >= smin) { *k_out = kNumCUs / S; return S; }
  *k_out = 1;
  return int(8 * ((smin + 7) / 8));
}

// 0: no window format, 1: accumulate, 2: slices (auto policy).
inline double slice_min_mat() {   // matrix bytes below which slices + combine do not pay
  static const double v = tuning_value("KRCN_SLICE_MIN_MB", 48.0) * 1e6;   // A/B knob
  return v;
}
inline int window_choice(int rows, int64_t cols, int64_t nnz, size_t vs) {
  if (nnz == 0 || rows == 0 || cols == 0) return 0;
  const int64_t Wmax = vs == 8 ? WinGeom<double>::kW : WinGeom<float>::kW;
  const int64_t S = (cols + Wmax - 1) / Wmax;
  const double mean = double(nnz) / (double(rows) * double(S));   // nonzeros per row and slice
  if (mean > 24.0) return 0;                 // one lane per row: short rows only
  const double mat = double(nnz) * double(vs + 2);
  const double win = double(std::min<int64_t>(cols, Wmax)) * double(vs);
  if (S <= 4 && double(kNumCUs) * double(S) * win <= mat) return 1;
  int k = 1;
  const int Ss = win_slices_mode(cols, Wmax, &k);
  const double part = 2.0 * double(Ss) * double(rows) * double(vs);
  const double wbytes = double(Ss) * double(k) * double((cols + Ss - 1) / Ss) * double(vs);
  // partials (written once, read once by the combine) up to 1.25x the matrix
  // bytes still pay against cache-served gathers: synth 2M x 1M (100 nnz per
  // row, part / mat = 1.02) HVP 2,753 -> 2,173 us against the wave format
  // and the combine launch (≈5 us of latency) must be small next to the pass:
  // rcv1's X^T (15 MB) ran 34.9 us per HVP with window slices + combine
  // against 29.6 us with unsliced sorted tiles (tools/lz_fmt.py)
  if (Ss > 1 && part <= 1.25 * mat && wbytes <= 0.6 * mat && mat >= slice_min_mat()) return 2;
  return 0;
}
// The forced window format (KRCN_FORMAT_WINDOW): 1 accumulate, 2 slices.
template <typename T>
inline int window_forced(int64_t cols) {
  const int64_t W = WinGeom<T>::kW;
  return (cols + W - 1) / W <= 4 ? 1 : 2;
}

// Step 1, from the shape: the slices (build_slices cuts the CSR at `bounds`).
struct WinShape {
  int S = 1, W = 0, kpb = 1, kind = KRCN_PLAN_WINDOW_ACCUM;
  std::vector<int> bounds;   // S + 1 column bounds
};
template <typename T>
inline WinShape win_shape(int64_t cols, int accum) {
  const int64_t Wmax = WinGeom<T>::kW;
  WinShape sh;
  if (accum) {
    sh.S = int((cols + Wmax - 1) / Wmax);
  } else {
    sh.S = win_slices_mode(cols, Wmax, &sh.kpb);
  }
  sh.W = int((cols + sh.S - 1) / sh.S);
  sh.kind = accum ? KRCN_PLAN_WINDOW_ACCUM : KRCN_PLAN_WINDOW_SLICES;
  sh.bounds.resize(sh.S + 1);
  for (int k = 0; k <= sh.S; ++k) sh.bounds[k] = int(std::min<int64_t>(int64_t(k) * sh.W, cols));
  return sh;
}

// Step 2, from the slice-major row pointers hp (S * rows + 1): the tiles and
// every block's segment list.
//   accumulate: tiles of R rows, the same in every slice (tile t: rows
//           [t R, t R + R)); ntiles = ceil(rows / R).
//   slices: every slice has its own tiles, given by their row starts (trow).
//           Fixed tiles of R rows are one case (every slice alike).  Data-cut
//           tiles (`datacut`) are the other: a tile is the longest run of
//           consecutive rows of its slice with at most kWinTileRows rows whose
//           nonzeros, counted from the 4-aligned element win_load starts at,
//           fit one staging chunk ((e0 & 3) + nnz <= kWinChunk); a row that
//           alone exceeds a chunk is its own tile (the extra-chunk loop).
//           Tile counts then differ from slice to slice: tcount holds them,
//           ntiles is the largest (the stride of tb / trow, and what
//           krcn_csr_plan_info reports), R the lane cap kWinTileRows.
constexpr int kWinTileRows = 64;   // rows of a tile: one lane per row
struct WinLayout {
  krcn_status refused = KRCN_OK;
  int R = 64, ntiles = 0, stride = 1, grid = 1, kpb = 0;
  bool datacut = false;
  std::vector<WinSeg> segs;   // block b runs segs[b * stride + i]
  std::vector<int> cut;       // accumulate: grid + 1 tile cuts (block b owns tiles [cut[b], cut[b + 1]))
  std::vector<int> trow;      // slices: S x (ntiles + 1) tile row starts (past a slice's count: rows)
  std::vector<int> tcount;    // slices: S tile counts
};
// Row starts of the data-cut tiles of one slice (rp: its rows + 1 absolute row
// pointers), with the closing entry `rows`.
inline void win_cut_tiles(const int* rp, int rows, std::vector<int>& out) {
  out.clear();
  int r = 0;
  while (r < rows) {
    out.push_back(r);
    const int64_t lo = rp[r] & ~3;
    int r1 = r + 1;
    while (r1 < rows && r1 - r < kWinTileRows && int64_t(rp[r1 + 1]) - lo <= kWinChunk) ++r1;
    r = r1;
  }
  out.push_back(rows);
}
// forced: the tiling a caller asks for instead of the rule's (tuning builds'
// KRCN_WIN_R, the layout tests): 16 / 32 / 64 fixed rows, 1 data-cut tiles
// (slices mode), 0 the rule.
inline WinLayout win_layout(const WinShape& sh, int rows, int64_t nnz, const int* hp, int forced = 0) {
  const int S = sh.S, kpb = sh.kpb;
  const bool accum = sh.kind == KRCN_PLAN_WINDOW_ACCUM;
  WinLayout L;
  // rows per tile: up to one staging chunk of nonzeros per tile and slice.
  // The tile stream is latency-bound (a wave keeps two tiles' chunks in
  // flight), so the tiles are taken as large as a chunk allows: news20's X
  // (3.55 nonzeros per row and slice, 227 per 64-row tile) ran its fused
  // pass 1 in 32.5 us with 64-row tiles against 38.0 us with 32-row tiles
  // (profiles/r03_news20_winR.txt); the few tiles past 256 take one extra chunk.
  const double mean = double(nnz) / (double(rows) * double(S));
  L.R = mean * 64.0 <= 0.95 * kWinChunk ? 64 : mean * 32.0 <= 0.95 * kWinChunk ? 32 : 16;
  // A/B knob: 16 / 32 / 64 rows per tile, 1 data-cut tiles (slices mode)
  if (forced == 0) forced = tuning_value("KRCN_WIN_R", 0);
  if (forced == 16 || forced == 32 || forced == 64) L.R = forced;
  const int R = L.R;
  const int nfixed = (rows + R - 1) / R;
  // Slices mode, data-cut tiles.  A fixed R below 64 leaves the chunks partly
  // empty: the rule above only knows 16 / 32 / 64, and where 64 mean rows pass
  // a chunk it halves them (news20 at 85 slices: 5.35 nonzeros per row and
  // slice, 171 of 256 slots a tile), yet every tile pays its loads, gathers,
  // slab writes and row walk for all 256.  Tiles cut from the data fill the
  // chunk (news20: 0.67 -> 0.985, 625 -> ~424 tiles a slice).  They are taken
  // where the fixed rule gives R < 64 and the fixed tiling gives a slice's
  // blocks kWinWaves * kWinRing tiles each on average (the cuts balance
  // nonzeros, so a block's count scatters round that mean): a wave with
  // fewer than kWinRing tiles never fills its ring, the stream is start-up
  // and not fill.  At R = 64 the fixed tiles are already row-capped.
  L.datacut = !accum && (forced == 1 || (forced == 0 && R < kWinTileRows &&
                                         int64_t(nfixed) >= int64_t(kpb) * kWinWaves * kWinRing));
  if (L.datacut) L.R = kWinTileRows;
  int ntiles = nfixed;
  if (!accum) {
    std::vector<std::vector<int>> starts(static_cast<size_t>(S));
    for (int sl = 0; sl < S; ++sl) {
      std::vector<int>& st = starts[size_t(sl)];
      if (L.datacut) {
        win_cut_tiles(hp + size_t(sl) * rows, rows, st);
      } else {
        for (int t = 0; t < nfixed; ++t) st.push_back(t * R);
        st.push_back(rows);
      }
    }
    if (L.datacut) {
      ntiles = 0;
      for (int sl = 0; sl < S; ++sl) ntiles = std::max(ntiles, int(starts[size_t(sl)].size()) - 1);
    }
    L.tcount.resize(size_t(S));
    L.trow.assign(size_t(S) * (size_t(ntiles) + 1), rows);
    for (int sl = 0; sl < S; ++sl) {
      const std::vector<int>& st = starts[size_t(sl)];
      L.tcount[size_t(sl)] = int(st.size()) - 1;
      std::copy(st.begin(), st.end(), L.trow.begin() + size_t(sl) * (size_t(ntiles) + 1));
    }
  }
  L.ntiles = ntiles;
  auto tcount = [&](int sl) { return accum ? ntiles : L.tcount[size_t(sl)]; };
  auto tnnz = [&](int sl, int t) -> int64_t {
    const int* rp = hp + size_t(sl) * rows;
    const int* tr = accum ? nullptr : L.trow.data() + size_t(sl) * (size_t(ntiles) + 1);
    const int r0 = accum ? t * R : tr[t], r1 = accum ? std::min(rows, r0 + R) : tr[t + 1];
    return int64_t(rp[r1]) - rp[r0];
  };
  // compact row pointers (16-bit row ends inside a tile): every tile of every
  // slice must hold < 65536 nonzeros, else the format does not apply
  for (int sl = 0; sl < S; ++sl)
    for (int t = 0; t < tcount(sl); ++t)
      if (tnnz(sl, t) > 65535) {
        L.refused = fail(KRCN_ERR_UNSUPPORTED, "window plan: a tile holds > 65535 nonzeros");
        return L;
      }
  // cut [0, n) into B ranges of equal cost(t) (prefix-sum cuts)
  auto cut_ranges = [&](int n, int B, auto&& cost) {
    std::vector<int64_t> pre(size_t(n) + 1, 0);
    for (int t = 0; t < n; ++t) pre[t + 1] = pre[t] + cost(t);
    std::vector<int> cut(B + 1, 0);
    balanced_cuts(pre, n, B, cut.data());
    return cut;
  };
  if (accum) {
    auto cost = [&](int t) {
      int64_t c = kWinTileCost * int64_t(S);
      for (int sl = 0; sl < S; ++sl) c += tnnz(sl, t);
      return c;
    };
    const int cap = kWinWaves * kWinTMax;   // tiles per block (register sums)
    int B = std::max(1, tuning_value("KRCN_WIN_ACC_B", kNumCUs));   // A/B knob: first grid tried
    for (;;) {
      L.cut = cut_ranges(ntiles, B, cost);
      int mx = 0;
      for (int b = 0; b < B; ++b) mx = std::max(mx, L.cut[b + 1] - L.cut[b]);
      if (mx <= cap || B >= 64 * kNumCUs) break;
      B += kNumCUs;
    }
    L.stride = S;
    L.segs.assign(size_t(B) * S, WinSeg{0, 0, 0, 0});
    for (int b = 0; b < B; ++b) {
      if (L.cut[b + 1] == L.cut[b]) continue;      // an empty block: segment count 0
      for (int sl = 0; sl < S; ++sl)
        L.segs[size_t(b) * S + sl] =
            WinSeg{sl, L.cut[b], L.cut[b + 1], kSegLoad | (sl == S - 1 ? kSegFlush : 0) | (sl == 0 ? S << 8 : 0)};
    }
    L.grid = B;
  } else {
    L.stride = 1;
    L.grid = S * kpb;
    L.kpb = (kpb & (kpb - 1)) != 0 ? kpb : 0;   // win_block_slice's mapping
    // a block whose row chunk is empty still names its slice (no segments to
    // run): the fused Lanczos prologue has it store its share of that slice
    std::vector<std::vector<int>> cuts(static_cast<size_t>(S));
    for (int sl = 0; sl < S; ++sl)
      cuts[size_t(sl)] = cut_ranges(tcount(sl), kpb, [&](int t) { return tnnz(sl, t) + kWinTileCost; });
    L.segs.resize(size_t(S) * kpb);
    for (int b = 0; b < L.grid; ++b) {
      int sl = 0, c = 0;
      win_block_slice(b, L.grid, S, L.kpb, sl, c);
      const std::vector<int>& cut = cuts[size_t(sl)];
      L.segs[size_t(b)] = cut[c + 1] > cut[c] ? WinSeg{sl, cut[c], cut[c + 1], kSegLoad | kSegFlush | (1 << 8)}
                                             : WinSeg{sl, 0, 0, 0};
    }
  }
  return L;
}

// One-piece window-accum plans (d <= kWinNT): each block's rows once more as a
// column-major copy, so the fused Lanczos pass 1 also forms the block's share
// of X^T u (EpiLz1X, krcn_window.hpp).  Every column's run (rows ascending) is
// padded to whole chunks of kXtChunk (value 0, row kXtPad); cp holds per
// block the cols + 1 absolute chunk ids.  Skipped when a block's chunk sums do
// not fit the LDS past the window and its rows.  The copy is made from the
// plan's own values (stored as TS) and holds them widened to T: under
// narrowed storage X^T u runs over the same rounded matrix as X z, in 8-byte
// entries (EpiLz1X and k_xt_combine are the full-width code).
template <typename T>
struct XtLayout {
  bool skipped = true;
  std::vector<int> cp;               // B x (cols + 1)
  std::vector<unsigned short> xr;    // row offsets in the block's rows, column-major per block
  std::vector<T> xv;
};
// hidx / hval: the plan's 16-bit column offsets and values; hp: its row
// pointers (one slice); cut: the accumulate layout's B + 1 tile cuts.
template <typename T, typename TS>
inline XtLayout<T> xt_layout(int rows, int R, int cols, const unsigned short* hidx, const TS* hval, const int* hp,
                             const std::vector<int>& cut, int B) {
  XtLayout<T> X;
  const size_t ncp = size_t(B) * (size_t(cols) + 1);
  std::vector<int> cp(ncp);
  std::vector<int> cnt(static_cast<size_t>(cols));
  int64_t chunks = 0;   // first pass: chunk ids
  for (int b = 0; b < B; ++b) {
    const int r0 = std::min(rows, cut[b] * R), r1 = std::min(rows, cut[b + 1] * R);
    if (r1 - r0 > kXtRowCap) return X;
    std::fill(cnt.begin(), cnt.end(), 0);
    for (int e = hp[r0]; e < hp[r1]; ++e) ++cnt[hidx[size_t(e)]];
    int* bcp = cp.data() + size_t(b) * (size_t(cols) + 1);
    const int64_t c0 = chunks;
    for (int c = 0; c < cols; ++c) {
      bcp[c] = int(chunks);
      chunks += (cnt[size_t(c)] + kXtChunk - 1) / kXtChunk;
    }
    bcp[cols] = int(chunks);
    if (chunks - c0 > XtGeom<T>::kChunks) return X;
    if (chunks * kXtChunk >= (int64_t(1) << 31)) return X;
  }
  std::vector<unsigned short> xr(size_t(chunks) * kXtChunk, kXtPad);
  std::vector<T> xv(size_t(chunks) * kXtChunk, T(0));
  std::vector<int64_t> pos(static_cast<size_t>(cols));
  for (int b = 0; b < B; ++b) {   // second pass: rows in order, so each column's run stays in row order
    const int r0 = std::min(rows, cut[b] * R), r1 = std::min(rows, cut[b + 1] * R);
    const int* bcp = cp.data() + size_t(b) * (size_t(cols) + 1);
    for (int c = 0; c < cols; ++c) pos[size_t(c)] = int64_t(bcp[c]) * kXtChunk;
    for (int r = r0; r < r1; ++r)
      for (int e = hp[r]; e < hp[r + 1]; ++e) {
        const int64_t k = pos[hidx[size_t(e)]]++;
        xr[size_t(k)] = static_cast<unsigned short>(r - r0);
        xv[size_t(k)] = T(hval[size_t(e)]);
      }
  }
  const size_t ne = std::max<size_t>(xr.size(), kXtChunk);
  xr.resize(ne, kXtPad);
  xv.resize(ne, T(0));
  X.skipped = false;
  X.cp = std::move(cp);
  X.xr = std::move(xr);
  X.xv = std::move(xv);
  return X;
}

// ------------------------------------------------------ jagged plans
// (krcn_jag.hpp.)  S = 1 when the gathered vector fits one LDS window (fp64:
// 20,448 entries), else S slices of W <= 10,224 entries that every block
// walks over its own rows (double-buffered windows, register row sums).
constexpr int kJagGroupCost = 96;   // fixed work per group and slice, in nonzero equivalents

// KRCN_JAG (A/B knob): 0 never by the auto policy, 1 the cost model (default),
// 2 every pass the format can run
inline int jag_env() {
  static const int v = tuning_value("KRCN_JAG", 1);
  return v;
}

template <typename T>
inline int jag_slices(int64_t cols, int* W_out) {
  constexpr int kE = JagGeom<T>::kE;
  if (cols <= JagGeom<T>::kW1) {
    *W_out = int(cols);
    return 1;
  }
  const int64_t s0 = (cols + JagGeom<T>::kW2 - 1) / JagGeom<T>::kW2;
  int64_t W = (cols + s0 - 1) / s0;
  W = (W + kE - 1) / kE * kE;   // slice bases stay 16-byte aligned
  *W_out = int(W);
  return int((cols + W - 1) / W);
}

// Accumulate mode, slice groups: with G groups, block b walks the S / G
// slices of group b % G over row range b / G (256 / G ranges) and writes
// per-group partial row sums that k_slice_combine adds in group order.  More
// groups give each block fewer slices and more row groups per wave (K, at
// most 8).  Per-block time model, fitted on the synth passes at HEAD (round 3:
// pass 1 S = 109, K = 8: 485 us; pass 2 S = 218, K = 4: 608 us; pass 2 at
// G = 2, S = 109 a block, K = 8: 486-502 us with its combine): every slice
// costs ~1.13 us (window pieces, lane counts, the barrier) plus ~0.415 us per
// unit a wave carries.  G > 1 adds the group partials (written and read once)
// and a combine launch (~8 us); it changes the summation order (no longer
// scipy's), so it is taken only when the model gains 10 % or more.
template <typename T>
inline int jag_groups(int rows, int64_t cols, int64_t nnz, int S, int pass) {
  const double vs = double(sizeof(T));
  const int64_t groups = (int64_t(rows) + 63) / 64;
  constexpr double kSliceUs = 1.13, kUnitUs = 0.415, kCombineUs = 8.0, kPartBps = 5e12;
  int best = 0;
  double bc = 1e300;
  for (int G = 1; G <= 8 && G <= S; G *= 2) {
    const int R = std::max(1, kNumCUs / G);
    const int64_t per_block = (groups + R - 1) / R;
    const int64_t K = (per_block + kJagWaves - 1) / kJagWaves;
    if (K > kJagK2) continue;
    const double slices = double((S + G - 1) / G);
    double c = slices * (kSliceUs + double(std::max<int64_t>(K, 1)) * kUnitUs);
    if (G > 1) c = (c + 2.0 * G * double(rows) * vs / kPartBps * 1e6 + kCombineUs) / 0.9;
    if (c < bc) {
      bc = c;
      best = G;
    }
  }
  // An X^T pass whose window (the whole gathered vector, walked by every
  // block) outweighs a block's share of the matrix by more than half takes
  // two groups even where the model keeps one: the synth rank-of-8 pass 2
  // (250 K-entry u = 2 MB a block against 1 MB of matrix) ran 97.8-98.4 ->
  // 93.4-93.6 us per step with G = 2 (1 MB of window a block), 5,428-5,443 ->
  // 5,615-5,621 HVP/s (round 6, profiles/r06w_synth8_pass2_groups.txt;
  // a layout whose window bytes do not exceed its matrix
  // bytes).
  if (best == 1 && pass == 2 && S >= 2 && nnz >= (int64_t(1) << 23)) {   // (heavy passes only: >= 8 M nonzeros)
    const double win = double(cols) * vs, mat = double(nnz) * (vs + 2.0) / double(kNumCUs);
    const int64_t K2 = ((groups + kNumCUs / 2 - 1) / (kNumCUs / 2) + kJagWaves - 1) / kJagWaves;
    if (win > 1.5 * mat && K2 <= kJagK2) best = 2;
  }
  return best;
}

// Auto policy: enough row groups to give every wave work, short rows per
// slice (one lane per row), and — with several slices — a block's share of
// the matrix not small next to the windows it loads (L2/MALL-served).
// Single-window X^T passes (pass 2: the gathered u fits one LDS window) need
// only a row group per CU: rcv1's X^T (738 groups) ran 13.2 -> 10.5 us a pass
// on 123 blocks against the sorted tiles (interleaved, profiles/r03_rcv1_jag_ab.txt).
// Pass 1 keeps the full bar: a one-piece X z (w8a) keeps its fused step B.
constexpr int kJagS1MinGroupsXt = kNumCUs;
constexpr int kJagS1GroupsPerBlock = 6;   // below a group per wave: blocks of >= 6 groups
template <typename T>
inline bool jag_choice(int rows, int64_t cols, int64_t nnz, int pass) {
  const int mode = jag_env();
  if (mode == 0 || nnz == 0 || rows == 0 || cols < 16) return false;
  const int64_t G = (int64_t(rows) + 63) / 64;
  int W = 0;
  const int S = jag_slices<T>(cols, &W);
  const double mean = double(nnz) / double(rows) / double(S);   // elements per row and slice
  if (S == 1) {
    // A/B knob: KRCN_JAG_S1G=g sets the row groups a single-window plan needs
    static const int64_t genv = tuning_value("KRCN_JAG_S1G", 0);
    const bool relaxed = pass == 2 && sizeof(T) == 8;   // (fp32 rcv1 stress: 10.4 -> 14.7 us, kept off)
    const int64_t gmin = genv > 0 ? genv : relaxed ? int64_t(kJagS1MinGroupsXt) : int64_t(kNumCUs) * kJagWaves;
    return G >= gmin && mean <= 48.0;
  }
  if (G < int64_t(kNumCUs) * 4) return false;   // accumulate: >= 4 groups a block
  if (mean > 1.5) return false;   // a 64-row group's slice must fit the 128-entry products slab
  const int sg = jag_groups<T>(rows, cols, nnz, S, pass);
  if (sg == 0) return false;
  if (mode == 2) return true;
  const double mat = double(nnz) * double(sizeof(T) + 2) / double(kNumCUs);
  const double win = double(cols) * double(sizeof(T)) / sg;
  return mat >= 0.25 * win;
}

// Every choice of a jagged plan (slices, groups, K, the long-row rule, the
// grid) from the pass's CSR row pointers hp (rows + 1).
struct JagLayout {
  krcn_status refused = KRCN_OK;
  int S = 1, W = 0, SG = 1, Sg = 1;    // slices, their width, slice groups, slices per group
  int G = 0, R = 0, K = 0, B = 0;      // 64-row groups, row ranges, groups per wave, blocks (R x SG)
  int lpiece = 0, tcap = 0, lthr = 0;  // long rows: LDS piece of their partials, tasks a block can hold, the threshold
  int ubits = 1;
  int64_t NU = 0, nrec = 0, lnnz = 0;  // units, (block, slice, wave) records, elements of the long rows
  std::vector<int64_t> pre;            // G + 1 prefix sums of the groups' cost
  std::vector<int> cut, gblk;          // R + 1 group cuts; the row range of every group
  std::vector<int> lrows, ltask, lbeg; // long rows: row ids, first task, first element (+ 1 end entry each)
  std::vector<int> lcut, tasks;        // per block: long rows, then tasks (2 x (B + 1)); per task: start, count
};
template <typename T>
inline JagLayout jag_layout(int rows, int64_t cols, int64_t nnz, int pass, bool seq, const int* hp) {
  JagLayout J;
  if (cols < JagGeom<T>::kE || rows == 0 || nnz == 0) {
    J.refused = fail(KRCN_ERR_UNSUPPORTED, "jag plan: empty or too narrow (%lld columns)", (long long)cols);
    return J;
  }
  int W = 0;
  const int S = jag_slices<T>(cols, &W);
  const int Kmax = S == 1 ? kJagK1 : kJagK2;
  const int G = (rows + 63) / 64;
  // A/B knob: force the slice-group count of accumulate plans, KRCN_JAG_G=g
  // (both passes) or g1,g2 (pass 1 / pass 2; 0 keeps the cost model's)
  static const std::pair<int, int> g_env = [] {
    const int a = tuning_value("KRCN_JAG_G", 0);
    return std::make_pair(a, tuning_value("KRCN_JAG_G", a, 1));
  }();
  const int gf = pass == 1 ? g_env.first : g_env.second;
  // slice groups (their partials change the summation order: never under the
  // sequential lane policy, whose contract is scipy's order bit for bit)
  int SG = S == 1 || seq ? 1 : (gf > 0 ? std::min(gf, S) : jag_groups<T>(rows, cols, nnz, S, pass));
  if (SG == 0) SG = 1;                                       // (forced format: block count grows instead)
  const int Sg = (S + SG - 1) / SG;                          // slices per group
  // single window: rows longer than kJagLong are summed apart by whole waves
  // (jag_long_rows) when their task partials fit the LDS past the window.
  // Their wave-tree order is not scipy's, so the sequential lane policy keeps
  // such rows lane-per-row (a row over 255 elements then refuses the plan)
  std::vector<int>& lrows = J.lrows;
  const int lpiece = int((cols * int64_t(sizeof(T)) + 15) / 16);
  // task partials a block can keep in the LDS past the window (round 6: a
  // window within 256 tasks' partials of the LDS — rcv1's 20,242-entry u —
  // used to refuse the plan, and a skewed rcv1 X^T then ran sorted tiles at
  // 318 us a pass; a block now takes at most as many tasks as fit)
  const int tcap = std::min<int64_t>(kJagLongTasks, int64_t(kJagPieces - lpiece) * 16 / int64_t(sizeof(T)));
  // which rows go long: past kJagLong when the window leaves room for all 256
  // task partials (round 5's rule: news20's X^T); with less room only when some
  // row is longer than the 8-bit lane counts hold (> 254, since a count byte
  // of 0xFF marks a long row: a skewed rcv1's hot columns) —
  // sending a uniform rcv1's 33-60-element X^T rows to 128-element tasks cost
  // its pass 2 11.2 -> 17.5 us (profiles/r06t_bench_rcv1.json)
  int lthr = 0;
  if (S == 1 && !seq && tcap >= kJagWaves) {
    if (lpiece + kJagLongTasks * int(sizeof(T)) / 16 <= kJagPieces) {
      lthr = kJagLong;
    } else {
      // (the rows past 32 then go long too: a skewed rcv1 ran 24.6 k HVP/s so,
      // 19.7 k with only the rows past 254 long, r06t / r06t2)
      for (int r = 0; r < rows && lthr == 0; ++r)
        if (hp[r + 1] - hp[r] > 254) lthr = kJagLong;
    }
  }
  {
    // A/B knob KRCN_JAG_LONG=t: rows past t elements go long (8..254)
    static const int long_env = tuning_value("KRCN_JAG_LONG", 0);
    if (lthr > 0 && long_env >= 8 && long_env <= 254) lthr = long_env;
  }
  if (lthr > 0)
    for (int r = 0; r < rows; ++r)
      if (hp[r + 1] - hp[r] > lthr) lrows.push_back(r);
  std::vector<char> is_long(lrows.empty() ? 0 : size_t(rows), 0);
  for (int r : lrows) is_long[size_t(r)] = 1;
  std::vector<int64_t>& pre = J.pre;
  pre.assign(size_t(G) + 1, 0);
  for (int g = 0; g < G; ++g) {
    int64_t e = int64_t(hp[std::min(rows, 64 * (g + 1))]) - hp[64 * g];
    if (!lrows.empty())
      for (int r = 64 * g; r < std::min(rows, 64 * (g + 1)); ++r)
        if (is_long[size_t(r)]) e -= hp[r + 1] - hp[r];
    pre[g + 1] = pre[g] + e + int64_t(kJagGroupCost) * S;
  }
  // nonzero-balanced row ranges of at most 16 K groups (K per wave); the
  // grid is R ranges x SG slice groups
  const int Rstep = std::max(1, kNumCUs / SG);
  int R = std::min(G, Rstep), mx = 0;
  if (S == 1) {
    // fewer groups than waves: blocks of >= kJagS1GroupsPerBlock groups, so
    // fewer blocks load the whole window (A/B knob: KRCN_JAG_R=r caps them)
    static const int rcap = tuning_value("KRCN_JAG_R", 0);
    if (G < kNumCUs * kJagWaves) R = std::max(1, std::min(R, G / kJagS1GroupsPerBlock));
    if (rcap > 0) R = std::min(R, rcap);
  }
  std::vector<int>& cut = J.cut;
  for (;;) {
    cut.assign(size_t(R) + 1, 0);
    balanced_cuts(pre, G, R, cut.data());
    mx = 0;
    for (int b = 0; b < R; ++b) mx = std::max(mx, cut[b + 1] - cut[b]);
    if (mx <= kJagWaves * Kmax) break;
    if (R * SG >= 64 * kNumCUs) {
      J.refused = fail(KRCN_ERR_UNSUPPORTED, "jag plan: %d row groups exceed the block cap", G);
      return J;
    }
    R += Rstep;
  }
  const int B = R * SG;
  // the smallest unrolled variant the block's groups allow: a wave issues the
  // loads of all K unit slots whether they hold a group or not (a sharded
  // news20 X^T with 21 groups per block ran its jagged pass 2 at rank-of-4 in
  // the same 26 us as at rank-of-2 with K = 6)
  const int K = S == 1 ? (mx <= kJagWaves ? 1 : mx <= 2 * kJagWaves ? 2 : mx <= 3 * kJagWaves ? 3 : kJagK1)
                       : (mx <= kJagWaves * 4 ? 4 : 8);
  J.gblk.resize(G);
  for (int b = 0; b < R; ++b)
    for (int g = cut[b]; g < cut[b + 1]; ++g) J.gblk[g] = b;
  const int64_t NU = int64_t(B) * Sg * K * kJagWaves;   // units
  int ubits = 1;
  while ((int64_t(1) << ubits) <= NU) ++ubits;
  if (ubits + 22 > 63) {
    J.refused = fail(KRCN_ERR_UNSUPPORTED, "jag plan: too many units");
    return J;
  }
  J.S = S, J.W = W, J.SG = SG, J.Sg = Sg, J.G = G, J.R = R, J.K = K, J.B = B;
  J.lpiece = lpiece, J.tcap = tcap, J.lthr = lthr, J.ubits = ubits, J.NU = NU;
  J.nrec = int64_t(B) * Sg * kJagWaves;   // (block, slice, wave) records

  // long rows: tasks of kJagTask elements, rows cut into B contiguous ranges by
  // task count (a block's tasks' partials must fit its tcap LDS slots)
  const int nl = int(lrows.size());
  std::vector<int>&ltask = J.ltask, &lbeg = J.lbeg, &lcut = J.lcut, &tasks = J.tasks;
  if (nl > 0) {
    ltask.assign(size_t(nl) + 1, 0);
    lbeg.assign(size_t(nl) + 1, 0);
    for (int i = 0; i < nl; ++i) {
      const int len = hp[lrows[i] + 1] - hp[lrows[i]];
      ltask[i + 1] = ltask[i] + (len + kJagTask - 1) / kJagTask;
      lbeg[i + 1] = lbeg[i] + ((len + 1) & ~1);
      J.lnnz += len;
    }
    const int64_t tt = ltask[nl];
    lcut.assign(2 * (size_t(B) + 1), 0);
    balanced_cuts(ltask, nl, B, lcut.data());
    for (int bb = 0; bb <= B; ++bb) lcut[B + 1 + bb] = ltask[lcut[bb]];
    for (int bb = 0; bb < B; ++bb)
      if (lcut[B + 2 + bb] - lcut[B + 1 + bb] > tcap) {
        J.refused = fail(KRCN_ERR_UNSUPPORTED, "jag plan: a block's long rows need %d tasks (max %d)",
                         lcut[B + 2 + bb] - lcut[B + 1 + bb], tcap);
        return J;
      }
    tasks.assign(2 * (size_t(tt) + 1), 0);   // one spare entry: the clamped read of an empty block
    for (int k = 0; k < nl; ++k) {
      const int len = hp[lrows[k] + 1] - hp[lrows[k]];
      for (int t = ltask[k]; t < ltask[k + 1]; ++t) {
        const int off = (t - ltask[k]) * kJagTask;
        tasks[2 * size_t(t)] = lbeg[k] + off;
        tasks[2 * size_t(t) + 1] = std::min(kJagTask, len - off);
      }
    }
  }
  return J;
}

// The plan kinds that honour the handle's value storage policy.
inline bool plan_narrows(int kind) {
  return kind == KRCN_PLAN_DENSE || kind == KRCN_PLAN_WINDOW_SLICES || kind == KRCN_PLAN_WINDOW_ACCUM ||
         kind == KRCN_PLAN_JAG;
}

}   // namespace krcn
