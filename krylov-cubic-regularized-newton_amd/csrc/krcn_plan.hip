// krcn_plan.hip — the pass plans (tile / sorted / LDS-window / jagged formats),
// ensure_plans and the reorthogonalisation workspace.
#include "krcn_internal.hpp"

#include <hipcub/hipcub.hpp>

using namespace krcn;

// ----------------------------------------------------------- pass plans
static constexpr int64_t kSliceThresholdBytes = 3 << 20;   // gathered vector above this: slice
static constexpr int64_t kSliceTargetBytes = 2 << 20;      // x window per slice
static constexpr int kBlocksPerGroup = 256;                // sliced: 8 groups x 256 = 2048 blocks (8 per CU)
static constexpr int kMaxGrid = 2048;

void free_plan(PassPlan& P) {
  P.own.free_all();
  static_cast<PlanFields&>(P) = PlanFields();
}

// An empty plan of the given shape: what every builder starts from (vs: the
// handle's value size; a builder that narrows its values sets P.vbytes itself).
static void reset_plan(PassPlan& P, int rows, int64_t cols, int64_t nnz, size_t vs) {
  free_plan(P);
  P.rows = rows;
  P.cols = cols;
  P.nnz = nnz;
  P.vbytes = int(vs);
}

// Cut [0, n) into B ranges of equal weight by the prefix sums pre[0 .. n]:
// cut[b] is the first i with pre[i] >= pre[n] b / B (cut[0] = 0, cut[B] = n).
template <class Pre>
static void balanced_cuts(const Pre& pre, int n, int B, int* cut) {
  cut[0] = 0;
  int i = 0;
  for (int b = 1; b < B; ++b) {
    const int64_t target = int64_t(pre[n]) * b / B;
    while (i < n && pre[i] < target) ++i;
    cut[b] = i;
  }
  cut[B] = n;
}

static int slices_for(int64_t bytes) {
  if (bytes <= kSliceThresholdBytes) return 1;
  const int64_t per8 = 8 * kSliceTargetBytes;
  return int(8 * ((bytes + per8 - 1) / per8));
}

// Sliced copy of a CSR: slice s holds columns [bounds[s], bounds[s+1]) with
// global column ids, rows in order; row pointers flattened slice-major.
// The values are stored as TS (static_cast<TS>(v); T but for a narrowed
// window plan).
template <typename T, typename TS = T>
static krcn_status build_slices(PassPlan& P, const int* ptr, const int* idx, const T* val, hipStream_t s,
                                const std::vector<int>* bounds_in = nullptr, int64_t pad = 0) {
  const int S = P.S, rows = P.rows;
  const int64_t nnz = P.nnz, cols = P.cols;
  std::vector<int> hb(S + 1);
  for (int k = 0; k <= S; ++k) hb[k] = bounds_in ? (*bounds_in)[k] : int((cols * k) / S);
  DevTmp<int> counts, perm, iota, sid_out, sid, bounds;   // (scope exit frees in reverse: bounds first)
  CHK(bounds.alloc(sizeof(int) * (S + 1)));
  HIPCHK(hipMemcpyAsync(bounds.p, hb.data(), sizeof(int) * (S + 1), hipMemcpyHostToDevice, s));
  const size_t nptr = size_t(S) * rows + 1;
  CHK(P.own.alloc(&P.own_ptr, sizeof(int) * nptr));
  CHK(P.own.alloc(&P.own_idx, sizeof(int) * std::max<int64_t>(nnz, 1)));
  CHK(P.own.alloc(&P.own_val, sizeof(TS) * size_t(std::max<int64_t>(nnz, 1) + pad)));
  if (pad) HIPCHK(hipMemsetAsync(static_cast<TS*>(P.own_val) + nnz, 0, sizeof(TS) * size_t(pad), s));
  CHK(counts.alloc(sizeof(int) * nptr));
  HIPCHK(hipMemsetAsync(counts.p, 0, sizeof(int) * nptr, s));
  if (nnz > 0) {
    CHK(sid.alloc(sizeof(int) * nnz));
    CHK(sid_out.alloc(sizeof(int) * nnz));
    CHK(iota.alloc(sizeof(int) * nnz));
    CHK(perm.alloc(sizeof(int) * nnz));
    hipLaunchKernelGGL(k_slice_of, dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, idx, bounds.p, S, sid.p);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_iota, dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, iota.p);
    LAUNCHCHK();
    int bits = 1;
    while ((1 << bits) < S) ++bits;
    size_t tmpb = 0;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmpb, sid.p, sid_out.p, iota.p, perm.p, int(nnz), 0, bits, s));
    DevTmp<void> tmp, t2;
    CHK(tmp.alloc(tmpb));
    // stable: inside a slice the nonzeros keep their row-major order
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmpb, sid.p, sid_out.p, iota.p, perm.p, int(nnz), 0, bits, s));
    hipLaunchKernelGGL(k_slice_counts, dim3(vec_grid(int64_t(rows) * 64)), dim3(kNT), 0, s, rows, ptr, sid.p, counts.p);
    LAUNCHCHK();
    hipLaunchKernelGGL((k_slice_gather<T, TS>), dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, perm.p, idx, val,
                       P.own_idx, static_cast<TS*>(P.own_val));
    LAUNCHCHK();
    size_t tmp2 = 0;
    HIPCHK(hipcub::DeviceScan::InclusiveSum(nullptr, tmp2, counts.p, P.own_ptr, int(nptr), s));
    CHK(t2.alloc(tmp2));
    HIPCHK(hipcub::DeviceScan::InclusiveSum(t2.p, tmp2, counts.p, P.own_ptr, int(nptr), s));
    HIPCHK(hipStreamSynchronize(s));
    t2.reset();
    tmp.reset();
  } else {
    HIPCHK(hipMemsetAsync(P.own_ptr, 0, sizeof(int) * nptr, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  P.ptr = P.own_ptr;
  P.idx = P.own_idx;
  P.val = P.own_val;
  return KRCN_OK;
}

// Tile list (host greedy over the row pointers), grouped by XCD group.
// Wave tiles: <= kWaveTileNnz nonzeros in the 4-aligned window, <= kWaveTileRows
// rows.  Sorted block tiles: <= kSortTile nonzeros, <= kSortTileRows rows, and
// `segs` receives the sort segments (a normal tile, or kSortTile chunks of a
// long row) as nonzero offsets.
static krcn_status build_tiles(PassPlan& P, hipStream_t s, std::vector<int>* segs, std::vector<int>* segbase) {
  const int S = P.S, rows = P.rows;
  const bool sorted = P.kind == KRCN_PLAN_SORTED;
  const int sort_tile = P.sort_nt * kSortPerThread;
  const int cap_nnz = sorted ? sort_tile : kWaveTileNnz;
  const int cap_rows = sorted ? sort_tile / 4 : kWaveTileRows;
  const int per_block = sorted ? 1 : kWavesPerBlock;
  const size_t nptr = size_t(S) * rows + 1;
  std::vector<int> hp(nptr);
  HIPCHK(hipMemcpyAsync(hp.data(), P.ptr, sizeof(int) * nptr, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  auto win = [&](const int* rp, int a, int b) { return sorted ? rp[b] - rp[a] : rp[b] - (rp[a] & ~3); };
  // Greedy tiling of one slice with nonzero cap `cap`; emit(long, r0, r1).
  auto walk = [&](int sl, int cap, auto&& emit) {
    const int* rp = hp.data() + size_t(sl) * rows;
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
  const int per_group = sorted ? kBlocksPerGroup * kNT / P.sort_nt : kBlocksPerGroup;
  const int max_grid = sorted ? kMaxGrid * kNT / P.sort_nt : kMaxGrid;
  std::vector<int> gcap(P.groups, cap_nnz);
  if (sorted) {
    const int B = P.groups > 1 ? per_group : max_grid;
    for (int g = 0; g < P.groups; ++g) {
      auto count = [&](int cap) {
        int64_t c = 0;
        for (int sl = g; sl < S; sl += P.groups) walk(sl, cap, [&](int, int, int) { ++c; });
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
  std::vector<std::vector<TileDesc>> per(P.groups);
  if (segs) segs->clear();
  if (segbase) segbase->clear();
  for (int sl = 0; sl < S; ++sl) {
    const int* rp = hp.data() + size_t(sl) * rows;
    const int g = sl % P.groups;
    // sorted tiles gather relative to their slice's first column (slice_bounds)
    const int base = sorted ? int((P.cols * sl) / S) : 0;
    auto seg = [&](int c) {
      if (segs) segs->push_back(c);
      if (segbase) segbase->push_back(base);
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
  if (segs) segs->push_back(hp[nptr - 1]);
  std::vector<TileDesc> all;
  std::vector<int> beg(P.groups + 1, 0), mid(P.groups, 0);
  int maxg = 0;
  for (int g = 0; g < P.groups; ++g) {
    beg[g] = int(all.size());
    // sorted tiles: ordinary tiles first, single long rows after tmid[g]
    if (sorted)
      std::stable_partition(per[g].begin(), per[g].end(), [](const TileDesc& d) { return d.long_row == 0; });
    int nshort = 0;
    for (const TileDesc& d : per[g]) nshort += d.long_row == 0;
    mid[g] = beg[g] + nshort;
    all.insert(all.end(), per[g].begin(), per[g].end());
    maxg = std::max<int>(maxg, int(per[g].size()));
  }
  beg[P.groups] = int(all.size());
  if (sorted) {
    CHK(P.own.alloc(&P.tmid, sizeof(int) * mid.size()));
    HIPCHK(hipMemcpyAsync(P.tmid, mid.data(), sizeof(int) * mid.size(), hipMemcpyHostToDevice, s));
  }
  P.ntiles = int(all.size());
  CHK(P.own.alloc(&P.tiles, sizeof(TileDesc) * std::max<size_t>(all.size(), 1)));
  CHK(P.own.alloc(&P.tbeg, sizeof(int) * beg.size()));
  if (!all.empty())
    HIPCHK(hipMemcpyAsync(P.tiles, all.data(), sizeof(TileDesc) * all.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(P.tbeg, beg.data(), sizeof(int) * beg.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  const int units = (maxg + per_block - 1) / per_block;
  if (P.groups > 1)
    P.grid = P.groups * std::max(1, std::min(units, per_group));
  else
    P.grid = std::max(1, std::min((P.ntiles + per_block - 1) / per_block, max_grid));
  P.combine_grid = combine_grid(rows);
  return KRCN_OK;
}

// Store the pass's nonzeros sorted by gather index inside every sort segment
// (stable: ties keep CSR order), with their slot in the segment.
template <typename T>
static krcn_status build_sorted(PassPlan& P, const std::vector<int>& segs, const std::vector<int>& segbase,
                               hipStream_t s) {
  const int64_t nnz = P.nnz;
  const int nseg = int(segs.size()) - 1;
  CHK(P.own.alloc(&P.gword, sizeof(unsigned) * std::max<int64_t>(nnz, 1)));
  CHK(P.own.alloc(&P.gval, sizeof(T) * std::max<int64_t>(nnz, 1)));
  if (nnz == 0 || nseg <= 0) return KRCN_OK;
  // (scope exit frees in reverse: the hipCUB scratch, then dsegs, dbase, key, skey, iota, perm)
  DevTmp<int> perm, iota;
  DevTmp<unsigned long long> skey, key;
  DevTmp<int> dbase, dsegs;
  CHK(dsegs.alloc(sizeof(int) * segs.size()));
  HIPCHK(hipMemcpyAsync(dsegs.p, segs.data(), sizeof(int) * segs.size(), hipMemcpyHostToDevice, s));
  CHK(dbase.alloc(sizeof(int) * segbase.size()));
  HIPCHK(hipMemcpyAsync(dbase.p, segbase.data(), sizeof(int) * segbase.size(), hipMemcpyHostToDevice, s));
  CHK(key.alloc(sizeof(unsigned long long) * nnz));
  CHK(skey.alloc(sizeof(unsigned long long) * nnz));
  CHK(iota.alloc(sizeof(int) * nnz));
  CHK(perm.alloc(sizeof(int) * nnz));
  hipLaunchKernelGGL(k_seg_keys, dim3(std::min(nseg, 65535)), dim3(kNT), 0, s, nseg, dsegs.p, P.idx, key.p);
  LAUNCHCHK();
  hipLaunchKernelGGL(k_iota, dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, iota.p);
  LAUNCHCHK();
  int sbits = 1;
  while ((int64_t(1) << sbits) < nseg) ++sbits;
  int slot_bits = 0;
  while ((1 << slot_bits) < P.sort_nt * kSortPerThread) ++slot_bits;
  size_t tmpb = 0;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmpb, key.p, skey.p, iota.p, perm.p, int(nnz), 0, 32 + sbits, s));
  DevTmp<void> tmp;
  CHK(tmp.alloc(tmpb));
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmpb, key.p, skey.p, iota.p, perm.p, int(nnz), 0, 32 + sbits, s));
  hipLaunchKernelGGL((k_sorted_gather<T>), dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, perm.p, skey.p, dsegs.p, dbase.p,
                     static_cast<const T*>(P.val), slot_bits, P.gword, static_cast<T*>(P.gval));
  LAUNCHCHK();
  HIPCHK(hipStreamSynchronize(s));
  // the sorted arrays replace the slice copies (the row pointers stay)
  CHK(P.own.release(&P.own_idx));
  CHK(P.own.release(&P.own_val));
  P.idx = nullptr;
  P.val = nullptr;
  return KRCN_OK;
}

// Sorted tiles pay when the gathered window per slice is dense enough for a
// 2 K-nonzero tile to put several lanes on one cache line: at most
// kSortWindow entries per slice, and the slice partials (S x rows, written
// and re-read) cheap next to the matrix stream.
static constexpr int64_t kSortWindowDefault = 24576;

static int64_t sort_window() {
  static const int64_t w = [] {
    const int64_t v = tuning_value("KRCN_SORT_WINDOW", int64_t(0));   // tuning knob
    return v >= 1024 ? v : kSortWindowDefault;
  }();
  return w;
}

static int sorted_slices(int64_t cols) {
  const int64_t kSortWindow = sort_window();
  if (cols <= kSortWindow) return 1;
  const int64_t per8 = 8 * kSortWindow;
  return int(8 * ((cols + per8 - 1) / per8));
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
static constexpr int kWinTileCost = 24;   // fixed per-tile work, in nonzero equivalents

template <typename T>
static int64_t win_width() { return WinGeom<T>::kW; }

static int win_slices_mode(int64_t cols, int64_t Wmax, int* k_out) {
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

// A/B knob KRCN_PLAN_RELOC (placement): 1 moves a plan's element
// arrays into physically contiguous allocations (hipDeviceMallocContiguous),
// 2 into fresh plain allocations made after the build's temporaries are gone.
static int plan_reloc_env() {
  static const int v = tuning_value("KRCN_PLAN_RELOC", 0);
  return v;
}

static krcn_status plan_reloc(PassPlan& P, void* field, hipStream_t s) {
  const int mode = plan_reloc_env();
  const DevOwner::Slot* sl = P.own.find(field);
  if (mode == 0 || !sl || !*sl->field || sl->bytes == 0) return KRCN_OK;
  void** p = sl->field;
  const size_t bytes = sl->bytes;
  void* q = nullptr;
  if (mode == 1) HIPCHK(hipExtMallocWithFlags(&q, bytes, hipDeviceMallocContiguous));
  else HIPCHK(hipMalloc(&q, bytes));
  HIPCHK(hipMemcpyAsync(q, *p, bytes, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipFree(*p));
  *p = q;
  return KRCN_OK;
}

// 0: no window format, 1: accumulate, 2: slices (auto policy).
static double slice_min_mat() {   // matrix bytes below which slices + combine do not pay
  static const double v = tuning_value("KRCN_SLICE_MIN_MB", 48.0) * 1e6;   // A/B knob
  return v;
}
static int window_choice(int rows, int64_t cols, int64_t nnz, size_t vs) {
  if (nnz == 0 || rows == 0 || cols == 0) return 0;
  const int64_t Wmax = vs == 8 ? win_width<double>() : win_width<float>();
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

// One-piece window-accum plans (d <= kWinNT): each block's rows once more as a
// column-major copy, so the fused Lanczos pass 1 also forms the block's share
// of X^T u (EpiLz1X, krcn_window.hpp).  Every column's run (rows ascending) is
// padded to whole chunks of kXtChunk (value 0, row kXtPad); xcp holds per
// block the cols + 1 absolute chunk ids.  Skipped (P.xt = 0) when a block's
// chunk sums do not fit the LDS past the window and its rows.  The copy is made
// from the plan's own values (stored as TS) and holds them widened to T: under
// narrowed storage X^T u runs over the same rounded matrix as X z, in 8-byte
// entries (EpiLz1X and k_xt_combine are the full-width code).
template <typename T, typename TS>
static krcn_status build_xt(PassPlan& P, const std::vector<int>& hp, const std::vector<int>& cut, int B,
                            hipStream_t s) {
  const int rows = P.rows, R = P.R, cols = int(P.cols);
  const int64_t nnz = P.nnz;
  std::vector<unsigned short> hidx(size_t(std::max<int64_t>(nnz, 1)));
  std::vector<TS> hval(size_t(std::max<int64_t>(nnz, 1)));
  if (nnz > 0) {
    HIPCHK(hipMemcpy(hidx.data(), P.widx, sizeof(unsigned short) * size_t(nnz), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hval.data(), P.val, sizeof(TS) * size_t(nnz), hipMemcpyDeviceToHost));
  }
  const size_t ncp = size_t(B) * (size_t(cols) + 1);
  std::vector<int> cp(ncp);
  std::vector<int> cnt(static_cast<size_t>(cols));
  int64_t chunks = 0;   // first pass: chunk ids
  for (int b = 0; b < B; ++b) {
    const int r0 = std::min(rows, cut[b] * R), r1 = std::min(rows, cut[b + 1] * R);
    if (r1 - r0 > kXtRowCap) return KRCN_OK;
    std::fill(cnt.begin(), cnt.end(), 0);
    for (int e = hp[r0]; e < hp[r1]; ++e) ++cnt[hidx[size_t(e)]];
    int* bcp = cp.data() + size_t(b) * (size_t(cols) + 1);
    const int64_t c0 = chunks;
    for (int c = 0; c < cols; ++c) {
      bcp[c] = int(chunks);
      chunks += (cnt[size_t(c)] + kXtChunk - 1) / kXtChunk;
    }
    bcp[cols] = int(chunks);
    if (chunks - c0 > XtGeom<T>::kChunks) return KRCN_OK;
    if (chunks * kXtChunk >= (int64_t(1) << 31)) return KRCN_OK;
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
  CHK(P.own.alloc(&P.xcp, sizeof(int) * ncp));
  CHK(P.own.alloc(&P.xrow, sizeof(unsigned short) * ne));
  CHK(P.own.alloc(&P.xval, sizeof(T) * ne));
  CHK(P.own.alloc(&P.xpart, sizeof(T) * size_t(B) * size_t(cols)));
  HIPCHK(hipMemcpyAsync(P.xcp, cp.data(), sizeof(int) * ncp, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(P.xrow, xr.data(), sizeof(unsigned short) * ne, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(P.xval, xv.data(), sizeof(T) * ne, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  P.xt = 1;
  return KRCN_OK;
}

// TS: the stored type of the values.  The geometry (slices, tiles, segments,
// grids) is T's whatever TS is: only the element type of own_val changes.
template <typename T, typename TS>
static krcn_status build_window_as(PassPlan& P, const int* ptr, const int* idx, const T* val, int accum,
                                   hipStream_t s) {
  const int64_t Wmax = WinGeom<T>::kW;
  P.vbytes = int(sizeof(TS));
  const int rows = P.rows;
  const int64_t cols = P.cols, nnz = P.nnz;
  int S = 1, kpb = 1;
  if (accum) {
    S = int((cols + Wmax - 1) / Wmax);
  } else {
    S = win_slices_mode(cols, Wmax, &kpb);
  }
  const int W = int((cols + S - 1) / S);
  P.S = S;
  P.W = W;
  P.kind = accum ? KRCN_PLAN_WINDOW_ACCUM : KRCN_PLAN_WINDOW_SLICES;
  P.L = 1;
  P.groups = 1;
  std::vector<int> hb(S + 1);
  for (int k = 0; k <= S; ++k) hb[k] = int(std::min<int64_t>(int64_t(k) * W, cols));
  CHK((build_slices<T, TS>(P, ptr, idx, val, s, &hb, kWinPad)));
  CHK(P.own.alloc(&P.widx, sizeof(unsigned short) * size_t(nnz + kWinPad)));
  HIPCHK(hipMemsetAsync(P.widx, 0, sizeof(unsigned short) * size_t(nnz + kWinPad), s));
  if (nnz > 0) {
    hipLaunchKernelGGL(k_local_u16, dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, P.own_idx, W, P.widx);
    LAUNCHCHK();
  }
  HIPCHK(hipStreamSynchronize(s));
  CHK(P.own.release(&P.own_idx));
  P.idx = nullptr;
  const size_t nptr = size_t(S) * rows + 1;
  std::vector<int> hp(nptr);
  HIPCHK(hipMemcpy(hp.data(), P.ptr, sizeof(int) * nptr, hipMemcpyDeviceToHost));
  // rows per tile: up to one staging chunk of nonzeros per tile and slice.
  // The tile stream is latency-bound (a wave keeps two tiles' chunks in
  // flight), so the tiles are taken as large as a chunk allows: news20's X
  // (3.55 nonzeros per row and slice, 227 per 64-row tile) ran its fused
  // pass 1 in 32.5 us with 64-row tiles against 38.0 us with 32-row tiles
  // (profiles/r03_news20_winR.txt); the few tiles past 256 take one extra chunk.
  const double mean = double(nnz) / (double(rows) * double(S));
  P.R = mean * 64.0 <= 0.95 * kWinChunk ? 64 : mean * 32.0 <= 0.95 * kWinChunk ? 32 : 16;
  {
    const int r = tuning_value("KRCN_WIN_R", 0);   // A/B knob: rows per tile (16 / 32 / 64)
    if (r == 16 || r == 32 || r == 64) P.R = r;
  }
  const int R = P.R;
  const int ntiles = (rows + R - 1) / R;
  auto tnnz = [&](int sl, int t) -> int64_t {
    const int* rp = hp.data() + size_t(sl) * rows;
    const int r0 = t * R, r1 = std::min(rows, r0 + R);
    return int64_t(rp[r1]) - rp[r0];
  };
  // compact row pointers (16-bit row ends inside a tile): every tile of every
  // slice must hold < 65536 nonzeros, else the format does not apply
  for (int sl = 0; sl < S; ++sl)
    for (int t = 0; t < ntiles; ++t)
      if (tnnz(sl, t) > 65535) return fail(KRCN_ERR_UNSUPPORTED, "window plan: a tile holds > 65535 nonzeros");
  CHK(plan_reloc(P, &P.widx, s));
  CHK(plan_reloc(P, &P.own_val, s));
  P.val = P.own_val;
  CHK(P.own.alloc(&P.tb, sizeof(int) * size_t(S) * (ntiles + 1)));
  CHK(P.own.alloc(&P.ro, sizeof(unsigned short) * std::max<size_t>(size_t(S) * rows, 1)));
  hipLaunchKernelGGL(k_compact_rows, dim3(vec_grid(int64_t(S) * rows)), dim3(kNT), 0, s, S, rows, R, ntiles, P.ptr,
                     P.tb, P.ro);
  LAUNCHCHK();
  HIPCHK(hipStreamSynchronize(s));
  // the kernels read the compact form only
  CHK(P.own.release(&P.own_ptr));
  P.ptr = nullptr;
  // cut [0, ntiles) into B ranges of equal cost(t) (prefix-sum cuts)
  auto cut_ranges = [&](int B, auto&& cost) {
    std::vector<int64_t> pre(ntiles + 1, 0);
    for (int t = 0; t < ntiles; ++t) pre[t + 1] = pre[t] + cost(t);
    std::vector<int> cut(B + 1, 0);
    balanced_cuts(pre, ntiles, B, cut.data());
    return cut;
  };
  std::vector<WinSeg> segs;
  if (accum) {
    auto cost = [&](int t) {
      int64_t c = kWinTileCost * int64_t(S);
      for (int sl = 0; sl < S; ++sl) c += tnnz(sl, t);
      return c;
    };
    const int cap = kWinWaves * kWinTMax;   // tiles per block (register sums)
    int B = std::max(1, tuning_value("KRCN_WIN_ACC_B", kNumCUs));   // A/B knob: first grid tried
    std::vector<int> cut;
    for (;;) {
      cut = cut_ranges(B, cost);
      int mx = 0;
      for (int b = 0; b < B; ++b) mx = std::max(mx, cut[b + 1] - cut[b]);
      if (mx <= cap || B >= 64 * kNumCUs) break;
      B += kNumCUs;
    }
    P.stride = S;
    segs.assign(size_t(B) * S, WinSeg{0, 0, 0, 0});
    for (int b = 0; b < B; ++b) {
      if (cut[b + 1] == cut[b]) continue;      // an empty block: segment count 0
      for (int sl = 0; sl < S; ++sl)
        segs[size_t(b) * S + sl] =
            WinSeg{sl, cut[b], cut[b + 1], kSegLoad | (sl == S - 1 ? kSegFlush : 0) | (sl == 0 ? S << 8 : 0)};
    }
    P.grid = B;
    if (S == 1 && cols <= kWinNT) CHK((build_xt<T, TS>(P, hp, cut, B, s)));
  } else {
    P.stride = 1;
    P.grid = S * kpb;
    P.kpb = (kpb & (kpb - 1)) != 0 ? kpb : 0;   // win_block_slice's mapping
    // a block whose row chunk is empty still names its slice (no segments to
    // run): the fused Lanczos prologue has it store its share of that slice
    std::vector<std::vector<int>> cuts(static_cast<size_t>(S));
    for (int sl = 0; sl < S; ++sl)
      cuts[size_t(sl)] = cut_ranges(kpb, [&](int t) { return tnnz(sl, t) + kWinTileCost; });
    segs.resize(size_t(S) * kpb);
    for (int b = 0; b < P.grid; ++b) {
      int sl = 0, c = 0;
      win_block_slice(b, P.grid, S, P.kpb, sl, c);
      const std::vector<int>& cut = cuts[size_t(sl)];
      segs[size_t(b)] = cut[c + 1] > cut[c] ? WinSeg{sl, cut[c], cut[c + 1], kSegLoad | kSegFlush | (1 << 8)}
                                           : WinSeg{sl, 0, 0, 0};
    }
    CHK(P.own.alloc(&P.part, sizeof(T) * size_t(S) * std::max(rows, 1)));
    P.combine_grid = combine_grid(rows);
  }
  P.nseg = int(segs.size());
  P.ntiles = ntiles;
  CHK(P.own.alloc(&P.segs, sizeof(WinSeg) * std::max<size_t>(segs.size(), 1)));
  if (!segs.empty())
    HIPCHK(hipMemcpy(P.segs, segs.data(), sizeof(WinSeg) * segs.size(), hipMemcpyHostToDevice));
  return KRCN_OK;
}

template <typename T>
static krcn_status build_window(PassPlan& P, const int* ptr, const int* idx, const T* val, int accum, size_t vs,
                                hipStream_t s) {
  if constexpr (std::is_same<T, double>::value)
    if (vs == 4) return build_window_as<T, float>(P, ptr, idx, val, accum, s);
  return build_window_as<T, T>(P, ptr, idx, val, accum, s);
}

// ------------------------------------------------------ jagged plans
// (krcn_jag.hpp.)  S = 1 when the gathered vector fits one LDS window (fp64:
// 20,448 entries), else S slices of W <= 10,224 entries that every block
// walks over its own rows (double-buffered windows, register row sums).
static constexpr int kJagGroupCost = 96;   // fixed work per group and slice, in nonzero equivalents

// KRCN_JAG (A/B knob): 0 never by the auto policy, 1 the cost model (default),
// 2 every pass the format can run
static int jag_env() {
  static const int v = tuning_value("KRCN_JAG", 1);
  return v;
}

template <typename T>
static int jag_slices(int64_t cols, int* W_out) {
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
static int jag_groups(int rows, int64_t cols, int64_t nnz, int S, int pass) {
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
static constexpr int kJagS1MinGroupsXt = kNumCUs;
static constexpr int kJagS1GroupsPerBlock = 6;   // below a group per wave: blocks of >= 6 groups
template <typename T>
static bool jag_choice(int rows, int64_t cols, int64_t nnz, int pass) {
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

// TS: the stored type of the values (own_val and the long rows' jlval).  Every
// choice below (slices, groups, K, the long-row rule, the grid) is T's.
template <typename T, typename TS>
static krcn_status build_jag_as(PassPlan& P, const int* ptr, const int* idx, const T* val, int pass, bool seq,
                                hipStream_t s) {
  const int rows = P.rows;
  P.vbytes = int(sizeof(TS));
  const int64_t cols = P.cols, nnz = P.nnz;
  if (cols < JagGeom<T>::kE || rows == 0 || nnz == 0)
    return fail(KRCN_ERR_UNSUPPORTED, "jag plan: empty or too narrow (%lld columns)", (long long)cols);
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
  std::vector<int> hp(size_t(rows) + 1);
  HIPCHK(hipMemcpy(hp.data(), ptr, sizeof(int) * (size_t(rows) + 1), hipMemcpyDeviceToHost));
  // single window: rows longer than kJagLong are summed apart by whole waves
  // (jag_long_rows) when their task partials fit the LDS past the window.
  // Their wave-tree order is not scipy's, so the sequential lane policy keeps
  // such rows lane-per-row (a row over 255 elements then refuses the plan)
  std::vector<int> lrows;
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
  std::vector<int64_t> pre(size_t(G) + 1, 0);
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
  std::vector<int> cut;
  for (;;) {
    cut.assign(size_t(R) + 1, 0);
    balanced_cuts(pre, G, R, cut.data());
    mx = 0;
    for (int b = 0; b < R; ++b) mx = std::max(mx, cut[b + 1] - cut[b]);
    if (mx <= kJagWaves * Kmax) break;
    if (R * SG >= 64 * kNumCUs) return fail(KRCN_ERR_UNSUPPORTED, "jag plan: %d row groups exceed the block cap", G);
    R += Rstep;
  }
  const int B = R * SG;
  // the smallest unrolled variant the block's groups allow: a wave issues the
  // loads of all K unit slots whether they hold a group or not (a sharded
  // news20 X^T with 21 groups per block ran its jagged pass 2 at rank-of-4 in
  // the same 26 us as at rank-of-2 with K = 6)
  const int K = S == 1 ? (mx <= kJagWaves ? 1 : mx <= 2 * kJagWaves ? 2 : mx <= 3 * kJagWaves ? 3 : kJagK1)
                       : (mx <= kJagWaves * 4 ? 4 : 8);
  std::vector<int> gblk(G);
  for (int b = 0; b < R; ++b)
    for (int g = cut[b]; g < cut[b + 1]; ++g) gblk[g] = b;
  const int64_t NU = int64_t(B) * Sg * K * kJagWaves;   // units
  int ubits = 1;
  while ((int64_t(1) << ubits) <= NU) ++ubits;
  if (ubits + 22 > 63) return fail(KRCN_ERR_UNSUPPORTED, "jag plan: too many units");
  const int64_t nrec = int64_t(B) * Sg * kJagWaves;   // (block, slice, wave) records

  // long rows: tasks of kJagTask elements, rows cut into B contiguous ranges by
  // task count (a block's tasks' partials must fit its tcap LDS slots)
  const int nl = int(lrows.size());
  std::vector<int> ltask, lbeg, lcut, tasks;
  if (nl > 0) {
    ltask.assign(size_t(nl) + 1, 0);
    lbeg.assign(size_t(nl) + 1, 0);
    for (int i = 0; i < nl; ++i) {
      const int len = hp[lrows[i] + 1] - hp[lrows[i]];
      ltask[i + 1] = ltask[i] + (len + kJagTask - 1) / kJagTask;
      lbeg[i + 1] = lbeg[i] + ((len + 1) & ~1);
    }
    const int64_t tt = ltask[nl];
    lcut.assign(2 * (size_t(B) + 1), 0);
    balanced_cuts(ltask, nl, B, lcut.data());
    for (int bb = 0; bb <= B; ++bb) lcut[B + 1 + bb] = ltask[lcut[bb]];
    for (int bb = 0; bb < B; ++bb)
      if (lcut[B + 2 + bb] - lcut[B + 1 + bb] > tcap)
        return fail(KRCN_ERR_UNSUPPORTED, "jag plan: a block's long rows need %d tasks (max %d)",
                    lcut[B + 2 + bb] - lcut[B + 1 + bb], tcap);
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
  CHK(P.own.alloc(&P.jgcut, sizeof(int) * (size_t(R) + 1)));
  CHK(P.own.alloc(&P.jumeta, sizeof(int) * size_t(nrec) * 2 * K));
  HIPCHK(hipMemcpyAsync(P.jgcut, cut.data(), sizeof(int) * (size_t(R) + 1), hipMemcpyHostToDevice, s));
  if (SG > 1) {   // per-group partial row sums
    CHK(P.own.alloc(&P.part, sizeof(T) * size_t(SG) * size_t(rows)));
    P.combine_grid = combine_grid(rows);
  }

  // (scope exit frees in reverse: gblk_d first, the hipCUB scratch last)
  DevTmp<void> tmp;
  DevTmp<unsigned char> cnt8;
  DevTmp<unsigned long long> keys_out, keys;
  DevTmp<int> pbase, first, usize, perm, iota, flags, gblk_d;
  int hflags[3] = {0, 0, 0};
  // single window: pair-level order, one pad key slot per row after the nonzeros
  const bool pairs = S == 1;
  const int64_t nitems = pairs ? nnz + rows : nnz;
  const unsigned long long sentinel = (1ull << (ubits + 22)) - 1ull;   // unit id >= NU: sorts past every real key
  if (nitems >= (int64_t(1) << 31)) return fail(KRCN_ERR_UNSUPPORTED, "jag plan: too many elements");
  CHK(gblk_d.alloc(sizeof(int) * size_t(G)));
  CHK(flags.alloc(3 * sizeof(int)));
  CHK(iota.alloc(sizeof(int) * size_t(nitems)));
  CHK(perm.alloc(sizeof(int) * size_t(nitems)));
  CHK(keys.alloc(sizeof(unsigned long long) * size_t(nitems)));
  CHK(keys_out.alloc(sizeof(unsigned long long) * size_t(nitems)));
  CHK(cnt8.alloc(size_t(NU) * 64));
  CHK(usize.alloc(sizeof(int) * size_t(NU)));
  CHK(first.alloc(sizeof(int) * size_t(NU)));
  HIPCHK(hipMemsetAsync(first.p, 0, sizeof(int) * size_t(NU), s));
  HIPCHK(hipMemsetAsync(usize.p, 0, sizeof(int) * size_t(NU), s));
  HIPCHK(hipMemcpyAsync(gblk_d.p, gblk.data(), sizeof(int) * size_t(G), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(flags.p, 0, 3 * sizeof(int), s));
  HIPCHK(hipMemsetAsync(cnt8.p, 0, size_t(NU) * 64, s));
  hipLaunchKernelGGL(k_jag_keys, dim3(vec_grid(rows)), dim3(kNT), 0, s, rows, Sg, SG, W, K, pairs ? 0 : 1, nnz,
                     sentinel, nl > 0 ? lthr : 0, ptr, idx, P.jgcut, gblk_d.p, keys.p, cnt8.p, usize.p, flags.p);
  LAUNCHCHK();
  HIPCHK(hipMemcpyAsync(hflags, flags.p, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
  std::vector<int> hsz(S > 1 ? size_t(NU) : 0);
  if (S > 1) HIPCHK(hipMemcpyAsync(hsz.data(), usize.p, sizeof(int) * size_t(NU), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (hflags[0]) return fail(KRCN_ERR_UNSUPPORTED, "jag plan: rows with descending column indices");
  if (hflags[1] > 255) return fail(KRCN_ERR_UNSUPPORTED, "jag plan: %d elements of a row in one slice (max 255)", hflags[1]);
  const int umax = hsz.empty() ? 0 : *std::max_element(hsz.begin(), hsz.end());
  if (umax > kJagSlab)
    return fail(KRCN_ERR_UNSUPPORTED, "jag plan: a group holds %d elements of one slice (accumulate mode: max %d)",
                umax, kJagSlab);
  hipLaunchKernelGGL(k_iota, dim3(vec_grid(nitems)), dim3(kNT), 0, s, nitems, iota.p);
  LAUNCHCHK();
  size_t tb = 0;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys.p, keys_out.p, iota.p, perm.p, int(nitems), 0, ubits + 22, s));
  CHK(tmp.alloc(tb));
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, keys.p, keys_out.p, iota.p, perm.p, int(nitems), 0, ubits + 22, s));
  hipLaunchKernelGGL(k_jag_firsts, dim3(vec_grid(nitems)), dim3(kNT), 0, s, nitems, NU, keys_out.p, first.p);
  LAUNCHCHK();
  // single window: the nonzeros and their pads in sorted (pair-level) order
  // (long rows' elements sort past them, as sentinels); accumulate layout:
  // every unit padded to an even count (two elements a lane)
  int64_t total = pairs ? nnz + hflags[2] : nnz;
  if (nl > 0) {
    int64_t lnnz = 0;
    for (int r : lrows) lnnz += hp[r + 1] - hp[r];
    total -= lnnz;
  }
  if (S > 1) {
    CHK(pbase.alloc(sizeof(int) * size_t(NU)));
    hipLaunchKernelGGL(k_jag_pad2, dim3(vec_grid(NU)), dim3(kNT), 0, s, NU, usize.p, first.p);   // first := padded sizes
    LAUNCHCHK();
    HIPCHK(hipStreamSynchronize(s));
    tmp.reset();
    size_t tb2 = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, first.p, pbase.p, int(NU), s));
    CHK(tmp.alloc(tb2));
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb2, first.p, pbase.p, int(NU), s));
    int last[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&last[0], pbase.p + NU - 1, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&last[1], first.p + NU - 1, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    total = int64_t(last[0]) + last[1];
    hipLaunchKernelGGL(k_jag_firsts, dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, NU, keys_out.p, first.p);   // restore
    LAUNCHCHK();
  }
  CHK(P.own.alloc(&P.widx, sizeof(unsigned short) * size_t(total + kJagPad)));
  CHK(P.own.alloc(&P.own_val, sizeof(TS) * size_t(total + kJagPad)));
  HIPCHK(hipMemsetAsync(P.widx, 0, sizeof(unsigned short) * size_t(total + kJagPad), s));
  HIPCHK(hipMemsetAsync(P.own_val, 0, sizeof(TS) * size_t(total + kJagPad), s));
  hipLaunchKernelGGL((k_jag_gather<T, TS>), dim3(vec_grid(pairs ? total : nnz)), dim3(kNT), 0, s, pairs ? total : nnz,
                     nnz, W, perm.p, idx, val, keys_out.p, first.p, pbase.p, P.widx, static_cast<TS*>(P.own_val));
  LAUNCHCHK();
  hipLaunchKernelGGL(k_jag_umeta, dim3(vec_grid(nrec * 2 * K)), dim3(kNT), 0, s, nrec, K, pbase.p ? pbase.p : first.p,
                     usize.p, P.jumeta);
  LAUNCHCHK();
  CHK(plan_reloc(P, &P.widx, s));
  CHK(plan_reloc(P, &P.own_val, s));
  if (nl > 0) {
    const size_t lsz = size_t(lbeg[nl]) + kJagPad;
    CHK(P.own.alloc(&P.jlcut, sizeof(int) * lcut.size()));
    CHK(P.own.alloc(&P.jlrow, sizeof(int) * size_t(nl)));
    CHK(P.own.alloc(&P.jltask, sizeof(int) * ltask.size()));
    CHK(P.own.alloc(&P.jtask, sizeof(int) * tasks.size()));
    CHK(P.own.alloc(&P.jlidx, sizeof(unsigned short) * lsz));
    CHK(P.own.alloc(&P.jlval, sizeof(TS) * lsz));
    DevTmp<int> lbeg_d;
    CHK(lbeg_d.alloc(sizeof(int) * size_t(nl)));
    HIPCHK(hipMemcpyAsync(P.jlcut, lcut.data(), sizeof(int) * lcut.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(P.jlrow, lrows.data(), sizeof(int) * size_t(nl), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(P.jltask, ltask.data(), sizeof(int) * ltask.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(P.jtask, tasks.data(), sizeof(int) * tasks.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(lbeg_d.p, lbeg.data(), sizeof(int) * size_t(nl), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(P.jlidx, 0, sizeof(unsigned short) * lsz, s));
    HIPCHK(hipMemsetAsync(P.jlval, 0, sizeof(TS) * lsz, s));
    hipLaunchKernelGGL((k_jag_long_fill<T, TS>), dim3(std::min(nl, 4096)), dim3(kNT), 0, s, nl, W, P.jlrow, lbeg_d.p, ptr,
                       idx, val, P.jlidx, static_cast<TS*>(P.jlval));
    LAUNCHCHK();
    HIPCHK(hipStreamSynchronize(s));
    lbeg_d.reset();
  }
  // 8-bit lane counts: a 32-bit word for the K = 4 accumulate kernel, else 64-bit
  const bool w32 = S > 1 && K <= 4;
  const size_t cbytes = size_t(nrec) * 64 * (w32 ? 4 : 8);
  CHK(P.own.alloc(&P.jcnt, cbytes));
  if (w32)
    hipLaunchKernelGGL((k_jag_words<unsigned>), dim3(vec_grid(nrec * 64)), dim3(kNT), 0, s, nrec, K, cnt8.p,
                       reinterpret_cast<unsigned*>(P.jcnt));
  else
    hipLaunchKernelGGL((k_jag_words<unsigned long long>), dim3(vec_grid(nrec * 64)), dim3(kNT), 0, s, nrec, K,
                       cnt8.p, reinterpret_cast<unsigned long long*>(P.jcnt));
  LAUNCHCHK();
  HIPCHK(hipStreamSynchronize(s));
  P.kind = KRCN_PLAN_JAG;
  P.jlong = nl;
  P.jlpiece = lpiece;
  P.jK = K;
  P.jG = SG;
  P.jSg = Sg;
  P.S = S;
  P.W = W;
  P.L = 1;
  P.groups = 1;
  P.grid = B;
  P.ntiles = G;
  P.val = P.own_val;
  return KRCN_OK;
}

template <typename T>
static krcn_status build_jag(PassPlan& P, const int* ptr, const int* idx, const T* val, int pass, bool seq, size_t vs,
                             hipStream_t s) {
  if constexpr (std::is_same<T, double>::value)
    if (vs == 4) return build_jag_as<T, float>(P, ptr, idx, val, pass, seq, s);
  return build_jag_as<T, T>(P, ptr, idx, val, pass, seq, s);
}

// ----------------------------------------------------------- dense format
// The image of one pass (krcn_dense.hpp): zero fill plus a scatter of the CSR
// on the build stream; the slice partials when the geometry slices the pass.
// TS is the stored type of the image's values: T, or float on an fp64 handle
// under KRCN_VALUES_F32 (the geometry is then that of an fp32 image).
template <typename T, typename TS>
static krcn_status build_dense_as(PassPlan& P, const int* ptr, const int* idx, const T* val, int lanes, int slicing,
                                  hipStream_t s) {
  const DenseGeom g = dense_geometry(P.rows, P.cols, sizeof(TS), lanes, slicing);
  CHK(P.own.alloc(&P.own_val, size_t(g.bytes)));
  HIPCHK(hipMemsetAsync(P.own_val, 0, size_t(g.bytes), s));
  if (P.nnz > 0) {
    const int64_t blocks = (int64_t(P.rows) + kDenseNT / 64 - 1) / (kDenseNT / 64);
    hipLaunchKernelGGL((k_dense_scatter<T, TS>), dim3(unsigned(std::min<int64_t>(blocks, 65536))), dim3(kDenseNT), 0,
                       s, P.rows, ptr, idx, val, g.ld, static_cast<TS*>(P.own_val));
    LAUNCHCHK();
  }
  if (g.S > 1) CHK(P.own.alloc(&P.part, sizeof(T) * size_t(g.S) * size_t(std::max(P.rows, 1))));
  HIPCHK(hipStreamSynchronize(s));
  P.kind = KRCN_PLAN_DENSE;
  P.dld = g.ld;
  P.vbytes = int(sizeof(TS));
  P.S = g.S;
  P.L = g.L;
  P.ntiles = int(g.groups);
  P.grid = g.grid;
  P.combine_grid = combine_grid(P.rows);
  P.val = P.own_val;
  return KRCN_OK;
}

template <typename T>
static krcn_status build_dense(PassPlan& P, const int* ptr, const int* idx, const T* val, int lanes, int slicing,
                               size_t vs, hipStream_t s) {
  if (vs == sizeof(T)) return build_dense_as<T, T>(P, ptr, idx, val, lanes, slicing, s);
  return build_dense_as<T, float>(P, ptr, idx, val, lanes, slicing, s);
}

// KRCN_VALUES_F32_EXACT: *flag |= 1 when some value does not survive the round
// trip through fp32 (a NaN never does).
__global__ __launch_bounds__(256) void k_values_f32_exact(const double* __restrict__ val, int64_t nnz,
                                                          int* __restrict__ flag) {
  bool bad = false;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < nnz; i += int64_t(gridDim.x) * blockDim.x) {
    const double v = val[i];
    bad |= !(double(static_cast<float>(v)) == v);
  }
  if (bad) atomicOr(flag, 1);
}

// Bytes per stored value of the passes a plan build may narrow (dense, window
// and jagged plans): the handle's policy (krcn_csr_set_value_storage), decided
// once per build.
template <typename T>
static krcn_status stored_value_bytes(const krcn_csr* h, hipStream_t s, size_t* vs) {
  *vs = sizeof(T);
  if (sizeof(T) == 4 || h->values == KRCN_VALUES_FULL) return KRCN_OK;
  if (h->values == KRCN_VALUES_F32_EXACT && h->nnz > 0) {
    DevTmp<int> flag;
    CHK(flag.alloc(sizeof(int)));
    HIPCHK(hipMemsetAsync(flag.p, 0, sizeof(int), s));
    const int64_t blocks = (h->nnz + 255) / 256;
    hipLaunchKernelGGL(k_values_f32_exact, dim3(unsigned(std::min<int64_t>(blocks, 4096))), dim3(256), 0, s,
                       static_cast<const double*>(h->val), h->nnz, flag.p);
    LAUNCHCHK();
    int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bad) return KRCN_OK;
  }
  *vs = 4;
  return KRCN_OK;
}

// The format policy of one pass: krcn_csr_set_pass_format over
// krcn_csr_set_format, under the A/B knobs KRCN_FMT1 / KRCN_FMT2 (KRCN_FORMAT_*
// values; unset keeps the handle's).
static int pass_format(const krcn_csr* h, int pass) {
  int fmt = h->format_pass[pass - 1] >= 0 ? h->format_pass[pass - 1] : h->format;
  static const int f1 = tuning_value("KRCN_FMT1", -1);
  static const int f2 = tuning_value("KRCN_FMT2", -1);
  const int f = pass == 2 ? f2 : f1;
  if (f >= KRCN_FORMAT_AUTO && f <= KRCN_FORMAT_DENSE) fmt = f;
  return fmt;
}

extern "C" krcn_status krcn_dense_geometry(int64_t rows, int64_t cols, int dtype, int lanes, int slicing,
                                           int64_t* out_host) {
  if (!out_host) return fail(KRCN_ERR_INVALID, "krcn_dense_geometry: null argument");
  if (rows < 0 || cols < 0 || rows > INT32_MAX || cols > INT32_MAX || (dtype != KRCN_F64 && dtype != KRCN_F32))
    return fail(KRCN_ERR_INVALID, "krcn_dense_geometry: expected 0 <= rows, cols < 2^31 and a KRCN_F64 / KRCN_F32 dtype");
  const bool lanes_ok = lanes == KRCN_LANES_AUTO || lanes == KRCN_LANES_SEQUENTIAL ||
                        (lanes >= 2 && lanes <= 64 && (lanes & (lanes - 1)) == 0);
  const bool slicing_ok = slicing == KRCN_SLICING_AUTO || slicing == KRCN_SLICING_OFF || (slicing >= 8 && slicing % 8 == 0);
  if (!lanes_ok || !slicing_ok)
    return fail(KRCN_ERR_INVALID, "krcn_dense_geometry: lanes and slicing as krcn_csr_set_lanes / krcn_csr_set_slicing take them");
  const DenseGeom g = dense_geometry(rows, cols, dtype == KRCN_F64 ? 8 : 4, lanes, slicing);
  out_host[0] = g.ld;
  out_host[1] = g.L;
  out_host[2] = g.S;
  out_host[3] = g.width;
  out_host[4] = g.groups;
  out_host[5] = g.grid;
  out_host[6] = g.bytes;
  out_host[7] = g.nvec;
  return KRCN_OK;
}

template <typename T>
static krcn_status build_plan(krcn_csr* h, int pass, int rows, int64_t cols, int64_t nnz, const int* ptr,
                              const int* idx, const T* val, int lanes, size_t csr_vs, hipStream_t s) {
  // csr_vs: bytes per stored value of a window or jagged plan (build_plans:
  // sizeof(T), or the build's stored width when the other pass narrows too)
  PassPlan& P = pass == 2 ? h->p2 : h->p1;
  reset_plan(P, rows, cols, nnz, sizeof(T));
  const bool seq = lanes == KRCN_LANES_SEQUENTIAL;
  const int fmt = pass_format(h, pass);
  if (fmt == KRCN_FORMAT_DENSE) {
    if (h->shard != KRCN_SHARD_NONE)
      return fail(KRCN_ERR_UNSUPPORTED, "the dense format does not run on a sharded handle");
    return build_dense<T>(P, ptr, idx, val, lanes, h->slicing, h->store_vs, s);
  }
  // jagged format: forced, or by the auto policy (its summation order is
  // scipy's, so the sequential lane policy may use it too)
  if (fmt == KRCN_FORMAT_JAG ||
      (fmt == KRCN_FORMAT_AUTO && h->slicing == KRCN_SLICING_AUTO && jag_choice<T>(rows, cols, nnz, pass))) {
    const krcn_status r = build_jag<T>(P, ptr, idx, val, pass, seq, csr_vs, s);
    if (r != KRCN_ERR_UNSUPPORTED || fmt == KRCN_FORMAT_JAG) return r;
    reset_plan(P, rows, cols, nnz, sizeof(T));
  }
  // LDS-window format: forced, or by the auto policy (never under the
  // sequential lane policy, whose sliced passes must stay unsliced)
  {
    int wc = 0;
    if (fmt == KRCN_FORMAT_WINDOW) {
      const int64_t W = win_width<T>();
      wc = (cols + W - 1) / W <= 4 ? 1 : 2;
    } else if (fmt == KRCN_FORMAT_AUTO && !seq && h->slicing == KRCN_SLICING_AUTO) {
      wc = window_choice(rows, cols, nnz, sizeof(T));
    }
    if (wc) {
      const krcn_status r = build_window<T>(P, ptr, idx, val, wc == 1, csr_vs, s);
      if (r != KRCN_ERR_UNSUPPORTED || fmt == KRCN_FORMAT_WINDOW) return r;
      reset_plan(P, rows, cols, nnz, sizeof(T));   // not applicable to this matrix: fall through to the other formats
    }
  }
  // format
  bool sorted = false;
  int S_sorted = sorted_slices(cols);
  // sharded passes run without the fused step B, so the slices' combine is
  // pure overhead while the gathered vector is L2-sized: a news20 rank of 8
  // (170 K columns, 1.36 MB) ran 27.4 k HVP/s unsliced against 25.3 k sliced;
  // a rank of 4 (2.7 MB) 20.4 k against 23.8 k
  if (h->shard != KRCN_SHARD_NONE && cols * int64_t(sizeof(T)) <= int64_t(3) << 19) S_sorted = 1;
  // pass 1 beside a single-window jagged pass 2: unsliced sorted tiles (no
  // slice partials, no combine launch: the two-launch Lanczos step)
  if (pass == 1 && h->p1_unsliced) S_sorted = 1;
  if (h->slicing >= 8) S_sorted = h->slicing;
  // largest block tile that still leaves >= one tile per CU
  int sort_nt = h->sort_nt;
  if (sort_nt == 0)
    sort_nt = nnz >= int64_t(kNumCUs) * 1024 * kSortPerThread ? 1024
              : nnz >= int64_t(kNumCUs) * 512 * kSortPerThread ? 512 : 256;
  const int64_t max_window = sort_nt == 256 ? SortGeom<256>::kMaxWindow
                             : sort_nt == 512 ? SortGeom<512>::kMaxWindow : SortGeom<1024>::kMaxWindow;
  const bool one_slice = h->slicing == KRCN_SLICING_OFF || seq;
  if (one_slice) S_sorted = 1;
  // the packed gather word addresses kSortMaxWindow columns past a slice's base
  while (!one_slice && (cols + S_sorted - 1) / S_sorted >= max_window) S_sorted = S_sorted < 8 ? 8 : S_sorted + 8;
  const bool sortable = (cols + S_sorted - 1) / S_sorted < max_window;
  const bool unsliced_pick = pass == 1 && h->p1_unsliced && S_sorted == 1;
  if (fmt == KRCN_FORMAT_SORTED && sortable) {
    sorted = true;
  } else if (fmt == KRCN_FORMAT_AUTO && !seq && nnz > 0) {
    const double part_bytes = S_sorted > 1 ? 16.0 * double(S_sorted) * double(rows) : 0.0;
    const double mat_bytes = double(nnz) * (sizeof(T) + sizeof(int));
    const int64_t window = (cols + S_sorted - 1) / S_sorted;
    sorted = (window <= sort_window() || unsliced_pick) && part_bytes <= 0.25 * mat_bytes;
  }
  if (sorted) {
    P.S = S_sorted;
  } else if (seq || h->slicing == KRCN_SLICING_OFF) {
    P.S = 1;
  } else if (h->slicing >= 8) {
    P.S = h->slicing;
  } else {
    P.S = slices_for(cols * int64_t(sizeof(T)));
  }
  if (P.S > 1 && cols < P.S) P.S = 1;
  P.kind = sorted ? KRCN_PLAN_SORTED : KRCN_PLAN_WAVE;
  P.sort_nt = sort_nt;
  P.groups = P.S > 1 ? 8 : 1;
  // a sliced row holds ~1/S of its nonzeros: pick lanes from the slice-local mean
  P.L = resolve_lanes(lanes, int64_t(rows) * P.S, nnz);
  if (sorted && lanes == KRCN_LANES_AUTO && pass == 1 && rows > 0 && nnz > 0) {
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
    std::vector<int> hp(size_t(rows) + 1);
    HIPCHK(hipMemcpyAsync(hp.data(), ptr, sizeof(int) * hp.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    double sq = 0.0;
    for (int r = 0; r < rows; ++r) {
      const double len = double(hp[r + 1] - hp[r]);
      sq += len * len;
    }
    const double mean = double(nnz) / double(rows);
    const double wmean = sq / double(nnz);
    if (wmean >= 2.0 * mean) P.L = std::max(P.L, auto_lanes(int64_t(P.S), int64_t(4.0 * wmean)));
  }
  if (P.S == 1) {
    P.ptr = ptr;
    P.idx = idx;
    P.val = val;
  } else {
    CHK(build_slices<T>(P, ptr, idx, val, s));
    CHK(P.own.alloc(&P.part, sizeof(T) * size_t(P.S) * std::max(rows, 1)));
  }
  std::vector<int> segs, segbase;
  CHK(build_tiles(P, s, sorted ? &segs : nullptr, sorted ? &segbase : nullptr));
  if (sorted) CHK(build_sorted<T>(P, segs, segbase, s));
  return KRCN_OK;
}

// The plan kinds that honour the handle's value storage policy.
static bool plan_narrows(int kind) {
  return kind == KRCN_PLAN_DENSE || kind == KRCN_PLAN_WINDOW_SLICES || kind == KRCN_PLAN_WINDOW_ACCUM ||
         kind == KRCN_PLAN_JAG;
}

template <typename T>
static krcn_status build_plans(krcn_csr* h, bool lz2, hipStream_t s) {
  h->store_vs = sizeof(T);
  if (h->shard == KRCN_SHARD_NONE) CHK(stored_value_bytes<T>(h, s, &h->store_vs));   // (one scan per build)
  // dense passes: the images must fit the device's free memory (with what the
  // plans about to be replaced give back), checked before anything is
  // allocated or freed so that a refusal leaves the handle as it was
  {
    const bool dn[2] = {pass_format(h, 1) == KRCN_FORMAT_DENSE, pass_format(h, 2) == KRCN_FORMAT_DENSE};
    if ((dn[0] || dn[1]) && h->shard == KRCN_SHARD_NONE) {
      const int64_t b1 = dn[0] ? dense_geometry(h->n, h->d, h->store_vs, h->lanes_x, h->slicing).bytes : 0;
      const int64_t b2 = dn[1] ? dense_geometry(h->d, h->n, h->store_vs, h->lanes_xt, h->slicing).bytes : 0;
      const int64_t need = b1 > INT64_MAX - b2 ? INT64_MAX : b1 + b2;
      size_t mfree = 0, mtotal = 0;
      HIPCHK(hipMemGetInfo(&mfree, &mtotal));
      const size_t avail = mfree + h->p1.own.bytes() + h->p2.own.bytes();
      if (uint64_t(need) > uint64_t(avail))
        return fail(KRCN_ERR_UNSUPPORTED, "the dense format needs %lld bytes of images for this %lld x %lld matrix, "
                    "the device has %lld bytes free", (long long)need, (long long)h->n, (long long)h->d,
                    (long long)avail);
      free_plan(h->p1);   // (both before either image is allocated: the peak holds no old plan)
      free_plan(h->p2);
    }
  }
  // One matrix per operator: a window or jagged pass narrows only beside a
  // pass that narrows too (dense, window or jagged), so no plan pair computes
  // A32^T diag(w) A.  Pass 2 is built first at the build's stored width; pass
  // 1 takes that width when pass 2 came out a narrowing kind, and pass 2 is
  // rebuilt at full width when pass 1 did not (an AUTO plan like rcv1's:
  // sorted pass 1, jagged pass 2).  The formats' choices do not depend on the
  // width, so the rebuilt plan has the same kind and geometry.  (A dense image
  // narrows whatever its partner is: the dense + wave mix keeps that.)
  auto pass2 = [&](size_t vs) {
    return build_plan<T>(h, 2, int(h->d), h->n, h->nnz, h->tptr, h->tidx, static_cast<const T*>(h->tval), h->lanes_xt,
                         vs, s);
  };
  CHK(pass2(h->store_vs));
  h->p1_unsliced = lz2 && h->p2.kind == KRCN_PLAN_JAG && h->p2.S == 1 && h->shard == KRCN_SHARD_NONE;
  CHK(build_plan<T>(h, 1, int(h->n), h->d, h->nnz, h->ptr, h->idx, static_cast<const T*>(h->val), h->lanes_x,
                    plan_narrows(h->p2.kind) ? h->store_vs : sizeof(T), s));
  if (h->p2.vbytes != int(sizeof(T)) && h->p2.kind != KRCN_PLAN_DENSE && !plan_narrows(h->p1.kind)) CHK(pass2(sizeof(T)));
  return KRCN_OK;
}

krcn_status ensure_plans(krcn_csr* h) {
  if (h->plans_ready) return KRCN_OK;
  std::lock_guard<std::mutex> lk(build_mutex());
  h->rows_pq = -1;   // new plans: row shards agree again (agree_rows)
  lzp_abort(h);      // (and the Lanczos-call placement search starts over)
  h->lzp_best = -1;
  h->lzp_ran = 0;
  hipStream_t s = nullptr;
  HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  // pass 2 first: whether it is a single-window jagged plan may decide pass
  // 1's slicing.  Off by default: unslicing rcv1's sorted pass 1 for the
  // two-launch step ran 33.4-34.1 k HVP/s against 43.3-44.2 k for the sliced
  // pass + combine (pass 1 16 against 10 us, pass 2 13.7 against 10.3 us;
  // profiles/r04_rcv1_lz2.txt).  A/B knob KRCN_LZ2=1 turns it on.  (The
  // step itself reads the same knob as on unless 0, krcn_lanczos_impl.hpp
  // lanczos_impl fuse_u: it runs wherever a plan allows it.)
  static const bool lz2_env = tuning_off("KRCN_LZ2");
  krcn_status r = h->dtype == KRCN_F64 ? build_plans<double>(h, lz2_env, s) : build_plans<float>(h, lz2_env, s);
  (void)hipStreamDestroy(s);
  CHK(r);
  // size the partials buffers to the plans' largest reducing grid (an
  // accumulate-mode window plan over a tall X^T can run up to 64 x 256 blocks)
  int64_t need = kMaxPartials;
  for (const PassPlan* P : {&h->p1, &h->p2}) need = std::max<int64_t>(need, std::max(P->grid, P->combine_grid));
  if (need > h->pcap) {
    for (double** b : {&h->pa, &h->pb, &h->pz, &h->pq}) {
      CHK(h->own.release(b));
      CHK(dalloc(h, b, size_t(need)));
    }
    h->pcap = need;
  } else if (!h->pz) {   // the fused step B's ||z||^2 (early-alpha step: z.v) and the combine's alpha partials
    CHK(dalloc(h, &h->pz, size_t(h->pcap)));
    CHK(dalloc(h, &h->pq, size_t(h->pcap)));
  }
  h->p1.pcap = h->p2.pcap = h->pcap;
#if KRCN_FOLD
  CHK(h->own.release(&h->fcnt));
  if (h->p1.kind == KRCN_PLAN_WINDOW_SLICES && h->p1.ntiles > 0) {   // tickets (ntiles), then the per-block won lists
    const size_t cnt = size_t(h->p1.ntiles) * size_t(kFoldPad + h->p1.grid);
    CHK(h->own.alloc(&h->fcnt, sizeof(int) * cnt));
    HIPCHK(hipMemset(h->fcnt, 0, sizeof(int) * cnt));
  }
#endif
  h->plans_ready = true;
  ++h->ws_gen;   // a recorded Lanczos graph points into the old plans
  return tune_placement(h);
}

krcn_status reserve_reorth(krcn_csr* h, int m) {
  // dot partials: k_cgs_rowdots (chunks x rows, <= kCgsRdParts + rows) in
  // pr, k_cgs_update_dots ((column slabs) x rows) in pr2
  if (m <= h->reorth_m) return KRCN_OK;
  std::lock_guard<std::mutex> lk(build_mutex());
  const int64_t cap = ((h->d + kCgsUpdCols - 1) / kCgsUpdCols) * int64_t(m);
  CHK(h->own.release(&h->pr));
  CHK(h->own.release(&h->pr2));
  h->pr_cap = 0;
  h->prv_cap = 0;
  h->reorth_m = 0;
  // chunk partials of either path: the batched k_cgs_rowdots (C k <= kCgsRdPartsV)
  // and k_cgs_rowdots_v (C k, C = the 1 KiB-piece chunks of a row: past
  // 16 x 16 x 256 vectors a row takes more than kCgsRdChunksV of them)
  const int64_t nv = h->d / int64_t(16 / h->vs);
  const int64_t cv = std::max<int64_t>(kCgsRdChunksV, nv > 0 ? cgs_rdv_chunks_of(nv) : 0);
  const int64_t prv = std::max<int64_t>(kCgsRdPartsV, cv * m) + 4 * int64_t(m);
  CHK(dalloc(h, &h->pr, size_t(prv)));
  h->prv_cap = prv;
  CHK(dalloc(h, &h->pr2, size_t(cap)));
  // k_cgs_colsweep: the row ranges of a sweep over up to m - 1 rows (one range
  // needs no partials), V^T h partials of each, and one arrival counter per
  // 64-vector column group; not allocated where the 1 KiB-piece path never
  // runs (column shards, rows not whole 16-byte vectors)
  CHK(h->own.release(&h->cy));
  CHK(h->own.release(&h->ccnt));
  h->cy_q = 0;
  const int q = cgs_col_ranges(m);
  if (q > 1 && h->shard != KRCN_SHARD_COLS && h->d % int64_t(16 / h->vs) == 0) {
    const int64_t ncg = (h->d + 63) / 64;   // >= the column groups of either dtype
    CHK(dalloc(h, &h->cy, size_t(q) * size_t(h->d)));
    CHK(dalloc(h, &h->ccnt, size_t(ncg)));
    HIPCHK(hipMemsetAsync(h->ccnt, 0, sizeof(int) * size_t(ncg), nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));   // zero before any stream of the handle counts on it
    h->cy_q = q;
  }
  h->pr_cap = cap;
  h->reorth_m = m;
  ++h->ws_gen;
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_reserve(krcn_csr* h, int m_max, int reorth) {
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_csr_reserve: null handle");
  if (m_max < 1 || m_max > kLzMaxM) return fail(KRCN_ERR_INVALID, "krcn_csr_reserve: m_max must be 1..%d", kLzMaxM);
  CHK(set_device(h));
  CHK(ensure_plans(h));
  CHK(agree_rows(h));   // (outside the build lock: virtual ranks are threads of one process)
  if (reorth) CHK(reserve_reorth(h, m_max));
  return KRCN_OK;
}
