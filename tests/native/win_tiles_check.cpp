// The tiles of window-slices plans (csrc/krcn_layout.hpp win_layout), checked
// on the host under ASan + UBSan (tests/test_win_tiles.py builds and runs this
// program; it takes no arguments and makes its own inputs).
//
// A slices-mode layout gives every slice its own tiles by their row starts.
// Where the rule takes data-cut tiles, a tile is the longest run of rows of its
// slice with at most 64 rows whose nonzeros fit one staging chunk from the
// 4-aligned element the chunk load starts at; elsewhere the tiles are the fixed
// R rows.  Invariants, for every input below:
//   * the tiles partition each slice's rows, in order, none empty;
//   * a tile has at most 64 rows;
//   * data-cut: (e0 & 3) + nnz <= kWinChunk unless the tile is a single row,
//     and no tile could have taken its next row (the longest run);
//   * a tile holds at most 65,535 nonzeros (16-bit row ends);
//   * the segments of a slice's blocks cover its tiles exactly once, in order;
//   * where the rule does not apply the layout is the fixed tiling.
// Prints one line per input; exits 1 at the first violated invariant.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "krcn_layout.hpp"

using namespace krcn;

#define REQUIRE(cond)                                                            \
  do {                                                                           \
    if (!(cond)) {                                                               \
      std::fprintf(stderr, "win_tiles_check: %s: line %d: %s\n", g_case, __LINE__, #cond); \
      std::exit(1);                                                              \
    }                                                                            \
  } while (0)

static const char* g_case = "";

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static double uniform01() { return double(next_u64() >> 11) * (1.0 / 9007199254740992.0); }

// counts[sl * rows + r]: nonzeros of row r in slice sl
struct Counts {
  int rows = 0, S = 0;
  std::vector<int> c;
  int& at(int sl, int r) { return c[size_t(sl) * rows + r]; }
};

// about `mean` nonzeros per row and slice, every (row, slice) within +-2 of it
static Counts uniform_counts(int rows, int S, int mean) {
  Counts C{rows, S, std::vector<int>(size_t(rows) * S)};
  for (int& v : C.c) v = std::max(0, mean - 2 + int(next_u64() % 5));
  return C;
}

// the skewed generator: lognormal row lengths (sigma 1), every nonzero in slice
// floor(S u^3) — hot first slices, rows from empty to hundreds in one slice
static Counts skewed_counts(int rows, int S, double mean_row) {
  Counts C{rows, S, std::vector<int>(size_t(rows) * S, 0)};
  for (int r = 0; r < rows; ++r) {
    const double g = std::sqrt(-2.0 * std::log(std::max(uniform01(), 1e-300))) * std::cos(6.283185307179586 * uniform01());
    const int len = std::max(1, int(mean_row * std::exp(g - 0.5)));
    for (int k = 0; k < len; ++k) {
      const double u = uniform01();
      ++C.at(std::min(S - 1, int(S * u * u * u)), r);
    }
  }
  return C;
}

static std::vector<int> slice_major_ptr(const Counts& C) {
  std::vector<int> hp(C.c.size() + 1, 0);
  for (size_t i = 0; i < C.c.size(); ++i) hp[i + 1] = hp[i] + C.c[i];
  return hp;
}

static WinShape slices_shape(int S, int kpb) {
  WinShape sh;
  sh.S = S, sh.kpb = kpb, sh.kind = KRCN_PLAN_WINDOW_SLICES;
  return sh;
}

struct Seen {
  int exact256 = 0;      // tiles with (e0 & 3) + nnz == kWinChunk and e0 & 3 != 0
  int single_long = 0;   // single rows past a chunk
  int64_t tiles = 0;
  double fill = 0.0;
};

// expect: 1 data-cut tiles, 0 the fixed tiling, R rows (fixedR)
static Seen check(const char* name, const Counts& C, int kpb, int forced, int expect, int fixedR) {
  g_case = name;
  const int rows = C.rows, S = C.S;
  const std::vector<int> hp = slice_major_ptr(C);
  const int64_t nnz = hp.back();
  const WinShape sh = slices_shape(S, kpb);
  const WinLayout L = win_layout(sh, rows, nnz, hp.data(), forced);
  REQUIRE(L.refused == KRCN_OK);
  REQUIRE(L.datacut == (expect == 1));
  REQUIRE(int(L.tcount.size()) == S && L.trow.size() == size_t(S) * (size_t(L.ntiles) + 1));
  REQUIRE(L.stride == 1 && L.grid == S * kpb && L.segs.size() == size_t(L.grid));
  if (expect == 1) REQUIRE(L.R == kWinTileRows);
  else REQUIRE(L.R == fixedR && L.ntiles == (rows + fixedR - 1) / fixedR);
  Seen seen;
  int mx = 0;
  for (int sl = 0; sl < S; ++sl) {
    const int* rp = hp.data() + size_t(sl) * rows;
    const int* tr = L.trow.data() + size_t(sl) * (size_t(L.ntiles) + 1);
    const int nt = L.tcount[size_t(sl)];
    mx = std::max(mx, nt);
    REQUIRE(nt >= 1 && nt <= L.ntiles && tr[0] == 0 && tr[nt] == rows);
    for (int t = nt; t <= L.ntiles; ++t) REQUIRE(tr[t] == rows);   // the slots past the slice's count
    for (int t = 0; t < nt; ++t) {
      const int r0 = tr[t], r1 = tr[t + 1], nr = r1 - r0;
      REQUIRE(nr >= 1 && nr <= kWinTileRows);
      const int64_t n = int64_t(rp[r1]) - rp[r0], mis = rp[r0] & 3;
      REQUIRE(n <= 65535);
      if (expect == 1) {
        REQUIRE(mis + n <= kWinChunk || nr == 1);
        if (r1 < rows && nr < kWinTileRows) REQUIRE(mis + int64_t(rp[r1 + 1]) - rp[r0] > kWinChunk);   // the longest run
        seen.exact256 += mis != 0 && mis + n == kWinChunk;
        seen.single_long += nr == 1 && mis + n > kWinChunk;
      } else {
        REQUIRE(r0 == t * fixedR && r1 == std::min(rows, r0 + fixedR));
      }
      ++seen.tiles;
      seen.fill += double(std::min<int64_t>(n, kWinChunk));
    }
  }
  REQUIRE(mx == L.ntiles);
  // the non-empty segments of a slice's blocks, in chunk order, cover its tiles once
  std::vector<int> next(size_t(S), 0), blocks(size_t(S), 0);
  for (int c = 0; c < kpb; ++c)
    for (int b = 0; b < L.grid; ++b) {
      int sl = 0, cc = 0;
      win_block_slice(b, L.grid, S, L.kpb, sl, cc);
      REQUIRE(sl >= 0 && sl < S && cc >= 0 && cc < kpb);
      if (cc != c) continue;
      ++blocks[size_t(sl)];
      const WinSeg& g = L.segs[size_t(b)];
      REQUIRE(g.slice == sl);
      if (g.flags == 0) {
        REQUIRE(g.t0 == 0 && g.t1 == 0);
        continue;
      }
      REQUIRE(g.flags == (kSegLoad | kSegFlush | (1 << 8)));
      REQUIRE(g.t0 == next[size_t(sl)] && g.t1 > g.t0 && g.t1 <= L.tcount[size_t(sl)]);
      next[size_t(sl)] = g.t1;
    }
  for (int sl = 0; sl < S; ++sl) REQUIRE(blocks[size_t(sl)] == kpb && next[size_t(sl)] == L.tcount[size_t(sl)]);
  seen.fill /= double(seen.tiles) * kWinChunk;
  std::printf("%s: rows=%d S=%d kpb=%d datacut=%d R=%d ntiles=%d tiles=%lld fill=%.3f exact256=%d single_long=%d\n", name,
              rows, S, kpb, int(L.datacut), L.R, L.ntiles, (long long)seen.tiles, seen.fill, seen.exact256,
              seen.single_long);
  return seen;
}

int main() {
  // 50,000 rows (no multiple of 64), 8 slices x 32 blocks, ~5 nonzeros per row
  // and slice: the fixed rule takes R = 32, 1563 tiles >= 32 x 48: data-cut
  {
    Counts C = uniform_counts(50000, 8, 5);
    for (int r = 1000; r < 1101; ++r) C.at(1, r) = 0;   // > 64 consecutive empty rows
    for (int r = 0; r < C.rows; ++r) C.at(3, r) = 0;    // an entirely empty slice
    C.at(2, 5000) = 300;                                // a row that alone exceeds a chunk
    C.at(2, 0) = 300;                                   // ... and one at the slice's first row
    C.at(4, C.rows - 1) = 700;                          // ... and at its last, three chunks long
    // slice 0: row 0 alone (250; a second row would pass 256), then rows 1-2 from
    // e0 = 250 (e0 & 3 = 2) with 7 + 247 = 254 nonzeros: 2 + 254 = 256 exactly
    C.at(0, 0) = 250, C.at(0, 1) = 7, C.at(0, 2) = 247, C.at(0, 3) = 1;
    const Seen s = check("uniform+edges", C, 32, 0, 1, 0);
    REQUIRE(s.exact256 >= 1 && s.single_long >= 3);
    REQUIRE(s.tiles < int64_t(8) * 1563);   // fewer tiles than the fixed R = 32
    check("uniform+edges forced R=32", C, 32, 32, 0, 32);   // the knob's fixed tiling of the same matrix
  }
  {
    const Counts C = skewed_counts(50001, 8, 40.0);
    check("skewed", C, 32, 0, 1, 0);
  }
  {   // 85 slices x 3 blocks (win_block_slice's packed mapping), 20,000 rows
    const Counts C = uniform_counts(20000, 85, 5);
    check("85x3", C, 3, 0, 1, 0);
  }
  // the rule does not apply: fewer than 48 tiles a block (500 < 32 x 48) ...
  check("short stream", uniform_counts(16000, 8, 5), 32, 0, 0, 32);
  // ... one tile short of it (1535 tiles of 32 rows) and exactly at it (1536)
  check("one tile short", uniform_counts(1535 * 32, 8, 5), 32, 0, 0, 32);
  check("at the threshold", uniform_counts(1535 * 32 + 1, 8, 5), 32, 0, 1, 0);
  // ... or the fixed rule already takes 64 rows (2 nonzeros per row and slice)
  check("row-capped", uniform_counts(120000, 8, 2), 32, 0, 0, 64);
  // ... or 16 (12 per row and slice: 32 rows pass 0.95 of a chunk), long enough: data-cut
  check("R=16 becomes data-cut", uniform_counts(50000, 8, 12), 32, 0, 1, 0);
  // forced data-cut tiles on a short stream (the tuning knob), 300 rows
  check("forced data-cut", uniform_counts(300, 8, 5), 32, 1, 1, 0);
  std::printf("ok\n");
  return 0;
}
