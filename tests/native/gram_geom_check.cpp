// gram_geom_check.cpp — csrc/krcn_gram_geom.hpp over inputs of its own, built with
// g++ under ASan + UBSan (Makefile target gram_geom, tests/test_gram_geom.py):
// the tile-id map and its inverse, the slab ranges of the splits, the auto
// split rule and the workspace bytes at the largest d.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "krcn_gram_geom.hpp"

using namespace krcn;

static int failures = 0;
#define EXPECT(cond, ...)                 \
  do {                                    \
    if (!(cond)) {                        \
      if (++failures <= 20) {             \
        std::printf("FAIL %s: ", #cond);  \
        std::printf(__VA_ARGS__);         \
        std::printf("\n");                \
      }                                   \
    }                                     \
  } while (0)

// For every nt in 1..40: ids 0 .. nt (nt + 1) / 2 - 1 map one-to-one onto
// {(ta, tb): ta <= tb < nt}, and gram_tile_id inverts gram_tile_of.
static void tile_map() {
  const int before = failures;
  for (int64_t nt = 1; nt <= 40; ++nt) {
    const int64_t tiles = nt * (nt + 1) / 2;
    std::vector<int> seen(size_t(nt * nt), 0);
    for (int64_t id = 0; id < tiles; ++id) {
      int64_t ta = -1, tb = -1;
      gram_tile_of(id, ta, tb);
      EXPECT(0 <= ta && ta <= tb && tb < nt, "nt %lld id %lld -> (%lld, %lld)", (long long)nt, (long long)id,
             (long long)ta, (long long)tb);
      if (!(0 <= ta && ta <= tb && tb < nt)) continue;
      EXPECT(gram_tile_id(ta, tb) == id, "nt %lld id %lld -> (%lld, %lld) -> %lld", (long long)nt, (long long)id,
             (long long)ta, (long long)tb, (long long)gram_tile_id(ta, tb));
      ++seen[size_t(ta * nt + tb)];
    }
    for (int64_t ta = 0; ta < nt; ++ta)
      for (int64_t tb = 0; tb < nt; ++tb)
        EXPECT(seen[size_t(ta * nt + tb)] == (ta <= tb ? 1 : 0), "nt %lld (%lld, %lld) seen %d times", (long long)nt,
               (long long)ta, (long long)tb, seen[size_t(ta * nt + tb)]);
  }
  // far ids: the largest geometry (d = 2^20: nt = 16,384) at both ends of its last columns
  const int64_t nt = (int64_t(1) << 20) / kGramT;
  for (int64_t tb = nt - 3; tb < nt; ++tb)
    for (int64_t ta : {int64_t(0), int64_t(1), tb / 2, tb - 1, tb}) {
      int64_t a = -1, b = -1;
      gram_tile_of(gram_tile_id(ta, tb), a, b);
      EXPECT(a == ta && b == tb, "far (%lld, %lld) -> (%lld, %lld)", (long long)ta, (long long)tb, (long long)a,
             (long long)b);
    }
  std::printf("tile map: %s\n", failures == before ? "ok" : "FAILED");
}

// The slab ranges of the splits partition [0, ceil(n / KS)) in split order, for
// n around 0, 1, KS +- 1 and the split boundaries, splits with no slab included.
static void split_ranges() {
  const int before = failures;
  std::vector<int64_t> ns = {0, 1, 2, kGramKS - 1, kGramKS, kGramKS + 1, 2 * kGramKS - 1, 2 * kGramKS, 2 * kGramKS + 1,
                             3 * kGramKS + 2, 1000, 50000, (int64_t(1) << 31) - 1};
  for (int split : {2, 3, 7, 8, 255, 256})
    for (int64_t q = 0; q <= 2; ++q)
      for (int64_t e = -1; e <= 1; ++e) ns.push_back((int64_t(split) * q) * kGramKS + e < 0 ? 0 : (int64_t(split) * q) * kGramKS + e);
  for (int64_t n : ns)
    for (int split : {1, 2, 3, 5, 7, 8, 64, 255, 256}) {
      const GramGeom g = gram_geometry(64, n, split);
      EXPECT(g.slabs == (n + kGramKS - 1) / kGramKS, "n %lld slabs %lld", (long long)n, (long long)g.slabs);
      EXPECT(g.split == split, "forced split %d came back as %d", split, g.split);
      int64_t at = 0, empty = 0;
      for (int s = 0; s < split; ++s) {
        int64_t s0 = -1, s1 = -1;
        gram_split_range(g.slabs, split, s, s0, s1);
        EXPECT(s0 == at && s1 >= s0 && s1 <= g.slabs, "n %lld split %d/%d: [%lld, %lld) after %lld", (long long)n, s,
               split, (long long)s0, (long long)s1, (long long)at);
        if (s1 == s0) ++empty;
        at = s1;
      }
      EXPECT(at == g.slabs, "n %lld split %d ends at %lld of %lld", (long long)n, split, (long long)at,
             (long long)g.slabs);
      if (split > g.slabs) EXPECT(empty == split - g.slabs, "n %lld split %d: %lld empty", (long long)n, split, (long long)empty);
      // slabs cover [0, n) and nothing past the last slab
      EXPECT(g.slabs * kGramKS >= n && (g.slabs == 0 || (g.slabs - 1) * kGramKS < n), "n %lld slabs %lld", (long long)n,
             (long long)g.slabs);
    }
  std::printf("split ranges: %s\n", failures == before ? "ok" : "FAILED");
}

// The rule: 1 when the tiles fill the CUs; else the smallest split that reaches
// one workgroup per CU, under the slab minimum and the byte cap.
static void auto_rule() {
  const int before = failures;
  for (int64_t d : {1, 63, 64, 65, 500, 1100, 1408, 1409, 1472, 5000, 7129, 100000})
    for (int64_t n : {0, 1, 31, 32, 255, 256, 257, 2000, 6000, 50000, 10000000}) {
      const GramGeom g = gram_geometry(d, n, 0);
      EXPECT(g.nt == (d + kGramT - 1) / kGramT && g.tiles == g.nt * (g.nt + 1) / 2, "d %lld: nt %lld tiles %lld",
             (long long)d, (long long)g.nt, (long long)g.tiles);
      EXPECT(g.split >= 1 && g.split <= kGramMaxSplit, "d %lld n %lld: split %d", (long long)d, (long long)n, g.split);
      EXPECT(g.grid == g.tiles * g.split, "grid");
      EXPECT(g.ws_bytes == (g.split > 1 ? g.grid * int64_t(kGramT) * kGramT * 8 : 0), "ws bytes");
      if (g.tiles >= kNumCUs) EXPECT(g.split == 1, "d %lld n %lld: %lld tiles fill the CUs, split %d", (long long)d,
                                     (long long)n, (long long)g.tiles, g.split);
      if (g.split > 1) {
        EXPECT(g.slabs / g.split >= kGramMinSlabs, "d %lld n %lld: split %d of %lld slabs", (long long)d, (long long)n,
               g.split, (long long)g.slabs);
        EXPECT(g.ws_bytes <= kGramWsCap, "d %lld n %lld: %lld bytes", (long long)d, (long long)n, (long long)g.ws_bytes);
        EXPECT(g.tiles * (g.split - 1) < kNumCUs, "d %lld n %lld: split %d is not the smallest", (long long)d,
               (long long)n, g.split);
      } else if (g.tiles > 0 && g.tiles < kNumCUs) {
        // a larger split was refused by the slab minimum alone (the byte cap cannot bind below 256 tiles x 2)
        EXPECT(g.slabs / 2 < kGramMinSlabs, "d %lld n %lld: split 1 with %lld slabs", (long long)d, (long long)n,
               (long long)g.slabs);
      }
    }
  // the shapes DESIGN.md names
  EXPECT(gram_geometry(5000, 6000, 0).split == 1, "gisette");
  EXPECT(gram_geometry(7129, 44, 0).split == 1, "duke");
  EXPECT(gram_geometry(500, 2000, 0).split == 7, "madelon: 36 tiles, 63 slabs -> min(8, 63 / 8) = %d",
         gram_geometry(500, 2000, 0).split);
  EXPECT(gram_geometry(1100, 50000, 0).split == 2, "d = 1,100: 171 tiles -> %d", gram_geometry(1100, 50000, 0).split);
  std::printf("auto rule: %s\n", failures == before ? "ok" : "FAILED");
}

// d = 2^20: tiles, grid and workspace bytes stay exact in 64 bits at every split.
static void large() {
  const int before = failures;
  const int64_t d = int64_t(1) << 20;
  for (int split : {0, 1, 2, 256}) {
    const GramGeom g = gram_geometry(d, (int64_t(1) << 31) - 1, split);
    EXPECT(g.nt == 16384 && g.tiles == int64_t(16384) * 16385 / 2, "nt %lld tiles %lld", (long long)g.nt,
           (long long)g.tiles);
    EXPECT(g.grid == g.tiles * g.split && g.grid > 0, "grid %lld", (long long)g.grid);
    if (g.split > 1) {
      EXPECT(g.ws_bytes / (int64_t(kGramT) * kGramT * 8) == g.grid && g.ws_bytes > 0, "split %d: %lld bytes", g.split,
             (long long)g.ws_bytes);
    } else {
      EXPECT(g.ws_bytes == 0, "split 1 needs no workspace");
    }
  }
  EXPECT(gram_geometry(d, 1000, 0).split == 1, "tiles fill the CUs");
  std::printf("large: %s\n", failures == before ? "ok" : "FAILED");
}

int main() {
  tile_map();
  split_ranges();
  auto_rule();
  large();
  std::printf(failures ? "FAILED (%d)\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
