// How the waves of a window-slices block share their segment's tiles
// (csrc/krcn_geom.hpp win_claim_start / win_static_tile / win_claim_run /
// win_tile_clamp), checked on the host under ASan + UBSan
// (tests/test_win_claim.py builds and runs this program; no arguments).
//
// The program replays win_stream's protocol for the 16 waves of one block: a
// wave's first kWinRing tiles are its static deal; it draws a claim before its
// first tile, and per tile finished it resolves the claim drawn a tile ago,
// draws the next, puts the claimed tile into the ring slot that came free and
// stops at the first slot without a tile.  A scheduler decides which wave
// takes its next step, so the order in which the block's counter is drawn
// varies: one wave running to its end before any other has drawn (it takes
// every claim of the pool), the last wave first after all have drawn once,
// round-robin, round-robin with one wave 8 times slower, and 200 seeded
// random orders.
// For every segment length in {0, 1, 2, 15, 16, 17, 33, 47, 48, 49, 141, 417,
// 1000}, first tile t0 in {0, 7, 1000} and run length in {1, 3}:
//   * every tile of [t0, t1) is run exactly once, over the static deals and
//     the claims together, and no tile outside [t0, t1) is run;
//   * the tiles a wave runs are increasing;
//   * a wave without a first static tile draws no claim;
//   * claims past the pool denote no tiles (n == 0, first at the pool's end),
//     up to the largest counter value (no overflow);
//   * the tile whose bounds are read for a tile (win_tile_clamp) lies in
//     [0, max(t1 - 1, 0)] and is the tile itself below t1.
// Prints one line per run length; exits 1 at the first violated invariant.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "krcn_geom.hpp"

using namespace krcn;

static int g_n = 0, g_t0 = 0, g_run = 0;
static const char* g_order = "";
#define REQUIRE(cond)                                                                                   \
  do {                                                                                                  \
    if (!(cond)) {                                                                                      \
      std::fprintf(stderr, "win_claim_check: n=%d t0=%d run=%d order=%s: line %d: %s\n", g_n, g_t0, g_run, \
                   g_order, __LINE__, #cond);                                                           \
      std::exit(1);                                                                                     \
    }                                                                                                   \
  } while (0)

static uint64_t g_rng = 0;
static uint64_t next_u64() {
  uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct Wave {
  int slot[kWinRing];   // the ring: tile per slot, -1 where it has none
  int pos = 0;          // the slot of the current tile
  int pending = -1;     // the claim drawn and not yet resolved
  int sub = 0;          // tiles taken from the run claimed last
  WinRun rn{0, 0};
  bool done = false;
  int draws = 0;
  std::vector<int> ran;
};

struct Block {
  int t0, t1, run;
  int counter = 0;   // claims drawn
  Wave w[kWinWaves];
  // eager: every wave draws its first claim before any wave's first tile
  // (the waves leave the window barrier together); else a wave draws it as it
  // starts, so a wave may run to its end before another has drawn at all
  Block(int t0_, int t1_, int run_, bool eager) : t0(t0_), t1(t1_), run(run_) {
    for (int i = 0; i < kWinWaves; ++i) {
      Wave& v = w[i];
      for (int k = 0; k < kWinRing; ++k) v.slot[k] = win_static_tile(t0, t1, i, k);
      v.sub = run;
      if (v.slot[0] < 0) v.done = true;   // no tile: the wave only takes part in the window store
      else if (eager) first_draw(v);
    }
  }
  void first_draw(Wave& v) {
    v.pending = counter++;
    ++v.draws;
  }
  // one tile of wave i: win_stream's fetch_next, finish, take and the loop test
  void step(int i) {
    Wave& v = w[i];
    REQUIRE(!v.done && v.slot[v.pos] >= 0);
    if (v.draws == 0) first_draw(v);
    if (run == 1 || v.sub == run) {
      v.rn = win_claim_run(t0, t1, v.pending, run);
      REQUIRE(v.rn.n >= 0 && v.rn.n <= run);
      REQUIRE(v.rn.n == 0 || (v.rn.first >= win_claim_start(t0, t1) && v.rn.first + v.rn.n <= t1));
      v.pending = counter++;
      ++v.draws;
      v.sub = 0;
    }
    const int next = v.sub < v.rn.n ? v.rn.first + v.sub : -1;
    const int read = win_tile_clamp(v.rn.first + v.sub, t1);   // the bounds the wave loads for it
    REQUIRE(read >= 0 && read <= (t1 > 0 ? t1 - 1 : 0) && (next < 0 || read == next));
    ++v.sub;
    v.ran.push_back(v.slot[v.pos]);
    v.slot[v.pos] = next;
    v.pos = (v.pos + 1) % kWinRing;
    if (v.slot[v.pos] < 0) v.done = true;
  }
  bool live(int i) const { return !w[i].done; }
  bool any() const {
    for (int i = 0; i < kWinWaves; ++i)
      if (live(i)) return true;
    return false;
  }
  void check() {
    const int n = t1 - t0;
    std::vector<int> seen(size_t(n > 0 ? n : 0), 0);
    for (int i = 0; i < kWinWaves; ++i) {
      const Wave& v = w[i];
      if (win_static_tile(t0, t1, i, 0) < 0) REQUIRE(v.draws == 0 && v.ran.empty());
      for (size_t k = 0; k < v.ran.size(); ++k) {
        REQUIRE(v.ran[k] >= t0 && v.ran[k] < t1);
        REQUIRE(k == 0 || v.ran[k] > v.ran[k - 1]);
        ++seen[size_t(v.ran[k] - t0)];
      }
    }
    for (int t = 0; t < n; ++t) REQUIRE(seen[size_t(t)] == 1);
  }
};

static void run_to_end(Block& b, int i) {
  while (b.live(i)) b.step(i);
}

static long check_case(int n, int t0, int run) {
  g_n = n;
  g_t0 = t0;
  g_run = run;
  const int t1 = t0 + n;
  long orders = 0;
  REQUIRE(win_claim_start(t0, t1) == t0 + (n < kWinWaves * kWinRing ? n : kWinWaves * kWinRing));
  {
    g_order = "wave 0 first";
    Block b(t0, t1, run, false);
    for (int i = 0; i < kWinWaves; ++i) run_to_end(b, i);
    // the wave that ran alone took every claim: the whole pool
    if (n > 0) REQUIRE(int(b.w[0].ran.size()) == (n < kWinRing * kWinWaves ? (n + kWinWaves - 1) / kWinWaves
                                                                           : kWinRing + n - kWinRing * kWinWaves));
    b.check();
    ++orders;
  }
  {
    g_order = "wave 15 first";
    Block b(t0, t1, run, true);
    for (int i = kWinWaves - 1; i >= 0; --i) run_to_end(b, i);
    b.check();
    ++orders;
  }
  {
    g_order = "round-robin";
    Block b(t0, t1, run, true);
    while (b.any())
      for (int i = 0; i < kWinWaves; ++i)
        if (b.live(i)) b.step(i);
    // equal speeds: the waves' counts differ by at most one run
    int lo = INT_MAX, hi = 0;
    for (int i = 0; i < kWinWaves; ++i) {
      const int c = int(b.w[i].ran.size());
      lo = c < lo ? c : lo;
      hi = c > hi ? c : hi;
    }
    REQUIRE(hi - lo <= run);
    b.check();
    ++orders;
  }
  for (int slow = 0; slow < kWinWaves; slow += 5) {
    g_order = "round-robin, one slow wave";
    Block b(t0, t1, run, slow % 2 == 0);
    for (int round = 0; b.any(); ++round)
      for (int i = 0; i < kWinWaves; ++i)
        if (b.live(i) && (i != slow || round % 8 == 0)) b.step(i);
    b.check();
    ++orders;
  }
  for (int seed = 0; seed < 200; ++seed) {
    g_order = "seeded";
    g_rng = uint64_t(seed) * 1000003ull + uint64_t(n) * 7919ull + uint64_t(run);
    Block b(t0, t1, run, seed % 2 == 0);
    // every third seed skews the draw: low waves are picked more often
    while (b.any()) {
      int i = int(next_u64() % kWinWaves);
      if (seed % 3 == 0) i = int(next_u64() % uint64_t(i + 1));
      if (b.live(i)) b.step(i);
    }
    b.check();
    ++orders;
  }
  // claims far past the pool: no tiles, no overflow
  g_order = "past the pool";
  const int cs[] = {n, n + 1, 1 << 20, INT_MAX >> 6, INT_MAX};
  for (int c : cs) {
    const WinRun r = win_claim_run(t0, t1, c, run);
    const int start = win_claim_start(t0, t1);
    if (int64_t(c) * run >= t1 - start) REQUIRE(r.n == 0 && r.first == (t1 > start ? t1 : start));
  }
  return orders;
}

int main() {
  const int lens[] = {0, 1, 2, 15, 16, 17, 33, 47, 48, 49, 141, 417, 1000};
  const int firsts[] = {0, 7, 1000};
  const int runs[] = {1, 3};
  for (int run : runs) {
    long orders = 0;
    for (int n : lens)
      for (int t0 : firsts) orders += check_case(n, t0, run);
    std::printf("run %d: lengths=%zu firsts=%zu orders=%ld\n", run, sizeof(lens) / sizeof(lens[0]),
                sizeof(firsts) / sizeof(firsts[0]), orders);
  }
  REQUIRE(kWinClaimRun == 1 || kWinClaimRun == 3);   // the run lengths checked above cover the build's
  std::printf("ok\n");
  return 0;
}
