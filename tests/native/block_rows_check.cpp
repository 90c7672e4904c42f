// How the host cuts the work of the block products (csrc/krcn_block_rows.hpp),
// for the host sanitizer build (tests/test_block_rows.py): the lane group of
// every k, the short-row grid around every workgroup's row count and at the
// largest row count, the long-row list on both sides of the threshold, and a
// walk of every (workgroup, lane group) and every (long row, segment) the
// kernels would run, which must cover each row and each element exactly once.
// Prints one line per check and "ok"; exits 1 at the first violation.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "krcn_block_rows.hpp"

using namespace krcn;

static int fail(const char* what, long long a = 0, long long b = 0) {
  std::printf("FAIL %s (%lld, %lld)\n", what, a, b);
  return 1;
}

// every row of a CSR with these row lengths is owned exactly once: by a lane
// group of the short-row grid or by a workgroup of the long-row list, whose
// segments cover its elements once, in order
static int cover(const std::vector<int>& lens, int K) {
  const int64_t rows = int64_t(lens.size());
  std::vector<int32_t> ptr(lens.size() + 1, 0);
  for (size_t r = 0; r < lens.size(); ++r) ptr[r + 1] = ptr[r] + lens[r];
  std::vector<int> owners(lens.size(), 0);
  const int64_t grid = block_grid(rows, K);
  for (int64_t b = 0; b < grid; ++b)
    for (int g = 0; g < block_rows(K); ++g) {
      const int64_t r = b * block_rows(K) + g;
      if (r >= rows) continue;
      if (ptr[size_t(r) + 1] - ptr[size_t(r)] > kBlockLongRow) continue;
      ++owners[size_t(r)];
    }
  const std::vector<int32_t> lr = block_long_rows(ptr.data(), rows, kBlockLongRow);
  for (size_t i = 0; i < lr.size(); ++i) {
    if (i && lr[i] <= lr[i - 1]) return fail("long rows not ascending", lr[i], K);
    const int r = lr[i];
    ++owners[size_t(r)];
    const int lb = ptr[size_t(r)], le = ptr[size_t(r) + 1];
    const int seg = block_segment(le - lb, K);
    int64_t next = lb;
    for (int g = 0; g < block_long_segments(K); ++g) {
      const int64_t sb64 = int64_t(lb) + int64_t(g) * seg;
      const int64_t sb = sb64 < le ? sb64 : le;
      const int64_t se = sb64 + seg < le ? sb64 + seg : le;
      if (sb != next && sb != le) return fail("segments leave a gap", r, g);
      if (se < sb || se > le) return fail("segment outside its row", r, g);
      if (se > sb) next = se;
    }
    if (next != le) return fail("segments do not reach the row's end", r, K);
  }
  for (size_t r = 0; r < owners.size(); ++r)
    if (owners[r] != 1) return fail("row not owned exactly once", (long long)r, owners[r]);
  return 0;
}

int main() {
  for (int k = 1; k <= KRCN_BLOCK_MAX; ++k) {
    const int K = block_lanes(k);
    if (K < k || K >= 2 * k || (K & (K - 1)) || kBlockNT % K || kBlockLongNT % K) return fail("block_lanes", k, K);
  }
  std::printf("lanes: ok\n");
  for (int K = 1; K <= 16; K *= 2) {
    const int G = block_rows(K);
    for (int64_t rows : {int64_t(1), int64_t(G - 1), int64_t(G), int64_t(G + 1), int64_t(7 * G), int64_t(7 * G + 1),
                         int64_t(INT32_MAX)}) {
      const int64_t grid = block_grid(rows, K);
      if (grid * G < rows || (grid - 1) * G >= rows || grid > INT32_MAX) return fail("block_grid", rows, K);
    }
    if (block_grid(0, K) != 0) return fail("block_grid of no rows", 0, K);
    const int S = block_long_segments(K);
    for (int len : {kBlockLongRow + 1, S - 1, S, S + 1, 3 * kBlockLongRow + 7, 20000, INT32_MAX}) {
      const int seg = block_segment(len, K);
      if (int64_t(seg) * S < len || int64_t(seg - 1) * S >= len) return fail("block_segment", len, K);
    }
  }
  std::printf("grids: ok\n");
  {
    const int32_t ptr[] = {0, 0, kBlockLongRow, 2 * kBlockLongRow + 1, 2 * kBlockLongRow + 1, 5 * kBlockLongRow};
    const std::vector<int32_t> lr = block_long_rows(ptr, 5, kBlockLongRow);
    if (lr.size() != 2 || lr[0] != 2 || lr[1] != 4) return fail("threshold", (long long)lr.size());
    if (!block_long_rows(ptr, 0, kBlockLongRow).empty()) return fail("no rows");
    if (block_long_rows(ptr, 5, 0).size() != 3) return fail("threshold 0");
  }
  std::printf("threshold: ok\n");
  std::srand(7);
  for (int K = 1; K <= 16; K *= 2) {
    std::vector<int> lens;
    for (int r = 0; r < 3 * block_rows(K) + 5; ++r) {
      const int pick = std::rand() % 10;
      lens.push_back(pick == 0 ? kBlockLongRow + 1 + std::rand() % 4000 : pick == 1 ? kBlockLongRow : std::rand() % 7);
    }
    lens.push_back(20000);
    lens.push_back(0);
    if (cover(lens, K)) return 1;
    if (cover(std::vector<int>(300, 1933), K)) return 1;   // every row long
    if (cover(std::vector<int>(), K)) return 1;
  }
  std::printf("cover: ok\nok\n");
  return 0;
}
