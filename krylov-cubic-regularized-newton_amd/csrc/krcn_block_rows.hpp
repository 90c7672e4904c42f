// krcn_block_rows.hpp — how the host cuts the work of the block products
// (krcn_block.hip).  Plain C++17, no HIP header: it also builds with g++ under
// the host sanitizers (tests/native/block_rows_check.cpp).
//
// A block of k vectors runs with lane groups of K = the next power of two >= k
// lanes.  The short-row kernel gives every row a lane group: 256 / K rows per
// 256-thread workgroup, ceil(rows / (256 / K)) workgroups, no cap.  Rows of more
// than KRCN_BLOCK_LONG_ROW stored elements are left out of it and get one
// 1024-thread workgroup each, in the order of the list block_long_rows returns.
#pragma once
#include "krcn.h"

#include <cstdint>
#include <vector>

namespace krcn {

constexpr int kBlockNT = 256;        // threads of a short-row workgroup
constexpr int kBlockLongNT = 1024;   // threads of a long-row workgroup
constexpr int kBlockLongRow = KRCN_BLOCK_LONG_ROW;

// lane group width of a block of k vectors (1 <= k <= KRCN_BLOCK_MAX)
inline int block_lanes(int k) {
  int K = 1;
  while (K < k) K *= 2;
  return K;
}

// rows a short-row workgroup owns
constexpr int block_rows(int K) { return kBlockNT / K; }

// workgroups of the short-row kernel over `rows` rows (rows < 2^31)
inline int64_t block_grid(int64_t rows, int K) { return (rows + block_rows(K) - 1) / block_rows(K); }

// segments a long row is cut into: one per lane group of its workgroup
constexpr int block_long_segments(int K) { return kBlockLongNT / K; }

// elements per segment of a long row of len elements (the last segments may be short or empty)
inline int block_segment(int len, int K) {
  return int((int64_t(len) + block_long_segments(K) - 1) / block_long_segments(K));
}

// Rows of a CSR (ptr: rows + 1 entries) with more than `threshold` stored elements, ascending.
inline std::vector<int32_t> block_long_rows(const int32_t* ptr, int64_t rows, int threshold) {
  std::vector<int32_t> out;
  for (int64_t r = 0; r < rows; ++r)
    if (int64_t(ptr[r + 1]) - int64_t(ptr[r]) > threshold) out.push_back(int32_t(r));
  return out;
}

}  // namespace krcn
