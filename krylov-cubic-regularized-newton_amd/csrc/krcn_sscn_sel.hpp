// krcn_sscn_sel.hpp — the selection of an SSCN step as the step stages it:
// cols | sorted cols | permutation (k int32 each, packed: position a of the
// selection is sorted column perm[a]), or why the selection is refused.
// Host-only C++17, no HIP header: it builds with g++ alone
// (tests/native/sscn_sel_check.cpp runs it under ASan + UBSan).  The front of
// krcn_sscn_step / krcn_sscn_step_tridiag (krcn_sscn_step.hpp) words the
// refusals; there is no second copy of the sort.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace krcn {

struct SscnSel {
  enum Error { Ok, Range, Repeat };
  Error error = Ok;
  int at = 0;      // Range: cols[at] lies outside [0, d); Repeat: cols[at] ...
  int first = 0;   //   ... repeats cols[first]
  std::vector<int32_t> triple;
};

// A column outside [0, d) is reported first, at its first position in input
// order; then a repeat, at the smallest repeated column: its second position
// against its first.
inline SscnSel sscn_selection(const int32_t* cols, int k, int64_t d) {
  SscnSel r;
  for (int a = 0; a < k; ++a)
    if (cols[a] < 0 || int64_t(cols[a]) >= d) {
      r.error = SscnSel::Range;
      r.at = a;
      return r;
    }
  r.triple.resize(size_t(3 * k));
  std::copy(cols, cols + k, r.triple.begin());
  std::vector<int> order(size_t(k), 0);
  for (int a = 0; a < k; ++a) order[size_t(a)] = a;
  std::sort(order.begin(), order.end(), [&](int p, int q) { return cols[p] != cols[q] ? cols[p] < cols[q] : p < q; });
  for (int i = 0; i < k; ++i) {
    const int a = order[size_t(i)];
    if (i > 0 && cols[a] == cols[order[size_t(i - 1)]]) {
      r.error = SscnSel::Repeat;
      r.at = a;
      r.first = order[size_t(i - 1)];
      r.triple.clear();
      return r;
    }
    r.triple[size_t(k + i)] = cols[a];
    r.triple[size_t(2 * k + a)] = i;
  }
  return r;
}

}   // namespace krcn
