// Command-line face of the SSCN step's staged selection (csrc/krcn_sscn_sel.hpp)
// for the host sanitizer build: tests/test_sscn_selection.py gives d and the
// selection and reads the triple or the refusal.
//   sscn_sel_check D COL [COL ...]
// Prints "cols=.. sorted=.. perm=.." (comma-separated) and exits 0; a refused
// selection prints "range at=A value=V" or "repeat at=A value=V first=F" and
// exits 2; a malformed input exits 1.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "krcn_sscn_sel.hpp"

using namespace krcn;

static bool number(const char* text, long long lo, long long hi, long long* out) {
  char* end = nullptr;
  errno = 0;
  const long long v = std::strtoll(text, &end, 10);
  if (errno || end == text || *end || v < lo || v > hi) return false;
  *out = v;
  return true;
}

static void print_part(const char* name, const int32_t* v, int k, const char* tail) {
  std::printf("%s=", name);
  for (int a = 0; a < k; ++a) std::printf(a ? ",%d" : "%d", int(v[a]));
  std::printf("%s", tail);
}

int main(int argc, char** argv) {
  long long d = 0;
  if (argc < 3 || !number(argv[1], 0, INT64_MAX, &d)) {
    std::fprintf(stderr, "usage: sscn_sel_check D COL [COL ...]\n");
    return 1;
  }
  // a heap array of exactly k entries, so that a read past either end is the sanitizer's to report
  std::vector<int32_t> cols;
  for (int i = 2; i < argc; ++i) {
    long long c = 0;
    if (!number(argv[i], INT32_MIN, INT32_MAX, &c)) {
      std::fprintf(stderr, "sscn_sel_check: bad column %s\n", argv[i]);
      return 1;
    }
    cols.push_back(int32_t(c));
  }
  cols.shrink_to_fit();
  const int k = int(cols.size());
  const SscnSel r = sscn_selection(cols.data(), k, d);
  if (r.error == SscnSel::Range) {
    std::printf("range at=%d value=%d\n", r.at, int(cols[size_t(r.at)]));
    return 2;
  }
  if (r.error == SscnSel::Repeat) {
    std::printf("repeat at=%d value=%d first=%d\n", r.at, int(cols[size_t(r.at)]), r.first);
    return 2;
  }
  if (r.triple.size() != size_t(3 * k)) return 1;
  print_part("cols", r.triple.data(), k, " ");
  print_part("sorted", r.triple.data() + k, k, " ");
  print_part("perm", r.triple.data() + 2 * k, k, "\n");
  return 0;
}
