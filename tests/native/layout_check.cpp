// Command-line face of the pass-plan layouts (csrc/krcn_layout.hpp) for the
// host sanitizer build: tests/test_sanitizers.py and tests/test_plan_layouts.py
// run the layout of one pass on a sparsity pattern, the program checks the
// layout's invariants and prints its scalars.
//   layout_check <pattern.bin> fmt=F dtype=f64|f32 pass=P seq=0|1 accum=-1|0|1 lanes=L slicing=S
// pattern.bin: int32 rows, cols, nnz, ptr[rows + 1], idx[nnz] (the pass's CSR;
// a window plan's 16-bit column offsets are idx minus the slice's first column).
// fmt: 1 wave tiles, 2 sorted tiles, 3 LDS windows (accum = -1: the forced
// format's choice of mode), 4 jagged.
// Prints one line of key=value pairs (kind S L ntiles grid as
// krcn_csr_plan_info reports them, then the format's own scalars) and exits 0;
// a refused plan prints the library's message on stderr and exits 2; a
// violated invariant prints it and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "krcn_layout.hpp"

using namespace krcn;

#define REQUIRE(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "layout_check: line %d: %s\n", __LINE__, #cond);  \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

struct Pattern {
  int rows = 0, cols = 0, nnz = 0;
  std::vector<int> ptr, idx;
};

struct Args {
  int fmt = 1, pass = 1, seq = 0, accum = -1, lanes = 0, slicing = 0;
  bool f64 = true;
};

static int refusal() {
  std::fprintf(stderr, "%s\n", krcn_last_error_string());
  return 2;
}

// build_slices on the host: the slice-major row pointers (S * rows + 1) of the
// pattern cut at the column bounds.
static std::vector<int> slice_ptr(const Pattern& A, const std::vector<int>& bounds) {
  const int S = int(bounds.size()) - 1;
  std::vector<int> hp(size_t(S) * A.rows + 1, 0);
  for (int r = 0; r < A.rows; ++r)
    for (int e = A.ptr[r]; e < A.ptr[r + 1]; ++e) {
      int sl = 0;
      while (sl + 1 < S && A.idx[e] >= bounds[sl + 1]) ++sl;
      ++hp[size_t(sl) * A.rows + r + 1];
    }
  for (size_t i = 1; i < hp.size(); ++i) hp[i] += hp[i - 1];
  return hp;
}

// ---------------------------------------------------------------- tiles
static int check_tiles(const Pattern& A, const Args& a) {
  const int rows = A.rows;
  const TilePolicyIn in{a.fmt == 2 ? KRCN_FORMAT_SORTED : KRCN_FORMAT_WAVE, a.pass, a.lanes, a.slicing, 0, false, false,
                        size_t(a.f64 ? 8 : 4)};
  const TilePolicy tp = tile_policy(rows, A.cols, A.nnz, in, A.ptr.data());
  std::vector<int> bounds(tp.S + 1);
  for (int k = 0; k <= tp.S; ++k) bounds[k] = slice_base(A.cols, k, tp.S);
  const std::vector<int> hp = tp.S == 1 ? A.ptr : slice_ptr(A, bounds);
  const TileLayout tl = tile_layout(rows, A.cols, tp, hp.data());
  const int S = tp.S, sort_tile = tp.sort_nt * kSortPerThread;
  const int cap_nnz = tp.sorted ? sort_tile : kWaveTileNnz, cap_rows = tp.sorted ? sort_tile / 4 : kWaveTileRows;
  REQUIRE(tl.ntiles == int(tl.tiles.size()) && int(tl.tbeg.size()) == tp.groups + 1);
  REQUIRE(tl.tbeg[0] == 0 && tl.tbeg[tp.groups] == tl.ntiles);
  // the tiles of a slice partition its rows in order (sorted: long rows after tmid, each in order)
  std::vector<int> next(S, 0), next_long(S, 0);
  std::vector<std::vector<char>> seen(S, std::vector<char>(size_t(rows), 0));
  for (int g = 0; g < tp.groups; ++g) {
    REQUIRE(tl.tbeg[g] <= tl.tmid[g] && tl.tmid[g] <= tl.tbeg[g + 1]);
    for (int t = tl.tbeg[g]; t < tl.tbeg[g + 1]; ++t) {
      const TileDesc& d = tl.tiles[size_t(t)];
      REQUIRE(d.slice >= 0 && d.slice < S && d.slice % tp.groups == g);
      REQUIRE(0 <= d.row0 && d.row0 < d.row1 && d.row1 <= rows);
      const int* rp = hp.data() + size_t(d.slice) * rows;
      REQUIRE(d.p0 == rp[d.row0] && d.p1 == rp[d.row1]);
      if (tp.sorted) REQUIRE((t < tl.tmid[g]) == (d.long_row == 0));
      int& nx = tp.sorted && d.long_row ? next_long[d.slice] : next[d.slice];
      REQUIRE(d.row0 >= nx);   // in order
      nx = d.row1;
      for (int r = d.row0; r < d.row1; ++r) {
        REQUIRE(!seen[d.slice][size_t(r)]);
        seen[d.slice][size_t(r)] = 1;
      }
      if (d.long_row) {
        REQUIRE(d.row1 == d.row0 + 1);
      } else {   // within the nonzero and row caps
        REQUIRE(d.row1 - d.row0 <= cap_rows);
        REQUIRE((tp.sorted ? d.p1 - d.p0 : d.p1 - (d.p0 & ~3)) <= cap_nnz);
      }
      REQUIRE(d.pad0 == (tp.sorted ? slice_base(A.cols, d.slice, S) : 0));
    }
  }
  for (int sl = 0; sl < S; ++sl)
    for (int r = 0; r < rows; ++r) REQUIRE(seen[sl][size_t(r)]);
  if (tp.sorted) {   // the sort segments ascend and end at nnz
    REQUIRE(!tl.segs.empty() && tl.segs.back() == A.nnz && tl.segs.size() == tl.segbase.size() + 1);
    for (size_t i = 0; i + 1 < tl.segs.size(); ++i) {
      REQUIRE(tl.segs[i] < tl.segs[i + 1]);
      REQUIRE(tl.segs[i + 1] - tl.segs[i] <= sort_tile);
    }
  } else {
    REQUIRE(tl.segs.empty() && tl.segbase.empty());
  }
  const int per_group = tp.sorted ? kBlocksPerGroup * kNT / tp.sort_nt : kBlocksPerGroup;
  const int cap = tp.groups > 1 ? tp.groups * per_group : (tp.sorted ? kMaxGrid * kNT / tp.sort_nt : kMaxGrid);
  REQUIRE(1 <= tl.grid && tl.grid <= cap);
  std::printf("kind=%d S=%d L=%d ntiles=%d grid=%d groups=%d sort_nt=%d\n", tp.sorted ? KRCN_PLAN_SORTED : KRCN_PLAN_WAVE,
              S, tp.L, tl.ntiles, tl.grid, tp.groups, tp.sort_nt);
  return 0;
}

// ---------------------------------------------------------------- LDS windows
template <typename T>
static int check_xt(const Pattern& A, const WinLayout& wl) {
  const int rows = A.rows, cols = A.cols, B = wl.grid;
  std::vector<unsigned short> hidx(size_t(A.nnz) + 1);
  std::vector<T> hval(size_t(A.nnz) + 1);
  for (int e = 0; e < A.nnz; ++e) {
    hidx[size_t(e)] = static_cast<unsigned short>(A.idx[e]);
    hval[size_t(e)] = T(e + 1);   // names the nonzero (exact in either dtype at these sizes)
  }
  const XtLayout<T> x = xt_layout<T, T>(rows, wl.R, cols, hidx.data(), hval.data(), A.ptr.data(), wl.cut, B);
  if (x.skipped) return 0;
  REQUIRE(x.cp.size() == size_t(B) * (size_t(cols) + 1) && x.xr.size() == x.xv.size());
  REQUIRE(x.xr.size() % kXtChunk == 0);
  std::vector<char> seen(size_t(A.nnz) + 1, 0);
  int prev = 0;
  for (int b = 0; b < B; ++b) {
    const int* cp = x.cp.data() + size_t(b) * (size_t(cols) + 1);
    const int r0 = std::min(rows, wl.cut[b] * wl.R), r1 = std::min(rows, wl.cut[b + 1] * wl.R);
    REQUIRE(cp[cols] - cp[0] <= XtGeom<T>::kChunks);
    for (int c = 0; c <= cols; ++c) {   // chunk ids are monotone, across blocks too
      REQUIRE(cp[c] >= prev);
      prev = cp[c];
    }
    REQUIRE(size_t(cp[cols]) * kXtChunk <= x.xr.size());
    for (int c = 0; c < cols; ++c) {
      int last = -1;
      bool pad = false;
      for (int k = cp[c] * kXtChunk; k < cp[c + 1] * kXtChunk; ++k) {
        if (x.xr[size_t(k)] == kXtPad) {   // pads: after the run, value 0
          REQUIRE(x.xv[size_t(k)] == T(0));
          pad = true;
          continue;
        }
        REQUIRE(!pad && int(x.xr[size_t(k)]) > last && int(x.xr[size_t(k)]) < r1 - r0);   // rows ascend
        last = x.xr[size_t(k)];
        const int e = int(x.xv[size_t(k)]) - 1;
        REQUIRE(e >= A.ptr[r0 + last] && e < A.ptr[r0 + last + 1] && A.idx[e] == c && !seen[size_t(e)]);
        seen[size_t(e)] = 1;
      }
    }
  }
  for (int e = 0; e < A.nnz; ++e) REQUIRE(seen[size_t(e)]);   // every nonzero exactly once
  return 1;
}

template <typename T>
static int check_window(const Pattern& A, const Args& a) {
  const int rows = A.rows;
  const int accum = a.accum >= 0 ? a.accum : window_forced<T>(A.cols) == 1;
  const WinShape sh = win_shape<T>(A.cols, accum);
  const int S = sh.S;
  REQUIRE(int(sh.bounds.size()) == S + 1 && sh.bounds[0] == 0 && sh.bounds[S] == A.cols && sh.W <= WinGeom<T>::kW);
  const std::vector<int> hp = slice_ptr(A, sh.bounds);
  const WinLayout wl = win_layout(sh, rows, A.nnz, hp.data());
  if (wl.refused != KRCN_OK) return refusal();
  const int nt = wl.ntiles;
  REQUIRE(nt == (rows + wl.R - 1) / wl.R && (wl.R == 16 || wl.R == 32 || wl.R == 64));
  for (int sl = 0; sl < S; ++sl)   // every tile holds at most 65,535 nonzeros
    for (int t = 0; t < nt; ++t) {
      const int* rp = hp.data() + size_t(sl) * rows;
      REQUIRE(rp[std::min(rows, (t + 1) * wl.R)] - rp[t * wl.R] <= 65535);
    }
  REQUIRE(wl.segs.size() == size_t(wl.grid) * wl.stride);
  int xt = 0;
  if (accum) {
    REQUIRE(wl.stride == S && int(wl.cut.size()) == wl.grid + 1 && wl.cut[0] == 0 && wl.cut[wl.grid] == nt);
    for (int b = 0; b < wl.grid; ++b) {   // the block ranges partition [0, ntiles)
      const int t0 = wl.cut[b], t1 = wl.cut[b + 1];
      REQUIRE(t0 <= t1);
      if (wl.grid < 64 * kNumCUs) REQUIRE(t1 - t0 <= kWinWaves * kWinTMax);
      for (int sl = 0; sl < S; ++sl) {
        const WinSeg& g = wl.segs[size_t(b) * S + sl];
        if (t0 == t1) {
          REQUIRE(g.slice == 0 && g.t0 == 0 && g.t1 == 0 && g.flags == 0);
          continue;
        }
        REQUIRE(g.slice == sl && g.t0 == t0 && g.t1 == t1);
        REQUIRE(g.flags == (kSegLoad | (sl == S - 1 ? kSegFlush : 0) | (sl == 0 ? S << 8 : 0)));
      }
    }
    if (S == 1 && A.cols <= kWinNT) xt = check_xt<T>(A, wl);
  } else {
    REQUIRE(wl.stride == 1 && wl.grid == S * sh.kpb);
    std::vector<int> next(S, 0), chunks(S, 0), last_chunk(S, -1);
    for (int b = 0; b < wl.grid; ++b) {
      int sl = 0, c = 0;
      win_block_slice(b, wl.grid, S, wl.kpb, sl, c);
      REQUIRE(sl >= 0 && sl < S && c >= 0 && c < sh.kpb);
      ++chunks[sl];
      const WinSeg& g = wl.segs[size_t(b)];
      REQUIRE(g.slice == sl);   // every block names a valid slice: its own
      if (g.flags == 0) {
        REQUIRE(g.t0 == 0 && g.t1 == 0);
        continue;
      }
      REQUIRE(g.flags == (kSegLoad | kSegFlush | (1 << 8)) && g.t0 < g.t1 && g.t1 <= nt);
    }
    // the non-empty segments of a slice partition its tiles, in chunk order
    for (int c = 0; c < sh.kpb; ++c)
      for (int b = 0; b < wl.grid; ++b) {
        int sl = 0, cc = 0;
        win_block_slice(b, wl.grid, S, wl.kpb, sl, cc);
        const WinSeg& g = wl.segs[size_t(b)];
        if (cc != c || g.flags == 0) continue;
        REQUIRE(g.t0 == next[sl]);
        next[sl] = g.t1;
      }
    for (int sl = 0; sl < S; ++sl) REQUIRE(chunks[sl] == sh.kpb && next[sl] == nt);
  }
  int empty = 0;
  for (const WinSeg& g : wl.segs) empty += g.flags == 0;
  std::printf("kind=%d S=%d L=1 ntiles=%d grid=%d W=%d R=%d kpb=%d xt=%d empty=%d\n", sh.kind, S, nt, wl.grid, sh.W,
              wl.R, sh.kpb, xt, empty);
  return 0;
}

// ---------------------------------------------------------------- jagged
template <typename T>
static int check_jag(const Pattern& A, const Args& a) {
  const int rows = A.rows;
  const int* hp = A.ptr.data();
  const JagLayout J = jag_layout<T>(rows, A.cols, A.nnz, a.pass, a.seq != 0, hp);
  if (J.refused != KRCN_OK) return refusal();
  const int G = J.G, R = J.R, B = J.B;
  REQUIRE(G == (rows + 63) / 64 && B == R * J.SG && J.Sg == (J.S + J.SG - 1) / J.SG);
  REQUIRE(J.S == (A.cols + J.W - 1) / J.W && J.W <= (J.S == 1 ? JagGeom<T>::kW1 : JagGeom<T>::kW2));
  // cut starts at 0, ends at G, never decreases; the largest range holds <= kJagWaves K groups
  REQUIRE(int(J.cut.size()) == R + 1 && J.cut[0] == 0 && J.cut[R] == G);
  int mx = 0;
  for (int b = 0; b < R; ++b) {
    REQUIRE(J.cut[b] <= J.cut[b + 1]);
    mx = std::max(mx, J.cut[b + 1] - J.cut[b]);
    for (int g = J.cut[b]; g < J.cut[b + 1]; ++g) REQUIRE(J.gblk[size_t(g)] == b);   // gblk agrees with cut
  }
  REQUIRE(int(J.gblk.size()) == G && mx <= kJagWaves * J.K);
  // K is the smallest variant the rule allows
  if (J.S == 1) {
    REQUIRE(J.K == 1 || J.K == 2 || J.K == 3 || J.K == kJagK1);
    if (J.K > 1) REQUIRE(mx > kJagWaves * (J.K == kJagK1 ? 3 : J.K - 1));
  } else {
    REQUIRE(J.K == 4 || J.K == 8);
    if (J.K == 8) REQUIRE(mx > kJagWaves * 4);
  }
  REQUIRE(J.NU == int64_t(B) * J.Sg * J.K * kJagWaves && (int64_t(1) << J.ubits) > J.NU);
  // every row longer than lthr is in lrows once, ascending
  const int nl = int(J.lrows.size());
  if (J.lthr == 0) REQUIRE(nl == 0);
  int k = 0;
  int64_t lnnz = 0;
  for (int r = 0; r < rows; ++r)
    if (J.lthr > 0 && hp[r + 1] - hp[r] > J.lthr) {
      REQUIRE(k < nl && J.lrows[size_t(k)] == r);
      lnnz += hp[r + 1] - hp[r];
      ++k;
    }
  REQUIRE(k == nl && lnnz == J.lnnz);
  int maxtasks = 0;
  if (nl > 0) {
    REQUIRE(int(J.ltask.size()) == nl + 1 && int(J.lbeg.size()) == nl + 1 && J.ltask[0] == 0 && J.lbeg[0] == 0);
    REQUIRE(J.tasks.size() == 2 * (size_t(J.ltask[size_t(nl)]) + 1));
    for (int i = 0; i < nl; ++i) {   // a long row's tasks tile [lbeg, lbeg + len) in order, each <= kJagTask
      const int len = hp[J.lrows[size_t(i)] + 1] - hp[J.lrows[size_t(i)]];
      int at = J.lbeg[size_t(i)];
      REQUIRE(J.lbeg[size_t(i) + 1] >= at + len && J.ltask[size_t(i) + 1] > J.ltask[size_t(i)]);
      for (int t = J.ltask[size_t(i)]; t < J.ltask[size_t(i) + 1]; ++t) {
        REQUIRE(J.tasks[2 * size_t(t)] == at && J.tasks[2 * size_t(t) + 1] >= 1 && J.tasks[2 * size_t(t) + 1] <= kJagTask);
        at += J.tasks[2 * size_t(t) + 1];
      }
      REQUIRE(at == J.lbeg[size_t(i)] + len);
    }
    // lcut is monotone and no block holds more than tcap tasks
    REQUIRE(J.lcut.size() == 2 * (size_t(B) + 1) && J.lcut[0] == 0 && J.lcut[size_t(B)] == nl);
    for (int b = 0; b < B; ++b) {
      REQUIRE(J.lcut[size_t(b)] <= J.lcut[size_t(b) + 1]);
      const int nt = J.lcut[size_t(B) + 2 + b] - J.lcut[size_t(B) + 1 + b];
      REQUIRE(nt >= 0 && nt <= J.tcap);
      maxtasks = std::max(maxtasks, nt);
    }
    for (int b = 0; b <= B; ++b) REQUIRE(J.lcut[size_t(B) + 1 + b] == J.ltask[size_t(J.lcut[size_t(b)])]);
  }
  std::printf("kind=%d S=%d L=1 ntiles=%d grid=%d W=%d SG=%d K=%d R=%d lthr=%d nlong=%d tcap=%d maxtasks=%d\n",
              KRCN_PLAN_JAG, J.S, G, B, J.W, J.SG, J.K, R, J.lthr, nl, J.tcap, maxtasks);
  return 0;
}

template <typename T>
static int run(const Pattern& A, const Args& a) {
  if (a.fmt == 3) return check_window<T>(A, a);
  if (a.fmt == 4) return check_jag<T>(A, a);
  return check_tiles(A, a);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: layout_check <pattern.bin> fmt=F dtype=f64|f32 pass=P seq=0|1 accum=-1|0|1 lanes=L slicing=S\n");
    return 1;
  }
  Args a;
  for (int i = 2; i < argc; ++i) {
    const std::string kv = argv[i];
    const size_t eq = kv.find('=');
    REQUIRE(eq != std::string::npos);
    const std::string key = kv.substr(0, eq), v = kv.substr(eq + 1);
    if (key == "dtype") a.f64 = v == "f64";
    else if (key == "fmt") a.fmt = std::atoi(v.c_str());
    else if (key == "pass") a.pass = std::atoi(v.c_str());
    else if (key == "seq") a.seq = std::atoi(v.c_str());
    else if (key == "accum") a.accum = std::atoi(v.c_str());
    else if (key == "lanes") a.lanes = std::atoi(v.c_str());
    else if (key == "slicing") a.slicing = std::atoi(v.c_str());
    else REQUIRE(!"a known key");
  }
  REQUIRE(a.fmt >= 1 && a.fmt <= 4 && (a.pass == 1 || a.pass == 2));
  Pattern A;
  std::ifstream f(argv[1], std::ios::binary);
  int head[3] = {0, 0, 0};
  f.read(reinterpret_cast<char*>(head), sizeof(head));
  REQUIRE(f && head[0] >= 0 && head[1] >= 0 && head[2] >= 0);
  A.rows = head[0], A.cols = head[1], A.nnz = head[2];
  A.ptr.resize(size_t(A.rows) + 1);
  A.idx.resize(size_t(A.nnz) + 1);
  f.read(reinterpret_cast<char*>(A.ptr.data()), std::streamsize(sizeof(int) * (size_t(A.rows) + 1)));
  if (A.nnz > 0) f.read(reinterpret_cast<char*>(A.idx.data()), std::streamsize(sizeof(int) * size_t(A.nnz)));
  REQUIRE(f && A.ptr[0] == 0 && A.ptr[size_t(A.rows)] == A.nnz);
  for (int r = 0; r < A.rows; ++r) REQUIRE(A.ptr[size_t(r)] <= A.ptr[size_t(r) + 1]);
  for (int e = 0; e < A.nnz; ++e) REQUIRE(A.idx[size_t(e)] >= 0 && A.idx[size_t(e)] < A.cols);
  return a.f64 ? run<double>(A, a) : run<float>(A, a);
}
