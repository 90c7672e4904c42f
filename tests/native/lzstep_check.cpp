// Command-line face of the Lanczos step choice (csrc/krcn_lzstep.hpp) for the
// host sanitizer build: tests/test_lanczos_step.py gives the inputs of
// lanczos_step as key=value pairs (a key left out keeps LzStepIn's default;
// every knob defaults to on) and reads the choice.
//   lzstep_check shard=none|rows|cols multi=0|1 f64=0|1 reorth=0|1 n=N d=D pcap=P
//                p1=KIND p1_S=S p1_grid=G p1_combine_grid=G p1_xt=0|1 p2=KIND p2_S=S p2_jG=G
//                pq=0|1 pq_local=P rows_pq=P rows_early=0|1
//                fuse= zw= xt_small= xt_comb= xt_rb= lz2= early= pack= cgs_fuseb=
// KIND: wave, sorted, window-slices, window-accum, jagged, dense.
// Prints "step=NAME id=I zw=Z pack=P Pc=C" and exits 0; a refusal prints the
// library's message on stderr and exits 2; a malformed input exits 1.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "krcn_lzstep.hpp"

using namespace krcn;

static int usage(const std::string& what) {
  std::fprintf(stderr, "lzstep_check: bad argument %s\n", what.c_str());
  return 1;
}

static int plan_kind(const std::string& v) {
  static const char* const names[] = {"wave", "sorted", "window-slices", "window-accum", "jagged", "dense"};
  for (int i = 0; i < 6; ++i)
    if (v == names[i]) return KRCN_PLAN_WAVE + i;
  return -1;
}

int main(int argc, char** argv) {
  LzStepIn in;
  for (int i = 1; i < argc; ++i) {
    const std::string kv = argv[i];
    const size_t eq = kv.find('=');
    if (eq == std::string::npos) return usage(kv);
    const std::string key = kv.substr(0, eq), v = kv.substr(eq + 1);
    const long long x = std::atoll(v.c_str());
    if (key == "shard") {
      if (v != "none" && v != "rows" && v != "cols") return usage(kv);
      in.shard = v == "none" ? KRCN_SHARD_NONE : v == "rows" ? KRCN_SHARD_ROWS : KRCN_SHARD_COLS;
    } else if (key == "p1" || key == "p2") {
      const int kind = plan_kind(v);
      if (kind < 0) return usage(kv);
      (key == "p1" ? in.p1_kind : in.p2_kind) = kind;
    }
    else if (key == "multi") in.multi = x != 0;
    else if (key == "f64") in.f64 = x != 0;
    else if (key == "reorth") in.reorth = x != 0;
    else if (key == "n") in.n = x;
    else if (key == "d") in.d = x;
    else if (key == "pcap") in.pcap = x;
    else if (key == "p1_S") in.p1_S = int(x);
    else if (key == "p1_grid") in.p1_grid = int(x);
    else if (key == "p1_combine_grid") in.p1_combine_grid = int(x);
    else if (key == "p1_xt") in.p1_xt = int(x);
    else if (key == "p2_S") in.p2_S = int(x);
    else if (key == "p2_jG") in.p2_jG = int(x);
    else if (key == "pq") in.pq = x != 0;
    else if (key == "pq_local") in.pq_local = int(x);
    else if (key == "rows_pq") in.rows_pq = int(x);
    else if (key == "rows_early") in.rows_early = int(x);
    else if (key == "fuse") in.knobs.fuse = x != 0;
    else if (key == "zw") in.knobs.zw = x != 0;
    else if (key == "xt_small") in.knobs.xt_small = x != 0;
    else if (key == "xt_comb") in.knobs.xt_comb = x != 0;
    else if (key == "xt_rb") in.knobs.xt_rb = int(x);
    else if (key == "lz2") in.knobs.lz2 = x != 0;
    else if (key == "early") in.knobs.early = x != 0;
    else if (key == "pack") in.knobs.pack = x != 0;
    else if (key == "cgs_fuseb") in.knobs.cgs_fuseb = x != 0;
    else return usage(kv);
  }
  if (in.p1_S < 1 || in.p2_S < 1 || in.p1_grid < 1 || in.n < 0 || in.d < 0) return usage("a plan shape below 1");
  const LzStepChoice c = lanczos_step(in);
  if (c.refusal != KRCN_OK) {
    std::fprintf(stderr, "%s\n", krcn_last_error_string());
    return 2;
  }
  std::printf("step=%s id=%d zw=%d pack=%d Pc=%d\n", lz_step_name(c.step), int(c.step), int(c.zw), int(c.pack), c.Pc);
  return 0;
}
