// krcn_lzstep.hpp — which Lanczos step a handle runs: one rule from plain
// scalars (the shard mode, the two plans' shapes, the buffers, the tuning
// switches) to one of nine steps, or to a refusal.  Host-only C++17, no HIP
// header: it builds with g++ alone (tests/native/lzstep_check.cpp runs it under
// ASan + UBSan).  lanczos_impl (krcn_lanczos_impl.hpp) enqueues the step this
// returns and krcn_csr_lanczos_step reports it; there is no second copy of
// the rule.
#pragma once
#include <algorithm>

#include "krcn_geom.hpp"
#include "krcn_host.hpp"

namespace krcn {

// Every tuning switch the recurrence reads (A/B knobs: tuning builds only,
// krcn_geom.hpp; each is on unless set to 0).
struct LzKnobs {
  bool fuse = true;       // KRCN_LANCZOS_FUSE: 0 keeps the separate step B
  bool zw = true;         // KRCN_ZW: 0 keeps the fused window pass 1's store of z_j
  bool xt_small = true;   // KRCN_XT_SMALL: 0 keeps the X^T pass of one-piece plans
  bool xt_comb = true;    // KRCN_XT_COMB: 0 adds the X^T partials with k_slice_combine
  int xt_rb = 32;         // KRCN_XT_RB: rows per k_xt_combine block (16 / 32 / 64)
  // KRCN_LZ2: 0 turns the two-launch step off.  It runs wherever a plan allows
  // it; whether the auto plan policy BUILDS such a pair of plans (unsliced
  // sorted pass 1 beside a single-window jagged pass 2) is the same knob read
  // the other way round, off unless 1 (krcn_plan.hip ensure_plans: the policy
  // lost its A/B on rcv1, krcn_csr_set_pass_format still reaches the step).
  bool lz2 = true;
  bool early = true;      // KRCN_LZ_EARLY: 0 keeps the steps of rounds 2-4 (fused, generic)
  bool pack = true;       // KRCN_PACK_NORM: 0 keeps the column shards' separate ||z||^2 all-reduce
  bool cgs_fuseb = true;  // KRCN_CGS_FUSEB: 0 keeps k_lz_step_b ahead of the 1 KiB-piece CGS2 sweeps
};
inline const LzKnobs& lz_knobs() {
  static const LzKnobs k = [] {
    LzKnobs v;
    v.fuse = tuning_on("KRCN_LANCZOS_FUSE");
    v.zw = tuning_on("KRCN_ZW");
    v.xt_small = tuning_on("KRCN_XT_SMALL");
    v.xt_comb = tuning_on("KRCN_XT_COMB");
    const int rb = tuning_value("KRCN_XT_RB", 32);
    v.xt_rb = rb == 16 || rb == 64 ? rb : 32;
    v.lz2 = tuning_on("KRCN_LZ2");
    v.early = tuning_on("KRCN_LZ_EARLY");
    v.pack = tuning_on("KRCN_PACK_NORM");
    v.cgs_fuseb = tuning_on("KRCN_CGS_FUSEB");
    return v;
  }();
  return k;
}

struct LzStepIn {
  int shard = KRCN_SHARD_NONE;
  bool multi = false;   // a communicator of several ranks
  bool f64 = true;
  bool reorth = false;
  int64_t n = 0, d = 0, pcap = kMaxPartials;
  int p1_kind = KRCN_PLAN_WAVE, p1_S = 1, p1_grid = 1, p1_combine_grid = 1, p1_xt = 0;
  int p2_kind = KRCN_PLAN_WAVE, p2_S = 1, p2_jG = 1;
  bool pq = false;      // the handle holds the alpha partials buffer
  int pq_local = 1;     // pass_partials(p1): the partials this rank's pass 1 writes
  int rows_pq = -1;     // row shards, multi: the agreed packed count (-1: not agreed), agree_rows
  int rows_early = 0;   //   and whether every rank's pass-1 grids fit
  LzKnobs knobs;
};

// Stable values (krcn.h KRCN_LZ_*): krcn_csr_lanczos_step reports them.
enum LzStep {
  LZ_GENERIC = KRCN_LZ_GENERIC,                // pass 1, pass 2 + step A, k_lz_step_b (+ CGS2); every shard mode
  LZ_FUSED_WINDOW = KRCN_LZ_FUSED_WINDOW,      // step B in a window-slices pass 1 (SrcLzZ), beta in its combine
  LZ_FUSED_SORTED = KRCN_LZ_FUSED_SORTED,      // the same over sliced sorted tiles
  LZ_FUSED_SMALL = KRCN_LZ_FUSED_SMALL,        // one-piece window pass 1 forms z and beta itself (SrcLzSmall)
  LZ_FUSED_SMALL_XT = KRCN_LZ_FUSED_SMALL_XT,  //   and the blocks' shares of X^T u: pass 2 is their combine
  LZ_TWO_LAUNCH = KRCN_LZ_TWO_LAUNCH,          // unsliced sorted pass 1 + single-window jagged pass 2 (SrcLzU)
  LZ_EARLY = KRCN_LZ_EARLY,                    // early alpha: pass 2 settles alpha_j and runs step B (EpiLz2E)
  LZ_EARLY_COLS = KRCN_LZ_EARLY_COLS,          // column shards: one collective per step
  LZ_EARLY_ROWS = KRCN_LZ_EARLY_ROWS,          // row shards: the alpha partials travel with the d-vector
  LZ_STEPS = 9
};
inline const char* lz_step_name(int step) {
  static const char* const names[LZ_STEPS] = {"generic", "fused-window", "fused-sorted", "fused-small",
                                               "fused-small-xt", "two-launch", "early", "early-cols", "early-rows"};
  return step >= 0 && step < LZ_STEPS ? names[step] : "?";
}

struct LzStepChoice {
  LzStep step = LZ_GENERIC;
  bool zw = false;     // fused-window: pass 1 stores no z_j, pass 2 re-forms it (EpiLz2::zw)
  bool pack = false;   // generic over column shards: ||z||^2 rides the next row-sum all-reduce
  int Pc = 0;          // early-rows: the packed alpha partials every rank sends
  krcn_status refusal = KRCN_OK;
};

// This rank's pass-1 grids fit kMaxPartials (row shards: the alpha partials
// are packed past the d-vector, whose buffer holds d + kMaxPartials).
inline bool lz_rows_fit(int p1_grid, int p1_combine_grid) {
  return std::max(p1_grid, p1_combine_grid) <= kMaxPartials;
}

inline LzStepChoice lanczos_step(const LzStepIn& in) {
  const LzKnobs& k = in.knobs;
  const bool none = in.shard == KRCN_SHARD_NONE, rows = in.shard == KRCN_SHARD_ROWS, cols = in.shard == KRCN_SHARD_COLS;
  LzStepChoice c;
  // Every rank must issue the same collectives with the same lengths: with a
  // multi-rank communicator the row shards' gate and packed count are the
  // values the ranks agreed on after the plan build (the maximum over ranks; a
  // rank whose combine writes fewer zero-fills the rest).
  if (rows && in.multi && in.rows_pq < 0) {
    c.refusal = fail(KRCN_ERR_INVALID, "krcn_lanczos: the row shards have not agreed on their plans (krcn_csr_reserve "
                     "or krcn_csr_attach_comm on every rank)");
    return c;
  }
  c.Pc = in.multi ? in.rows_pq : in.pq_local;
  // Step B fused into the next pass 1: unsharded, no reorthogonalisation, a
  // pass 1 that can form z_j = w - alpha v in its gathers, its grid's norm
  // partials within the buffers.
  const bool fuse_win = in.p1_kind == KRCN_PLAN_WINDOW_SLICES && in.p1_grid % in.p1_S == 0;
  const bool fuse_sorted = in.p1_kind == KRCN_PLAN_SORTED && in.p1_S > 1;
  const bool fuse_small = in.p1_kind == KRCN_PLAN_WINDOW_ACCUM && in.p1_S == 1 && in.d <= kWinNT;
  const bool fuse = k.fuse && none && !in.reorth && (fuse_win || fuse_sorted || fuse_small) && in.p1_grid <= in.pcap;
  // Early alpha: pass 2 must reduce two sums per block (Red2) — the
  // single-window and one-group accumulate jagged passes and the accumulate
  // window pass do.
  const bool p2_red2 = (in.p2_kind == KRCN_PLAN_JAG && (in.p2_S == 1 || in.p2_jG == 1)) ||
                       in.p2_kind == KRCN_PLAN_WINDOW_ACCUM;
  const bool shard_early = in.f64 && !in.reorth && k.early;
  if (fuse && (fuse_win || fuse_sorted) && k.early && p2_red2 && in.pq) {
    c.step = LZ_EARLY;
  } else if (cols && shard_early && k.pack && apply_grid(in.n) <= in.pcap) {
    c.step = LZ_EARLY_COLS;
  } else if (rows && shard_early && (in.multi ? in.rows_early != 0 : lz_rows_fit(in.p1_grid, in.p1_combine_grid)) &&
             c.Pc >= in.pq_local && c.Pc <= kMaxPartials) {
    c.step = LZ_EARLY_ROWS;
  } else if (k.fuse && k.lz2 && none && !in.reorth && in.p1_kind == KRCN_PLAN_SORTED && in.p1_S == 1 &&
             in.p2_kind == KRCN_PLAN_JAG && in.p2_S == 1 && in.p1_grid <= in.pcap) {
    c.step = LZ_TWO_LAUNCH;
  } else if (fuse && fuse_small) {
    c.step = in.p1_xt && k.xt_small ? LZ_FUSED_SMALL_XT : LZ_FUSED_SMALL;
  } else if (fuse) {
    c.step = fuse_win ? LZ_FUSED_WINDOW : LZ_FUSED_SORTED;
    c.zw = fuse_win && k.zw;
  } else {
    c.pack = cols && in.f64 && !in.reorth && k.pack;
  }
  return c;
}

}   // namespace krcn
