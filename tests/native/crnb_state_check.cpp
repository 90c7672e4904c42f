// crnb_state_check — the per-column state rule of the batched Krylov-CRN step
// (csrc/krcn_crnb_state.hpp) against the reference's line search, on the host.
//
// For every max_trials <= 4 and every sequence of trial outcomes — the test
// value_new > value - model_decrease holds (R), fails (A), is false because
// value_new is a NaN (N), or the solve fails with status 1 or 2 (F, G) — the
// program runs optimizer/cubic.py:293-303 as written (a plain restatement:
// first solve, then the while loop) and then drives the rule the way the device
// does: max_trials + 1 trials are enqueued whatever happens, each a solve
// (crnb_after_solve) and a judge (crnb_judge), a column that has ended being
// skipped by both.  It compares what each leaves: how the chain ended, the
// trial count, M (bitwise) and which trials ran a solve.  A column that starts
// inactive is walked too.  Prints one line per case; exit status 1 on a mismatch.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "krcn_crnb_state.hpp"

using namespace krcn;

namespace {

constexpr double kValue = 1.0, kDec = 0.25, kBeta = 0.5, kReg = 1e-3;

struct Outcome {
  int end = 0;       // kCrnb* at the end of the chain
  int trials = 0;
  double M = 0.0;
  int solves = 0;    // solves run
  bool operator==(const Outcome& o) const {
    return end == o.end && trials == o.trials && M == o.M && solves == o.solves;
  }
};

double value_of(char c) {
  if (c == 'R') return 0.9;                                   // > value - dec = 0.75: rejected
  if (c == 'N') return std::numeric_limits<double>::quiet_NaN();   // the comparison is false
  return 0.5;                                                 // accepted
}
int status_of(char c) { return c == 'F' ? 1 : (c == 'G' ? 2 : 0); }

// cubic.py:293-303 (with the cap of Cubic_Krylov_LS.step): seq[t] is what trial t meets
Outcome reference(const std::string& seq, int max_trials) {
  Outcome o;
  double reg = kReg * kBeta;                    // reg_coef = self.reg_coef * self.beta
  size_t t = 0;
  ++o.solves;                                   // s_new, ... = cubic_solver_root(...)
  if (status_of(seq[t])) {                      //   (raises)
    o.end = kCrnbFailed, o.M = reg;
    return o;
  }
  double value_new = value_of(seq[t]);          // value_new = self.loss.value(x_new)
  int trials = 0;
  while (value_new > kValue - kDec && trials < max_trials) {
    reg = reg / kBeta;                          //   reg_coef = reg_coef / self.beta
    ++t;
    ++o.solves;                                 //   s_new, ... = cubic_solver_root(...)
    if (status_of(seq[t])) {
      o.end = kCrnbFailed, o.M = reg, o.trials = trials + 1;
      return o;
    }
    value_new = value_of(seq[t]);
    trials += 1;
  }
  o.end = value_new > kValue - kDec ? kCrnbCapped : kCrnbAccepted;
  o.trials = trials;
  o.M = reg;
  return o;
}

// the device's view: every trial enqueued, the phase carried from launch to launch
Outcome device(const std::string& seq, int max_trials, bool active) {
  Outcome o;
  int phase = crnb_start(active), trials = 0;
  double M = kReg * kBeta;
  for (int t = 0; t < crnb_total_trials(max_trials); ++t) {
    if (!crnb_live(phase)) continue;            // k_crnb_solve returns; so does the rest of the trial
    ++o.solves;
    const int st = status_of(seq[size_t(t)]);
    phase = crnb_after_solve(phase, st);   // (a failing solve of trial t follows t rejections: trials == t)
    const CrnbVerdict v = crnb_judge(phase, trials, M, kValue, kDec, value_of(seq[size_t(t)]), kBeta, max_trials);
    phase = v.phase, trials = v.trials, M = v.M;
  }
  o.end = phase, o.trials = trials, o.M = M;
  return o;
}

const char* name_of(int end) {
  switch (end) {
    case kCrnbLive: return "live";
    case kCrnbAccepted: return "accepted";
    case kCrnbCapped: return "capped";
    case kCrnbFailed: return "failed";
    default: return "inactive";
  }
}

void print(const char* who, int max_trials, const std::string& seq, const Outcome& o) {
  std::printf("%s max=%d seq=%s end=%s trials=%d solves=%d M=%a\n", who, max_trials, seq.c_str(), name_of(o.end),
              o.trials, o.solves, o.M);
}

}  // namespace

int main() {
  const char kinds[] = {'R', 'A', 'N', 'F', 'G'};
  int bad = 0, cases = 0;
  for (int max_trials = 0; max_trials <= 4; ++max_trials) {
    const int len = max_trials + 1;
    int total = 1;
    for (int i = 0; i < len; ++i) total *= 5;
    for (int code = 0; code < total; ++code) {
      std::string seq;
      for (int i = 0, c = code; i < len; ++i, c /= 5) seq.push_back(kinds[c % 5]);
      const Outcome r = reference(seq, max_trials), g = device(seq, max_trials, true);
      print("rule", max_trials, seq, g);
      ++cases;
      if (!(r == g)) {
        print("REFERENCE", max_trials, seq, r);
        ++bad;
      }
      if (g.end == kCrnbLive) {   // max_trials + 1 trials always end a chain
        std::printf("STILL-LIVE max %d seq %s\n", max_trials, seq.c_str());
        ++bad;
      }
    }
    // a column that starts as done: nothing runs, nothing changes
    const Outcome in = device(std::string(size_t(len), 'R'), max_trials, false);
    print("inactive", max_trials, std::string(size_t(len), 'R'), in);
    ++cases;
    if (in.end != kCrnbInactive || in.trials != 0 || in.solves != 0 || in.M != kReg * kBeta) ++bad;
  }
  // the info fields' rules
  if (!crnb_accepted(kCrnbAccepted) || crnb_accepted(kCrnbCapped) || !crnb_moved(kCrnbCapped) ||
      !crnb_moved(kCrnbAccepted) || crnb_moved(kCrnbFailed) || crnb_moved(kCrnbInactive) || crnb_solve_failed(0) ||
      crnb_solve_failed(3) || !crnb_solve_failed(1) || !crnb_solve_failed(2)) {
    std::printf("INFO-RULES\n");
    ++bad;
  }
  std::printf("cases=%d bad=%d\n", cases, bad);
  return bad ? 1 : 0;
}
