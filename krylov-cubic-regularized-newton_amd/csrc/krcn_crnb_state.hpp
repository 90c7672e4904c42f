// krcn_crnb_state.hpp — the per-column state rule of the batched Krylov-CRN
// step (krcn_crn_block.hip, kernels: krcn_crnb.hpp).  Plain C++17, no HIP
// header: the kernels call these functions, the host reads the records
// through them, and tests/native/crnb_state_check.cpp walks them with g++
// under the host sanitizers.
//
// A column runs the reference's line search (optimizer/cubic.py:293-303) on
// its own: M = reg_coef * beta, a solve, the test value_new > value -
// model_decrease, and while it holds and trials < max_trials: M /= beta, the
// next solve, trials += 1.  Its control state is one phase:
//   live      the next trial solves, combines, evaluates and judges the column;
//   accepted  a trial met value_new <= value - model_decrease (also when the
//             comparison is false for a NaN, as the reference's while);
//   capped    the trial after max_trials rejections failed the test too;
//   failed    a solve ended with status 1 (T + lam I not positive definite) or
//             2 (zero derivative): the reference raises there;
//   inactive  the caller started the column as done.
// Every phase but live is final: a later trial's launches leave the column's
// record, x_new and Ax_new alone.  The chain has ended when no column is live.
#pragma once

#ifndef KRCN_HD
#ifdef __HIPCC__
#define KRCN_HD __host__ __device__
#else
#define KRCN_HD
#endif
#endif

namespace krcn {

enum { kCrnbLive = 0, kCrnbAccepted = 1, kCrnbCapped = 2, kCrnbFailed = 3, kCrnbInactive = 4 };

// One column's record (device state, and the mapped host copy the judge writes).
struct CrnbCol {
  int phase;           // kCrnb*
  int trials;          // backtracking trials after the first solve
  int solver_it;       // Newton iterations of the last solve
  int solver_status;   // kCubic* of the last solve
  int m_eff;           // basis vectors kept by the column's recurrence (blz_m_eff)
  int pad0, pad1, pad2;
  double M;            // regularisation of the next (after the end: the last) solve
  double lam;          // its root
  double model_decrease;
  double value_new;
  double gnorm;        // ||g_c||: the subproblem's g is gnorm e1
  double dx2;          // ||x_new,c - x_c||^2, formed once the chain has ended
  double value;        // f_c(x_c), the caller's
  double l2;
  double r0;           // every solve of the column starts from it
};
static_assert(sizeof(CrnbCol) % sizeof(double) == 0, "records are copied as doubles");

// The head of the state block: the chain's one flag, written by the judge alone.
struct CrnbHead {
  int all_done;
  int pad;
};

KRCN_HD inline bool crnb_live(int phase) { return phase == kCrnbLive; }
KRCN_HD inline int crnb_start(bool active) { return active ? kCrnbLive : kCrnbInactive; }
// solver status 1 / 2: nothing to try (the host path raises LinAlgError / ArithmeticError)
KRCN_HD inline bool crnb_solve_failed(int solver_status) { return solver_status == 1 || solver_status == 2; }

// What the subproblem launch of a trial leaves: a failed solve ends the column's chain.
KRCN_HD inline int crnb_after_solve(int phase, int solver_status) {
  return crnb_live(phase) && crnb_solve_failed(solver_status) ? kCrnbFailed : phase;
}

// What the judge of a trial does to a column (cubic.py:293-303): accept, stop
// at the cap, or divide M by beta for the next trial.  A column that is not
// live keeps everything.
struct CrnbVerdict {
  int phase;
  int trials;
  double M;
};
KRCN_HD inline CrnbVerdict crnb_judge(int phase, int trials, double M, double value, double model_decrease,
                                      double value_new, double ls_beta, int max_trials) {
  CrnbVerdict v{phase, trials, M};
  if (!crnb_live(phase)) return v;
  if (!(value_new > value - model_decrease)) v.phase = kCrnbAccepted;
  else if (trials >= max_trials) v.phase = kCrnbCapped;
  else {
    v.M = M / ls_beta;
    v.trials = trials + 1;
  }
  return v;
}

// Trials a chain can need: the one after max_trials rejections ends it itself.
KRCN_HD inline int crnb_total_trials(int max_trials) { return max_trials + 1; }
// What the caller reads back (krcn_crn_info): a failed or inactive column moved nowhere.
KRCN_HD inline bool crnb_accepted(int phase) { return phase == kCrnbAccepted; }
KRCN_HD inline bool crnb_moved(int phase) { return phase == kCrnbAccepted || phase == kCrnbCapped; }

}  // namespace krcn
