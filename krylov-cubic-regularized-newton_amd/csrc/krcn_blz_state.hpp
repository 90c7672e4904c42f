// krcn_blz_state.hpp — the per-column state rule of the batched Lanczos
// (krcn_lanczos_block.hip, kernels: krcn_blz.hpp).  Plain C++17, no HIP header:
// the kernels call these functions, the host reads its results through them,
// and tests/native/blz_state_check.cpp walks them with g++ under the host
// sanitizers.
//
// A column runs the reference's recurrence (optimizer/cubic.py:77-111) on its
// own.  Its whole control state is one integer, j_break: -1 while the column
// is live, else the loop index j at which |beta| < tol ended it.  Everything
// the reference derives from `j` after its loop follows from (j_break, m):
//   * the basis is truncated only when j_break < m - 2 (cubic.py:105-108); a
//     break at j_break == m - 2 keeps m columns, the last of them zero, and
//     betas[m - 2] = 0;
//   * the final quotient (cubic.py:109) uses the column's current v, which is
//     slab j_break of a broken column and slab m - 1 otherwise, and overwrites
//     alphas[m_eff - 1];
//   * m = 1 runs no loop step.
#pragma once

#ifndef KRCN_HD
#ifdef __HIPCC__
#define KRCN_HD __host__ __device__
#else
#define KRCN_HD
#endif
#endif

namespace krcn {

constexpr int kBlzLive = -1;   // j_break of a column that has not broken down

// cubic.py:98: np.abs(beta) < tol (false for a NaN beta, as there)
KRCN_HD inline bool blz_breaks(double beta, double tol) { return (beta < 0.0 ? -beta : beta) < tol; }

// The column broke at an earlier loop step than j: step j leaves its alphas,
// betas, state and vectors alone.  (A launch that settles step j may read
// j_break while its block 0 stores j there: both values answer "not frozen".)
KRCN_HD inline bool blz_frozen(int j_break, int j) { return j_break >= 0 && j_break < j; }

// What loop step j (0 <= j <= m - 2) does to a column, given the norm beta of
// its unnormalised next vector.
struct BlzStep {
  bool live;        // the column ran step j: alphas[j] and beta_last are its
  bool breaks;      // ... and |beta| < tol ends it here: j_break = j, betas[j] stays 0, slab j + 1 is zero
  int j_break;      // the column's state after the step
};
KRCN_HD inline BlzStep blz_step(int j_break, int j, double beta, double tol) {
  BlzStep s{};
  s.live = !blz_frozen(j_break, j);   // (j_break == j: this step's own break, seen through the race above)
  s.breaks = s.live && blz_breaks(beta, tol);
  s.j_break = s.live ? (s.breaks ? j : kBlzLive) : j_break;
  return s;
}

// After the loop (cubic.py:105-111).
KRCN_HD inline bool blz_truncated(int j_break, int m) { return j_break >= 0 && j_break < m - 2; }
KRCN_HD inline int blz_m_eff(int j_break, int m) { return blz_truncated(j_break, m) ? j_break + 1 : m; }
// Hessian-vector products the reference runs: one per loop step up to the break, and the final quotient's
KRCN_HD inline int blz_hvps(int j_break, int m) { return (j_break >= 0 ? j_break + 1 : m - 1) + 1; }
// the slab that holds the column's current v (the final quotient's operand)
KRCN_HD inline int blz_current(int j_break, int m) { return j_break >= 0 ? j_break : m - 1; }
// the alpha the final quotient overwrites: alphas[-1] of the (possibly truncated) array
KRCN_HD inline int blz_final_slot(int j_break, int m) { return blz_m_eff(j_break, m) - 1; }
// slab s (0 <= s < m) holds a basis vector of the column; every other slab of the column is zero
KRCN_HD inline bool blz_is_basis(int j_break, int m, int s) { return s <= blz_current(j_break, m); }

}  // namespace krcn
