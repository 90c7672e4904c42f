// cgn_state_check — the state rule of krcn_cubic_cg (csrc/krcn_cgn_state.hpp)
// driven the way the kernels drive it, on the host, over a diagonal H.
//
// The vectors are plain arrays and every kernel of a tick is restated as a
// loop: pass 1 + pass 2 form q = (H + shift I) p and p.q; the update is the
// exact solve (one "CG iteration": x = rhs / (h + shift) elementwise, r = 0,
// so r.r = 0 and the solve has converged); the direction kernel's ended branch
// does the phase's vector part and forms its sums; the turn calls cgn_turn.
// Sums run left to right.  Prints one line per case: solver_it, status, lam
// (hex), the solve count, the CG iteration count, the ticks and whether s is
// all zeros; tests/test_cgn_state.py reruns each case through scipy.
// Exit status 1 when a chain does not end within its tick bound.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "krcn_cgn_state.hpp"

using namespace krcn;

namespace {

struct Case {
  const char* name;
  std::vector<double> h, g;
  double M, r0, eps;
  int it_max;
};

int run(const Case& c) {
  const size_t d = c.h.size();
  const CgnParams a{c.M, 0.0, c.r0, c.eps, 1e-10, c.it_max, 10 * int(d)};
  std::vector<double> s(d, 0.0), z(d, 0.0), r(c.g), p(c.g), q(d, 0.0);   // k_cg_begin on g
  double gg = 0.0;
  for (size_t i = 0; i < d; ++i) gg += c.g[i] * c.g[i];
  CgnState st = cgn_start(a, gg);                                        // k_cgn_init
  const int64_t bound = cgn_tick_bound(a.it_max, a.cg_maxiter);
  int64_t t = 0;
  for (; t < bound && !st.done; ++t) {
    double rho = 0.0;
    if (!st.skip) {
      double pq = 0.0;
      for (size_t i = 0; i < d; ++i) {                                   // pass 1 + pass 2
        q[i] = (c.h[i] + st.shift) * p[i];
        pq += p[i] * q[i];
      }
      st.pq = pq;                                                        // k_cgn_update: the exact solve
      std::vector<double>& x = st.phase == kCgnSolveY ? z : s;
      for (size_t i = 0; i < d; ++i) {
        x[i] = p[i] / (c.h[i] + st.shift);
        r[i] = 0.0;
      }
    }
    double sa = 0.0, sb = 0.0;
    if (cgn_solve_ended(st.skip, st.k, a.cg_maxiter, st.atol, rho)) {     // k_cgn_dir's ended branch
      for (size_t i = 0; i < d; ++i) {
        if (st.phase == kCgnSolveG) {
          sa += s[i] * s[i];
          z[i] = 0.0, r[i] = p[i] = s[i];
        } else if (st.phase == kCgnSolveY) {
          sa += s[i] * z[i];
          s[i] = 0.0, r[i] = p[i] = c.g[i];
        } else if (st.phase == kCgnClose) {
          sa += s[i] * s[i];
          sb += c.g[i] * s[i];
          s[i] = -s[i];
        } else {
          s[i] = 0.0;
        }
      }
    } else {
      std::printf("NOT-ENDED %s\n", c.name);                             // (an exact solve always ends)
      return 1;
    }
    st = cgn_turn(st, a, rho, sa, sb);                                   // k_cgn_turn
  }
  bool zero = true;
  for (size_t i = 0; i < d; ++i) zero = zero && s[i] == 0.0;
  double ns2 = 0.0;
  for (size_t i = 0; i < d; ++i) ns2 += s[i] * s[i];
  std::printf("case %s its=%d status=%d lam=%a solves=%d cg_iterations=%lld ticks=%lld s_zero=%d dec=%a ns=%a\n", c.name,
              st.solver_it, st.solver_status, st.lam, st.cg_solves, (long long)st.cg_iterations, (long long)st.ticks,
              int(zero), st.model_decrease, st.s_norm);
  if (!st.done || st.ticks != t) {
    std::printf("STILL-RUNNING %s\n", c.name);
    return 1;
  }
  if (st.solver_status != kCgnOk && st.solver_status != kCgnItMax ? !zero : std::sqrt(ns2) != st.s_norm) {
    std::printf("S-MISMATCH %s\n", c.name);
    return 1;
  }
  return 0;
}

}  // namespace

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const std::vector<double> h{0.5, 1.25, 2.0, 3.5, 0.75}, g{0.3, -0.2, 0.45, 0.1, -0.6};
  const Case cases[] = {
      {"well", h, g, 1.0, 0.1, 1e-8, 100},
      {"smallM", h, g, 5e-4, 0.1, 1e-8, 100},
      {"itmax1", h, g, 1.0, 0.1, 1e-8, 1},
      {"itmax3", h, g, 1.0, 0.1, 1e-8, 3},
      {"gzero", h, std::vector<double>(5, 0.0), 1.0, 0.1, 1e-8, 100},
      {"phizero", {0.0}, {1.0}, 1.0, 1.0, 1e-8, 100},   // phi(r0) = 1 - 1 = 0: newton() returns r0 at once
      {"notpd",{0.5, -2.0, 2.0}, {0.0, 1.0, 0.0}, 1.0, 0.1, 1e-8, 100},
      {"nan", h, {0.3, nan, 0.45, 0.1, -0.6}, 1.0, 0.1, 1e-8, 100},
  };
  int bad = 0, n = 0;
  for (const Case& c : cases) {
    bad += run(c);
    ++n;
  }
  std::printf("cases=%d bad=%d\n", n, bad);
  return bad ? 1 : 0;
}
