// blz_state_check — the per-column state rule of the batched Lanczos
// (csrc/krcn_blz_state.hpp) against the reference's loop, on the host.
//
// For every m <= 6 and every breakdown index (none, or 0 .. m - 2) the program
// runs the control flow of optimizer/cubic.py:77-111 on a synthetic beta
// sequence (1 + j at a surviving step, 1e-9 at the breaking one), recording
// what the reference leaves behind: which alphas and betas it writes, which
// columns of V, the truncation and which alpha the final quotient overwrites.
// It then drives the rule the way the kernels do, one blz_step per loop step
// with the state carried in j_break alone, and every further step after the
// break (the device keeps stepping: the other columns are still running),
// and compares.  Prints one line per case; exit status 1 on a mismatch.
#include <cstdio>
#include <limits>
#include <vector>

#include "krcn_blz_state.hpp"

using namespace krcn;

namespace {

constexpr double kTol = 1e-6;

struct Outcome {
  std::vector<int> alpha_set, beta_set, slab_set;   // written by the loop (alphas[j], betas[j], V[:, j])
  int m_eff = 0, j_break = -1, hvps = 0, final_slot = 0, current = 0;
  double beta_last = 0.0;
  bool operator==(const Outcome& o) const {
    return alpha_set == o.alpha_set && beta_set == o.beta_set && slab_set == o.slab_set && m_eff == o.m_eff &&
           j_break == o.j_break && hvps == o.hvps && final_slot == o.final_slot && current == o.current &&
           beta_last == o.beta_last;
  }
};

double beta_of(int j, int brk) { return j == brk ? 1e-9 : 1.0 + j; }

// cubic.py:77-111, its control flow line by line
Outcome reference(int m, int brk) {
  Outcome o;
  o.alpha_set.assign(m, 0);
  o.beta_set.assign(m > 1 ? m - 1 : 1, 0);
  o.slab_set.assign(m, 0);
  double beta = 0.0;
  int cur = 0, j = -1;
  bool broke = false;
  o.slab_set[0] = 1;                       // V[:,0] = v
  for (j = 0; j < m - 1; ++j) {            // for j in range(m-1)
    ++o.hvps;                              //   w = A(v) - beta * v_pre
    o.alpha_set[j] = 1;                    //   alphas[j] = alpha
    beta = beta_of(j, brk);                //   beta = np.linalg.norm(w)
    if ((beta < 0 ? -beta : beta) < kTol) {   // if np.abs(beta) < 1e-6: break
      broke = true;
      break;
    }
    o.beta_set[j] = 1;                     //   betas[j] = beta
    cur = j + 1;                           //   v = w / beta; V[:,j+1] = v
    o.slab_set[j + 1] = 1;
  }
  if (!broke) j = m - 2;                   // Python leaves j at the last value of the range
  o.m_eff = m;
  if (m > 1 && j < m - 2) {                // V = V[:,:j+1]; alphas = alphas[:j+1]; betas = betas[:j]
    o.m_eff = j + 1;
    for (int i = j + 1; i < m; ++i) o.alpha_set[i] = 0, o.slab_set[i] = 0;
    for (int i = j; i < m - 1; ++i) o.beta_set[i] = 0;
  }
  ++o.hvps;                                // alphas[-1] = np.dot(v, A(v))
  o.final_slot = o.m_eff - 1;
  o.alpha_set[o.final_slot] = 1;
  o.current = cur;
  o.j_break = broke ? j : -1;
  o.beta_last = beta;
  return o;
}

// the kernels' view: j_break carried from launch to launch, every loop step enqueued
Outcome device(int m, int brk) {
  Outcome o;
  o.alpha_set.assign(m, 0);
  o.beta_set.assign(m > 1 ? m - 1 : 1, 0);
  o.slab_set.assign(m, 0);
  int jb = kBlzLive;
  o.slab_set[0] = 1;                       // k_blz_norm at the start
  for (int j = 0; j + 1 < m; ++j) {
    const bool live_before = !blz_frozen(jb, j);
    if (jb == kBlzLive) o.alpha_set[j] = 1;                 // k_blz_form: alphas[j] of a live column
    const BlzStep s = blz_step(jb, j, beta_of(j, brk), kTol);   // k_blz_norm
    if (s.live != live_before) std::printf("live mismatch m %d brk %d j %d\n", m, brk, j), o.m_eff = -99;
    // the racy read: a block that sees this step's own store decides the same
    if (s.breaks) {
      const BlzStep again = blz_step(s.j_break, j, beta_of(j, brk), kTol);
      if (again.live != s.live || again.breaks != s.breaks || again.j_break != s.j_break) o.m_eff = -98;
    }
    if (s.live) {
      o.beta_last = beta_of(j, brk);
      if (!s.breaks) o.beta_set[j] = 1, o.slab_set[j + 1] = 1;
    }
    jb = s.j_break;
  }
  if (o.m_eff < 0) return o;
  o.j_break = jb;
  o.m_eff = blz_m_eff(jb, m);
  o.hvps = blz_hvps(jb, m);
  o.final_slot = blz_final_slot(jb, m);
  o.current = blz_current(jb, m);
  o.alpha_set[o.final_slot] = 1;
  // the host keeps alphas[0 .. m_eff) and betas[0 .. m_eff - 1); a slab is a basis vector by blz_is_basis
  for (int i = 0; i < m; ++i) {
    if (i >= o.m_eff) o.alpha_set[i] = 0;
    if (i + 1 < m && i >= o.m_eff - 1) o.beta_set[i] = 0;
    if (o.slab_set[i] != (blz_is_basis(jb, m, i) ? 1 : 0)) o.m_eff = -97;
    if (blz_truncated(jb, m) && i >= o.m_eff) o.slab_set[i] = 0;
  }
  return o;
}

void print(const char* who, int m, int brk, const Outcome& o) {
  std::printf("%s m=%d break=%d m_eff=%d j_break=%d hvps=%d slot=%d current=%d alphas=", who, m, brk, o.m_eff,
              o.j_break, o.hvps, o.final_slot, o.current);
  for (int x : o.alpha_set) std::printf("%d", x);
  std::printf(" betas=");
  for (int x : o.beta_set) std::printf("%d", x);
  std::printf(" slabs=");
  for (int x : o.slab_set) std::printf("%d", x);
  std::printf("\n");
}

}  // namespace

int main() {
  int bad = 0, cases = 0;
  for (int m = 1; m <= 6; ++m)
    for (int brk = -1; brk <= m - 2; ++brk) {
      const Outcome r = reference(m, brk), g = device(m, brk);
      print("rule", m, brk, g);
      ++cases;
      if (!(r == g)) {
        print("REFERENCE", m, brk, r);
        ++bad;
      }
      // the structure stated in words
      const bool trunc = brk >= 0 && brk < m - 2;
      if (g.m_eff != (trunc ? brk + 1 : m) || g.hvps != (brk >= 0 ? brk + 2 : m) ||
          g.final_slot != (trunc ? brk : m - 1) || g.current != (brk >= 0 ? brk : m - 1)) {
        std::printf("STRUCTURE m %d break %d\n", m, brk);
        ++bad;
      }
      if (brk == m - 2 && m > 1 && (g.slab_set[m - 1] != 0 || g.beta_set[m - 2] != 0 || g.m_eff != m)) {
        std::printf("ZERO-LAST m %d\n", m);
        ++bad;
      }
    }
  // the breakdown test itself: absolute, strict, false for NaN
  const double nan = std::numeric_limits<double>::quiet_NaN();
  if (!blz_breaks(9.9e-7, kTol) || !blz_breaks(-9.9e-7, kTol) || blz_breaks(1e-6, kTol) || blz_breaks(nan, kTol) ||
      !blz_breaks(0.0, kTol)) {
    std::printf("BREAK-TEST\n");
    ++bad;
  }
  std::printf("cases=%d bad=%d\n", cases, bad);
  return bad ? 1 : 0;
}
