// krcn_sytd.hpp — the dense cubic subproblem over one tridiagonal reduction:
// Householder tridiagonalisation of the bordered matrix
//
//        | 0   g^T |
//    B = |         |      of order K = k + 1 <= 1025 (fp64, full storage),
//        | g   H   |
//
// whose first reflector maps g to b_0 e1 and whose later reflectors leave that
// direction fixed: T = Q^T H Q is tridiagonal (alphas, betas), g = b_0 Q e1, so
// SSCN's subproblem (reference cubic.py:40-75 as :352-398 calls it) becomes the
// one k_cubic_tridiag solves with gnorm = b_0 (signed: the solves are odd in
// it) and s = Q s_T.  One reduction serves every lam of every trial of a step.
//
// dlarfg's conventions (without its rescaling of tiny columns): for the column
// x below the diagonal, alpha = x[0] and xnorm = ||x[1:]||.  xnorm == 0 gives
// tau = 0 (the identity), b = alpha and v = e1; otherwise
// b = -sign(alpha) sqrt(alpha^2 + xnorm^2) (sign(0) = +), tau = (b - alpha) / b
// and v = (1, x[1:] / (alpha - b)).  No division happens on the tau = 0 branch:
// g = 0, a diagonal H and a decoupled block pass through it.
//
// Launch sequence (krcn_sytd.hip: sytd_reduce): k_sytd_fill, then one k_sytd_col per
// column j = 0 .. K - 3, then k_sytd_close.  No workgroup waits on another:
// the order of the launches in their stream is the only dependence.
//
//   k_sytd_col, launch j: one workgroup per kSytdR consecutive rows of the
//   trailing block (rows j + 1 .. K - 1).  Every workgroup runs the same
//   prologue on the same data in the same order, so all hold the same bits:
//   v_{j-1}, tau_{j-1}, p_{j-1} from the workspace; w = p - (tau / 2)(p.v) v;
//   row j of B with the pending update applied in LDS (row j lies outside the
//   new trailing block and is read by this launch alone); v_j, tau_j, b_j from
//   it and a_j from its diagonal.  Workgroup 0 stores them.  Then one wave per
//   row: B[i][c] -= v[i] w[c] + w[i] v[c] in place (the sum commutes, so B stays
//   symmetric to the bit) and p_j[i] = tau_j sum_c B[i][c] v_j[c].  p has two
//   buffers (j & 1): p_{j-1} is read while p_j is written.  Whole rows belong
//   to one wave: no partial sum crosses a wave's boundary, no atomics.
//
// Order of every sum: a wave's row sum takes columns c = j + 1 + lane, + 64, ..
// ascending per lane, then wave_sum's xor tree; the prologue's p.v and xnorm^2
// take c = j + tid, + 256, .. ascending per thread, then block_sum's tree; the
// back-transform's v.s is one product per thread, wave_sum, then the 16 wave
// sums pairwise.  The bits depend on k and the data alone.
//
// Every loop is bounded by K or kSytdR.
#pragma once
#include "krcn_cubic.hpp"

namespace krcn {

constexpr int kSytdMaxK = 1024;             // = KRCN_SSCN_TRIDIAG_MAX (krcn_sytd.hip static_asserts it)
constexpr int kSytdMaxOrder = kSytdMaxK + 1;   // K
constexpr int kSytdR = 4;                   // rows of the trailing block per workgroup: one per wave
constexpr int kSytdBackNT = 1024;           // the back-transform's workgroup: a thread per entry of s
static_assert(kSytdR % (kNT / 64) == 0, "a workgroup's waves share its rows evenly");
static_assert(kSytdBackNT >= kSytdMaxK, "the back-transform keeps s in registers, one entry a thread");

// Doubles per row of B and of the reflector workspace: K rounded up to a whole
// 64-byte line.
constexpr int64_t sytd_ld(int64_t k) { return (k + 1 + 7) / 8 * 8; }
// Column launches of a reduction.
constexpr int64_t sytd_launches(int64_t k) { return k >= 2 ? k - 1 : 0; }
// The workspace in doubles: B (K rows) | reflector rows (K) | p (2 rows) | tau |
// alphas | betas | g | s_T | the selection (3 k int32 in two rows).
constexpr int64_t sytd_ws_doubles(int64_t k) { return sytd_ld(k) * (2 * (k + 1) + 9); }

struct SytdWs {
  double *B, *V, *p, *tau, *al, *be, *g, *sT;
  int* cols;
  int K, ld;
};

inline SytdWs sytd_ws_of(double* base, int k) {
  const int64_t ld = sytd_ld(k), K = k + 1;
  SytdWs w;
  w.B = base;
  w.V = w.B + K * ld;
  w.p = w.V + K * ld;
  w.tau = w.p + 2 * ld;
  w.al = w.tau + ld;
  w.be = w.al + ld;
  w.g = w.be + ld;
  w.sT = w.g + ld;
  w.cols = reinterpret_cast<int*>(w.sT + ld);
  w.K = int(K);
  w.ld = int(ld);
  return w;
}

// B from the k x k block H (element (a, b), a <= b, at H[pm(a) * ldh + pm(b)],
// pm = perm or the identity: the triangle k_cubic_dense reads; l2 added on the
// diagonal) and g.  One workgroup per row of B.
[[maybe_unused]] static __global__ __launch_bounds__(kNT) void k_sytd_fill(int K, int ld,
                                                                          const double* __restrict__ H, int ldh,
                                                                          const int* __restrict__ perm, double l2,
                                                                          const double* __restrict__ g,
                                                                          double* __restrict__ B) {
  const int i = blockIdx.x;
  if (i >= K) return;
  const int pi = i == 0 ? 0 : (perm ? perm[i - 1] : i - 1);
  for (int c = threadIdx.x; c < K; c += kNT) {
    double v;
    if (i == 0) {
      v = c == 0 ? 0.0 : g[c - 1];
    } else if (c == 0) {
      v = g[i - 1];
    } else {
      const int pc = perm ? perm[c - 1] : c - 1;
      v = c >= i ? H[int64_t(pi) * ldh + pc] : H[int64_t(pc) * ldh + pi];
      if (c == i && l2 != 0.0) v = v + l2;
    }
    B[int64_t(i) * ld + c] = v;
  }
}

// The pending rank-2 update of reflector jp, for every thread of a kNT
// workgroup: vp[c] = v_jp[c] and w[c] = p[c] - (tau / 2)(p.v) v[c] for
// c = jp + 1 .. K - 1 (LDS, indexed by c); returns tau_jp.
__device__ __forceinline__ double sytd_pending(int jp, int K, int ld, const double* __restrict__ V,
                                               const double* __restrict__ tau, const double* __restrict__ p,
                                               double* vp, double* w, double* sm) {
  const double t = tau[jp];
  const double* vrow = V + int64_t(jp) * ld;
  const double* prow = p + int64_t(jp & 1) * ld;
  double acc = 0.0;
  for (int c = jp + 1 + threadIdx.x; c < K; c += kNT) {
    const double v = vrow[c], pc = prow[c];
    vp[c] = v;
    w[c] = pc;
    acc += pc * v;
  }
  const double pv = block_sum(acc, sm);   // (its barriers publish vp and w)
  const double half = t / 2.0 * pv;
  for (int c = jp + 1 + threadIdx.x; c < K; c += kNT) w[c] = w[c] - half * vp[c];
  __syncthreads();
  return t;
}

// B[i][c] with the pending update of the previous reflector applied.
__device__ __forceinline__ double sytd_upd(double b, double vi, double wi, double vc, double wc) {
  return b - (vi * wc + wi * vc);
}

[[maybe_unused]] static __global__ __launch_bounds__(kNT) void k_sytd_col(int j, int K, int ld,
                                                                         double* __restrict__ B,
                                                                         double* __restrict__ V,
                                                                         double* __restrict__ tau,
                                                                         double* __restrict__ p,
                                                                         double* __restrict__ al,
                                                                         double* __restrict__ be) {
  __shared__ double vp[kSytdMaxOrder], w[kSytdMaxOrder], vn[kSytdMaxOrder];
  __shared__ double sm[kNT / 64];
  const int tid = threadIdx.x;
  const bool pend = j > 0;
  if (pend) (void)sytd_pending(j - 1, K, ld, V, tau, p, vp, w, sm);
  // row j, columns j .. K - 1, into vn
  const double* rowj = B + int64_t(j) * ld;
  double acc = 0.0;
  for (int c = j + tid; c < K; c += kNT) {
    double x = rowj[c];
    if (pend) x = sytd_upd(x, vp[j], w[j], vp[c], w[c]);
    vn[c] = x;
    if (c >= j + 2) acc += x * x;
  }
  const double xn2 = block_sum(acc, sm);   // (its barriers publish vn)
  const double aj = vn[j], alpha = vn[j + 1];
  double t, b, scale;
  if (xn2 == 0.0) {
    t = 0.0;
    b = alpha;
    scale = 0.0;
  } else {
    const double r = sqrt(alpha * alpha + xn2);
    b = alpha >= 0.0 ? 0.0 - r : r;
    t = (b - alpha) / b;
    scale = 1.0 / (alpha - b);
  }
  __syncthreads();   // every thread has read vn[j] and vn[j + 1]
  for (int c = j + 1 + tid; c < K; c += kNT) {
    const double v = c == j + 1 ? 1.0 : (xn2 == 0.0 ? 0.0 : vn[c] * scale);
    vn[c] = v;
    if (blockIdx.x == 0) V[int64_t(j) * ld + c] = v;
  }
  if (blockIdx.x == 0 && tid == 0) {
    tau[j] = t;
    if (j > 0) al[j - 1] = aj;
    be[j] = b;
  }
  __syncthreads();
  // this workgroup's rows: the pending update in place, and p_j
  double* pout = p + int64_t(j & 1) * ld;
  const int lane = tid & 63, wave = tid >> 6;
  const int row0 = j + 1 + int(blockIdx.x) * kSytdR;
  for (int r = wave; r < kSytdR; r += kNT / 64) {
    const int i = row0 + r;   // (uniform over the wave)
    if (i >= K) break;
    double* row = B + int64_t(i) * ld;
    const double vi = pend ? vp[i] : 0.0, wi = pend ? w[i] : 0.0;
    double s = 0.0;
    for (int c = j + 1 + lane; c < K; c += 64) {
      double x = row[c];
      if (pend) {
        x = sytd_upd(x, vi, wi, vp[c], w[c]);
        row[c] = x;
      }
      s += x * vn[c];
    }
    s = wave_sum(s);
    if (lane == 0) pout[i] = t * s;
  }
}

// The last pending update on the final 2 x 2 block, and the last a's and b.
[[maybe_unused]] static __global__ __launch_bounds__(kNT) void k_sytd_close(int K, int ld,
                                                                           const double* __restrict__ B,
                                                                           const double* __restrict__ V,
                                                                           const double* __restrict__ tau,
                                                                           const double* __restrict__ p,
                                                                           double* __restrict__ al,
                                                                           double* __restrict__ be) {
  __shared__ double vp[kSytdMaxOrder], w[kSytdMaxOrder];
  __shared__ double sm[kNT / 64];
  const bool pend = K >= 3;
  if (pend) (void)sytd_pending(K - 3, K, ld, V, tau, p, vp, w, sm);
  if (threadIdx.x != 0) return;
  const int a = K - 2, b = K - 1;
  double daa = B[int64_t(a) * ld + a], dab = B[int64_t(a) * ld + b], dbb = B[int64_t(b) * ld + b];
  if (pend) {
    daa = sytd_upd(daa, vp[a], w[a], vp[a], w[a]);
    dab = sytd_upd(dab, vp[a], w[a], vp[b], w[b]);
    dbb = sytd_upd(dbb, vp[b], w[b], vp[b], w[b]);
  }
  if (a >= 1) al[a - 1] = daa;
  al[b - 1] = dbb;
  be[a] = dab;
}

// Start of the chain over the reduction: the subproblem's g is b_0 e1.
[[maybe_unused]] static __global__ void k_sytd_begin(int k, double M0, const double* __restrict__ be, CrnState* st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  CrnState s{};
  s.m_eff = k;
  s.M = M0;
  s.gnorm = be[0];
  *st = s;
}

// Sum over the kSytdBackNT threads, the same value in every thread: wave_sum,
// then the 16 wave sums pairwise.  sm holds kSytdBackNT / 64 doubles; the
// caller alternates two such buffers, so one barrier a call suffices.
__device__ __forceinline__ double sytd_back_sum(double v, double* sm) {
  constexpr int W = kSytdBackNT / 64;
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
  __syncthreads();
  double r[W];
#pragma unroll
  for (int i = 0; i < W; ++i) r[i] = sm[i];
#pragma unroll
  for (int h = W / 2; h > 0; h >>= 1)
#pragma unroll
    for (int i = 0; i < h; ++i) r[i] = r[2 * i] + r[2 * i + 1];
  return r[0];
}

// s = H_0 H_1 .. H_{K-3} s_T, reflectors applied last to first; thread t owns
// entry t of s (row t + 1 of B) in a register.  sT == nullptr: s_T is the unit
// vector e_{blockIdx.x} (the test path that forms Q, one workgroup a column).
// out + blockIdx.x * k receives s; with cols, xn[cols[a]] = x[cols[a]] + T(s_a)
// (the dense kernel's epilogue); with st, the launch is guarded by st->done and
// records ||s||^2 = ||s_T||^2 as the step length.
template <typename T>
__global__ __launch_bounds__(kSytdBackNT) void k_sytd_back(CrnState* st, int K, int ld,
                                                            const double* __restrict__ V,
                                                            const double* __restrict__ tau,
                                                            const double* __restrict__ sT, double* __restrict__ out,
                                                            const int* __restrict__ cols, const T* __restrict__ x,
                                                            T* __restrict__ xn, CrnState* res) {
  if (st && st->done) return;
  __shared__ double sm[2][kSytdBackNT / 64];
  const int tid = threadIdx.x, k = K - 1;
  const int c = tid + 1;   // this thread's row of B
  double s = 0.0;
  if (tid < k) s = sT ? sT[tid] : (tid == int(blockIdx.x) ? 1.0 : 0.0);
  int buf = 0;
  if (st) {
    const double n2 = sytd_back_sum(s * s, sm[buf]);
    buf ^= 1;
    if (tid == 0) {
      st->dx2 = n2;
      res->dx2 = n2;
    }
  }
  double v = 0.0;
  if (K >= 3 && c > K - 3 && c < K) v = V[int64_t(K - 3) * ld + c];
  for (int j = K - 3; j >= 0; --j) {
    double vnext = 0.0;
    if (j > 0 && c > j - 1 && c < K) vnext = V[int64_t(j - 1) * ld + c];
    const double t = tau[j];
    if (t != 0.0) {   // (uniform: tau = 0 is the identity)
      const double dot = sytd_back_sum(v * s, sm[buf]);
      buf ^= 1;
      s = s - t * dot * v;
    }
    v = vnext;
  }
  if (tid < k) {
    out[int64_t(blockIdx.x) * k + tid] = s;
    if (cols) {
      const int cc = cols[tid];
      xn[cc] = x[cc] + T(s);
    }
  }
}

}  // namespace krcn
