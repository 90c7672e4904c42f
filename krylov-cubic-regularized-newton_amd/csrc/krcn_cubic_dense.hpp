// krcn_cubic_dense.hpp — the cubic subproblem over a dense symmetric k x k
// block in one workgroup: argmin_s <g,s> + 1/2 s^T H s + M/3 ||s||^3 for a
// general g, 1 <= k <= KRCN_SSCN_MAX (reference cubic.py:40-75, the dense branch
// of cubic_solver_root; SSCN's subproblem, cubic.py:352-398).  fp64 whatever
// the handle's dtype.
//
// The Newton loop is cubic_newton (krcn_cubic.hpp), shared with the
// tridiagonal kernels; this header supplies the linear algebra per lam:
//
//   fill     the upper triangle of H is read from global memory (mirrored; through
//            the selection's permutation, l2 then lam added on the diagonal)
//            into the LDS matrix, and g into the row below it (row k).
//   factor   an in-place left-looking Cholesky H + lam I = L L^T over the k + 1
//            rows: column j of row i is (A[i][j] - sum_{p<j} L[i][p] L[j][p]) /
//            L[j][j], so row k becomes L^{-1} g — the forward substitution of
//            the first solve costs nothing extra.  Rows are dealt cyclically to
//            kCdRows = 64 groups of kCdLpr = 4 adjacent lanes (row i to
//            group i mod 64: the rows below column j stay spread over all
//            groups); a group's lanes take p = q, q + 4, .. of the sum and add
//            their parts in a fixed xor tree.  Two barriers per column: the
//            pivot's publication and the column's stores.  A pivot <= 0 or
//            non-finite ends the solve (status 1: the host's LinAlgError from
//            solve(assume_a='pos')).
//   sweeps   the triangular solves run on wave 0 alone with the vector in
//            registers (lane l owns entries l and l + 64): element j is
//            broadcast by a lane read, so the dependent chain per step is
//            read-lane, divide, multiply, subtract, with no LDS round trip and
//            no barrier; the L entries of a step do not depend on the chain.
//            y = L^{-T} (row k); z = L^{-T} L^{-1} y.
//   sums     block_sum's fixed-order tree.
//
// LDS: the matrix is a padded square, (k_max + 1) rows of kCdLd = 129
// doubles (133,128 bytes; only the lower triangle is ever read), plus g, y, z
// and the permutation: about 137 KiB of the 160.  The odd stride keeps both the
// row walks of the factorisation and the column walk of the forward sweep off
// a common bank; a packed triangle would halve the footprint but index every
// element through a multiply-add, and nothing else needs the space.
// Every loop is bounded by it_max or k; no other workgroup is waited on.
#pragma once
#include "krcn_cubic.hpp"

namespace krcn {

constexpr int kCdMax = 128;              // = KRCN_SSCN_MAX (krcn_sscn.hip static_asserts it)
constexpr int kCdLd = kCdMax + 1;     // doubles per LDS row
constexpr int kCdRows = 64;              // row groups
constexpr int kCdLpr = kNT / kCdRows; // lanes per row group
constexpr int kCdSlots = (kCdMax + 1 + kCdRows - 1) / kCdRows;   // rows a group owns at most (3)
constexpr int kCdU = 4;                  // steps of a row's sum whose operands are loaded together
static_assert(kCdLpr == 4, "a row group is one DPP quad");
static_assert(kNT % kCdMax == 0, "the fill deals whole rows to the block");

// Lane `lane` 's copy of v, the same in every lane of the wave (lane is uniform).
__device__ __forceinline__ double dense_read_lane(double v, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
  return __hiloint2double(hi, lo);
}

// v of the lane whose index inside its quad is this lane's, permuted by the DPP
// quad_perm kCtrl (0xB1: lane ^ 1, 0x4E: lane ^ 2): a row group is one quad.
template <int kCtrl>
__device__ __forceinline__ double dense_quad_xor(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), kCtrl, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), kCtrl, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

// s[r] = sum over p = q, q + 4, .. < j of rows[r][p] * Lj[p], ascending p, for R
// rows at once: the operands of kCdU steps are loaded first (independent LDS
// loads), then the R dependent chains of adds run register to register.
template <int R>
__device__ __forceinline__ void dense_row_sums(const double* Lj, const double* const (&rows)[R], int q, int j,
                                               double (&s)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) s[r] = 0.0;
  int p = q;
  for (; p + (kCdU - 1) * kCdLpr < j; p += kCdU * kCdLpr) {
    double lj[kCdU], lr[R][kCdU];
#pragma unroll
    for (int e = 0; e < kCdU; ++e) {
      lj[e] = Lj[p + e * kCdLpr];
#pragma unroll
      for (int r = 0; r < R; ++r) lr[r][e] = rows[r][p + e * kCdLpr];
    }
#pragma unroll
    for (int e = 0; e < kCdU; ++e)
#pragma unroll
      for (int r = 0; r < R; ++r) s[r] += lr[r][e] * lj[e];
  }
  for (; p < j; p += kCdLpr) {
    const double l = Lj[p];
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] += rows[r][p] * l;
  }
}

// Every thread of the workgroup calls this with the same arguments and gets
// the same result.  H: the upper triangle (column >= row) of the ldh-strided
// matrix is read — the triangle scipy's solve(assume_a='pos') hands LAPACK —,
// element (a, b) at H[pm(a) * ldh + pm(b)] with pm = perm or the identity
// (perm == nullptr).  On success s_g receives s and, when cols is
// given, xn[cols[a]] = x[cols[a]] + T(s[a]).
template <typename T>
__device__ __forceinline__ CubicSolve cubic_dense_solve(int k, double M, const double* __restrict__ H, int ldh,
                                                        const int* __restrict__ perm, double l2,
                                                        const double* __restrict__ g_g, double* __restrict__ s_g,
                                                        const int* __restrict__ cols, const T* __restrict__ x,
                                                        T* __restrict__ xn, double r0, double eps, int it_max) {
  __shared__ double Ls[(kCdMax + 1) * kCdLd];
  __shared__ double g[kCdMax], y[kCdMax], z[kCdMax];
  __shared__ int pm[kCdMax];
  __shared__ double sm[kNT / 64];
  __shared__ double piv_sm;
  const int tid = threadIdx.x;
  const int grp = tid / kCdLpr, q = tid % kCdLpr;
  for (int i = tid; i < k; i += kNT) {
    g[i] = g_g[i];
    pm[i] = perm ? perm[i] : i;
  }
  __syncthreads();

  // H + lam I = L L^T in place, row k = L^{-1} g; false: not positive definite
  auto factor = [&](double lam) -> bool {
    {
      // thread t fills row i = t mod 128 of the LDS triangle, every other column from t / 128:
      // adjacent threads read adjacent entries of a row of H (A[i][j] = H[j][i], i >= j)
      const int i = tid % kCdMax;
      if (i < k) {
        const int pi = pm[i];
        for (int j = tid / kCdMax; j <= i; j += kNT / kCdMax) {
          double v = H[int64_t(pm[j]) * ldh + pi];
          if (i == j) {
            if (l2 != 0.0) v = v + l2;
            v = v + lam;
          }
          Ls[i * kCdLd + j] = v;
        }
      }
    }
    for (int j = tid; j < k; j += kNT) Ls[k * kCdLd + j] = g[j];
    __syncthreads();
    for (int j = 0; j < k; ++j) {
      const double* Lj = Ls + j * kCdLd;
      // The sums of this thread's rows over its share p = q, q + 4, .. of column j's
      // predecessors, each in ascending p (dense_row_sums).  Rows grp and grp + 64
      // run together.  A row that is not
      // active (above column j, or past row k) reads row j instead and its sum is
      // dropped.  Row grp + 128 exists for k = 128 alone (the row of g, group 0).
      bool act[kCdSlots];
      double t[kCdSlots];
#pragma unroll
      for (int u = 0; u < kCdSlots; ++u) {
        const int i = grp + kCdRows * u;
        act[u] = i >= j && i <= k;
        t[u] = 0.0;
      }
      {
        const double* rows[2] = {Ls + (act[0] ? grp : j) * kCdLd, Ls + (act[1] ? grp + kCdRows : j) * kCdLd};
        double sums[2];
        dense_row_sums<2>(Lj, rows, q, j, sums);
        t[0] = sums[0];
        t[1] = sums[1];
      }
      if (act[2]) {
        const double* rows[1] = {Ls + (grp + 2 * kCdRows) * kCdLd};
        double sums[1];
        dense_row_sums<1>(Lj, rows, q, j, sums);
        t[2] = sums[0];
      }
#pragma unroll
      for (int u = 0; u < kCdSlots; ++u) {
        const int i = grp + kCdRows * u;
        double acc = t[u];
        acc += dense_quad_xor<0xB1>(acc);   // lane ^ 1
        acc += dense_quad_xor<0x4E>(acc);   // lane ^ 2
        t[u] = act[u] ? Ls[i * kCdLd + j] - acc : 0.0;
        if (i == j && q == 0) piv_sm = t[u];
      }
      __syncthreads();
      const double piv = piv_sm;
      if (!(piv > 0.0) || isinf(piv)) return false;   // (the same value in every thread)
      const double dj = sqrt(piv);
      if (q == 0) {
#pragma unroll
        for (int u = 0; u < kCdSlots; ++u) {
          const int i = grp + kCdRows * u;
          if (i == j) Ls[i * kCdLd + j] = dj;
          else if (i > j && i <= k) Ls[i * kCdLd + j] = t[u] / dj;
        }
      }
      __syncthreads();
    }
    return true;
  };
  // wave 0: out = L^{-T} in (forward: L^{-T} L^{-1} in); in may be out
  auto sweeps = [&](const double* in, double* out, bool forward) {
    if (tid < 64) {
      const int l0 = tid, l1 = tid + 64;
      double v0 = l0 < k ? in[l0] : 0.0, v1 = l1 < k ? in[l1] : 0.0;
      if (forward) {
        for (int j = 0; j < k; ++j) {
          const double a0 = l0 > j && l0 < k ? Ls[l0 * kCdLd + j] : 0.0;
          const double a1 = l1 > j && l1 < k ? Ls[l1 * kCdLd + j] : 0.0;
          const double vj = dense_read_lane(j < 64 ? v0 : v1, j & 63) / Ls[j * kCdLd + j];
          if (l0 == j) v0 = vj;
          if (l1 == j) v1 = vj;
          if (l0 > j) v0 = v0 - a0 * vj;
          if (l1 > j) v1 = v1 - a1 * vj;
        }
      }
      for (int j = k - 1; j >= 0; --j) {
        const double* Lj = Ls + j * kCdLd;
        const double a0 = l0 < j ? Lj[l0] : 0.0;
        const double a1 = l1 < j ? Lj[l1] : 0.0;
        const double vj = dense_read_lane(j < 64 ? v0 : v1, j & 63) / Lj[j];
        if (l0 == j) v0 = vj;
        if (l1 == j) v1 = vj;
        if (l0 < j) v0 = v0 - a0 * vj;
        if (l1 < j) v1 = v1 - a1 * vj;
      }
      if (l0 < k) out[l0] = v0;
      if (l1 < k) out[l1] = v1;
    }
    __syncthreads();
  };
  auto solve_g = [&](double lam) -> bool {
    if (!factor(lam)) return false;
    sweeps(Ls + k * kCdLd, y, false);
    return true;
  };
  auto solve_y = [&]() { sweeps(y, z, true); };
  auto dot = [&](const double* a, const double* b) -> double {
    double acc = 0.0;
    for (int i = tid; i < k; i += kNT) acc += a[i] * b[i];
    return block_sum(acc, sm);
  };

  return cubic_newton(
      M, r0, eps, it_max, solve_g, solve_y, [&]() { return dot(y, y); }, [&]() { return dot(y, z); },
      [&]() { return 0.0 - dot(g, y); },   // np.dot(g, s), s = -y
      [&]() {
        for (int i = tid; i < k; i += kNT) {
          const double si = 0.0 - y[i];
          s_g[i] = si;
          if (cols) {
            const int c = cols[i];
            xn[c] = x[c] + T(si);
          }
        }
      });
}

// One solve of the chain on its state's M (k_cubic_tridiag's contract): the
// solver fields and ||s||^2 go to the state and the mapped record, a failed
// solve ends the chain.
template <typename T>
__global__ __launch_bounds__(kNT) void k_cubic_dense(CrnState* st, int k, const double* __restrict__ H, int ldh,
                                                     const int* __restrict__ perm, double l2,
                                                     const double* __restrict__ g_g, double* __restrict__ s_g,
                                                     const int* __restrict__ cols, const T* __restrict__ x,
                                                     T* __restrict__ xn, double r0, double eps, int it_max,
                                                     CrnState* res) {
  if (st->done) return;
  const CubicSolve r = cubic_dense_solve<T>(k, st->M, H, ldh, perm, l2, g_g, s_g, cols, x, xn, r0, eps, it_max);
  if (threadIdx.x == 0) {
    st->solver_it = r.its;
    st->solver_status = r.status;
    st->lam = r.root;
    st->model_decrease = r.dec;
    st->dx2 = r.ns * r.ns;
    if (r.status == kCubicNotPd || r.status == kCubicDerZero) st->done = 1;   // nothing to try: the chain ends here
    *res = *st;
  }
}

}  // namespace krcn
