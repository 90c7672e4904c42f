// krcn_sytd.hip — the dense cubic subproblem and SSCN's step for blocks up to
// KRCN_SSCN_TRIDIAG_MAX over one tridiagonal reduction per step
// (krcn_sytd.hpp): krcn_dense_tridiag (the reduction alone),
// krcn_cubic_dense_tridiag (krcn_cubic_dense's contract) and
// krcn_sscn_step_tridiag (krcn_sscn_step's), whose trials are
// k_cubic_tridiag -> k_sytd_back -> the coordinate update of Ax -> the guards
// -> the judge over the chain state krcn_crn_step and krcn_sscn_step share.
// Replaces cubic_solver_root's dense and spsolve branches, cubic.py:40-75, and
// the body of SSCN.step, cubic.py:352-398, for subspace dimensions up to 1024.
#include "krcn_sytd.hpp"
#include "krcn_coord.hpp"
#include "krcn_coord_ws.hpp"

#include <cfloat>

static_assert(kSytdMaxK == KRCN_SSCN_TRIDIAG_MAX, "the reduction's LDS vectors hold the largest block");
static_assert(KRCN_SSCN_TRIDIAG_MAX == KRCN_COORD_MAX, "the step runs the coordinate kernels");
static_assert(KRCN_SSCN_TRIDIAG_MAX <= kCubicMaxM, "k_cubic_tridiag's LDS vectors hold the block");

namespace {

struct Chain {
  CrnState* st;
  CrnState* res;   // the mapped host record, by its device address
};

// The reduction's workspace for blocks of k columns (grown, never shrunk) and the chain state.
krcn_status sytd_reserve(krcn_csr* h, int k, SytdWs* ws, Chain* ch) {
  CHK(ensure_crn_ws(h));
  if (k > h->sytd_k) {
    CHK(h->own.release(&h->sytd_ws));
    h->sytd_k = 0;
    CHK(h->own.alloc(&h->sytd_ws, size_t(sytd_ws_doubles(k)) * sizeof(double)));
    h->sytd_k = k;
  }
  *ws = sytd_ws_of(h->sytd_ws, k);
  *ch = Chain{reinterpret_cast<CrnState*>(h->crn_ws), reinterpret_cast<CrnState*>(h->crn_res_dev)};
  return KRCN_OK;
}

// fill, the column launches, the closing kernel: alphas and betas of ws from the block H and ws.g
krcn_status sytd_reduce(const SytdWs& ws, const double* H, int ldh, const int* perm, double l2, hipStream_t s) {
  const int K = ws.K, ld = ws.ld;
  hipLaunchKernelGGL(k_sytd_fill, dim3(K), dim3(kNT), 0, s, K, ld, H, ldh, perm, l2, static_cast<const double*>(ws.g),
                     ws.B);
  LAUNCHCHK();
  for (int j = 0; j + 3 <= K; ++j) {
    const int rows = K - 1 - j;
    hipLaunchKernelGGL(k_sytd_col, dim3((rows + kSytdR - 1) / kSytdR), dim3(kNT), 0, s, j, K, ld, ws.B, ws.V, ws.tau,
                       ws.p, ws.al, ws.be);
    LAUNCHCHK();
  }
  hipLaunchKernelGGL(k_sytd_close, dim3(1), dim3(kNT), 0, s, K, ld, static_cast<const double*>(ws.B),
                     static_cast<const double*>(ws.V), static_cast<const double*>(ws.tau),
                     static_cast<const double*>(ws.p), ws.al, ws.be);
  LAUNCHCHK();
  return KRCN_OK;
}

// k_cubic_tridiag on the chain's M, then s = Q s_T into out (and x_new when cols is given)
template <typename T>
krcn_status sytd_solve(const SytdWs& ws, const Chain& ch, double r0, double eps, int it_max, double* out,
                       const int* cols, const T* x, T* x_new, hipStream_t s) {
  hipLaunchKernelGGL(k_cubic_tridiag, dim3(1), dim3(kNT), 0, s, ch.st, static_cast<const double*>(ws.al),
                     static_cast<const double*>(ws.be + 1), ws.sT, r0, eps, it_max, ch.res);
  LAUNCHCHK();
  hipLaunchKernelGGL((k_sytd_back<T>), dim3(1), dim3(kSytdBackNT), 0, s, ch.st, ws.K, ws.ld,
                     static_cast<const double*>(ws.V), static_cast<const double*>(ws.tau),
                     static_cast<const double*>(ws.sT), out, cols, x, x_new, ch.res);
  LAUNCHCHK();
  return KRCN_OK;
}

krcn_status check_block(const char* fn, const krcn_csr* h, int k) {
  if (!h) return fail(KRCN_ERR_INVALID, "%s: null handle", fn);
  if (k < 1 || k > KRCN_SSCN_TRIDIAG_MAX)
    return fail(KRCN_ERR_INVALID, "%s: k = %d outside [1, %d]", fn, k, int(KRCN_SSCN_TRIDIAG_MAX));
  return KRCN_OK;
}

// H and g of a host call into the coordinate workspace's result block and ws.g
krcn_status stage_host_block(krcn_csr* h, int k, const double* H_host, const double* g_host, const SytdWs& ws,
                             hipStream_t s) {
  // (pageable H2D copies are staged synchronously by the runtime: the host arrays may be reused)
  HIPCHK(hipMemcpyAsync(h->cw->res, H_host, size_t(k) * size_t(k) * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(ws.g, g_host, size_t(k) * sizeof(double), hipMemcpyHostToDevice, s));
  return KRCN_OK;
}

struct StepArgs {
  double value, l2, reg_coef, ls_beta, r0, solver_eps;
  int k, solver_it_max, max_trials;
};

template <typename T>
krcn_status step_impl(krcn_csr* h, const int32_t* sel, const T* x, const T* b, const T* Ax, const StepArgs& a,
                      T* x_new, T* Ax_new, krcn_crn_info* info, hipStream_t s) {
  const int k = a.k;
  const int64_t n = h->n, d = h->d;
  const bool empty = coord_empty(h);
  if (!Ax && n) {
    // X x into the n-vector scratch (unsharded handles leave it free).  The plans come first: a
    // plan build's placement probe may move tn, pa and pb, so none of them is read before it.
    CHK(plans_for_compute(h));
    T* tn = static_cast<T*>(h->tn);
    CHK(krcn_matvec(h, x, tn, s));
    Ax = tn;
  }
  SytdWs ws;
  Chain ch;
  CHK(sytd_reserve(h, k, &ws, &ch));
  CHK(coord_reserve(h, k, s));
  CoordWs* w = h->cw;
  // the selection as given, ascending (the Hessian kernel's order) and the map between them: one staged copy
  static_assert(3 * sizeof(int32_t) <= kCoordSlotPerCol, "the three staged int32 arrays fit a ring slot");
  CHK(coord_stage_bytes(h, sel, size_t(3 * k) * sizeof(int32_t), ws.cols, s));
  const int* cols = ws.cols;
  const int* ucols = ws.cols + k;
  const int* ua = ws.cols + 2 * k;
  if (empty) {
    hipLaunchKernelGGL((k_coord_l2x<T>), dim3((k + kNT - 1) / kNT), dim3(kNT), 0, s, k, cols, x, a.l2, ws.g);
    LAUNCHCHK();
    HIPCHK(hipMemsetAsync(w->res, 0, size_t(k) * size_t(k) * sizeof(double), s));
    if (n) HIPCHK(hipMemcpyAsync(Ax_new, Ax, size_t(n) * sizeof(T), hipMemcpyDeviceToDevice, s));
  } else {
    hipLaunchKernelGGL((k_coord_grad<T>), dim3(k), dim3(kCoordGradNT), 0, s, cols, h->tptr, h->tidx,
                       static_cast<const T*>(h->tval), Ax, b, x, double(h->n_global), a.l2, int(a.l2 != 0.0), ws.g);
    LAUNCHCHK();
    const int R = h->coord_window ? std::min(h->coord_window, kCoordWinMax) : kCoordWinMax;
    hipLaunchKernelGGL((k_coord_hess<T>), dim3(k), dim3(kCoordHessNT), 0, s, int(n), R, k, ucols, h->tptr, h->tidx,
                       static_cast<const T*>(h->tval), Ax, double(h->n_global), w->res);
    LAUNCHCHK();
  }
  // the one reduction of the step: every trial and every lam of its solves reuses it
  CHK(sytd_reduce(ws, w->res, k, ua, a.l2, s));
  HIPCHK(hipMemcpyAsync(x_new, x, size_t(d) * sizeof(T), hipMemcpyDeviceToDevice, s));
  hipLaunchKernelGGL(k_sytd_begin, dim3(1), dim3(64), 0, s, k, std::max(a.reg_coef * a.ls_beta, DBL_EPSILON),
                     static_cast<const double*>(ws.be), ch.st);   // cubic.py:366
  LAUNCHCHK();

  const int Pn = vec_grid(n), Pd = vec_grid(d);
  // (n == 0: no loss terms, the judge's mean is 0 / 1 and the value the l2 term alone)
  const double n_mean = h->n_global > 0 ? double(h->n_global) : 1.0;
  const int Rw = h->coord_window ? std::min(h->coord_window, kCoordUpdMax) : kCoordUpdAuto;
  const int64_t waves = (n + Rw - 1) / Rw;
  const int ugrid = int((waves + kCoordUpdWaves - 1) / kCoordUpdWaves);
  const size_t ulds = size_t(kCoordUpdWaves) * (size_t(Rw) + size_t(k)) * sizeof(double);   // <= 64 KiB
  auto trial = [&]() -> krcn_status {
    CHK(sytd_solve<T>(ws, ch, a.r0, a.solver_eps, a.solver_it_max, w->delta, cols, x, x_new, s));
    if (!empty) {
      hipLaunchKernelGGL((k_coord_update<T, true>), dim3(ugrid), dim3(kCoordUpdNT), ulds, s, int(n), Rw, k, cols,
                         static_cast<const double*>(w->delta), h->tptr, h->tidx, static_cast<const T*>(h->tval), Ax,
                         Ax_new, static_cast<const int*>(&ch.st->done));
      LAUNCHCHK();
    }
    hipLaunchKernelGGL((k_loss_terms_guard<T>), dim3(Pn), dim3(kNT), 0, s, n, static_cast<const T*>(Ax_new), b, h->pa,
                       static_cast<const CrnState*>(ch.st));
    LAUNCHCHK();
    if (a.l2 != 0.0) {
      hipLaunchKernelGGL((k_sqnorm_guard<T>), dim3(Pd), dim3(kNT), 0, s, d, static_cast<const T*>(x_new),
                         static_cast<const T*>(nullptr), h->pb, static_cast<const CrnState*>(ch.st), 0);
      LAUNCHCHK();
    }
    hipLaunchKernelGGL(k_crn_judge, dim3(1), dim3(kNT), 0, s, static_cast<const double*>(h->pa), Pn,
                       static_cast<const double*>(h->pb), Pd, n_mean, a.l2, a.value, a.ls_beta, a.max_trials, ch.st,
                       ch.res);
    LAUNCHCHK();
    return KRCN_OK;
  };
  CrnState st{};
  const int total = a.max_trials + 1;   // the trial after max_trials rejections ends the chain itself
  for (int enq = 0; enq < total && !st.done;) {
    const int batch = std::min(enq == 0 ? kCrnFirstBatch : kCrnBatch, total - enq);
    for (int t = 0; t < batch; ++t) CHK(trial());
    enq += batch;
    HIPCHK(hipStreamSynchronize(s));
    std::memcpy(&st, h->crn_res, sizeof(CrnState));
  }
  if (!st.done) return fail(KRCN_ERR_HIP, "krcn_sscn_step_tridiag: the trial chain did not end after %d trials", total);
  crn_solver_fields(st, info);
  info->accepted = st.accepted;
  info->trials = st.trials;
  info->value_new = st.value_new;
  const bool failed = st.solver_status == kCubicNotPd || st.solver_status == kCubicDerZero;
  info->dx_norm = failed ? 0.0 : std::sqrt(st.dx2);
  return KRCN_OK;
}

}  // namespace

extern "C" krcn_status krcn_dense_tridiag_geometry(int k, int64_t* launches_host, int64_t* workspace_bytes_host) {
  if (!launches_host || !workspace_bytes_host)
    return fail(KRCN_ERR_INVALID, "krcn_dense_tridiag_geometry: null argument");
  if (k < 1 || k > KRCN_SSCN_TRIDIAG_MAX)
    return fail(KRCN_ERR_INVALID, "krcn_dense_tridiag_geometry: k = %d outside [1, %d]", k,
                int(KRCN_SSCN_TRIDIAG_MAX));
  *launches_host = sytd_launches(k);
  *workspace_bytes_host = sytd_ws_doubles(k) * int64_t(sizeof(double));
  return KRCN_OK;
}

extern "C" krcn_status krcn_dense_tridiag(krcn_csr* h, int k, const double* H_host, const double* g_host,
                                          double* alphas_host, double* betas_host, double* Q_host, void* stream) {
  try {
    CHK(check_block("krcn_dense_tridiag", h, k));
    if (!H_host || !g_host || !alphas_host || !betas_host)
      return fail(KRCN_ERR_INVALID, "krcn_dense_tridiag: null argument");
    CHK(set_device(h));
    hipStream_t s = S(stream);
    SytdWs ws;
    Chain ch;
    CHK(sytd_reserve(h, k, &ws, &ch));
    CHK(coord_reserve(h, k, s));
    CHK(stage_host_block(h, k, H_host, g_host, ws, s));
    CHK(sytd_reduce(ws, h->cw->res, k, nullptr, 0.0, s));
    HIPCHK(hipMemcpyAsync(h->hostbuf, ws.al, size_t(k) * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h->hostbuf + k, ws.be, size_t(k) * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::memcpy(alphas_host, h->hostbuf, size_t(k) * sizeof(double));
    std::memcpy(betas_host, h->hostbuf + k, size_t(k) * sizeof(double));
    if (Q_host) {
      // column m of Q is the back-transform of e_m, one workgroup each, into B (free once reduced):
      // row m of the device block is column m of Q
      hipLaunchKernelGGL((k_sytd_back<double>), dim3(k), dim3(kSytdBackNT), 0, s, static_cast<CrnState*>(nullptr),
                         ws.K, ws.ld, static_cast<const double*>(ws.V), static_cast<const double*>(ws.tau),
                         static_cast<const double*>(nullptr), ws.B, static_cast<const int*>(nullptr),
                         static_cast<const double*>(nullptr), static_cast<double*>(nullptr),
                         static_cast<CrnState*>(nullptr));
      LAUNCHCHK();
      std::vector<double> qt(size_t(k) * size_t(k));
      HIPCHK(hipMemcpyAsync(qt.data(), ws.B, qt.size() * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      for (int m = 0; m < k; ++m)
        for (int a = 0; a < k; ++a) Q_host[size_t(a) * size_t(k) + size_t(m)] = qt[size_t(m) * size_t(k) + size_t(a)];
    }
    return KRCN_OK;
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_dense_tridiag: unexpected C++ exception");
  }
}

extern "C" krcn_status krcn_cubic_dense_tridiag(krcn_csr* h, int k, const double* H_host, const double* g_host,
                                                double M, double r0, double eps, int it_max, double* s_host,
                                                krcn_crn_info* info_host, void* stream) {
  try {
    CHK(check_block("krcn_cubic_dense_tridiag", h, k));
    if (!H_host || !g_host || !s_host || !info_host)
      return fail(KRCN_ERR_INVALID, "krcn_cubic_dense_tridiag: null argument");
    if (it_max < 1) return fail(KRCN_ERR_INVALID, "krcn_cubic_dense_tridiag: it_max must be >= 1");
    CHK(set_device(h));
    hipStream_t s = S(stream);
    SytdWs ws;
    Chain ch;
    CHK(sytd_reserve(h, k, &ws, &ch));
    CHK(coord_reserve(h, k, s));
    *info_host = krcn_crn_info{};
    CHK(stage_host_block(h, k, H_host, g_host, ws, s));
    CHK(sytd_reduce(ws, h->cw->res, k, nullptr, 0.0, s));
    hipLaunchKernelGGL(k_sytd_begin, dim3(1), dim3(64), 0, s, k, M, static_cast<const double*>(ws.be), ch.st);
    LAUNCHCHK();
    CHK(sytd_solve<double>(ws, ch, r0, eps, it_max, h->cw->delta, nullptr, nullptr, nullptr, s));
    HIPCHK(hipMemcpyAsync(h->hostbuf, h->cw->delta, size_t(k) * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    CrnState st;
    std::memcpy(&st, h->crn_res, sizeof(CrnState));
    crn_solver_fields(st, info_host);
    const bool solved = st.solver_status == kCubicOk || st.solver_status == kCubicItMax;
    for (int i = 0; i < k; ++i) s_host[i] = solved ? h->hostbuf[i] : 0.0;
    return KRCN_OK;
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_cubic_dense_tridiag: unexpected C++ exception");
  }
}

extern "C" krcn_status krcn_sscn_step_tridiag(krcn_csr* h, int k, const int32_t* cols_host, const void* x,
                                              const void* b, const void* Ax, double value, double l2, double reg_coef,
                                              double ls_beta, double r0, double solver_eps, int solver_it_max,
                                              int max_trials, void* x_new, void* Ax_new, krcn_crn_info* info_host,
                                              void* stream) {
  try {
    if (!h) return fail(KRCN_ERR_INVALID, "krcn_sscn_step_tridiag: null handle");
    if (h->shard != KRCN_SHARD_NONE)
      return fail(KRCN_ERR_UNSUPPORTED, "krcn_sscn_step_tridiag: sharded handles are not supported");
    CHK(check_block("krcn_sscn_step_tridiag", h, k));
    if (!cols_host || !x || !x_new || !info_host || (h->n && (!b || !Ax_new)))
      return fail(KRCN_ERR_INVALID, "krcn_sscn_step_tridiag: null argument");
    if (max_trials < 0) return fail(KRCN_ERR_INVALID, "krcn_sscn_step_tridiag: max_trials must be >= 0");
    if (!(ls_beta > 0.0 && ls_beta < 1.0))
      return fail(KRCN_ERR_INVALID, "krcn_sscn_step_tridiag: ls_beta must lie in (0, 1)");
    if (solver_it_max < 1) return fail(KRCN_ERR_INVALID, "krcn_sscn_step_tridiag: solver_it_max must be >= 1");
    if (x_new == x || (Ax_new && (Ax_new == Ax || Ax_new == b)))
      return fail(KRCN_ERR_INVALID, "krcn_sscn_step_tridiag: x_new and Ax_new must not alias the inputs");
    for (int a = 0; a < k; ++a)
      if (cols_host[a] < 0 || int64_t(cols_host[a]) >= h->d)
        return fail(KRCN_ERR_INVALID, "krcn_sscn_step_tridiag: cols_host[%d] = %d outside [0, %lld)", a,
                    int(cols_host[a]), (long long)h->d);
    // cols | sorted cols | permutation, as the step stages them
    std::vector<int32_t> sel(size_t(3 * k));
    std::copy(cols_host, cols_host + k, sel.begin());
    std::vector<int> order(size_t(k), 0);
    for (int a = 0; a < k; ++a) order[size_t(a)] = a;
    std::sort(order.begin(), order.end(), [&](int p, int q) {
      return cols_host[p] != cols_host[q] ? cols_host[p] < cols_host[q] : p < q;
    });
    for (int r = 0; r < k; ++r) {
      const int a = order[size_t(r)];
      if (r > 0 && cols_host[a] == cols_host[order[size_t(r - 1)]])
        return fail(KRCN_ERR_INVALID,
                    "krcn_sscn_step_tridiag: cols_host[%d] = %d repeats cols_host[%d] (indices must be distinct)", a,
                    int(cols_host[a]), order[size_t(r - 1)]);
      sel[size_t(k + r)] = cols_host[a];
      sel[size_t(2 * k + a)] = r;
    }
    CHK(set_device(h));
    *info_host = krcn_crn_info{};
    const StepArgs args{value, l2, reg_coef, ls_beta, r0, solver_eps, k, solver_it_max, max_trials};
    return h->dtype == KRCN_F64
               ? step_impl<double>(h, sel.data(), static_cast<const double*>(x), static_cast<const double*>(b),
                                   static_cast<const double*>(Ax), args, static_cast<double*>(x_new),
                                   static_cast<double*>(Ax_new), info_host, S(stream))
               : step_impl<float>(h, sel.data(), static_cast<const float*>(x), static_cast<const float*>(b),
                                  static_cast<const float*>(Ax), args, static_cast<float*>(x_new),
                                  static_cast<float*>(Ax_new), info_host, S(stream));
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_sscn_step_tridiag: unexpected C++ exception");
  }
}
