// krcn_sytd.hip — the dense cubic subproblem and SSCN's step for blocks up to
// KRCN_SSCN_TRIDIAG_MAX over one tridiagonal reduction per step
// (krcn_sytd.hpp): krcn_dense_tridiag (the reduction alone),
// krcn_cubic_dense_tridiag (krcn_cubic_dense's contract) and
// krcn_sscn_step_tridiag (krcn_sscn_step's): the tridiagonal route of the
// one-call SSCN step (krcn_sscn_step.hpp), whose trials are k_cubic_tridiag ->
// k_sytd_back -> the coordinate update of Ax -> the guards -> the judge over
// the chain state krcn_crn_step and krcn_sscn_step share.
// Replaces cubic_solver_root's dense and spsolve branches, cubic.py:40-75, and
// the body of SSCN.step, cubic.py:352-398, for subspace dimensions up to 1024.
#include "krcn_sytd.hpp"
#include "krcn_sscn_step.hpp"

static_assert(kSytdMaxK == KRCN_SSCN_TRIDIAG_MAX, "the reduction's LDS vectors hold the largest block");
static_assert(KRCN_SSCN_TRIDIAG_MAX == KRCN_COORD_MAX, "the step runs the coordinate kernels");
static_assert(KRCN_SSCN_TRIDIAG_MAX <= kCubicMaxM, "k_cubic_tridiag's LDS vectors hold the block");

namespace {

// The reduction's workspace for blocks of k columns (grown, never shrunk) and the chain state.
krcn_status sytd_reserve(krcn_csr* h, int k, SytdWs* ws, CrnRec* ch) {
  CHK(ensure_crn_ws(h));
  if (k > h->sytd_k) {
    CHK(h->own.release(&h->sytd_ws));
    h->sytd_k = 0;
    CHK(h->own.alloc(&h->sytd_ws, size_t(sytd_ws_doubles(k)) * sizeof(double)));
    h->sytd_k = k;
  }
  *ws = sytd_ws_of(h->sytd_ws, k);
  *ch = crn_rec(h);
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
krcn_status sytd_solve(const SytdWs& ws, const CrnRec& ch, double r0, double eps, int it_max, double* out,
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

struct TridiagRoute {
  SytdWs ws;
  CrnRec rec;
  int* cols;
  double* g;

  krcn_status reserve(krcn_csr* h, int k) {
    CHK(sytd_reserve(h, k, &ws, &rec));
    cols = ws.cols;
    g = ws.g;
    return KRCN_OK;
  }

  // the one reduction of the step: every trial and every lam of its solves reuses it
  krcn_status begin(const double* H, int k, const int* ua, double l2, double M0, hipStream_t s) {
    CHK(sytd_reduce(ws, H, k, ua, l2, s));
    hipLaunchKernelGGL(k_sytd_begin, dim3(1), dim3(64), 0, s, k, M0, static_cast<const double*>(ws.be), rec.st);
    LAUNCHCHK();
    return KRCN_OK;
  }

  template <typename T>
  krcn_status solve(double* delta, const int* sel, const int*, const T* x, T* x_new, double, double r0, double eps,
                    int it_max, hipStream_t s) {
    return sytd_solve<T>(ws, rec, r0, eps, it_max, delta, sel, x, x_new, s);
  }
};

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
    CrnRec ch;
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
    TridiagRoute route;
    CHK(route.reserve(h, k));
    CHK(coord_reserve(h, k, s));
    *info_host = krcn_crn_info{};
    CHK(stage_host_block(h, k, H_host, g_host, route.ws, s));
    CHK(route.begin(h->cw->res, k, nullptr, 0.0, M, s));
    CHK(route.solve<double>(h->cw->delta, nullptr, nullptr, nullptr, nullptr, 0.0, r0, eps, it_max, s));
    return crn_read_solve(h, h->cw->delta, k, s_host, info_host, s);
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_cubic_dense_tridiag: unexpected C++ exception");
  }
}

extern "C" krcn_status krcn_sscn_step_tridiag(krcn_csr* h, int k, const int32_t* cols_host, const void* x,
                                              const void* b, const void* Ax, double value, double l2, double reg_coef,
                                              double ls_beta, double r0, double solver_eps, int solver_it_max,
                                              int max_trials, void* x_new, void* Ax_new, krcn_crn_info* info_host,
                                              void* stream) {
  return sscn_step_entry<TridiagRoute>("krcn_sscn_step_tridiag", KRCN_SSCN_TRIDIAG_MAX, h, k, cols_host, x, b, Ax,
                                       value, l2, reg_coef, ls_beta, r0, solver_eps, solver_it_max, max_trials, x_new,
                                       Ax_new, info_host, stream);
}
