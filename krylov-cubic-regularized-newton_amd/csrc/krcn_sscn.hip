// krcn_sscn.hip — the dense cubic subproblem on the device (krcn_cubic_dense)
// and the Cholesky route of the one-call SSCN step (krcn_sscn_step): a trial's
// solve is k_cubic_dense, one factorisation of H + lam I per lam
// (krcn_cubic_dense.hpp).  The step itself and the entry point's checks are
// krcn_sscn_step.hpp's, shared with the tridiagonal route (krcn_sytd.hip).
#include "krcn_cubic_dense.hpp"
#include "krcn_sscn_step.hpp"

static_assert(kCdMax == KRCN_SSCN_MAX, "the dense kernel's LDS matrix holds the largest block");
static_assert(KRCN_SSCN_MAX <= KRCN_COORD_MAX, "the step runs the coordinate kernels");

namespace {

// The step's own device block: room for cols | sorted cols | permutation (k
// int32 each, packed: position a of the selection is sorted column ua[a]),
// then the gradient.
constexpr size_t kSscnInts = 3 * size_t(KRCN_SSCN_MAX);
constexpr size_t kSscnBytes = kSscnInts * sizeof(int32_t) + size_t(KRCN_SSCN_MAX) * sizeof(double);

struct CholeskyRoute {
  CrnRec rec;
  int* cols;   // cols[0..k) | ucols[0..k) | ua[0..k)
  double* g;
  const double* H;
  int k;

  krcn_status reserve(krcn_csr* h, int) {
    CHK(ensure_crn_ws(h));
    if (!h->sscn_ws) CHK(h->own.alloc(&h->sscn_ws, kSscnBytes));
    rec = crn_rec(h);
    cols = reinterpret_cast<int*>(h->sscn_ws);
    g = reinterpret_cast<double*>(h->sscn_ws + kSscnInts * sizeof(int32_t));
    return KRCN_OK;
  }

  // (the block is read through ua and l2 by every solve: nothing to prepare)
  krcn_status begin(const double* H_, int k_, const int*, double, double M0, hipStream_t s) {
    H = H_;
    k = k_;
    hipLaunchKernelGGL(k_crn_begin, dim3(1), dim3(kNT), 0, s, static_cast<const double*>(nullptr), 0, 0.0, M0, rec.st,
                       static_cast<double*>(nullptr), static_cast<double*>(nullptr));
    LAUNCHCHK();
    return KRCN_OK;
  }

  template <typename T>
  krcn_status solve(double* delta, const int* sel, const int* ua, const T* x, T* x_new, double l2, double r0,
                    double eps, int it_max, hipStream_t s) {
    hipLaunchKernelGGL((k_cubic_dense<T>), dim3(1), dim3(kNT), 0, s, rec.st, k, H, k, ua, l2,
                       static_cast<const double*>(g), delta, sel, x, x_new, r0, eps, it_max, rec.res);
    LAUNCHCHK();
    return KRCN_OK;
  }
};

}  // namespace

extern "C" krcn_status krcn_cubic_dense(krcn_csr* h, int k, const double* H_host, const double* g_host, double M,
                                        double r0, double eps, int it_max, double* s_host,
                                        krcn_crn_info* info_host, void* stream) {
  try {
    if (!h || !H_host || !g_host || !s_host || !info_host)
      return fail(KRCN_ERR_INVALID, "krcn_cubic_dense: null argument");
    if (k < 1 || k > KRCN_SSCN_MAX)
      return fail(KRCN_ERR_INVALID, "krcn_cubic_dense: k = %d outside [1, %d]", k, int(KRCN_SSCN_MAX));
    if (it_max < 1) return fail(KRCN_ERR_INVALID, "krcn_cubic_dense: it_max must be >= 1");
    CHK(set_device(h));
    hipStream_t s = S(stream);
    CholeskyRoute route;
    CHK(route.reserve(h, k));
    CHK(coord_reserve(h, k, s));
    CoordWs* w = h->cw;
    *info_host = krcn_crn_info{};
    // (pageable H2D copies are staged synchronously by the runtime: the host arrays may be reused)
    HIPCHK(hipMemcpyAsync(w->res, H_host, size_t(k) * size_t(k) * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(route.g, g_host, size_t(k) * sizeof(double), hipMemcpyHostToDevice, s));
    CHK(route.begin(w->res, k, nullptr, 0.0, M, s));
    CHK(route.solve<double>(w->delta, nullptr, nullptr, nullptr, nullptr, 0.0, r0, eps, it_max, s));
    return crn_read_solve(h, w->delta, k, s_host, info_host, s);
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_cubic_dense: unexpected C++ exception");
  }
}

extern "C" krcn_status krcn_sscn_step(krcn_csr* h, int k, const int32_t* cols_host, const void* x, const void* b,
                                      const void* Ax, double value, double l2, double reg_coef, double ls_beta,
                                      double r0, double solver_eps, int solver_it_max, int max_trials, void* x_new,
                                      void* Ax_new, krcn_crn_info* info_host, void* stream) {
  return sscn_step_entry<CholeskyRoute>("krcn_sscn_step", KRCN_SSCN_MAX, h, k, cols_host, x, b, Ax, value, l2,
                                        reg_coef, ls_beta, r0, solver_eps, solver_it_max, max_trials, x_new, Ax_new,
                                        info_host, stream);
}
