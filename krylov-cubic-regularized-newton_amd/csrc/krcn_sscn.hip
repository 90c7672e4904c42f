// krcn_sscn.hip — the dense cubic subproblem on the device (krcn_cubic_dense)
// and one SSCN step behind one call (krcn_sscn_step): the coordinate gradient
// and Hessian block stay on the device, then a chain of guarded backtracking
// trials — dense solve, coordinate update of Ax, loss terms, norm, judge —
// whose accept / reject decision is taken on the device (krcn_cubic_dense.hpp,
// krcn_cubic.hpp, krcn_coord.hpp).  Replaces the host loop of SSCN.step,
// optimizer/cubic.py (reference cubic.py:352-398).
#include "krcn_cubic_dense.hpp"
#include "krcn_coord.hpp"
#include "krcn_coord_ws.hpp"

#include <cfloat>

static_assert(kCdMax == KRCN_SSCN_MAX, "the dense kernel's LDS matrix holds the largest block");
static_assert(KRCN_SSCN_MAX <= KRCN_COORD_MAX, "the step runs the coordinate kernels");

namespace {

// The step's own device block: room for cols | sorted cols | permutation (k
// int32 each, packed: position a of the selection is sorted column ua[a]),
// then the gradient.
constexpr size_t kSscnInts = 3 * size_t(KRCN_SSCN_MAX);
constexpr size_t kSscnBytes = kSscnInts * sizeof(int32_t) + size_t(KRCN_SSCN_MAX) * sizeof(double);

struct SscnWs {
  CrnState* st;
  CrnState* res;   // the mapped host record, by its device address
  int* cols;       // cols[0..k) | ucols[0..k) | ua[0..k)
  double* g;
};

krcn_status sscn_ws(krcn_csr* h, SscnWs* ws) {
  CHK(ensure_crn_ws(h));
  if (!h->sscn_ws) CHK(h->own.alloc(&h->sscn_ws, kSscnBytes));
  int* ints = reinterpret_cast<int*>(h->sscn_ws);
  *ws = SscnWs{reinterpret_cast<CrnState*>(h->crn_ws), reinterpret_cast<CrnState*>(h->crn_res_dev), ints,
               reinterpret_cast<double*>(h->sscn_ws + kSscnInts * sizeof(int32_t))};
  return KRCN_OK;
}

krcn_status begin_chain(const SscnWs& ws, double M0, hipStream_t s) {
  hipLaunchKernelGGL(k_crn_begin, dim3(1), dim3(kNT), 0, s, static_cast<const double*>(nullptr), 0, 0.0, M0, ws.st,
                     static_cast<double*>(nullptr), static_cast<double*>(nullptr));
  LAUNCHCHK();
  return KRCN_OK;
}

struct StepArgs {
  double value, l2, reg_coef, ls_beta, r0, solver_eps;
  int k, solver_it_max, max_trials;
};

template <typename T>
krcn_status sscn_step_impl(krcn_csr* h, const int32_t* sel, const T* x, const T* b, const T* Ax, const StepArgs& a,
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
  SscnWs ws;
  CHK(sscn_ws(h, &ws));
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
  HIPCHK(hipMemcpyAsync(x_new, x, size_t(d) * sizeof(T), hipMemcpyDeviceToDevice, s));
  CHK(begin_chain(ws, std::max(a.reg_coef * a.ls_beta, DBL_EPSILON), s));   // cubic.py:366

  const int Pn = vec_grid(n), Pd = vec_grid(d);
  // (n == 0: no loss terms, the judge's mean is 0 / 1 and the value the l2 term alone)
  const double n_mean = h->n_global > 0 ? double(h->n_global) : 1.0;
  const int Rw = h->coord_window ? std::min(h->coord_window, kCoordUpdMax) : kCoordUpdAuto;
  const int64_t waves = (n + Rw - 1) / Rw;
  const int ugrid = int((waves + kCoordUpdWaves - 1) / kCoordUpdWaves);
  const size_t ulds = size_t(kCoordUpdWaves) * (size_t(Rw) + size_t(k)) * sizeof(double);   // <= 64 KiB
  auto trial = [&]() -> krcn_status {
    hipLaunchKernelGGL((k_cubic_dense<T>), dim3(1), dim3(kNT), 0, s, ws.st, k, static_cast<const double*>(w->res), k,
                       ua, a.l2, static_cast<const double*>(ws.g), w->delta, cols, x, x_new, a.r0, a.solver_eps,
                       a.solver_it_max, ws.res);
    LAUNCHCHK();
    if (!empty) {
      hipLaunchKernelGGL((k_coord_update<T, true>), dim3(ugrid), dim3(kCoordUpdNT), ulds, s, int(n), Rw, k, cols,
                         static_cast<const double*>(w->delta), h->tptr, h->tidx, static_cast<const T*>(h->tval), Ax,
                         Ax_new, static_cast<const int*>(&ws.st->done));
      LAUNCHCHK();
    }
    hipLaunchKernelGGL((k_loss_terms_guard<T>), dim3(Pn), dim3(kNT), 0, s, n, static_cast<const T*>(Ax_new), b, h->pa,
                       static_cast<const CrnState*>(ws.st));
    LAUNCHCHK();
    if (a.l2 != 0.0) {
      hipLaunchKernelGGL((k_sqnorm_guard<T>), dim3(Pd), dim3(kNT), 0, s, d, static_cast<const T*>(x_new),
                         static_cast<const T*>(nullptr), h->pb, static_cast<const CrnState*>(ws.st), 0);
      LAUNCHCHK();
    }
    hipLaunchKernelGGL(k_crn_judge, dim3(1), dim3(kNT), 0, s, static_cast<const double*>(h->pa), Pn,
                       static_cast<const double*>(h->pb), Pd, n_mean, a.l2, a.value, a.ls_beta, a.max_trials,
                       ws.st, ws.res);
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
  if (!st.done) return fail(KRCN_ERR_HIP, "krcn_sscn_step: the trial chain did not end after %d trials", total);
  crn_solver_fields(st, info);
  info->accepted = st.accepted;
  info->trials = st.trials;
  info->value_new = st.value_new;
  const bool failed = st.solver_status == kCubicNotPd || st.solver_status == kCubicDerZero;
  info->dx_norm = failed ? 0.0 : std::sqrt(st.dx2);
  return KRCN_OK;
}

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
    SscnWs ws;
    CHK(sscn_ws(h, &ws));
    CHK(coord_reserve(h, k, s));
    CoordWs* w = h->cw;
    *info_host = krcn_crn_info{};
    // (pageable H2D copies are staged synchronously by the runtime: the host arrays may be reused)
    HIPCHK(hipMemcpyAsync(w->res, H_host, size_t(k) * size_t(k) * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ws.g, g_host, size_t(k) * sizeof(double), hipMemcpyHostToDevice, s));
    CHK(begin_chain(ws, M, s));
    hipLaunchKernelGGL((k_cubic_dense<double>), dim3(1), dim3(kNT), 0, s, ws.st, k, static_cast<const double*>(w->res),
                       k, static_cast<const int*>(nullptr), 0.0, static_cast<const double*>(ws.g), w->delta,
                       static_cast<const int*>(nullptr), static_cast<const double*>(nullptr),
                       static_cast<double*>(nullptr), r0, eps, it_max, ws.res);
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(h->hostbuf, w->delta, size_t(k) * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    CrnState st;
    std::memcpy(&st, h->crn_res, sizeof(CrnState));
    crn_solver_fields(st, info_host);
    const bool solved = st.solver_status == kCubicOk || st.solver_status == kCubicItMax;
    for (int i = 0; i < k; ++i) s_host[i] = solved ? h->hostbuf[i] : 0.0;
    return KRCN_OK;
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_cubic_dense: unexpected C++ exception");
  }
}

extern "C" krcn_status krcn_sscn_step(krcn_csr* h, int k, const int32_t* cols_host, const void* x, const void* b,
                                      const void* Ax, double value, double l2, double reg_coef, double ls_beta,
                                      double r0, double solver_eps, int solver_it_max, int max_trials, void* x_new,
                                      void* Ax_new, krcn_crn_info* info_host, void* stream) {
  try {
    if (!h) return fail(KRCN_ERR_INVALID, "krcn_sscn_step: null handle");
    if (h->shard != KRCN_SHARD_NONE)
      return fail(KRCN_ERR_UNSUPPORTED, "krcn_sscn_step: sharded handles are not supported");
    if (k < 1 || k > KRCN_SSCN_MAX)
      return fail(KRCN_ERR_INVALID, "krcn_sscn_step: k = %d outside [1, %d]", k, int(KRCN_SSCN_MAX));
    if (!cols_host || !x || !x_new || !info_host || (h->n && (!b || !Ax_new)))
      return fail(KRCN_ERR_INVALID, "krcn_sscn_step: null argument");
    if (max_trials < 0) return fail(KRCN_ERR_INVALID, "krcn_sscn_step: max_trials must be >= 0");
    if (!(ls_beta > 0.0 && ls_beta < 1.0)) return fail(KRCN_ERR_INVALID, "krcn_sscn_step: ls_beta must lie in (0, 1)");
    if (solver_it_max < 1) return fail(KRCN_ERR_INVALID, "krcn_sscn_step: solver_it_max must be >= 1");
    if (x_new == x || (Ax_new && (Ax_new == Ax || Ax_new == b)))
      return fail(KRCN_ERR_INVALID, "krcn_sscn_step: x_new and Ax_new must not alias the inputs");
    for (int a = 0; a < k; ++a)
      if (cols_host[a] < 0 || int64_t(cols_host[a]) >= h->d)
        return fail(KRCN_ERR_INVALID, "krcn_sscn_step: cols_host[%d] = %d outside [0, %lld)", a, int(cols_host[a]),
                    (long long)h->d);
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
        return fail(KRCN_ERR_INVALID, "krcn_sscn_step: cols_host[%d] = %d repeats cols_host[%d] (indices must be distinct)",
                    a, int(cols_host[a]), order[size_t(r - 1)]);
      sel[size_t(k + r)] = cols_host[a];
      sel[size_t(2 * k + a)] = r;
    }
    CHK(set_device(h));
    *info_host = krcn_crn_info{};
    const StepArgs args{value, l2, reg_coef, ls_beta, r0, solver_eps, k, solver_it_max, max_trials};
    return h->dtype == KRCN_F64
               ? sscn_step_impl<double>(h, sel.data(), static_cast<const double*>(x), static_cast<const double*>(b),
                                        static_cast<const double*>(Ax), args, static_cast<double*>(x_new),
                                        static_cast<double*>(Ax_new), info_host, S(stream))
               : sscn_step_impl<float>(h, sel.data(), static_cast<const float*>(x), static_cast<const float*>(b),
                                       static_cast<const float*>(Ax), args, static_cast<float*>(x_new),
                                       static_cast<float*>(Ax_new), info_host, S(stream));
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_sscn_step: unexpected C++ exception");
  }
}
