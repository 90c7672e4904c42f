// krcn_sscn_step.hpp — one SSCN step on the device over either subproblem
// route, and the front of its two entry points (krcn_sscn_step, krcn_sscn.hip;
// krcn_sscn_step_tridiag, krcn_sytd.hip): the coordinate gradient and Hessian
// block stay on the device, then a chain of guarded backtracking trials —
// solve, coordinate update of Ax, loss terms, norm, judge — whose accept /
// reject decision is taken on the device (krcn_crn_chain.hpp, krcn_coord.hpp).
// Replaces the host loop of SSCN.step, optimizer/cubic.py (reference
// cubic.py:352-398).
//
// A route is a struct next to the kernels it launches:
//   reserve(h, k)   its workspace; afterwards rec is the chain's record, cols
//                   room for the staged selection (3 k int32) and g for the
//                   gradient (k doubles)
//   begin(H, k, ua, l2, M0, s)   what the block H (ld k, rows in ascending
//                   column order, ua the selection's permutation) needs once
//                   per step, and the chain's first state with M = M0
//   solve<T>(delta, cols, ua, x, x_new, l2, r0, eps, it_max, s)   the guarded
//                   subproblem of a trial: s into delta, x_new[cols] = x[cols] + s
#pragma once
#include "krcn_coord.hpp"
#include "krcn_coord_ws.hpp"
#include "krcn_crn_chain.hpp"
#include "krcn_sscn_sel.hpp"

#include <cfloat>

struct SscnStepArgs {
  double value, l2, reg_coef, ls_beta, r0, solver_eps;
  int k, solver_it_max, max_trials;
};

template <typename T, class Route>
krcn_status sscn_step_run(const char* fn, krcn_csr* h, const int32_t* sel, const T* x, const T* b, const T* Ax,
                          const SscnStepArgs& a, T* x_new, T* Ax_new, krcn_crn_info* info, hipStream_t s) {
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
  Route route;
  CHK(route.reserve(h, k));
  CHK(coord_reserve(h, k, s));
  CoordWs* w = h->cw;
  // the selection as given, ascending (the Hessian kernel's order) and the map between them: one staged copy
  static_assert(3 * sizeof(int32_t) <= kCoordSlotPerCol, "the three staged int32 arrays fit a ring slot");
  CHK(coord_stage_bytes(h, sel, size_t(3 * k) * sizeof(int32_t), route.cols, s));
  const int* cols = route.cols;
  const int* ucols = route.cols + k;
  const int* ua = route.cols + 2 * k;
  if (empty) {
    hipLaunchKernelGGL((k_coord_l2x<T>), dim3((k + kNT - 1) / kNT), dim3(kNT), 0, s, k, cols, x, a.l2, route.g);
    LAUNCHCHK();
    HIPCHK(hipMemsetAsync(w->res, 0, size_t(k) * size_t(k) * sizeof(double), s));
    if (n) HIPCHK(hipMemcpyAsync(Ax_new, Ax, size_t(n) * sizeof(T), hipMemcpyDeviceToDevice, s));
  } else {
    hipLaunchKernelGGL((k_coord_grad<T>), dim3(k), dim3(kCoordGradNT), 0, s, cols, h->tptr, h->tidx,
                       static_cast<const T*>(h->tval), Ax, b, x, double(h->n_global), a.l2, int(a.l2 != 0.0), route.g);
    LAUNCHCHK();
    const int R = h->coord_window ? std::min(h->coord_window, kCoordWinMax) : kCoordWinMax;
    hipLaunchKernelGGL((k_coord_hess<T>), dim3(k), dim3(kCoordHessNT), 0, s, int(n), R, k, ucols, h->tptr, h->tidx,
                       static_cast<const T*>(h->tval), Ax, double(h->n_global), w->res);
    LAUNCHCHK();
  }
  HIPCHK(hipMemcpyAsync(x_new, x, size_t(d) * sizeof(T), hipMemcpyDeviceToDevice, s));
  CHK(route.begin(w->res, k, ua, a.l2, std::max(a.reg_coef * a.ls_beta, DBL_EPSILON), s));   // cubic.py:366

  // (n == 0: no loss terms, the judge's mean is 0 / 1 and the value the l2 term alone)
  const double n_mean = h->n_global > 0 ? double(h->n_global) : 1.0;
  const int Rw = h->coord_window ? std::min(h->coord_window, kCoordUpdMax) : kCoordUpdAuto;
  const int64_t waves = (n + Rw - 1) / Rw;
  const int ugrid = int((waves + kCoordUpdWaves - 1) / kCoordUpdWaves);
  const size_t ulds = size_t(kCoordUpdWaves) * (size_t(Rw) + size_t(k)) * sizeof(double);   // <= 64 KiB
  auto trial = [&]() -> krcn_status {
    CHK(route.template solve<T>(w->delta, cols, ua, x, x_new, a.l2, a.r0, a.solver_eps, a.solver_it_max, s));
    if (!empty) {
      hipLaunchKernelGGL((k_coord_update<T, true>), dim3(ugrid), dim3(kCoordUpdNT), ulds, s, int(n), Rw, k, cols,
                         static_cast<const double*>(w->delta), h->tptr, h->tidx, static_cast<const T*>(h->tval), Ax,
                         Ax_new, static_cast<const int*>(&route.rec.st->done));
      LAUNCHCHK();
    }
    return crn_judge_trial<T>(h, route.rec, Ax_new, b, x_new, n_mean, a.l2, a.value, a.ls_beta, a.max_trials, s);
  };
  CrnState st;
  CHK(crn_run_chain(h, fn, a.max_trials, s, trial, crn_no_tail, &st));
  crn_step_fields(st, info);
  return KRCN_OK;
}

// The front of an entry point named fn that takes up to kmax columns: the
// checks in their order, the staged selection, the dtype dispatch.
template <class Route>
krcn_status sscn_step_entry(const char* fn, int kmax, krcn_csr* h, int k, const int32_t* cols_host, const void* x,
                            const void* b, const void* Ax, double value, double l2, double reg_coef, double ls_beta,
                            double r0, double solver_eps, int solver_it_max, int max_trials, void* x_new,
                            void* Ax_new, krcn_crn_info* info_host, void* stream) {
  try {
    if (!h) return fail(KRCN_ERR_INVALID, "%s: null handle", fn);
    if (h->shard != KRCN_SHARD_NONE) return fail(KRCN_ERR_UNSUPPORTED, "%s: sharded handles are not supported", fn);
    if (k < 1 || k > kmax) return fail(KRCN_ERR_INVALID, "%s: k = %d outside [1, %d]", fn, k, kmax);
    if (!cols_host || !x || !x_new || !info_host || (h->n && (!b || !Ax_new)))
      return fail(KRCN_ERR_INVALID, "%s: null argument", fn);
    if (max_trials < 0) return fail(KRCN_ERR_INVALID, "%s: max_trials must be >= 0", fn);
    if (!(ls_beta > 0.0 && ls_beta < 1.0)) return fail(KRCN_ERR_INVALID, "%s: ls_beta must lie in (0, 1)", fn);
    if (solver_it_max < 1) return fail(KRCN_ERR_INVALID, "%s: solver_it_max must be >= 1", fn);
    if (x_new == x || (Ax_new && (Ax_new == Ax || Ax_new == b)))
      return fail(KRCN_ERR_INVALID, "%s: x_new and Ax_new must not alias the inputs", fn);
    const SscnSel sel = sscn_selection(cols_host, k, h->d);
    if (sel.error == SscnSel::Range)
      return fail(KRCN_ERR_INVALID, "%s: cols_host[%d] = %d outside [0, %lld)", fn, sel.at, int(cols_host[sel.at]),
                  (long long)h->d);
    if (sel.error == SscnSel::Repeat)
      return fail(KRCN_ERR_INVALID, "%s: cols_host[%d] = %d repeats cols_host[%d] (indices must be distinct)", fn,
                  sel.at, int(cols_host[sel.at]), sel.first);
    CHK(set_device(h));
    *info_host = krcn_crn_info{};
    const SscnStepArgs args{value, l2, reg_coef, ls_beta, r0, solver_eps, k, solver_it_max, max_trials};
    return h->dtype == KRCN_F64
               ? sscn_step_run<double, Route>(fn, h, sel.triple.data(), static_cast<const double*>(x),
                                              static_cast<const double*>(b), static_cast<const double*>(Ax), args,
                                              static_cast<double*>(x_new), static_cast<double*>(Ax_new), info_host,
                                              S(stream))
               : sscn_step_run<float, Route>(fn, h, sel.triple.data(), static_cast<const float*>(x),
                                             static_cast<const float*>(b), static_cast<const float*>(Ax), args,
                                             static_cast<float*>(x_new), static_cast<float*>(Ax_new), info_host,
                                             S(stream));
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "%s: unexpected C++ exception", fn);
  }
}
