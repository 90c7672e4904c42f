// krcn_crn_chain.hpp — the host side of a CrnState chain (krcn_cubic.hpp), one
// definition for krcn_crn_step, krcn_sscn_step, krcn_sscn_step_tridiag and the
// subproblem-only calls: where the handle keeps the record, the batch loop with
// its one synchronisation per batch (kCrnFirstBatch / kCrnBatch), the judged
// tail of a trial, and how the host reads the record back.  The batched step
// (krcn_crn_block.hip) and krcn_cubic_cg keep records and loops of their own.
#pragma once
#include "krcn_cubic.hpp"
#include "krcn_internal.hpp"

// The chain's state on the device and the mapped host record by its device
// address (both allocated by ensure_crn_ws).
struct CrnRec {
  CrnState* st;
  CrnState* res;
};
inline CrnRec crn_rec(const krcn_csr* h) {
  return CrnRec{reinterpret_cast<CrnState*>(h->crn_ws), reinterpret_cast<CrnState*>(h->crn_res_dev)};
}

// The solver fields of a chain's record, as the host reads them back.
inline void crn_solver_fields(const CrnState& st, krcn_crn_info* info) {
  info->solver_it = st.solver_it;
  info->solver_status = st.solver_status;
  info->reg_coef = st.M;
  info->lam = st.lam;
  info->model_decrease = st.model_decrease;
}

// A step's record: the solver fields and the line search's.
inline void crn_step_fields(const CrnState& st, krcn_crn_info* info) {
  crn_solver_fields(st, info);
  info->accepted = st.accepted;
  info->trials = st.trials;
  info->value_new = st.value_new;
  const bool failed = st.solver_status == kCubicNotPd || st.solver_status == kCubicDerZero;
  info->dx_norm = failed ? 0.0 : std::sqrt(st.dx2);
}

inline krcn_status crn_no_tail() { return KRCN_OK; }

// Enqueues trial() in batches until the record read after a batch's one
// synchronisation has done set; after_batch() closes each submission (the
// step-length tail of krcn_crn_step; crn_no_tail otherwise).
template <class Trial, class AfterBatch>
krcn_status crn_run_chain(krcn_csr* h, const char* fn, int max_trials, hipStream_t s, Trial&& trial,
                          AfterBatch&& after_batch, CrnState* st) {
  *st = CrnState{};
  const int total = max_trials + 1;   // the trial after max_trials rejections ends the chain itself
  for (int enq = 0; enq < total && !st->done;) {
    const int batch = std::min(enq == 0 ? kCrnFirstBatch : kCrnBatch, total - enq);
    for (int t = 0; t < batch; ++t) CHK(trial());
    enq += batch;
    CHK(after_batch());
    HIPCHK(hipStreamSynchronize(s));
    std::memcpy(st, h->crn_res, sizeof(CrnState));
  }
  if (!st->done) return fail(KRCN_ERR_HIP, "%s: the trial chain did not end after %d trials", fn, total);
  return KRCN_OK;
}

// The guarded tail of a trial: the loss terms of Ax_new, ||x_new||^2 when
// l2 != 0, and the judge over n_mean rows.
template <typename T>
krcn_status crn_judge_trial(const krcn_csr* h, const CrnRec& rec, const T* Ax_new, const T* b, const T* x_new,
                            double n_mean, double l2, double value, double ls_beta, int max_trials, hipStream_t s) {
  const int64_t n = h->n, d = h->d;
  const int Pn = vec_grid(n), Pd = vec_grid(d);
  hipLaunchKernelGGL((k_loss_terms_guard<T>), dim3(Pn), dim3(kNT), 0, s, n, Ax_new, b, h->pa,
                     static_cast<const CrnState*>(rec.st));
  LAUNCHCHK();
  if (l2 != 0.0) {
    hipLaunchKernelGGL((k_sqnorm_guard<T>), dim3(Pd), dim3(kNT), 0, s, d, x_new, static_cast<const T*>(nullptr), h->pb,
                       static_cast<const CrnState*>(rec.st), 0);
    LAUNCHCHK();
  }
  hipLaunchKernelGGL(k_crn_judge, dim3(1), dim3(kNT), 0, s, static_cast<const double*>(h->pa), Pn,
                     static_cast<const double*>(h->pb), Pd, n_mean, l2, value, ls_beta, max_trials, rec.st, rec.res);
  LAUNCHCHK();
  return KRCN_OK;
}

// The read-back of a subproblem-only call: the n entries of the solve at dev_s
// and the record, after one synchronisation; s_host is zero unless the solve
// ended Ok or at it_max.
inline krcn_status crn_read_solve(krcn_csr* h, const double* dev_s, int n, double* s_host, krcn_crn_info* info,
                                  hipStream_t s) {
  HIPCHK(hipMemcpyAsync(h->hostbuf, dev_s, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  CrnState st;
  std::memcpy(&st, h->crn_res, sizeof(CrnState));
  crn_solver_fields(st, info);
  const bool solved = st.solver_status == kCubicOk || st.solver_status == kCubicItMax;
  for (int i = 0; i < n; ++i) s_host[i] = solved ? h->hostbuf[i] : 0.0;
  return KRCN_OK;
}
