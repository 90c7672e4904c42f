// krcn_crn.hip — the tridiagonal cubic subproblem on the device
// (krcn_cubic_tridiag) and one Krylov-CRN step behind one call (krcn_crn_step):
// gradient, weights, the Lanczos recurrence, then a chain of guarded
// backtracking trials whose accept / reject decision is taken on the device
// (krcn_cubic.hpp; the chain's host side is krcn_crn_chain.hpp's).  Replaces
// the host loop of Cubic_Krylov_LS.step, optimizer/cubic.py:239-270 (reference
// cubic.py:265-309).
#include "krcn_crn_chain.hpp"

static_assert(kCubicMaxM == kLzMaxM, "the subproblem kernel's LDS vectors hold the largest Lanczos m");

namespace {

constexpr size_t kCrnStateDoubles = sizeof(CrnState) / sizeof(double);

struct CrnWs : CrnRec {
  double *al, *be, *s;
};

CrnWs crn_ws(const krcn_csr* h) {
  double* v = h->crn_ws + kCrnStateDoubles;
  return CrnWs{crn_rec(h), v, v + kLzMaxM, v + 2 * size_t(kLzMaxM)};
}

struct StepArgs {
  double value, tol, l2, reg_coef, ls_beta, r0, solver_eps;
  int m, reorth, solver_it_max, max_trials;
};

template <typename T>
krcn_status crn_step_impl(krcn_csr* h, const T* x, const T* b, const T* Ax, const StepArgs& a, T* V, T* x_new,
                          T* Ax_new, double* alphas_host, double* betas_host, krcn_crn_info* info, hipStream_t s) {
  const int64_t d = h->d;
  CHK(plans_for_compute(h));   // before any scratch pointer is read: a plan build may move them
  CHK(ensure_crn_ws(h));
  const CrnWs ws = crn_ws(h);
  T* g = static_cast<T*>(h->td);   // unsharded handles leave td and (after the gradient) tn free
  T* w = static_cast<T*>(h->tn);
  // 1.-3. Ax if it was not given, the gradient (its residual passes through tn), the weights
  if (!Ax) {
    CHK(krcn_matvec(h, x, Ax_new, s));
    Ax = Ax_new;
  }
  CHK(krcn_gradient(h, Ax, b, x, a.l2, g, s));
  CHK(krcn_weights(h, Ax, w, s));
  // 4. the recurrence: its launches alone, alphas / betas / state stay on the device
  if constexpr (std::is_same<T, double>::value)
    CHK(lanczos_f64(h, w, g, a.m, a.reorth, a.tol, a.l2, V, nullptr, nullptr, nullptr, s, true));
  else
    CHK(lanczos_f32(h, w, g, a.m, a.reorth, a.tol, a.l2, V, nullptr, nullptr, nullptr, s, true));
  // 5. the chain
  hipLaunchKernelGGL(k_crn_begin, dim3(1), dim3(kNT), 0, s, static_cast<const double*>(h->hostres_dev), a.m, 0.0,
                     a.reg_coef * a.ls_beta, ws.st, ws.al, ws.be);
  LAUNCHCHK();
  const LanczosState* guard = reinterpret_cast<const LanczosState*>(ws.st);
  const int Pd = vec_grid(d);
  auto trial = [&]() -> krcn_status {
    hipLaunchKernelGGL(k_cubic_tridiag, dim3(1), dim3(kNT), 0, s, ws.st, static_cast<const double*>(ws.al),
                       static_cast<const double*>(ws.be), ws.s, a.r0, a.solver_eps, a.solver_it_max, ws.res);
    LAUNCHCHK();
    hipLaunchKernelGGL((k_basis_combine_dev<T>), dim3(Pd), dim3(kNT), 0, s, d, static_cast<const CrnState*>(ws.st),
                       static_cast<const T*>(V), static_cast<const double*>(ws.s), x, x_new);
    LAUNCHCHK();
    const SrcGuard<T> src{x_new, guard, 0};
    CHK(run_pass<T>(h->p1, src, src, EpiStore<T>{Ax_new}, nullptr, nullptr, s));
    return crn_judge_trial<T>(h, ws, Ax_new, b, x_new, double(h->n_global), a.l2, a.value, a.ls_beta, a.max_trials,
                              s);
  };
  // the step length, in the submission of the batch that ends the chain (others skip it)
  auto step_length = [&]() -> krcn_status {
    hipLaunchKernelGGL((k_sqnorm_guard<T>), dim3(Pd), dim3(kNT), 0, s, d, static_cast<const T*>(x_new), x, h->pb,
                       static_cast<const CrnState*>(ws.st), 1);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_crn_dx_finish, dim3(1), dim3(kNT), 0, s, static_cast<const double*>(h->pb), Pd, ws.st,
                       ws.res);
    LAUNCHCHK();
    return KRCN_OK;
  };
  CrnState st;
  CHK(crn_run_chain(h, "krcn_crn_step", a.max_trials, s, trial, step_length, &st));
  double be1 = 0.0;   // (m = 1 has no betas)
  std::vector<double> al_tmp;
  if (!alphas_host || !betas_host) al_tmp.resize(2 * size_t(a.m));
  lanczos_results(h, a.m, alphas_host ? alphas_host : al_tmp.data(),
                  betas_host ? betas_host : (a.m > 1 ? al_tmp.data() + a.m : &be1), &info->lanczos);
  crn_step_fields(st, info);
  return KRCN_OK;
}

}  // namespace

krcn_status ensure_crn_ws(krcn_csr* h) {
  if (!h->crn_ws) CHK(dalloc(h, &h->crn_ws, kCrnStateDoubles + 3 * size_t(kLzMaxM)));
  if (!h->crn_res) {
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->crn_res), sizeof(CrnState),
                         hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(h->crn_res, 0, sizeof(CrnState));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->crn_res_dev), h->crn_res, 0));
  }
  return KRCN_OK;
}

extern "C" krcn_status krcn_cubic_tridiag(krcn_csr* h, int m, const double* alphas_host, const double* betas_host,
                                          double gnorm, double M, double r0, double eps, int it_max, double* s_host,
                                          krcn_crn_info* info_host, void* stream) {
  try {
    if (!h || !alphas_host || !s_host || !info_host || (m > 1 && !betas_host))
      return fail(KRCN_ERR_INVALID, "krcn_cubic_tridiag: null argument");
    if (m < 1 || m > kLzMaxM) return fail(KRCN_ERR_INVALID, "krcn_cubic_tridiag: m %d outside [1, %d]", m, kLzMaxM);
    if (it_max < 1) return fail(KRCN_ERR_INVALID, "krcn_cubic_tridiag: it_max must be >= 1");
    CHK(set_device(h));
    CHK(ensure_crn_ws(h));
    hipStream_t s = S(stream);
    const CrnWs ws = crn_ws(h);
    *info_host = krcn_crn_info{};
    // (pageable H2D copies are staged synchronously by the runtime: the host arrays may be reused)
    HIPCHK(hipMemcpyAsync(ws.al, alphas_host, size_t(m) * sizeof(double), hipMemcpyHostToDevice, s));
    if (m > 1) HIPCHK(hipMemcpyAsync(ws.be, betas_host, size_t(m - 1) * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_crn_begin, dim3(1), dim3(kNT), 0, s, static_cast<const double*>(nullptr), m, gnorm, M, ws.st,
                       ws.al, ws.be);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_cubic_tridiag, dim3(1), dim3(kNT), 0, s, ws.st, static_cast<const double*>(ws.al),
                       static_cast<const double*>(ws.be), ws.s, r0, eps, it_max, ws.res);
    LAUNCHCHK();
    return crn_read_solve(h, ws.s, m, s_host, info_host, s);
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_cubic_tridiag: unexpected C++ exception");
  }
}

extern "C" krcn_status krcn_crn_step(krcn_csr* h, const void* x, const void* b, const void* Ax, double value, int m,
                                     int reorth, double tol, double l2, double reg_coef, double ls_beta, double r0,
                                     double solver_eps, int solver_it_max, int max_trials, void* V, void* x_new,
                                     void* Ax_new, double* alphas_host, double* betas_host,
                                     krcn_crn_info* info_host, void* stream) {
  try {
    if (!h || !x || !b || !V || !x_new || !Ax_new || !info_host)
      return fail(KRCN_ERR_INVALID, "krcn_crn_step: null argument");
    if (h->shard != KRCN_SHARD_NONE)
      return fail(KRCN_ERR_UNSUPPORTED, "krcn_crn_step: sharded handles are not supported");
    if (m < 1 || m > kLzMaxM) return fail(KRCN_ERR_INVALID, "krcn_crn_step: m %d outside [1, %d]", m, kLzMaxM);
    if (max_trials < 0) return fail(KRCN_ERR_INVALID, "krcn_crn_step: max_trials must be >= 0");
    if (!(ls_beta > 0.0 && ls_beta < 1.0)) return fail(KRCN_ERR_INVALID, "krcn_crn_step: ls_beta must lie in (0, 1)");
    if (solver_it_max < 1) return fail(KRCN_ERR_INVALID, "krcn_crn_step: solver_it_max must be >= 1");
    if (h->n < 1 || h->d < 1) return fail(KRCN_ERR_INVALID, "krcn_crn_step: the matrix is empty");
    if (x_new == x || Ax_new == b || x_new == V)
      return fail(KRCN_ERR_INVALID, "krcn_crn_step: x_new and Ax_new must not alias the inputs");
    CHK(set_device(h));
    *info_host = krcn_crn_info{};
    const StepArgs a{value, tol, l2, reg_coef, ls_beta, r0, solver_eps, m, reorth, solver_it_max, max_trials};
    return h->dtype == KRCN_F64
               ? crn_step_impl<double>(h, static_cast<const double*>(x), static_cast<const double*>(b),
                                       static_cast<const double*>(Ax), a, static_cast<double*>(V),
                                       static_cast<double*>(x_new), static_cast<double*>(Ax_new), alphas_host,
                                       betas_host, info_host, S(stream))
               : crn_step_impl<float>(h, static_cast<const float*>(x), static_cast<const float*>(b),
                                      static_cast<const float*>(Ax), a, static_cast<float*>(V),
                                      static_cast<float*>(x_new), static_cast<float*>(Ax_new), alphas_host, betas_host,
                                      info_host, S(stream));
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_crn_step: unexpected C++ exception");
  }
}
