// krcn_crn_block.hip — the batched Krylov-CRN step: k problems over one X
// advance one step of Cubic_Krylov_LS.step (optimizer/cubic.py:265-309) behind
// one call (krcn_crn_step_block), with its pieces as entry points of their own:
// the block gradient and value (krcn_gradient_block, krcn_value_block) and the
// batched subproblem (krcn_cubic_tridiag_block).  Kernels: krcn_crnb.hpp; the
// per-column transition: krcn_crnb_state.hpp.
//
// One step enqueues
//   krcn_matvec_block (when AX is not given), k_crnb_residual + the X^T pass
//   (the gradients), krcn_weights_block, the batched Lanczos' launches without
//   its synchronisation, k_crnb_begin (records from the Lanczos states, on the
//   device), then trials in batches (kCrnbFirstBatch, then kCrnbBatch):
//     k_crnb_solve (grid k), k_crnb_combine, the guarded X V pass, k_crnb_loss,
//     k_crnb_sq where some l2_c != 0, k_crnb_judge
//   and after each batch k_crnb_sq + k_crnb_dx_finish (the step lengths, run
//   once the chain has ended) and one synchronisation.  The host reads the
//   mapped record block after each batch and nothing else; it never spins.
// The calls build no pass plans, run no graph replay or placement search and
// keep their blocks in the handle's owner table, apart from u / tn / W / td,
// the single step's workspace and the results block of krcn_lanczos.
#include "krcn_internal.hpp"
#include "krcn_crnb.hpp"

using namespace krcn;

namespace {

// Trials per submission, as krcn_crn_step's kCrnFirstBatch / kCrnBatch.
constexpr int kCrnbFirstBatch = 2;
constexpr int kCrnbBatch = 4;

constexpr size_t kCrnbStateDoubles = kCrnbHeadDoubles + size_t(KRCN_BLOCK_MAX) * kCrnbColDoubles;
constexpr size_t kCrnbHostDoubles = kCrnbStateDoubles + KRCN_BLOCK_MAX;   // the records, then krcn_value_block's values

struct CrnbWs {
  double* st;    // head | records
  double* par;   // the staged parameters
  double *al, *be, *s;   // k rows of kLzMaxM each
  double *pl, *pn;       // partials: loss terms, squared norms
  double* out;   // the mapped host block, by its device address
};

CrnbWs crnb_ws(const krcn_csr* h) {
  const size_t row = size_t(h->crnb_k) * kLzMaxM;
  return CrnbWs{h->crnb_st, h->crnb_st + kCrnbStateDoubles, h->crnb_sub, h->crnb_sub + row, h->crnb_sub + 2 * row,
                h->crnb_pa, h->crnb_pa + size_t(kBlzMaxGrid) * KRCN_BLOCK_MAX, h->crnb_host_dev};
}

// The workspace for k columns: allocates only when k grows (the fixed blocks once).
krcn_status crnb_reserve(krcn_csr* h, int k, hipStream_t s) {
  if (!h->crnb_st) CHK(dalloc(h, &h->crnb_st, kCrnbStateDoubles + size_t(KRCN_BLOCK_MAX) * kCrnbPar));
  if (!h->crnb_pa) CHK(dalloc(h, &h->crnb_pa, size_t(2) * kBlzMaxGrid * KRCN_BLOCK_MAX));
  if (!h->crnb_host) {
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->crnb_host), kCrnbHostDoubles * sizeof(double),
                         hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(h->crnb_host, 0, kCrnbHostDoubles * sizeof(double));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->crnb_host_dev), h->crnb_host, 0));
  }
  if (k > h->crnb_k) {
    if (h->crnb_g) {
      HIPCHK(hipStreamSynchronize(s));   // an earlier call's launches may still use the old blocks
      h->crnb_k = 0;
      CHK(h->own.release(&h->crnb_g));
      CHK(h->own.release(&h->crnb_w));
      CHK(h->own.release(&h->crnb_sub));
    }
    CHK(h->own.alloc(&h->crnb_g, std::max<size_t>(size_t(h->d) * size_t(k) * h->vs, 16)));
    CHK(h->own.alloc(&h->crnb_w, std::max<size_t>(size_t(h->n) * size_t(k) * h->vs, 16)));
    CHK(dalloc(h, &h->crnb_sub, size_t(3) * size_t(k) * kLzMaxM));
    h->crnb_k = k;
  }
  return KRCN_OK;
}

template <int K> struct CrnbLaneC { static constexpr int value = K; };
// f(CrnbLaneC<K>) for the lane group of k columns
template <class F>
void crnb_lanes(int k, F&& f) {
  switch (block_lanes(k)) {
    case 1: f(CrnbLaneC<1>{}); break;
    case 2: f(CrnbLaneC<2>{}); break;
    case 4: f(CrnbLaneC<4>{}); break;
    case 8: f(CrnbLaneC<8>{}); break;
    default: f(CrnbLaneC<16>{}); break;
  }
}

// The scalar ranges every entry point shares, checked before the handle is looked at.
krcn_status check_k(const char* fn, int k) {
  if (k < 1 || k > KRCN_BLOCK_MAX)
    return fail(KRCN_ERR_INVALID, "%s: k = %d outside [1, %d]", fn, k, int(KRCN_BLOCK_MAX));
  return KRCN_OK;
}
krcn_status check_b_cols(const char* fn, int k, int b_cols) {
  if (b_cols != 1 && b_cols != k)
    return fail(KRCN_ERR_INVALID, "%s: b_cols = %d is neither 1 nor k = %d", fn, b_cols, k);
  return KRCN_OK;
}
krcn_status check_handle(const char* fn, const krcn_csr* h) {
  if (!h) return fail(KRCN_ERR_INVALID, "%s: null handle", fn);
  if (h->shard != KRCN_SHARD_NONE) return fail(KRCN_ERR_UNSUPPORTED, "%s: implemented for unsharded handles", fn);
  return KRCN_OK;
}

bool any_nonzero(const double* l2_host, int k) {
  for (int c = 0; l2_host && c < k; ++c)
    if (l2_host[c] != 0.0) return true;
  return false;
}

// (a pageable H2D copy is staged before the call returns: par may leave scope)
krcn_status stage_params(const CrnbWs& ws, int k, const double* par, hipStream_t s) {
  HIPCHK(hipMemcpyAsync(ws.par, par, size_t(k) * kCrnbPar * sizeof(double), hipMemcpyHostToDevice, s));
  return KRCN_OK;
}

// G[:, c] = X^T (expit(AX[:, c]) - b_c) / n + l2_c X[:, c]; the residuals pass through the weights block.
template <typename T>
krcn_status gradient_block_impl(krcn_csr* h, int k, const T* AX, const T* b, int b_cols, const T* X,
                                const double* l2_host, T* Gm, hipStream_t s) {
  T* R = static_cast<T*>(h->crnb_w);
  if (h->n > 0) {
    crnb_lanes(k, [&](auto lc) {
      constexpr int K = decltype(lc)::value;
      hipLaunchKernelGGL((k_crnb_residual<T, K>), dim3(blz_grid(h->n, K)), dim3(kNT), 0, s, h->n, k, AX, b,
                         b_cols == 1 ? 0 : k, R);
    });
    LAUNCHCHK();
  }
  return block_rmatvec_l2(h, k, R, X, l2_host, Gm, s);
}

// Partials of the loss terms over AX, and of ||X_c||^2 where some l2_c != 0 (st: a trial's guard, or null).
template <typename T>
krcn_status value_partials(krcn_csr* h, const CrnbWs& ws, int k, const T* AX, const T* b, int b_cols, const T* X,
                           bool any_l2, const double* st, hipStream_t s) {
  crnb_lanes(k, [&](auto lc) {
    constexpr int K = decltype(lc)::value;
    hipLaunchKernelGGL((k_crnb_loss<T, K>), dim3(blz_grid(h->n, K)), dim3(kNT), 0, s, h->n, k, AX, b,
                       b_cols == 1 ? 0 : k, ws.pl, st);
    if (any_l2)
      hipLaunchKernelGGL((k_crnb_sq<T, K>), dim3(blz_grid(h->d, K)), dim3(kNT), 0, s, h->d, k, X,
                         static_cast<const T*>(nullptr), ws.pn, st, 0);
  });
  LAUNCHCHK();
  return KRCN_OK;
}

template <typename T>
krcn_status value_block_impl(krcn_csr* h, int k, const T* AX, const T* b, int b_cols, const T* X,
                             const double* l2_host, double* values_host, hipStream_t s) {
  CHK(crnb_reserve(h, k, s));
  const CrnbWs ws = crnb_ws(h);
  double par[KRCN_BLOCK_MAX * kCrnbPar] = {};
  for (int c = 0; c < k; ++c) par[c * kCrnbPar + kCrnbParL2] = l2_host ? l2_host[c] : 0.0;
  CHK(stage_params(ws, k, par, s));
  const bool any_l2 = any_nonzero(l2_host, k);
  CHK(value_partials<T>(h, ws, k, AX, b, b_cols, X, any_l2, nullptr, s));
  crnb_lanes(k, [&](auto lc) {
    constexpr int K = decltype(lc)::value;
    hipLaunchKernelGGL((k_crnb_value_finish<K>), dim3(1), dim3(kNT), 0, s, k, static_cast<const double*>(ws.pl),
                       blz_grid(h->n, K), static_cast<const double*>(ws.pn), blz_grid(h->d, K), int(any_l2),
                       double(h->n_global), static_cast<const double*>(ws.par), ws.out + kCrnbStateDoubles);
  });
  LAUNCHCHK();
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(values_host, h->crnb_host + kCrnbStateDoubles, size_t(k) * sizeof(double));
  return KRCN_OK;
}

void solver_fields(const CrnbCol& col, krcn_crn_info* info) {
  info->solver_it = col.solver_it;
  info->solver_status = col.solver_status;
  info->reg_coef = col.M;
  info->lam = col.lam;
  info->model_decrease = col.model_decrease;
}

CrnbCol host_record(const krcn_csr* h, int c) {
  CrnbCol col;
  std::memcpy(&col, h->crnb_host + kCrnbHeadDoubles + size_t(c) * kCrnbColDoubles, sizeof(CrnbCol));
  return col;
}

struct StepArgs {
  const double *values, *l2, *reg_coef, *r0;
  const int* active;
  double tol, ls_beta, solver_eps;
  int m, b_cols, solver_it_max, max_trials;
};

template <typename T>
krcn_status crn_step_block_impl(krcn_csr* h, int k, const T* X, const T* b, const T* AX, const StepArgs& a, T* V,
                                T* Xn, T* AXn, double* alphas_host, double* betas_host, krcn_crn_info* info,
                                hipStream_t s) {
  const int64_t n = h->n, d = h->d;
  const int m = a.m;
  CHK(crnb_reserve(h, k, s));
  T* Gm = static_cast<T*>(h->crnb_g);
  T* W = static_cast<T*>(h->crnb_w);
  // 1.-3. AX if it was not given, the gradients (their residuals pass through W), the weights
  const bool ax_given = AX != nullptr;
  if (!ax_given) {
    CHK(krcn_matvec_block(h, k, X, AXn, s));
    AX = AXn;
  }
  CHK(gradient_block_impl<T>(h, k, AX, b, a.b_cols, X, a.l2, Gm, s));
  CHK(krcn_weights_block(h, k, AX, W, s));
  // 4. the recurrences: their launches alone, alphas / betas / states stay on the device
  CHK(lanczos_block_enqueue(h, k, W, k, Gm, m, a.tol, a.l2, V, s));
  // 5. the chain
  const CrnbWs ws = crnb_ws(h);
  double par[KRCN_BLOCK_MAX * kCrnbPar] = {};
  bool any_inactive = false;
  for (int c = 0; c < k; ++c) {
    double* p = par + c * kCrnbPar;
    p[kCrnbParValue] = a.values[c];
    p[kCrnbParL2] = a.l2 ? a.l2[c] : 0.0;
    p[kCrnbParM0] = a.reg_coef[c] * a.ls_beta;
    p[kCrnbParR0] = a.r0[c];
    p[kCrnbParActive] = (!a.active || a.active[c]) ? 1.0 : 0.0;
    any_inactive = any_inactive || p[kCrnbParActive] == 0.0;
  }
  CHK(stage_params(ws, k, par, s));
  const double* cst = ws.st;
  const double* blz_al = h->blz_res + 4 * k;
  const double* blz_be = blz_al + size_t(k) * m;
  const int mb = m > 1 ? m - 1 : 1;
  const bool any_l2 = any_nonzero(a.l2, k);
  hipLaunchKernelGGL(k_crnb_begin, dim3(1), dim3(kNT), 0, s, k, m, static_cast<const double*>(ws.par),
                     reinterpret_cast<const BlzCol*>(h->blz_res), ws.st);
  LAUNCHCHK();
  const int K = block_lanes(k);
  const int Pn = blz_grid(n, K), Pd = blz_grid(d, K);
  if (any_inactive) {
    crnb_lanes(k, [&](auto lc) {
      constexpr int KK = decltype(lc)::value;
      hipLaunchKernelGGL((k_crnb_copy_inactive<T, KK>), dim3(Pd), dim3(kNT), 0, s, d, k, X, Xn, cst);
      if (ax_given)   // (else AXn already holds X x_c in every column)
        hipLaunchKernelGGL((k_crnb_copy_inactive<T, KK>), dim3(Pn), dim3(kNT), 0, s, n, k, AX, AXn, cst);
    });
    LAUNCHCHK();
  }
  auto trial = [&]() -> krcn_status {
    hipLaunchKernelGGL(k_crnb_solve, dim3(k), dim3(kNT), 0, s, ws.st, m, blz_al, m, blz_be, mb, ws.s, int(kLzMaxM),
                       a.solver_eps, a.solver_it_max);
    LAUNCHCHK();
    crnb_lanes(k, [&](auto lc) {
      constexpr int KK = decltype(lc)::value;
      hipLaunchKernelGGL((k_crnb_combine<T, KK>), dim3(Pd), dim3(kNT), 0, s, d, k, m, static_cast<const T*>(V),
                         static_cast<const double*>(ws.s), int(kLzMaxM), X, Xn, cst);
    });
    LAUNCHCHK();
    CHK(block_matvec_live(h, k, Xn, AXn, cst, s));
    CHK(value_partials<T>(h, ws, k, AXn, b, a.b_cols, Xn, any_l2, cst, s));
    crnb_lanes(k, [&](auto lc) {
      constexpr int KK = decltype(lc)::value;
      hipLaunchKernelGGL((k_crnb_judge<KK>), dim3(1), dim3(kNT), 0, s, k, static_cast<const double*>(ws.pl), Pn,
                         static_cast<const double*>(ws.pn), Pd, int(any_l2), double(h->n_global), a.ls_beta,
                         a.max_trials, ws.st, ws.out);
    });
    LAUNCHCHK();
    return KRCN_OK;
  };
  CrnbHead head{};
  const int total = crnb_total_trials(a.max_trials);
  for (int enq = 0; enq < total && !head.all_done;) {
    const int batch = std::min(enq == 0 ? kCrnbFirstBatch : kCrnbBatch, total - enq);
    for (int t = 0; t < batch; ++t) CHK(trial());
    enq += batch;
    // the step lengths, in the submission of the batch that ends the chain (others skip them)
    crnb_lanes(k, [&](auto lc) {
      constexpr int KK = decltype(lc)::value;
      hipLaunchKernelGGL((k_crnb_sq<T, KK>), dim3(Pd), dim3(kNT), 0, s, d, k, static_cast<const T*>(Xn), X, ws.pn, cst,
                         1);
      hipLaunchKernelGGL((k_crnb_dx_finish<KK>), dim3(1), dim3(kNT), 0, s, k, static_cast<const double*>(ws.pn), Pd,
                         ws.st, ws.out);
    });
    LAUNCHCHK();
    HIPCHK(hipStreamSynchronize(s));
    std::memcpy(&head, h->crnb_host, sizeof(CrnbHead));
  }
  if (!head.all_done)
    return fail(KRCN_ERR_HIP, "krcn_crn_step_block: the trial chains did not end after %d trials", total);
  krcn_lanczos_info li[KRCN_BLOCK_MAX];
  lanczos_block_results(h, k, m, alphas_host, betas_host, li);
  for (int c = 0; c < k; ++c) {
    const CrnbCol col = host_record(h, c);
    info[c] = krcn_crn_info{};
    info[c].lanczos = li[c];
    if (col.phase == kCrnbInactive) {
      info[c].value_new = a.values[c];
      info[c].reg_coef = a.reg_coef[c];
      continue;
    }
    solver_fields(col, &info[c]);
    info[c].accepted = crnb_accepted(col.phase);
    info[c].trials = col.trials;
    info[c].value_new = col.value_new;
    info[c].dx_norm = crnb_moved(col.phase) ? std::sqrt(col.dx2) : 0.0;
  }
  return KRCN_OK;
}

}  // namespace

extern "C" krcn_status krcn_gradient_block(krcn_csr* h, int k, const void* AX, const void* b, int b_cols,
                                           const void* X, const double* l2_host, void* G, void* stream) {
  try {
    CHK(check_k("krcn_gradient_block", k));
    CHK(check_b_cols("krcn_gradient_block", k, b_cols));
    CHK(check_handle("krcn_gradient_block", h));
    if ((h->n && (!AX || !b)) || (h->d && !G) || (any_nonzero(l2_host, k) && h->d && !X))
      return fail(KRCN_ERR_INVALID, "krcn_gradient_block: null argument");
    if (h->d == 0) return KRCN_OK;
    CHK(set_device(h));
    hipStream_t s = S(stream);
    CHK(crnb_reserve(h, k, s));
    return h->dtype == KRCN_F64
               ? gradient_block_impl<double>(h, k, static_cast<const double*>(AX), static_cast<const double*>(b),
                                             b_cols, static_cast<const double*>(X), l2_host, static_cast<double*>(G), s)
               : gradient_block_impl<float>(h, k, static_cast<const float*>(AX), static_cast<const float*>(b), b_cols,
                                            static_cast<const float*>(X), l2_host, static_cast<float*>(G), s);
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_gradient_block: unexpected C++ exception");
  }
}

extern "C" krcn_status krcn_value_block(krcn_csr* h, int k, const void* AX, const void* b, int b_cols, const void* X,
                                        const double* l2_host, double* values_host, void* stream) {
  try {
    CHK(check_k("krcn_value_block", k));
    CHK(check_b_cols("krcn_value_block", k, b_cols));
    CHK(check_handle("krcn_value_block", h));
    if (!values_host || (h->n && (!AX || !b)) || (any_nonzero(l2_host, k) && h->d && !X))
      return fail(KRCN_ERR_INVALID, "krcn_value_block: null argument");
    CHK(set_device(h));
    return h->dtype == KRCN_F64
               ? value_block_impl<double>(h, k, static_cast<const double*>(AX), static_cast<const double*>(b), b_cols,
                                          static_cast<const double*>(X), l2_host, values_host, S(stream))
               : value_block_impl<float>(h, k, static_cast<const float*>(AX), static_cast<const float*>(b), b_cols,
                                         static_cast<const float*>(X), l2_host, values_host, S(stream));
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_value_block: unexpected C++ exception");
  }
}

extern "C" krcn_status krcn_cubic_tridiag_block(krcn_csr* h, int k, int m, const int* m_eff_host,
                                                const double* alphas_host, const double* betas_host,
                                                const double* gnorm_host, const double* M_host,
                                                const double* r0_host, double eps, int it_max, double* s_host,
                                                krcn_crn_info* info_host, void* stream) {
  try {
    const char* fn = "krcn_cubic_tridiag_block";
    CHK(check_k(fn, k));
    if (m < 1 || m > kLzMaxM) return fail(KRCN_ERR_INVALID, "%s: m = %d outside [1, %d]", fn, m, kLzMaxM);
    if (it_max < 1) return fail(KRCN_ERR_INVALID, "%s: it_max must be >= 1", fn);
    CHK(check_handle(fn, h));
    if (!m_eff_host || !alphas_host || !gnorm_host || !M_host || !r0_host || !s_host || !info_host ||
        (m > 1 && !betas_host))
      return fail(KRCN_ERR_INVALID, "%s: null argument", fn);
    for (int c = 0; c < k; ++c)
      if (m_eff_host[c] < 1 || m_eff_host[c] > m)
        return fail(KRCN_ERR_INVALID, "%s: m_eff[%d] = %d outside [1, m = %d]", fn, c, m_eff_host[c], m);
    CHK(set_device(h));
    hipStream_t s = S(stream);
    CHK(crnb_reserve(h, k, s));
    const CrnbWs ws = crnb_ws(h);
    const int mb = m > 1 ? m - 1 : 1;
    double par[KRCN_BLOCK_MAX * kCrnbPar] = {};
    for (int c = 0; c < k; ++c) {
      double* p = par + c * kCrnbPar;
      p[kCrnbParM0] = M_host[c];
      p[kCrnbParR0] = r0_host[c];
      p[kCrnbParActive] = 1.0;
      p[kCrnbParMeff] = double(m_eff_host[c]);
      p[kCrnbParGnorm] = gnorm_host[c];
    }
    CHK(stage_params(ws, k, par, s));
    // (pageable H2D copies are staged synchronously by the runtime: the host arrays may be reused)
    HIPCHK(hipMemcpyAsync(ws.al, alphas_host, size_t(k) * m * sizeof(double), hipMemcpyHostToDevice, s));
    if (m > 1) HIPCHK(hipMemcpyAsync(ws.be, betas_host, size_t(k) * mb * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_crnb_begin, dim3(1), dim3(kNT), 0, s, k, m, static_cast<const double*>(ws.par),
                       static_cast<const BlzCol*>(nullptr), ws.st);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_crnb_solve, dim3(k), dim3(kNT), 0, s, ws.st, m, static_cast<const double*>(ws.al), m,
                       static_cast<const double*>(ws.be), mb, ws.s, m, eps, it_max);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_crnb_publish, dim3(1), dim3(kNT), 0, s, k, static_cast<const double*>(ws.st), ws.out);
    LAUNCHCHK();
    HIPCHK(hipMemcpyAsync(s_host, ws.s, size_t(k) * m * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int c = 0; c < k; ++c) {
      const CrnbCol col = host_record(h, c);
      info_host[c] = krcn_crn_info{};
      solver_fields(col, &info_host[c]);
    }
    return KRCN_OK;
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_cubic_tridiag_block: unexpected C++ exception");
  }
}

extern "C" krcn_status krcn_crn_step_block(krcn_csr* h, int k, const void* X, const void* b, int b_cols,
                                           const void* AX, const double* values_host, const int* active_host, int m,
                                           double tol, const double* l2_host, const double* reg_coef_host,
                                           double ls_beta, const double* r0_host, double solver_eps,
                                           int solver_it_max, int max_trials, void* V, void* X_new, void* AX_new,
                                           double* alphas_host, double* betas_host, krcn_crn_info* info_host,
                                           void* stream) {
  try {
    const char* fn = "krcn_crn_step_block";
    CHK(check_k(fn, k));
    if (m < 1 || m > kLzMaxM) return fail(KRCN_ERR_INVALID, "%s: m = %d outside [1, %d]", fn, m, kLzMaxM);
    CHK(check_b_cols(fn, k, b_cols));
    if (max_trials < 0) return fail(KRCN_ERR_INVALID, "%s: max_trials must be >= 0", fn);
    if (!(ls_beta > 0.0 && ls_beta < 1.0)) return fail(KRCN_ERR_INVALID, "%s: ls_beta must lie in (0, 1)", fn);
    if (solver_it_max < 1) return fail(KRCN_ERR_INVALID, "%s: solver_it_max must be >= 1", fn);
    CHK(check_handle(fn, h));
    if (!X || !b || !values_host || !reg_coef_host || !r0_host || !V || !X_new || !AX_new || !info_host)
      return fail(KRCN_ERR_INVALID, "%s: null argument", fn);
    if (h->n < 1 || h->d < 1 || h->nnz < 1) return fail(KRCN_ERR_INVALID, "%s: the matrix is empty", fn);
    if (X_new == X || AX_new == b || X_new == V || AX_new == X)
      return fail(KRCN_ERR_INVALID, "%s: X_new and AX_new must not alias the inputs", fn);
    CHK(set_device(h));
    const StepArgs a{values_host, l2_host, reg_coef_host, r0_host, active_host, tol, ls_beta, solver_eps,
                     m, b_cols, solver_it_max, max_trials};
    return h->dtype == KRCN_F64
               ? crn_step_block_impl<double>(h, k, static_cast<const double*>(X), static_cast<const double*>(b),
                                             static_cast<const double*>(AX), a, static_cast<double*>(V),
                                             static_cast<double*>(X_new), static_cast<double*>(AX_new), alphas_host,
                                             betas_host, info_host, S(stream))
               : crn_step_block_impl<float>(h, k, static_cast<const float*>(X), static_cast<const float*>(b),
                                            static_cast<const float*>(AX), a, static_cast<float*>(V),
                                            static_cast<float*>(X_new), static_cast<float*>(AX_new), alphas_host,
                                            betas_host, info_host, S(stream));
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_crn_step_block: unexpected C++ exception");
  }
}
