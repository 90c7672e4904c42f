// krcn_cubic_cg.hip — krcn_cubic_cg: the cubic subproblem of the full-space CRN
// behind one call, scipy's scalar Newton on phi(lam) with every (H + lam I)^{-1}
// applied by krcn_cg_solve's conjugate gradients, control on the device
// (krcn_cgn.hpp, krcn_cgn_state.hpp).  Replaces the root_scalar loop of
// Cubic_LS.cubic_solver_root_CG, optimizer/cubic.py (reference cubic.py:152-182).
#include "krcn_cgn.hpp"
#include "krcn_internal.hpp"

namespace {

constexpr size_t kCgnStateDoubles = sizeof(CgnState) / sizeof(double);
static_assert((kCgnStateDoubles + 2 * size_t(kCgnMaxGrid)) * sizeof(double) == 16512, "the header states the size");

// Ticks per submission: the host synchronises and reads the mapped record
// once per batch (A/B knob KRCN_CGN_BATCH).
int cgn_batch() {
  static const int v = [] {
    const int x = tuning_value("KRCN_CGN_BATCH", 16);
    return x >= 1 && x <= 4096 ? x : 16;
  }();
  return v;
}

krcn_status ensure_cgn_ws(krcn_csr* h) {
  CHK(ensure_cg_ws(h));
  if (!h->cgn_z) CHK(h->own.alloc(&h->cgn_z, std::max<size_t>(size_t(h->d) * h->vs, 1)));
  if (!h->cgn_st) CHK(dalloc(h, &h->cgn_st, kCgnStateDoubles + 2 * size_t(kCgnMaxGrid)));
  if (!h->cgn_res) {
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->cgn_res), sizeof(CgnState),
                         hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(h->cgn_res, 0, sizeof(CgnState));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->cgn_res_dev), h->cgn_res, 0));
  }
  return KRCN_OK;
}

template <typename T>
krcn_status cubic_cg_impl(krcn_csr* h, const T* w, const T* g, const CgnParams& a, T* sv, krcn_cubic_cg_info* info,
                          hipStream_t s) {
  const int64_t d = h->d;
  CHK(plans_for_compute(h));   // before any scratch pointer is read: a plan build may move them
  CHK(ensure_cgn_ws(h));
  T* r = static_cast<T*>(h->cg_r);
  T* p = r + d;
  T* q = p + d;
  T* z = static_cast<T*>(h->cgn_z);
  T* u = static_cast<T*>(h->u);
  CgnState* st = reinterpret_cast<CgnState*>(h->cgn_st);
  double* pt = h->cgn_st + kCgnStateDoubles;
  CgnState* res = reinterpret_cast<CgnState*>(h->cgn_res_dev);
  const LanczosState* guard = reinterpret_cast<const LanczosState*>(st);
  const int P = vec_grid(d);
  static_assert(kCgnMaxGrid >= 1024, "vec_grid's cap");
  std::memset(h->cgn_res, 0, sizeof(CgnState));   // (the previous call's chain has been synchronised on)
  hipLaunchKernelGGL((k_cg_begin<T>), dim3(P), dim3(kNT), 0, s, d, g, sv, r, p, h->pb);
  LAUNCHCHK();
  hipLaunchKernelGGL(k_cgn_init, dim3(1), dim3(kNT), 0, s, static_cast<const double*>(h->pb), P, a, st);
  LAUNCHCHK();
  const T tn = T(h->n_global);
  auto tick = [&]() -> krcn_status {
    CHK(run_pass<T>(h->p1, SrcGuard<T>{p, guard, 0}, SrcGuard<T>{p, guard, 0}, EpiWeighted<T>{w, u}, nullptr,
                    nullptr, s));
    int Pq = 0;
    CHK(run_pass<T>(h->p2, SrcGuard<T>{u, guard, 0}, SrcGuard<T>{u, guard, 0}, EpiCgnQ<T>{p, q, tn, st, T(0)}, h->pa,
                    &Pq, s));
    hipLaunchKernelGGL((k_cgn_update<T>), dim3(P), dim3(kNT), 0, s, d, static_cast<const double*>(h->pa), Pq, st, sv, z,
                       r, static_cast<const T*>(p), static_cast<const T*>(q), h->pb);
    LAUNCHCHK();
    hipLaunchKernelGGL((k_cgn_dir<T>), dim3(P), dim3(kNT), 0, s, d, a.cg_maxiter, static_cast<const double*>(h->pb), P,
                       static_cast<const CgnState*>(st), g, sv, z, r, p, pt);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_cgn_turn, dim3(1), dim3(kNT), 0, s, a, static_cast<const double*>(h->pb), P,
                       static_cast<const double*>(pt), st, res);
    LAUNCHCHK();
    return KRCN_OK;
  };
  CgnState hs{};
  const int64_t total = cgn_tick_bound(a.it_max, a.cg_maxiter);
  int64_t enq = 0;
  while (enq < total && !hs.done) {
    const int64_t batch = std::min<int64_t>(cgn_batch(), total - enq);
    for (int64_t t = 0; t < batch; ++t) CHK(tick());
    enq += batch;
    HIPCHK(hipStreamSynchronize(s));
    std::memcpy(&hs, h->cgn_res, sizeof(CgnState));
  }
  if (!hs.done)
    return fail(KRCN_ERR_HIP, "krcn_cubic_cg: the chain did not end after %lld ticks", (long long)total);
  info->solver_it = hs.solver_it;
  info->solver_status = hs.solver_status;
  info->cg_solves = hs.cg_solves;
  info->cg_unconverged = hs.cg_unconverged;
  info->cg_iterations = hs.cg_iterations;
  info->ticks = enq;
  info->reg_coef = a.M;
  info->lam = hs.lam;
  info->model_decrease = hs.model_decrease;
  info->s_norm = hs.s_norm;
  return KRCN_OK;
}

}  // namespace

extern "C" krcn_status krcn_cubic_cg(krcn_csr* h, const void* w, const void* g, double l2, double M, double r0,
                                     double eps, int it_max, double cg_rtol, int cg_maxiter, void* s,
                                     krcn_cubic_cg_info* info_host, void* stream) {
  try {
    if (it_max < 1) return fail(KRCN_ERR_INVALID, "krcn_cubic_cg: it_max must be >= 1");
    if (!(cg_rtol >= 0.0)) return fail(KRCN_ERR_INVALID, "krcn_cubic_cg: cg_rtol must be >= 0");
    if (!(M > 0.0) || !std::isfinite(M)) return fail(KRCN_ERR_INVALID, "krcn_cubic_cg: M must be positive and finite");
    if (!(eps >= 0.0)) return fail(KRCN_ERR_INVALID, "krcn_cubic_cg: eps must be >= 0");
    if (!h) return fail(KRCN_ERR_INVALID, "krcn_cubic_cg: null handle");
    if (!g || !s || !info_host || (h->n && !w)) return fail(KRCN_ERR_INVALID, "krcn_cubic_cg: null argument");
    if (s == g) return fail(KRCN_ERR_INVALID, "krcn_cubic_cg: s must not alias g");
    if (h->shard != KRCN_SHARD_NONE)
      return fail(KRCN_ERR_UNSUPPORTED, "krcn_cubic_cg: sharded handles are not supported");
    *info_host = krcn_cubic_cg_info{};
    if (h->d == 0) return KRCN_OK;
    CHK(set_device(h));
    const int64_t auto_it = 10 * h->d;
    const int maxiter = cg_maxiter > 0 ? cg_maxiter : int(std::min<int64_t>(auto_it, INT32_MAX - 1));
    const CgnParams a{M, l2, r0, eps, cg_rtol, it_max, maxiter};
    return h->dtype == KRCN_F64
               ? cubic_cg_impl<double>(h, static_cast<const double*>(w), static_cast<const double*>(g), a,
                                       static_cast<double*>(s), info_host, S(stream))
               : cubic_cg_impl<float>(h, static_cast<const float*>(w), static_cast<const float*>(g), a,
                                      static_cast<float*>(s), info_host, S(stream));
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_cubic_cg: unexpected C++ exception");
  }
}
