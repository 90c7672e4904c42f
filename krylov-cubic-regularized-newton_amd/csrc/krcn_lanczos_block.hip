// krcn_lanczos_block.hip — the batched Lanczos: k independent recurrences of
// cubic.py:77-111 in lockstep over the block HVP, with the block forms of
// krcn_basis_combine and krcn_weights (kernels: krcn_blz.hpp; the per-column
// state rule: krcn_blz_state.hpp).
//
// One call enqueues, for m basis vectors,
//   k_blz_begin, k_blz_norm                          V[0] = G / ||g||, per column
//   m - 1 times: krcn_hvp_block(V[j] -> Y), k_blz_dots, k_blz_form, k_blz_norm
//   k_blz_pick, krcn_hvp_block(operand -> Y), k_blz_dots, k_blz_finish
// and synchronises once, after k_blz_finish has written the results block to
// mapped host memory.  The host reads nothing in between: which columns have
// broken down is known to the kernels alone, and a broken column's launches
// leave its bytes alone.  The call builds no pass plans and keeps its blocks
// (Y, the final operand, the partials, the results) in the handle's owner
// table, apart from u / tn / W / td and the single-vector results block.
#include "krcn_internal.hpp"
#include "krcn_blz.hpp"

using namespace krcn;

static size_t blz_res_doubles(int k, int m) { return size_t(k) * (4 + size_t(m) + size_t(m > 1 ? m - 1 : 1)); }

// The workspace for k columns and m vectors: allocates only when k, or the
// results block k (2 m + 3), grows.
static krcn_status blz_reserve(krcn_csr* h, int k, int m, hipStream_t s) {
  if (!h->blz_pa) CHK(dalloc(h, &h->blz_pa, size_t(3) * kBlzMaxGrid * KRCN_BLOCK_MAX));
  if (k > h->blz_k) {
    if (h->blz_y) {
      HIPCHK(hipStreamSynchronize(s));   // an earlier call's launches may still use the old blocks
      h->blz_k = 0;
      CHK(h->own.release(&h->blz_y));
      CHK(h->own.release(&h->blz_op));
    }
    const size_t bytes = std::max<size_t>(size_t(h->d) * size_t(k) * h->vs, 16);
    CHK(h->own.alloc(&h->blz_y, bytes));
    CHK(h->own.alloc(&h->blz_op, bytes));
    h->blz_k = k;
  }
  const size_t need = blz_res_doubles(k, m);
  if (need > h->blz_res_cap) {
    if (h->blz_res) {
      HIPCHK(hipStreamSynchronize(s));
      h->blz_res_cap = 0;
      CHK(h->own.release(&h->blz_res));
      (void)hipHostFree(h->blz_host);
      h->blz_host = nullptr;
    }
    CHK(dalloc(h, &h->blz_res, need));
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->blz_host), need * sizeof(double),
                         hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->blz_host_dev), h->blz_host, 0));
    h->blz_res_cap = need;
  }
  return KRCN_OK;
}

template <int K> struct BlzLaneC { static constexpr int value = K; };
// f(BlzLaneC<K>) for the lane group of k columns
template <class F>
static void blz_lanes(int k, F&& f) {
  switch (block_lanes(k)) {
    case 1: f(BlzLaneC<1>{}); break;
    case 2: f(BlzLaneC<2>{}); break;
    case 4: f(BlzLaneC<4>{}); break;
    case 8: f(BlzLaneC<8>{}); break;
    default: f(BlzLaneC<16>{}); break;
  }
}

// The launches of one call (the sequence above), without the synchronisation.
template <typename T>
static krcn_status blz_enqueue(krcn_csr* h, int k, const T* w, int w_cols, const T* Gm, int m, double tol,
                               const double* l2_host, T* V, hipStream_t s) {
  const int64_t d = h->d;
  CHK(blz_reserve(h, k, m, s));
  T* Y = static_cast<T*>(h->blz_y);
  T* op = static_cast<T*>(h->blz_op);
  double* pa = h->blz_pa;
  double* pn = h->blz_pa + size_t(2) * kBlzMaxGrid * KRCN_BLOCK_MAX;
  double* res = h->blz_res;
  BlzCol* st = reinterpret_cast<BlzCol*>(res);
  double* alphas = res + 4 * k;
  double* betas = alphas + size_t(k) * m;
  const int nres = int(blz_res_doubles(k, m));
  const int64_t slab = d * k;
  const int K = block_lanes(k);
  const int P = blz_grid(d, K);
  const dim3 grid(P), one(1), nt(kNT);

  blz_lanes(k, [&](auto lc) {
    constexpr int KK = decltype(lc)::value;
    hipLaunchKernelGGL((k_blz_begin<T, KK>), grid, nt, 0, s, d, k, m, Gm, alphas, betas, pn);
    hipLaunchKernelGGL((k_blz_norm<T, KK>), grid, nt, 0, s, d, k, m, -1, Gm, V, static_cast<const double*>(pn), P, tol,
                       st, betas);
  });
  LAUNCHCHK();
  for (int j = 0; j + 1 < m; ++j) {
    const T* vj = V + int64_t(j) * slab;
    const T* vp = j > 0 ? V + int64_t(j - 1) * slab : nullptr;
    T* zn = V + int64_t(j + 1) * slab;
    CHK(krcn_hvp_block(h, k, w, w_cols, vj, Y, l2_host, s));
    blz_lanes(k, [&](auto lc) {
      constexpr int KK = decltype(lc)::value;
      hipLaunchKernelGGL((k_blz_dots<T, KK>), grid, nt, 0, s, d, k, vj, vp, static_cast<const T*>(Y), pa);
      hipLaunchKernelGGL((k_blz_form<T, KK>), grid, nt, 0, s, d, k, m, j, vj, vp, static_cast<const T*>(Y), zn,
                         static_cast<const double*>(pa), P, static_cast<const BlzCol*>(st),
                         static_cast<const double*>(betas), alphas, pn);
      hipLaunchKernelGGL((k_blz_norm<T, KK>), grid, nt, 0, s, d, k, m, j, static_cast<const T*>(zn), zn,
                         static_cast<const double*>(pn), P, tol, st, betas);
    });
    LAUNCHCHK();
  }
  blz_lanes(k, [&](auto lc) {
    constexpr int KK = decltype(lc)::value;
    hipLaunchKernelGGL((k_blz_pick<T, KK>), grid, nt, 0, s, d, k, m, static_cast<const T*>(V),
                       static_cast<const BlzCol*>(st), op);
  });
  LAUNCHCHK();
  CHK(krcn_hvp_block(h, k, w, w_cols, op, Y, l2_host, s));
  blz_lanes(k, [&](auto lc) {
    constexpr int KK = decltype(lc)::value;
    hipLaunchKernelGGL((k_blz_dots<T, KK>), grid, nt, 0, s, d, k, static_cast<const T*>(op),
                       static_cast<const T*>(nullptr), static_cast<const T*>(Y), pa);
    hipLaunchKernelGGL((k_blz_finish<KK>), one, nt, 0, s, k, m, static_cast<const double*>(pa), P, res, nres,
                       h->blz_host_dev);
  });
  LAUNCHCHK();
  return KRCN_OK;
}

krcn_status lanczos_block_enqueue(krcn_csr* h, int k, const void* w, int w_cols, const void* G, int m, double tol,
                                  const double* l2_host, void* V, hipStream_t s) {
  return h->dtype == KRCN_F64
             ? blz_enqueue<double>(h, k, static_cast<const double*>(w), w_cols, static_cast<const double*>(G), m, tol,
                                   l2_host, static_cast<double*>(V), s)
             : blz_enqueue<float>(h, k, static_cast<const float*>(w), w_cols, static_cast<const float*>(G), m, tol,
                                  l2_host, static_cast<float*>(V), s);
}

void lanczos_block_results(const krcn_csr* h, int k, int m, double* alphas_host, double* betas_host,
                           krcn_lanczos_info* info) {
  const int mb = m > 1 ? m - 1 : 1;
  const double* hb = h->blz_host;
  for (int c = 0; c < k; ++c) {
    BlzCol col;
    std::memcpy(&col, hb + 4 * c, sizeof(BlzCol));
    const int jb = col.j_break;
    const int m_eff = blz_m_eff(jb, m);
    const double* al = hb + 4 * k + size_t(c) * m;
    const double* be = hb + 4 * k + size_t(k) * m + size_t(c) * mb;
    if (alphas_host)
      for (int i = 0; i < m; ++i) alphas_host[size_t(c) * m + i] = i < m_eff ? al[i] : 0.0;
    if (betas_host)
      for (int i = 0; i < mb; ++i) betas_host[size_t(c) * mb + i] = (i + 1 < m && i < m_eff - 1) ? be[i] : 0.0;
    info[c].m_eff = m_eff;
    info[c].breakdown = jb >= 0;
    info[c].j_break = jb >= 0 ? jb : -1;
    info[c].hvps = blz_hvps(jb, m);
    info[c].beta_last = col.beta_last;
    info[c].gnorm = col.gnorm;
  }
}

extern "C" krcn_status krcn_lanczos_block(krcn_csr* h, int k, const void* w, int w_cols, const void* G, int m,
                                          double tol, const double* l2_host, void* V, double* alphas_host,
                                          double* betas_host, krcn_lanczos_info* info_host, void* stream) {
  if (k < 1 || k > KRCN_BLOCK_MAX)
    return fail(KRCN_ERR_INVALID, "krcn_lanczos_block: k = %d outside [1, %d]", k, int(KRCN_BLOCK_MAX));
  if (m < 1 || m > kLzMaxM) return fail(KRCN_ERR_INVALID, "krcn_lanczos_block: m = %d outside [1, %d]", m, kLzMaxM);
  if (w_cols != 1 && w_cols != k)
    return fail(KRCN_ERR_INVALID, "krcn_lanczos_block: w_cols = %d is neither 1 nor k = %d", w_cols, k);
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_lanczos_block: null handle");
  if (!w || !G || !V || !alphas_host || !betas_host || !info_host)
    return fail(KRCN_ERR_INVALID, "krcn_lanczos_block: null argument");
  if (h->shard != KRCN_SHARD_NONE)
    return fail(KRCN_ERR_UNSUPPORTED, "krcn_lanczos_block: implemented for unsharded handles");
  CHK(set_device(h));
  CHK(lanczos_block_enqueue(h, k, w, w_cols, G, m, tol, l2_host, V, S(stream)));
  HIPCHK(hipStreamSynchronize(S(stream)));   // the call's one synchronisation
  lanczos_block_results(h, k, m, alphas_host, betas_host, info_host);
  return KRCN_OK;
}

extern "C" krcn_status krcn_basis_combine_block(krcn_csr* h, int k, int m, const void* V, const double* s_host,
                                                const void* X0, void* Xnew, void* stream) {
  if (k < 1 || k > KRCN_BLOCK_MAX)
    return fail(KRCN_ERR_INVALID, "krcn_basis_combine_block: k = %d outside [1, %d]", k, int(KRCN_BLOCK_MAX));
  if (m < 1 || m > kLzMaxM)
    return fail(KRCN_ERR_INVALID, "krcn_basis_combine_block: m = %d outside [1, %d]", m, kLzMaxM);
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_basis_combine_block: null handle");
  if (!V || !s_host || !X0 || !Xnew) return fail(KRCN_ERR_INVALID, "krcn_basis_combine_block: null argument");
  if (h->shard != KRCN_SHARD_NONE)
    return fail(KRCN_ERR_UNSUPPORTED, "krcn_basis_combine_block: implemented for unsharded handles");
  CHK(set_device(h));
  hipStream_t s = S(stream);
  const size_t ns = size_t(m) * size_t(k);
  if (ns > h->blz_s_cap) {
    if (h->blz_s) {
      HIPCHK(hipStreamSynchronize(s));
      h->blz_s_cap = 0;
      CHK(h->own.release(&h->blz_s));
    }
    CHK(dalloc(h, &h->blz_s, ns));
    h->blz_s_cap = ns;
  }
  // (a pageable H2D copy is staged before the call returns: s_host may be reused)
  HIPCHK(hipMemcpyAsync(h->blz_s, s_host, ns * sizeof(double), hipMemcpyHostToDevice, s));
  const int64_t len = h->d * k;
  if (len == 0) return KRCN_OK;
  if (h->dtype == KRCN_F64)
    hipLaunchKernelGGL((k_blz_combine<double>), dim3(vec_grid(len)), dim3(kNT), 0, s, len, k, m,
                       static_cast<const double*>(V), static_cast<const double*>(h->blz_s),
                       static_cast<const double*>(X0), static_cast<double*>(Xnew));
  else
    hipLaunchKernelGGL((k_blz_combine<float>), dim3(vec_grid(len)), dim3(kNT), 0, s, len, k, m,
                       static_cast<const float*>(V), static_cast<const double*>(h->blz_s),
                       static_cast<const float*>(X0), static_cast<float*>(Xnew));
  LAUNCHCHK();
  return KRCN_OK;
}

// The weights formula is elementwise: k_weights over the n k entries of the block.
extern "C" krcn_status krcn_weights_block(krcn_csr* h, int k, const void* AX, void* W, void* stream) {
  if (k < 1 || k > KRCN_BLOCK_MAX)
    return fail(KRCN_ERR_INVALID, "krcn_weights_block: k = %d outside [1, %d]", k, int(KRCN_BLOCK_MAX));
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_weights_block: null handle");
  if (!AX || !W) return fail(KRCN_ERR_INVALID, "krcn_weights_block: null argument");
  if (h->shard != KRCN_SHARD_NONE)
    return fail(KRCN_ERR_UNSUPPORTED, "krcn_weights_block: implemented for unsharded handles");
  CHK(set_device(h));
  const int64_t len = h->n * k;
  if (len == 0) return KRCN_OK;
  if (h->dtype == KRCN_F64)
    hipLaunchKernelGGL((k_weights<double>), dim3(vec_grid(len)), dim3(kNT), 0, S(stream), len,
                       static_cast<const double*>(AX), static_cast<double*>(W));
  else
    hipLaunchKernelGGL((k_weights<float>), dim3(vec_grid(len)), dim3(kNT), 0, S(stream), len,
                       static_cast<const float*>(AX), static_cast<float*>(W));
  LAUNCHCHK();
  return KRCN_OK;
}
