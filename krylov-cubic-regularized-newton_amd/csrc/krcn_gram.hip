// krcn_gram.hip — krcn_hessian_gram: the dense Hessian X^T diag(w) X / n + l2 I
// as one weighted Gram product over the dense image of X^T, on the fp64 matrix
// instruction (krcn_gram.hpp; geometry krcn_gram_geom.hpp).  Replaces hessian,
// optimizer/loss.py (reference loss.py:249-255).
#include "krcn_gram.hpp"
#include "krcn_internal.hpp"

namespace {

constexpr int64_t kGramMaxGrid = INT32_MAX;   // workgroups of one launch

krcn_status ensure_gram_ws(krcn_csr* h, int64_t bytes) {
  if (bytes <= int64_t(h->gram_ws_bytes)) return KRCN_OK;
  CHK(h->own.release(&h->gram_ws));
  h->gram_ws_bytes = 0;
  CHK(h->own.alloc(&h->gram_ws, size_t(bytes)));
  h->gram_ws_bytes = size_t(bytes);
  return KRCN_OK;
}

template <typename TS, typename TW>
krcn_status gram_launch(const GramArgs& g, const GramGeom& geo, const void* w, hipStream_t s) {
  hipLaunchKernelGGL((k_gram<TS, TW>), dim3(unsigned(geo.grid)), dim3(kGramNT), 0, s, g, static_cast<const TW*>(w));
  LAUNCHCHK();
  if (geo.split > 1) {
    hipLaunchKernelGGL(k_gram_reduce, dim3(unsigned(geo.tiles)), dim3(kGramNT), 0, s, g);
    LAUNCHCHK();
  }
  return KRCN_OK;
}

}  // namespace

extern "C" krcn_status krcn_gram_geometry(int64_t d, int64_t n, int split, int64_t* out_host) {
  if (!out_host) return fail(KRCN_ERR_INVALID, "krcn_gram_geometry: null argument");
  if (d < 0 || n < 0 || d > (int64_t(1) << 20) || n >= (int64_t(1) << 31))
    return fail(KRCN_ERR_INVALID, "krcn_gram_geometry: expected 0 <= d <= 2^20 and 0 <= n < 2^31");
  if (split < 0 || split > kGramMaxSplit)
    return fail(KRCN_ERR_INVALID, "krcn_gram_geometry: split must be 0 (auto) or 1..%d (got %d)", kGramMaxSplit, split);
  const GramGeom g = gram_geometry(d, n, split);
  const int64_t out[8] = {g.T, g.KS, g.nt, g.tiles, g.slabs, g.split, g.grid, g.ws_bytes};
  std::memcpy(out_host, out, sizeof(out));
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_set_gram_split(krcn_csr* h, int split) {
  if (split < 0 || split > kGramMaxSplit)   // (the scalar before the handle is looked at)
    return fail(KRCN_ERR_INVALID, "krcn_csr_set_gram_split: split must be 0 (auto) or 1..%d (got %d)", kGramMaxSplit,
                split);
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_csr_set_gram_split: null handle");
  h->gram_split = split;
  return KRCN_OK;
}

extern "C" krcn_status krcn_hessian_gram(krcn_csr* h, const void* w, double l2, double* H, void* stream) {
  try {
    if (!w) return fail(KRCN_ERR_INVALID, "krcn_hessian_gram: null w");
    if (!H) return fail(KRCN_ERR_INVALID, "krcn_hessian_gram: null H");
    if (!h) return fail(KRCN_ERR_INVALID, "krcn_hessian_gram: null handle");
    if (h->shard != KRCN_SHARD_NONE)
      return fail(KRCN_ERR_UNSUPPORTED, "krcn_hessian_gram: sharded handles are not supported");
    if (h->d == 0) return KRCN_OK;
    if (h->d > (int64_t(1) << 20))
      return fail(KRCN_ERR_UNSUPPORTED, "krcn_hessian_gram: d = %lld is above 2^20", (long long)h->d);
    CHK(set_device(h));
    CHK(plans_for_compute(h));   // before any plan pointer is read: a plan build may move them
    const PassPlan& P = h->p2;
    if (P.kind != KRCN_PLAN_DENSE)
      return fail(KRCN_ERR_UNSUPPORTED, "krcn_hessian_gram: pass 2 holds no dense image of X^T: call "
                  "krcn_csr_set_pass_format(h, 2, KRCN_FORMAT_DENSE) (pass 1 may keep any format)");
    hipStream_t s = S(stream);
    if (h->n == 0 || h->nnz == 0) {
      const int64_t blocks = std::min<int64_t>((h->d * h->d + kGramNT - 1) / kGramNT, 4096);
      hipLaunchKernelGGL(k_gram_l2, dim3(unsigned(blocks)), dim3(kGramNT), 0, s, h->d, l2, H);
      LAUNCHCHK();
      return KRCN_OK;
    }
    const GramGeom geo = gram_geometry(h->d, h->n, h->gram_split);
    if (geo.grid > kGramMaxGrid)
      return fail(KRCN_ERR_UNSUPPORTED, "krcn_hessian_gram: %lld tiles x split %d is more than one launch holds",
                  (long long)geo.tiles, geo.split);
    if (geo.ws_bytes) CHK(ensure_gram_ws(h, geo.ws_bytes));
    const GramArgs g{P.val, h->d, h->n, P.dld, geo.slabs, geo.split, double(h->n_global), l2, H, h->gram_ws};
    if (h->dtype == KRCN_F32) return gram_launch<float, float>(g, geo, w, s);
    return P.vbytes == 4 ? gram_launch<float, double>(g, geo, w, s) : gram_launch<double, double>(g, geo, w, s);
  } catch (...) {
    return fail(KRCN_ERR_INVALID, "krcn_hessian_gram: unexpected C++ exception");
  }
}
