// krcn_block.hip — block products: X V, X^T U / n and the block HVP for k
// vectors per pass over the matrix (kernels: krcn_block.hpp).
//
// Pass 1 walks the caller's CSR of X, pass 2 the handle's transposed CSR
// (h->tptr / tidx / tval, read at call time: the placement code may move
// buffers).  The calls need no pass plans and never build them; the block HVP
// keeps its (n, k) intermediate in a workspace of its own (h->blk_u, one block
// of the handle's owner table, grown when k grows), not in the handle's
// u / tn / W / td.  The first call that walks a matrix lists its rows of more
// than KRCN_BLOCK_LONG_ROW elements (krcn_block_rows.hpp: one copy of the row
// pointers to the host, once per handle and matrix); the list lives in the
// owner table too and is empty, without an allocation, for most matrices.
#include "krcn_internal.hpp"
#include "krcn_block.hpp"

using namespace krcn;

// Everything the three calls share, checked before any HIP call.
static krcn_status block_check(const char* fn, const krcn_csr* h, int k) {
  if (!h) return fail(KRCN_ERR_INVALID, "%s: null handle", fn);
  if (h->shard != KRCN_SHARD_NONE)
    return fail(KRCN_ERR_UNSUPPORTED, "%s: block products are implemented for unsharded handles", fn);
  if (k < 1 || k > KRCN_BLOCK_MAX)
    return fail(KRCN_ERR_INVALID, "%s: k = %d outside [1, %d]", fn, k, int(KRCN_BLOCK_MAX));
  return KRCN_OK;
}

static bool block_empty(const krcn_csr* h) { return h->n == 0 || h->nnz == 0; }

// The (n, k) intermediate of the block HVP for blocks of up to k vectors.
static krcn_status block_reserve(krcn_csr* h, int k, hipStream_t s) {
  if (h->blk_k >= k) return KRCN_OK;
  if (h->blk_u) {
    HIPCHK(hipStreamSynchronize(s));   // a block HVP still running reads the old buffer
    h->blk_k = 0;
    CHK(h->own.release(&h->blk_u));
  }
  CHK(h->own.alloc(&h->blk_u, size_t(h->n) * size_t(k) * h->vs));
  h->blk_k = k;
  return KRCN_OK;
}

// The long rows of one matrix (side 0: X, 1: X^T), listed at the first pass over it.
static krcn_status block_long_list(krcn_csr* h, int side, int64_t rows, const int* ptr, hipStream_t s) {
  if (h->blk_listed[side]) return KRCN_OK;
  std::vector<int32_t> hp(size_t(rows) + 1);
  HIPCHK(hipMemcpyAsync(hp.data(), ptr, hp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const std::vector<int32_t> lr = block_long_rows(hp.data(), rows, kBlockLongRow);
  if (!lr.empty()) {
    CHK(h->own.alloc(&h->blk_long[side], lr.size() * sizeof(int32_t)));
    HIPCHK(hipMemcpyAsync(h->blk_long[side], lr.data(), lr.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));   // lr leaves scope
  }
  h->blk_nlong[side] = int(lr.size());
  h->blk_listed[side] = true;
  return KRCN_OK;
}

template <typename T, int K, class Epi>
static void block_launch(int rows, const int* longrows, int nlong, const int* ptr, const int* idx, const T* val,
                         const T* V, int k, const Epi& epi, hipStream_t s) {
  hipLaunchKernelGGL((k_block_pass<T, K, Epi>), dim3(unsigned(block_grid(rows, K))), dim3(kBlockNT), 0, s, rows, ptr,
                     idx, val, V, k, epi);
  if (nlong)
    hipLaunchKernelGGL((k_block_long<T, K, Epi>), dim3(nlong), dim3(kBlockLongNT), 0, s, longrows, ptr, idx, val, V,
                       k, epi);
}

// One pass over a matrix of the handle (side 0: X's CSR, 1: X^T's) with the lane group of k.
template <typename T, class Epi>
static krcn_status block_pass(krcn_csr* h, int side, const T* V, int k, const Epi& epi, hipStream_t s) {
  const int64_t rows = side ? h->d : h->n;
  if (rows == 0) return KRCN_OK;
  const int* ptr = side ? h->tptr : h->ptr;
  const int* idx = side ? h->tidx : h->idx;
  const T* a = static_cast<const T*>(side ? h->tval : h->val);
  CHK(block_long_list(h, side, rows, ptr, s));
  const int* lr = h->blk_long[side];
  const int nl = h->blk_nlong[side], r = int(rows);
  switch (block_lanes(k)) {
    case 1: block_launch<T, 1>(r, lr, nl, ptr, idx, a, V, k, epi, s); break;
    case 2: block_launch<T, 2>(r, lr, nl, ptr, idx, a, V, k, epi, s); break;
    case 4: block_launch<T, 4>(r, lr, nl, ptr, idx, a, V, k, epi, s); break;
    case 8: block_launch<T, 8>(r, lr, nl, ptr, idx, a, V, k, epi, s); break;
    default: block_launch<T, 16>(r, lr, nl, ptr, idx, a, V, k, epi, s); break;
  }
  LAUNCHCHK();
  return KRCN_OK;
}

template <typename T>
static BlkHvpOut<T> hvp_out(const krcn_csr* h, int k, const T* V, T* Y, const double* l2_host) {
  BlkHvpOut<T> o{V, Y, T(h->n_global), {}};
  for (int j = 0; j < k; ++j) o.l2[j] = l2_host ? T(l2_host[j]) : T(0);
  return o;
}

// ------------------------------------------------------------------- X V
template <typename T>
static krcn_status matvec_block_impl(krcn_csr* h, int k, const T* V, T* Tn, hipStream_t s) {
  if (block_empty(h)) {
    HIPCHK(hipMemsetAsync(Tn, 0, size_t(h->n) * size_t(k) * sizeof(T), s));
    return KRCN_OK;
  }
  return block_pass<T>(h, 0, V, k, BlkStore<T>{Tn}, s);
}

extern "C" krcn_status krcn_matvec_block(krcn_csr* h, int k, const void* V, void* Tn, void* stream) {
  CHK(block_check("krcn_matvec_block", h, k));
  if ((!V && h->d) || (!Tn && h->n)) return fail(KRCN_ERR_INVALID, "krcn_matvec_block: null argument");
  if (h->n == 0) return KRCN_OK;
  CHK(set_device(h));
  return h->dtype == KRCN_F64
             ? matvec_block_impl<double>(h, k, static_cast<const double*>(V), static_cast<double*>(Tn), S(stream))
             : matvec_block_impl<float>(h, k, static_cast<const float*>(V), static_cast<float*>(Tn), S(stream));
}

// ------------------------------------------------------------ X^T U / n
template <typename T>
static krcn_status rmatvec_block_impl(krcn_csr* h, int k, const T* U, T* Y, hipStream_t s) {
  if (block_empty(h)) {
    HIPCHK(hipMemsetAsync(Y, 0, size_t(h->d) * size_t(k) * sizeof(T), s));
    return KRCN_OK;
  }
  return block_pass<T>(h, 1, U, k, hvp_out<T>(h, k, nullptr, Y, nullptr), s);
}

extern "C" krcn_status krcn_rmatvec_block(krcn_csr* h, int k, const void* U, void* Y, void* stream) {
  CHK(block_check("krcn_rmatvec_block", h, k));
  if ((!U && h->n) || (!Y && h->d)) return fail(KRCN_ERR_INVALID, "krcn_rmatvec_block: null argument");
  if (h->d == 0) return KRCN_OK;
  CHK(set_device(h));
  return h->dtype == KRCN_F64
             ? rmatvec_block_impl<double>(h, k, static_cast<const double*>(U), static_cast<double*>(Y), S(stream))
             : rmatvec_block_impl<float>(h, k, static_cast<const float*>(U), static_cast<float*>(Y), S(stream));
}

// ------------------------------- the batched Krylov-CRN step's passes
krcn_status block_rmatvec_l2(krcn_csr* h, int k, const void* U, const void* Xv, const double* l2_host, void* Y,
                             hipStream_t s) {
  auto run = [&](auto zero) -> krcn_status {
    using T = decltype(zero);
    const BlkHvpOut<T> out = hvp_out<T>(h, k, static_cast<const T*>(Xv), static_cast<T*>(Y), l2_host);
    if (block_empty(h)) {
      hipLaunchKernelGGL((k_block_l2v<T>), dim3(vec_grid(h->d * k)), dim3(kNT), 0, s, h->d, k, out);
      LAUNCHCHK();
      return KRCN_OK;
    }
    return block_pass<T>(h, 1, static_cast<const T*>(U), k, out, s);
  };
  return h->dtype == KRCN_F64 ? run(double(0)) : run(float(0));
}

krcn_status block_matvec_live(krcn_csr* h, int k, const void* V, void* Tn, const double* state, hipStream_t s) {
  const CrnbHead* head = reinterpret_cast<const CrnbHead*>(state);
  const CrnbCol* cols = reinterpret_cast<const CrnbCol*>(state + sizeof(CrnbHead) / sizeof(double));
  return h->dtype == KRCN_F64
             ? block_pass<double>(h, 0, static_cast<const double*>(V), k,
                                  BlkStoreLive<double>{static_cast<double*>(Tn), head, cols}, s)
             : block_pass<float>(h, 0, static_cast<const float*>(V), k,
                                 BlkStoreLive<float>{static_cast<float*>(Tn), head, cols}, s);
}

// ------------------------------------------------------------- block HVP
template <typename T>
static krcn_status hvp_block_impl(krcn_csr* h, int k, const T* w, int w_cols, const T* V, T* Y,
                                  const double* l2_host, hipStream_t s) {
  const BlkHvpOut<T> out = hvp_out<T>(h, k, V, Y, l2_host);
  if (block_empty(h)) {
    hipLaunchKernelGGL((k_block_l2v<T>), dim3(vec_grid(h->d * k)), dim3(kNT), 0, s, h->d, k, out);
    LAUNCHCHK();
    return KRCN_OK;
  }
  CHK(block_reserve(h, k, s));
  T* u = static_cast<T*>(h->blk_u);
  CHK(block_pass<T>(h, 0, V, k, BlkWeighted<T>{w, u, w_cols == 1 ? 0 : k}, s));
  return block_pass<T>(h, 1, static_cast<const T*>(u), k, out, s);
}

extern "C" krcn_status krcn_hvp_block(krcn_csr* h, int k, const void* w, int w_cols, const void* V, void* Y,
                                      const double* l2_host, void* stream) {
  CHK(block_check("krcn_hvp_block", h, k));
  if (w_cols != 1 && w_cols != k)
    return fail(KRCN_ERR_INVALID, "krcn_hvp_block: w_cols = %d is neither 1 nor k = %d", w_cols, k);
  if ((!w && h->n) || (h->d && (!V || !Y))) return fail(KRCN_ERR_INVALID, "krcn_hvp_block: null argument");
  if (h->d == 0) return KRCN_OK;
  CHK(set_device(h));
  return h->dtype == KRCN_F64
             ? hvp_block_impl<double>(h, k, static_cast<const double*>(w), w_cols, static_cast<const double*>(V),
                                      static_cast<double*>(Y), l2_host, S(stream))
             : hvp_block_impl<float>(h, k, static_cast<const float*>(w), w_cols, static_cast<const float*>(V),
                                     static_cast<float*>(Y), l2_host, S(stream));
}
