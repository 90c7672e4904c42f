// krcn_coord.hip — coordinate blocks (SSCN): the gradient, the Hessian block and
// the Ax update over k selected columns of X (kernels: krcn_coord.hpp).
//
// The entry points validate the selection on the host before anything is
// launched, read h->tptr / tidx / tval at call time (never cached: the
// placement code may move buffers), need no pass plans and use a workspace of
// their own (CoordWs, krcn_coord_ws.hpp), not the handle's u / tn / W / td.
#include "krcn_internal.hpp"
#include "krcn_coord.hpp"
#include "krcn_coord_ws.hpp"

using namespace krcn;

static void coord_release(krcn_csr* h) {
  CoordWs* w = h->cw;
  if (!w) return;
  (void)h->own.release(&w->dev);
  if (w->pin) (void)hipHostFree(w->pin);
  for (hipEvent_t e : w->ev)
    if (e) (void)hipEventDestroy(e);
  delete w;
  h->cw = nullptr;
}

void coord_free(krcn_csr* h) { coord_release(h); }

krcn_status coord_reserve(krcn_csr* h, int k, hipStream_t s) {
  if (h->cw && h->cw->cap >= k) return KRCN_OK;
  const int cap = (k + 63) / 64 * 64;
  if (h->cw) {
    HIPCHK(hipStreamSynchronize(s));   // an update still running reads the old buffers
    coord_release(h);
  }
  CoordWs* w = new CoordWs();
  h->cw = w;
  CHK(h->own.alloc(&w->dev, coord_slot_bytes(cap) + size_t(cap) * size_t(cap) * sizeof(double)));
  w->delta = reinterpret_cast<double*>(w->dev);
  w->cols = reinterpret_cast<int*>(w->dev + size_t(cap) * 8);
  w->res = reinterpret_cast<double*>(w->dev + coord_slot_bytes(cap));
  const size_t res_bytes = size_t(cap) * size_t(cap) * sizeof(double);
  HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&w->pin), res_bytes + kCoordSlots * coord_slot_bytes(cap), 0));
  w->res_host = reinterpret_cast<double*>(w->pin);
  for (int i = 0; i < kCoordSlots; ++i) {
    w->slot[i] = w->pin + res_bytes + size_t(i) * coord_slot_bytes(cap);
    HIPCHK(hipEventCreateWithFlags(&w->ev[i], hipEventDisableTiming));
  }
  w->cap = cap;   // (last: a failed build leaves cap = 0 and is rebuilt by the next call)
  return KRCN_OK;
}

krcn_status coord_stage_bytes(krcn_csr* h, const void* src, size_t bytes, void* dst, hipStream_t s) {
  CoordWs* w = h->cw;
  if (!w || bytes > coord_slot_bytes(w->cap))
    return fail(KRCN_ERR_INVALID, "coord_stage_bytes: %zu bytes do not fit a staging slot of %zu", bytes,
                w ? coord_slot_bytes(w->cap) : size_t(0));
  const int i = w->next;
  if (w->busy[i]) HIPCHK(hipEventSynchronize(w->ev[i]));
  std::memcpy(w->slot[i], src, bytes);
  HIPCHK(hipMemcpyAsync(dst, w->slot[i], bytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(w->ev[i], s));
  w->busy[i] = true;
  w->next = (i + 1) % kCoordSlots;
  return KRCN_OK;
}

// cols_host (and delta_host, if given) to the device through the next ring slot.
static krcn_status coord_stage(krcn_csr* h, int k, const int32_t* cols_host, const double* delta_host,
                               hipStream_t s) {
  CoordWs* w = h->cw;
  const int i = w->next;
  if (w->busy[i]) HIPCHK(hipEventSynchronize(w->ev[i]));
  char* p = w->slot[i];
  const size_t off = size_t(w->cap) * 8;
  std::memcpy(p + off, cols_host, size_t(k) * sizeof(int32_t));
  if (delta_host) {
    std::memcpy(p, delta_host, size_t(k) * sizeof(double));
    HIPCHK(hipMemcpyAsync(w->dev, p, off + size_t(k) * sizeof(int32_t), hipMemcpyHostToDevice, s));
  } else {
    HIPCHK(hipMemcpyAsync(w->cols, p + off, size_t(k) * sizeof(int32_t), hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipEventRecord(w->ev[i], s));
  w->busy[i] = true;
  w->next = (i + 1) % kCoordSlots;
  return KRCN_OK;
}

// Everything a selection must satisfy, checked before any HIP call.
static krcn_status coord_check(const char* fn, const krcn_csr* h, int k, const int32_t* cols_host) {
  if (!h) return fail(KRCN_ERR_INVALID, "%s: null handle", fn);
  if (h->shard != KRCN_SHARD_NONE)
    return fail(KRCN_ERR_UNSUPPORTED, "%s: coordinate blocks are implemented for unsharded handles", fn);
  if (k < 1 || k > KRCN_COORD_MAX)
    return fail(KRCN_ERR_INVALID, "%s: k = %d outside [1, %d]", fn, k, int(KRCN_COORD_MAX));
  if (!cols_host) return fail(KRCN_ERR_INVALID, "%s: cols_host is null", fn);
  for (int a = 0; a < k; ++a)
    if (cols_host[a] < 0 || int64_t(cols_host[a]) >= h->d)
      return fail(KRCN_ERR_INVALID, "%s: cols_host[%d] = %d outside [0, %lld)", fn, a, int(cols_host[a]),
                  (long long)h->d);
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_set_coord_window(krcn_csr* h, int rows) {
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_csr_set_coord_window: null handle");
  if (rows < 0 || rows % 64 != 0)
    return fail(KRCN_ERR_INVALID, "krcn_csr_set_coord_window: rows must be 0 (auto) or a multiple of 64 (got %d)", rows);
  h->coord_window = rows;
  return KRCN_OK;
}

// ------------------------------------------------------------------ gradient
template <typename T>
static krcn_status coord_gradient_impl(krcn_csr* h, int k, const int32_t* cols_host, const T* Ax, const T* b,
                                       const T* x, double l2, double* g_host, hipStream_t s) {
  CHK(coord_reserve(h, k, s));
  CHK(coord_stage(h, k, cols_host, nullptr, s));
  CoordWs* w = h->cw;
  if (coord_empty(h)) {
    hipLaunchKernelGGL((k_coord_l2x<T>), dim3((k + kNT - 1) / kNT), dim3(kNT), 0, s, k, w->cols, x, l2, w->res);
  } else {
    hipLaunchKernelGGL((k_coord_grad<T>), dim3(k), dim3(kCoordGradNT), 0, s, w->cols, h->tptr,
                       h->tidx, static_cast<const T*>(h->tval), Ax, b, x, double(h->n_global), l2,
                       int(l2 != 0.0), w->res);
  }
  LAUNCHCHK();
  HIPCHK(hipMemcpyAsync(w->res_host, w->res, size_t(k) * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::memcpy(g_host, w->res_host, size_t(k) * sizeof(double));
  return KRCN_OK;
}

extern "C" krcn_status krcn_coord_gradient(krcn_csr* h, int k, const int32_t* cols_host, const void* Ax,
                                           const void* b, const void* x, double l2, double* g_host,
                                           void* stream) {
  CHK(coord_check("krcn_coord_gradient", h, k, cols_host));
  if (!g_host || (!coord_empty(h) && (!Ax || !b)) || (l2 != 0.0 && !x))
    return fail(KRCN_ERR_INVALID, "krcn_coord_gradient: null argument");
  if (coord_empty(h) && l2 == 0.0) {
    std::fill(g_host, g_host + k, 0.0);
    return KRCN_OK;
  }
  CHK(set_device(h));
  return h->dtype == KRCN_F64
             ? coord_gradient_impl<double>(h, k, cols_host, static_cast<const double*>(Ax),
                                           static_cast<const double*>(b), static_cast<const double*>(x), l2,
                                           g_host, S(stream))
             : coord_gradient_impl<float>(h, k, cols_host, static_cast<const float*>(Ax),
                                          static_cast<const float*>(b), static_cast<const float*>(x), l2, g_host,
                                          S(stream));
}

// ------------------------------------------------------------------- Hessian
// The kernel works on the ku distinct columns (ascending); position a of the
// selection maps to distinct column ua[a].  H[a][b] = Hu[ua[a]][ua[b]], with
// l2 on the diagonal a == b alone (the reference's l2 * eye(k)): rows of a
// repeated index carry the same sums, and H is symmetric because Hu is
// written as mirrored pairs.
template <typename T>
static krcn_status coord_hessian_impl(krcn_csr* h, int k, const std::vector<int32_t>& ucols,
                                      const std::vector<int>& ua, const T* Ax, double l2, double* H_host,
                                      hipStream_t s) {
  const int ku = int(ucols.size());
  CHK(coord_reserve(h, ku, s));
  CHK(coord_stage(h, ku, ucols.data(), nullptr, s));
  CoordWs* w = h->cw;
  const int R = h->coord_window ? std::min(h->coord_window, kCoordWinMax) : kCoordWinMax;
  hipLaunchKernelGGL((k_coord_hess<T>), dim3(ku), dim3(kCoordHessNT), 0, s, int(h->n), R, ku, w->cols, h->tptr,
                     h->tidx, static_cast<const T*>(h->tval), Ax, double(h->n_global), w->res);
  LAUNCHCHK();
  HIPCHK(hipMemcpyAsync(w->res_host, w->res, size_t(ku) * size_t(ku) * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (int a = 0; a < k; ++a) {
    const double* row = w->res_host + size_t(ua[size_t(a)]) * ku;
    double* out = H_host + size_t(a) * k;
    for (int c = 0; c < k; ++c) out[c] = row[ua[size_t(c)]];
    if (l2 != 0.0) out[a] = out[a] + l2;
  }
  return KRCN_OK;
}

extern "C" krcn_status krcn_coord_hessian(krcn_csr* h, int k, const int32_t* cols_host, const void* Ax,
                                          double l2, double* H_host, void* stream) {
  CHK(coord_check("krcn_coord_hessian", h, k, cols_host));
  if (!H_host || (!coord_empty(h) && !Ax)) return fail(KRCN_ERR_INVALID, "krcn_coord_hessian: null argument");
  if (coord_empty(h)) {
    std::fill(H_host, H_host + size_t(k) * size_t(k), 0.0);
    for (int a = 0; a < k; ++a) H_host[size_t(a) * k + a] = l2;
    return KRCN_OK;
  }
  std::vector<int32_t> ucols(cols_host, cols_host + k);
  std::sort(ucols.begin(), ucols.end());
  ucols.erase(std::unique(ucols.begin(), ucols.end()), ucols.end());
  std::vector<int> ua(size_t(k), 0);
  for (int a = 0; a < k; ++a)
    ua[size_t(a)] = int(std::lower_bound(ucols.begin(), ucols.end(), cols_host[a]) - ucols.begin());
  CHK(set_device(h));
  return h->dtype == KRCN_F64
             ? coord_hessian_impl<double>(h, k, ucols, ua, static_cast<const double*>(Ax), l2, H_host, S(stream))
             : coord_hessian_impl<float>(h, k, ucols, ua, static_cast<const float*>(Ax), l2, H_host, S(stream));
}

// -------------------------------------------------------------------- update
template <typename T>
static krcn_status coord_update_impl(krcn_csr* h, int k, const int32_t* cols_host, const double* delta_host,
                                     const T* Ax_in, T* Ax_out, hipStream_t s) {
  CHK(coord_reserve(h, k, s));
  CHK(coord_stage(h, k, cols_host, delta_host, s));
  CoordWs* w = h->cw;
  const int Rw = h->coord_window ? std::min(h->coord_window, kCoordUpdMax) : kCoordUpdAuto;
  const int64_t waves = (h->n + Rw - 1) / Rw;
  const int grid = int((waves + kCoordUpdWaves - 1) / kCoordUpdWaves);
  const size_t lds = size_t(kCoordUpdWaves) * (size_t(Rw) + size_t(k)) * sizeof(double);   // <= 64 KiB
  hipLaunchKernelGGL((k_coord_update<T>), dim3(grid), dim3(kCoordUpdNT), lds, s, int(h->n), Rw, k, w->cols,
                     w->delta, h->tptr, h->tidx, static_cast<const T*>(h->tval), Ax_in, Ax_out,
                     static_cast<const int*>(nullptr));
  LAUNCHCHK();
  return KRCN_OK;
}

extern "C" krcn_status krcn_coord_update(krcn_csr* h, int k, const int32_t* cols_host, const double* delta_host,
                                         const void* Ax_in, void* Ax_out, void* stream) {
  CHK(coord_check("krcn_coord_update", h, k, cols_host));
  if (!delta_host || (h->n && !Ax_out)) return fail(KRCN_ERR_INVALID, "krcn_coord_update: null argument");
  if (h->n == 0) return KRCN_OK;
  CHK(set_device(h));
  hipStream_t s = S(stream);
  if (coord_empty(h)) {
    if (!Ax_in) HIPCHK(hipMemsetAsync(Ax_out, 0, size_t(h->n) * h->vs, s));
    else if (Ax_in != Ax_out)
      HIPCHK(hipMemcpyAsync(Ax_out, Ax_in, size_t(h->n) * h->vs, hipMemcpyDeviceToDevice, s));
    return KRCN_OK;
  }
  return h->dtype == KRCN_F64
             ? coord_update_impl<double>(h, k, cols_host, delta_host, static_cast<const double*>(Ax_in),
                                         static_cast<double*>(Ax_out), s)
             : coord_update_impl<float>(h, k, cols_host, delta_host, static_cast<const float*>(Ax_in),
                                        static_cast<float*>(Ax_out), s);
}
