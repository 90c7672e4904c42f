// krcn_handle.hip — the error recorder, the matrix handle (lifecycle, the
// transposed CSR, policy setters, info getters), the row shards' agreement,
// the profiling readout and the debug entry points.
#include "krcn_internal.hpp"

#include <hipcub/hipcub.hpp>

using namespace krcn;

// ------------------------------------------------------------------ errors
static thread_local std::string g_err;

krcn_status fail(krcn_status s, const char* fmt, ...) {
  char buf[2048];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return s;
}

// ---------------------------------------------------------------- library
extern "C" const char* krcn_last_error_string(void) { return g_err.c_str(); }

std::mutex& build_mutex() {
  static std::mutex m;
  return m;
}
extern "C" int krcn_version(void) { return 1; }

// ---------------------------------------------------------- matrix handle
template <typename T>
static krcn_status build_transpose(krcn_csr* h, hipStream_t s) {
  const int64_t n = h->n, d = h->d, nnz = h->nnz;
  CHK(dalloc(h, &h->tptr, size_t(d + 1)));
  CHK(dalloc(h, &h->tidx, size_t(nnz)));
  CHK(h->own.alloc(&h->tval, std::max<size_t>(size_t(nnz), 1) * sizeof(T)));
  T* tval = static_cast<T*>(h->tval);
  if (nnz == 0) {
    HIPCHK(hipMemsetAsync(h->tptr, 0, size_t(d + 1) * sizeof(int), s));
    return KRCN_OK;
  }
  DevTmp<int> perm, keys_out, iota, rowid;   // (scope exit frees in reverse: rowid first)
  CHK(rowid.alloc(size_t(nnz) * sizeof(int)));
  CHK(iota.alloc(size_t(nnz) * sizeof(int)));
  CHK(keys_out.alloc(size_t(nnz) * sizeof(int)));
  CHK(perm.alloc(size_t(nnz) * sizeof(int)));
  hipLaunchKernelGGL(k_expand_rows, dim3(vec_grid(n * 64)), dim3(kNT), 0, s, int(n), h->ptr, rowid.p);
  LAUNCHCHK();
  hipLaunchKernelGGL(k_iota, dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, iota.p);
  LAUNCHCHK();
  int bits = 1;
  while ((int64_t(1) << bits) < d) ++bits;
  size_t tmpb = 0;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmpb, h->idx, keys_out.p, iota.p, perm.p, int(nnz), 0,
                                            bits, s));
  DevTmp<void> tmp;
  CHK(tmp.alloc(tmpb));
  // LSD radix sort is stable: inside every column the entries keep their CSR
  // (row-ascending) order, i.e. the order csc_matvec scatters them in.
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmpb, h->idx, keys_out.p, iota.p, perm.p, int(nnz), 0,
                                            bits, s));
  hipLaunchKernelGGL(k_colptr_from_sorted, dim3(vec_grid(d + 1)), dim3(kNT), 0, s, d, nnz,
                     keys_out.p, h->tptr);
  LAUNCHCHK();
  hipLaunchKernelGGL((k_gather_transpose<T>), dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, perm.p,
                     rowid.p, static_cast<const T*>(h->val), h->tidx, tval);
  LAUNCHCHK();
  HIPCHK(hipStreamSynchronize(s));
  return KRCN_OK;
}

static krcn_status destroy_impl(krcn_csr* h) {
  if (!h) return KRCN_OK;
  (void)hipSetDevice(h->device);
  lzp_abort(h);    // (first: it tells the applied placement from the others by the tables' fields)
  coord_free(h);   // (before free_all: its device block is one of own's)
  h->own.free_all();
  if (h->hostbuf) (void)hipHostFree(h->hostbuf);
  if (h->hostres) (void)hipHostFree(h->hostres);
  if (h->crn_res) (void)hipHostFree(h->crn_res);
  if (h->cgn_res) (void)hipHostFree(h->cgn_res);
  if (h->blz_host) (void)hipHostFree(h->blz_host);
  if (h->crnb_host) (void)hipHostFree(h->crnb_host);
  if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
  if (h->gstream) (void)hipStreamDestroy(h->gstream);
  if (h->lzp_e0) (void)hipEventDestroy(h->lzp_e0);
  if (h->lzp_e1) (void)hipEventDestroy(h->lzp_e1);
  free_plan(h->p1);
  free_plan(h->p2);
  for (auto& r : h->prof_pool) {
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
    (void)hipEventDestroy(r.e2);
    (void)hipEventDestroy(r.em);
  }
  delete h;
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_create(int device, int64_t n, int64_t d, int64_t nnz,
                                       const int32_t* indptr, const int32_t* indices,
                                       const void* data, int dtype, int64_t n_global,
                                       int shard_mode, krcn_csr** out) {
  if (!out) return fail(KRCN_ERR_INVALID, "krcn_csr_create: out is null");
  *out = nullptr;
  if (n < 0 || d < 0 || nnz < 0) return fail(KRCN_ERR_INVALID, "krcn_csr_create: negative shape");
  if (nnz >= (int64_t(1) << 31) || n >= (int64_t(1) << 31) || d >= (int64_t(1) << 31))
    return fail(KRCN_ERR_UNSUPPORTED, "krcn_csr_create: int32 indices require n, d, nnz < 2^31");
  if (dtype != KRCN_F64 && dtype != KRCN_F32) return fail(KRCN_ERR_INVALID, "krcn_csr_create: bad dtype");
  if (shard_mode < KRCN_SHARD_NONE || shard_mode > KRCN_SHARD_COLS)
    return fail(KRCN_ERR_INVALID, "krcn_csr_create: bad shard_mode");
  if (!indptr || (nnz > 0 && (!indices || !data)))
    return fail(KRCN_ERR_INVALID, "krcn_csr_create: null CSR array");
  if ((reinterpret_cast<uintptr_t>(indices) | reinterpret_cast<uintptr_t>(data)) % 16 != 0)
    return fail(KRCN_ERR_INVALID, "krcn_csr_create: indices and data must be 16-byte aligned (16-B vector loads)");
  // every rank of a sharded run joins the collectives of each call: a rank
  // with an empty block would skip them (early returns on empty work) and
  // leave the others blocked, so an empty shard is rejected up front
  if (shard_mode != KRCN_SHARD_NONE && (n == 0 || d == 0))
    return fail(KRCN_ERR_INVALID, "krcn_csr_create: a shard must hold at least one row and one column (got %lld x %lld)",
                (long long)n, (long long)d);
  if (n_global <= 0) n_global = n;
  krcn_csr* h = new krcn_csr();
  {
    const int nt = tuning_value("KRCN_SORT_NT", 0);   // tuning knob
    if (nt == 256 || nt == 512 || nt == 1024) h->sort_nt = nt;
  }
  h->device = device;
  h->dtype = dtype;
  h->vs = dtype == KRCN_F64 ? 8 : 4;
  h->shard = shard_mode;
  h->n = n;
  h->d = d;
  h->nnz = nnz;
  h->n_global = n_global;
  h->ptr = indptr;
  h->idx = indices;
  h->val = data;
  krcn_status st = KRCN_OK;
  auto init = [&]() -> krcn_status {
    std::lock_guard<std::mutex> lk(build_mutex());
    HIPCHK(hipSetDevice(device));
    hipStream_t s = nullptr;
    HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    krcn_status r = dtype == KRCN_F64 ? build_transpose<double>(h, s) : build_transpose<float>(h, s);
    const hipError_t se = hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
    CHK(r);
    HIPCHK(se);
    CHK(dalloc(h, &h->pa, kMaxPartials));
    CHK(dalloc(h, &h->pb, kMaxPartials));
    CHK(dalloc(h, &h->scal, 16));
    CHK(dalloc(h, &h->st, 1));
    CHK(h->own.alloc(&h->u, size_t(n + 2) * h->vs));   // + 2: the packed d-space sums (lanczos_impl)
    CHK(h->own.alloc(&h->tn, std::max<size_t>(size_t(n) * h->vs, 1)));
    CHK(h->own.alloc(&h->W, std::max<size_t>(size_t(d) * h->vs, 1)));
    CHK(h->own.alloc(&h->td, size_t(d + kMaxPartials) * h->vs));   // + the packed alpha partials (lanczos_impl)
    // the Lanczos recurrence's alphas | betas for every m <= kLzMaxM (+ 4 spare
    // doubles), and the CGS2 coefficients (which read kCgsHPad zeros past k);
    // the packed results go to the mapped host block hostres (k_lz_final)
    CHK(dalloc(h, &h->alphas_dev, size_t(2 * kLzMaxM + 4)));
    h->betas_dev = h->alphas_dev + kLzMaxM;
    CHK(dalloc(h, &h->hcoef, size_t(kLzMaxM + kCgsHPad)));
    h->mcap = kLzMaxM;
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->hostbuf), 4096 * sizeof(double), 0));
    // the Lanczos results block: mapped, coherent host memory that k_lz_final
    // stores into (one kernel store stream over PCIe instead of a copy launch
    // per call: round 5, w8a's m = 10 calls)
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->hostres), size_t(kLzOut) * sizeof(double),
                         hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&h->hostres_dev), h->hostres, 0));
    HIPCHK(hipMemset(h->st, 0, sizeof(LanczosState)));
    HIPCHK(hipMemset(h->scal, 0, 16 * sizeof(double)));
    return KRCN_OK;
  };
  st = init();
  if (st != KRCN_OK) {
    std::string keep = g_err;
    destroy_impl(h);
    g_err = keep;
    return st;
  }
  *out = h;
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_destroy(krcn_csr* h) { return destroy_impl(h); }

extern "C" krcn_status krcn_csr_owned_bytes(const krcn_csr* h, int64_t* bytes_host) {
  if (!h || !bytes_host) return fail(KRCN_ERR_INVALID, "krcn_csr_owned_bytes: null argument");
  *bytes_host = int64_t(h->own.bytes() + h->p1.own.bytes() + h->p2.own.bytes());
  return KRCN_OK;
}

static bool lanes_ok(int L) {
  return L == KRCN_LANES_AUTO || L == KRCN_LANES_SEQUENTIAL || L == 2 || L == 4 || L == 8 ||
         L == 16 || L == 32 || L == 64;
}

extern "C" krcn_status krcn_csr_set_lanes(krcn_csr* h, int lanes_x, int lanes_xt) {
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_csr_set_lanes: null handle");
  if (!lanes_ok(lanes_x) || !lanes_ok(lanes_xt))
    return fail(KRCN_ERR_INVALID, "krcn_csr_set_lanes: lanes must be 0 (auto), 1 (sequential) or a power of two <= 64");
  if (h->lanes_x != lanes_x || h->lanes_xt != lanes_xt) h->plans_ready = false;
  h->lanes_x = lanes_x;
  h->lanes_xt = lanes_xt;
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_get_transpose(const krcn_csr* h, int32_t* colptr, int32_t* rowidx,
                                              void* vals, void* stream) {
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_csr_get_transpose: null handle");
  CHK(set_device(h));
  hipStream_t s = S(stream);
  if (colptr) HIPCHK(hipMemcpyAsync(colptr, h->tptr, size_t(h->d + 1) * sizeof(int), hipMemcpyDeviceToDevice, s));
  if (rowidx && h->nnz) HIPCHK(hipMemcpyAsync(rowidx, h->tidx, size_t(h->nnz) * sizeof(int), hipMemcpyDeviceToDevice, s));
  if (vals && h->nnz) HIPCHK(hipMemcpyAsync(vals, h->tval, size_t(h->nnz) * h->vs, hipMemcpyDeviceToDevice, s));
  return KRCN_OK;
}

// Row shards of a multi-rank communicator pack the pass-1 combine's alpha
// partials past the d-vector of their one all-reduce per Lanczos step
// (the early-rows step, krcn_lzstep.hpp).  Each rank's count depends on its own
// block (the partition balances nonzeros, not rows), so the ranks agree here,
// after every plan build and before any compute call: the packed length is
// the maximum over ranks (a rank with fewer zero-fills the rest), and the
// step runs only if every rank's grids fit.  One all-reduce of 2 x nranks
// doubles (rank r fills slots r and nranks + r).  Collective: every rank of
// the communicator calls it (krcn_csr_attach_comm, krcn_csr_reserve).
krcn_status agree_rows(krcn_csr* h) {
  if (!h->comm || h->comm->nranks <= 1 || h->shard != KRCN_SHARD_ROWS || h->rows_pq >= 0) return KRCN_OK;
  const int P = h->comm->nranks, me = h->comm->rank;
  std::vector<double> v(size_t(2 * P), 0.0);
  v[size_t(me)] = pass_partials(h->p1);
  v[size_t(P + me)] = lz_rows_fit(h->p1.grid, h->p1.combine_grid) ? 1.0 : 0.0;
  DevTmp<double> dv;
  hipStream_t s = nullptr;
  CHK(dv.alloc(v.size() * sizeof(double)));
  krcn_status r = KRCN_OK;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess ||
      hipMemcpyAsync(dv.p, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess)
    r = fail(KRCN_ERR_HIP, "agree_rows: staging");
  if (r == KRCN_OK) r = allreduce(h, dv.p, int64_t(v.size()), KRCN_F64, s);
  if (r == KRCN_OK && (hipMemcpyAsync(v.data(), dv.p, v.size() * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess ||
                       hipStreamSynchronize(s) != hipSuccess))
    r = fail(KRCN_ERR_HIP, "agree_rows: readback");
  if (s) (void)hipStreamDestroy(s);
  dv.reset();
  CHK(r);
  int pq = 0, ok = 1;
  for (int i = 0; i < P; ++i) {
    pq = std::max(pq, int(v[size_t(i)]));
    ok = ok && v[size_t(P + i)] == 1.0;
  }
  h->rows_pq = pq;
  h->rows_early = ok && pq <= kMaxPartials;
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_attach_comm(krcn_csr* h, krcn_comm* comm) {
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_csr_attach_comm: null handle");
  if (comm && h->shard == KRCN_SHARD_NONE && comm->nranks > 1)
    return fail(KRCN_ERR_INVALID, "krcn_csr_attach_comm: an unsharded handle cannot join a %d-rank communicator", comm->nranks);
  h->comm = comm;
  h->rows_pq = -1;
  // a multi-rank handle builds its plans now, before any collective (plans_for_compute)
  if (comm && comm->nranks > 1) {
    CHK(set_device(h));
    CHK(ensure_plans(h));
    CHK(agree_rows(h));
  }
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_set_slicing(krcn_csr* h, int slicing) {
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_csr_set_slicing: null handle");
  if (!(slicing == KRCN_SLICING_AUTO || slicing == KRCN_SLICING_OFF || (slicing >= 8 && slicing % 8 == 0)))
    return fail(KRCN_ERR_INVALID, "krcn_csr_set_slicing: expected 0 (auto), 1 (off) or a multiple of 8");
  if (h->slicing != slicing) {
    h->slicing = slicing;
    h->plans_ready = false;
  }
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_set_format(krcn_csr* h, int format) {
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_csr_set_format: null handle");
  if (format < KRCN_FORMAT_AUTO || format > KRCN_FORMAT_DENSE)
    return fail(KRCN_ERR_INVALID, "krcn_csr_set_format: expected 0 (auto), 1 (wave), 2 (sorted), 3 (window), 4 (jagged) or 5 (dense)");
  if (format == KRCN_FORMAT_DENSE && h->shard != KRCN_SHARD_NONE)
    return fail(KRCN_ERR_UNSUPPORTED, "krcn_csr_set_format: the dense format does not run on a sharded handle");
  if (h->format != format) {
    h->format = format;
    h->plans_ready = false;
  }
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_set_pass_format(krcn_csr* h, int pass, int format) {
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_csr_set_pass_format: null handle");
  if (pass != 1 && pass != 2) return fail(KRCN_ERR_INVALID, "krcn_csr_set_pass_format: pass must be 1 (X) or 2 (X^T)");
  if (format < -1 || format > KRCN_FORMAT_DENSE)
    return fail(KRCN_ERR_INVALID, "krcn_csr_set_pass_format: expected -1 (the handle's format) or a KRCN_FORMAT_* value");
  if (format == KRCN_FORMAT_DENSE && h->shard != KRCN_SHARD_NONE)
    return fail(KRCN_ERR_UNSUPPORTED, "krcn_csr_set_pass_format: the dense format does not run on a sharded handle");
  if (h->format_pass[pass - 1] != format) {
    h->format_pass[pass - 1] = format;
    h->plans_ready = false;
  }
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_set_value_storage(krcn_csr* h, int values) {
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_csr_set_value_storage: null handle");
  if (values < KRCN_VALUES_FULL || values > KRCN_VALUES_F32_EXACT)
    return fail(KRCN_ERR_INVALID, "krcn_csr_set_value_storage: expected 0 (full), 1 (f32) or 2 (f32 if exact)");
  if (values != KRCN_VALUES_FULL && h->shard != KRCN_SHARD_NONE)
    return fail(KRCN_ERR_UNSUPPORTED, "krcn_csr_set_value_storage: narrowed values do not run on a sharded handle");
  if (h->values != values) {
    h->values = values;
    h->plans_ready = false;
  }
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_plan_value_bytes(krcn_csr* h, int* out2_host) {
  if (!h || !out2_host) return fail(KRCN_ERR_INVALID, "krcn_csr_plan_value_bytes: null argument");
  CHK(set_device(h));
  CHK(ensure_plans(h));
  const PassPlan* ps[2] = {&h->p1, &h->p2};
  for (int i = 0; i < 2; ++i) out2_host[i] = ps[i]->vbytes;
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_set_placement_trials(krcn_csr* h, int trials) {
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_csr_set_placement_trials: null handle");
  if (trials < -1 || trials > krcn_csr::kPlaceMax)
    return fail(KRCN_ERR_INVALID, "krcn_csr_set_placement_trials: expected -1 (auto), 0 (off) or 1..%d",
                krcn_csr::kPlaceMax);
  if (h->place_trials != trials) {
    h->place_trials = trials;
    h->plans_ready = false;   // probed at the next plan build
  }
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_set_placement_keep(krcn_csr* h, int keep) {
  // (the range first: it needs no handle, so it can be checked without a device)
  if (keep < -1 || keep >= krcn_csr::kPlaceMax)
    return fail(KRCN_ERR_INVALID, "krcn_csr_set_placement_keep: expected -1 (the fastest) or 0..%d (got %d)",
                krcn_csr::kPlaceMax - 1, keep);
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_csr_set_placement_keep: null handle");
  if (h->place_keep != keep) {
    h->place_keep = keep;
    h->plans_ready = false;   // applied at the next plan build (and the Lanczos-call search starts over)
  }
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_get_placement_keep(const krcn_csr* h, int* keep_host) {
  if (!h || !keep_host) return fail(KRCN_ERR_INVALID, "krcn_csr_get_placement_keep: null argument");
  *keep_host = h->place_keep;
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_placement_info(krcn_csr* h, double* out24_host) {
  if (!h || !out24_host) return fail(KRCN_ERR_INVALID, "krcn_csr_placement_info: null argument");
  CHK(set_device(h));
  CHK(ensure_plans(h));
  double* o = out24_host;
  o[0] = h->place_ran;
  o[1] = h->place_best;
  o[2] = h->place_hot_mb;
  o[3] = h->place_trials;
  for (int i = 0; i < krcn_csr::kPlaceMax; ++i) o[4 + i] = i < h->place_ran ? h->place_us[i] : 0.0;
  o[12] = h->lzp_ran;
  o[13] = h->lzp_stage < 0 ? h->lzp_best : -1;
  o[14] = h->lzp_m;
  o[15] = h->lzp_stage;
  for (int i = 0; i < krcn_csr::kPlaceMax; ++i) o[16 + i] = i < h->lzp_ran ? h->lzp_ms[i] : 0.0;
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_set_graph(krcn_csr* h, int on) {
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_csr_set_graph: null handle");
  h->graph = on != 0;
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_plan_info(krcn_csr* h, int* out8_host) {
  if (!h || !out8_host) return fail(KRCN_ERR_INVALID, "krcn_csr_plan_info: null argument");
  CHK(set_device(h));
  CHK(ensure_plans(h));
  const PassPlan* ps[2] = {&h->p1, &h->p2};
  for (int i = 0; i < 2; ++i) {
    out8_host[4 * i + 0] = ps[i]->kind == KRCN_PLAN_SORTED ? -ps[i]->S : ps[i]->S;
    out8_host[4 * i + 1] = ps[i]->L;
    out8_host[4 * i + 2] = ps[i]->ntiles;
    out8_host[4 * i + 3] = ps[i]->grid;
  }
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_plan_format(krcn_csr* h, int* out2_host) {
  if (!h || !out2_host) return fail(KRCN_ERR_INVALID, "krcn_csr_plan_format: null argument");
  CHK(set_device(h));
  CHK(ensure_plans(h));
  out2_host[0] = h->p1.kind;
  out2_host[1] = h->p2.kind;
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_lanczos_step(krcn_csr* h, int reorth, int* step_host) {
  if (!h || !step_host) return fail(KRCN_ERR_INVALID, "krcn_csr_lanczos_step: null argument");
  CHK(set_device(h));
  CHK(plans_for_compute(h));
  const LzStepChoice ch = lanczos_step(lz_step_in(h, reorth));
  CHK(ch.refusal);
  *step_host = ch.step;
  return KRCN_OK;
}

// ------------------------------------------------------------- profiling
extern "C" krcn_status krcn_prof_enable(krcn_csr* h, int on) {
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_prof_enable: null handle");
  h->prof = on != 0;
  h->prof_used = 0;
  return KRCN_OK;
}

extern "C" krcn_status krcn_prof_read(krcn_csr* h, double* out8_host) {
  if (!h || !out8_host) return fail(KRCN_ERR_INVALID, "krcn_prof_read: null argument");
  CHK(set_device(h));
  double p1 = 0, p2 = 0, tot = 0, k1 = 0, cb = 0;
  for (size_t i = 0; i < h->prof_used; ++i) {
    ProfRec& r = h->prof_pool[i];
    HIPCHK(hipEventSynchronize(r.e2));
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, r.e0, r.e1));
    HIPCHK(hipEventElapsedTime(&b, r.e1, r.e2));
    p1 += a;
    p2 += b;
    tot += double(a) + double(b);
    if (r.mid) {
      float x = 0, y = 0;
      HIPCHK(hipEventElapsedTime(&x, r.e0, r.em));
      HIPCHK(hipEventElapsedTime(&y, r.em, r.e1));
      k1 += x;
      cb += y;
    } else {
      k1 += a;
    }
  }
  const double c = double(h->prof_used);
  out8_host[0] = c; out8_host[1] = p1;
  out8_host[2] = c; out8_host[3] = p2;
  out8_host[4] = c; out8_host[5] = tot;
  out8_host[6] = k1; out8_host[7] = cb;
  h->prof_used = 0;
  return KRCN_OK;
}

#ifdef KRCN_TUNING
// Placement diagnostics (tools/placement_rounds.py; not in krcn.h): move one
// of the handle's scratch buffers to a fresh allocation (allocated before the
// old one is freed, so it lands elsewhere).  which: 1 w, 2 u, 3 pass-1 slice
// partials, 4 td (rows-shard scratch d-vector), 5 the small partial buffers.
extern "C" int krcn_debug_realloc(krcn_csr* h, int which) {
  // (the field's size comes from its owner's table, which stays true: only the address changes)
  auto mv = [](DevOwner& own, const void* field) -> int {
    const DevOwner::Slot* sl = own.find(field);
    if (!sl || !*sl->field) return 0;
    void* q = nullptr;
    if (hipMalloc(&q, sl->bytes) != hipSuccess) return 1;
    if (hipFree(*sl->field) != hipSuccess) return 1;
    *sl->field = q;
    return 0;
  };
  if (!h || ensure_plans(h) != KRCN_OK) return 1;
  switch (which) {
    case 1: return mv(h->own, &h->W);
    case 2: return mv(h->own, &h->u);
    case 3: return mv(h->p1.own, &h->p1.part);
    case 4: return mv(h->own, &h->td);
    case 5: return mv(h->own, &h->pa) | mv(h->own, &h->pb) | mv(h->own, &h->pz);
    default: return 1;
  }
}
#endif

#ifdef KRCN_WIN_TIMING
// Debug builds only: read (and optionally clear) the window-pass stamps.
extern "C" int krcn_debug_win_stamps_ops(unsigned long long* out, int n, int reset);
extern "C" int krcn_debug_win_stamps_lz64(unsigned long long* out, int n, int reset);
extern "C" int krcn_debug_win_stamps_lz32(unsigned long long* out, int n, int reset);
extern "C" int krcn_debug_win_stamps(unsigned long long* out, int n, int reset) {
  std::vector<unsigned long long> t(size_t(n), 0);
  std::fill(out, out + n, 0ull);
  int (*rd[])(unsigned long long*, int, int) = {krcn_debug_win_stamps_ops, krcn_debug_win_stamps_lz64,
                                                 krcn_debug_win_stamps_lz32};
  for (auto f : rd) {
    if (f(t.data(), n, reset)) return 1;
    for (int i = 0; i < n; ++i) out[i] = std::max(out[i], t[i]);
  }
  return 0;
}
#endif

#ifdef KRCN_SORT_TIMING
// Debug builds only: read (and optionally clear) the phase cycles of k_sorted_pass.
extern "C" int krcn_debug_cycles(unsigned long long* out, int n, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(krcn::krcn_dbg_cycles), sizeof(unsigned long long) * n) != hipSuccess)
    return 1;
  if (reset) {
    std::vector<unsigned long long> z(1024 * 16 * 8, 0);
    if (hipMemcpyToSymbol(HIP_SYMBOL(krcn::krcn_dbg_cycles), z.data(), sizeof(unsigned long long) * z.size()) !=
        hipSuccess)
      return 1;
  }
  return 0;
}
#endif
