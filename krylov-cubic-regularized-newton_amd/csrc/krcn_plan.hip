// krcn_plan.hip — the pass plans (tile / sorted / LDS-window / jagged / dense
// formats) on the device, ensure_plans and the reorthogonalisation workspace.
// Every layout decision (slices, cuts, tiles, segments, tasks, grids, when a
// format is refused) is krcn_layout.hpp's, from host row pointers; a builder
// here calls its layout function, returns the refusal if there is one,
// allocates, copies, sorts and gathers, and sets the PlanFields from the
// layout struct.
#include "krcn_internal.hpp"
#include "krcn_layout.hpp"

#include <hipcub/hipcub.hpp>

using namespace krcn;

// ----------------------------------------------------------- pass plans
void free_plan(PassPlan& P) {
  P.own.free_all();
  static_cast<PlanFields&>(P) = PlanFields();
}

// An empty plan of the given shape: what every builder starts from (vs: the
// handle's value size; a builder that narrows its values sets P.vbytes itself).
static void reset_plan(PassPlan& P, int rows, int64_t cols, int64_t nnz, size_t vs) {
  free_plan(P);
  P.rows = rows;
  P.cols = cols;
  P.nnz = nnz;
  P.vbytes = int(vs);
}

// Sliced copy of a CSR: slice s holds columns [bounds[s], bounds[s+1]) with
// global column ids, rows in order; row pointers flattened slice-major.
// The values are stored as TS (static_cast<TS>(v); T but for a narrowed
// window plan).
template <typename T, typename TS = T>
static krcn_status build_slices(PassPlan& P, const int* ptr, const int* idx, const T* val, hipStream_t s,
                                const std::vector<int>* bounds_in = nullptr, int64_t pad = 0) {
  const int S = P.S, rows = P.rows;
  const int64_t nnz = P.nnz, cols = P.cols;
  std::vector<int> hb(S + 1);
  for (int k = 0; k <= S; ++k) hb[k] = bounds_in ? (*bounds_in)[k] : slice_base(cols, k, S);
  DevTmp<int> counts, perm, iota, sid_out, sid, bounds;   // (scope exit frees in reverse: bounds first)
  CHK(bounds.alloc(sizeof(int) * (S + 1)));
  HIPCHK(hipMemcpyAsync(bounds.p, hb.data(), sizeof(int) * (S + 1), hipMemcpyHostToDevice, s));
  const size_t nptr = size_t(S) * rows + 1;
  CHK(P.own.alloc(&P.own_ptr, sizeof(int) * nptr));
  CHK(P.own.alloc(&P.own_idx, sizeof(int) * std::max<int64_t>(nnz, 1)));
  CHK(P.own.alloc(&P.own_val, sizeof(TS) * size_t(std::max<int64_t>(nnz, 1) + pad)));
  if (pad) HIPCHK(hipMemsetAsync(static_cast<TS*>(P.own_val) + nnz, 0, sizeof(TS) * size_t(pad), s));
  CHK(counts.alloc(sizeof(int) * nptr));
  HIPCHK(hipMemsetAsync(counts.p, 0, sizeof(int) * nptr, s));
  if (nnz > 0) {
    CHK(sid.alloc(sizeof(int) * nnz));
    CHK(sid_out.alloc(sizeof(int) * nnz));
    CHK(iota.alloc(sizeof(int) * nnz));
    CHK(perm.alloc(sizeof(int) * nnz));
    hipLaunchKernelGGL(k_slice_of, dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, idx, bounds.p, S, sid.p);
    LAUNCHCHK();
    hipLaunchKernelGGL(k_iota, dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, iota.p);
    LAUNCHCHK();
    int bits = 1;
    while ((1 << bits) < S) ++bits;
    size_t tmpb = 0;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmpb, sid.p, sid_out.p, iota.p, perm.p, int(nnz), 0, bits, s));
    DevTmp<void> tmp, t2;
    CHK(tmp.alloc(tmpb));
    // stable: inside a slice the nonzeros keep their row-major order
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmpb, sid.p, sid_out.p, iota.p, perm.p, int(nnz), 0, bits, s));
    hipLaunchKernelGGL(k_slice_counts, dim3(vec_grid(int64_t(rows) * 64)), dim3(kNT), 0, s, rows, ptr, sid.p, counts.p);
    LAUNCHCHK();
    hipLaunchKernelGGL((k_slice_gather<T, TS>), dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, perm.p, idx, val,
                       P.own_idx, static_cast<TS*>(P.own_val));
    LAUNCHCHK();
    size_t tmp2 = 0;
    HIPCHK(hipcub::DeviceScan::InclusiveSum(nullptr, tmp2, counts.p, P.own_ptr, int(nptr), s));
    CHK(t2.alloc(tmp2));
    HIPCHK(hipcub::DeviceScan::InclusiveSum(t2.p, tmp2, counts.p, P.own_ptr, int(nptr), s));
    HIPCHK(hipStreamSynchronize(s));
    t2.reset();
    tmp.reset();
  } else {
    HIPCHK(hipMemsetAsync(P.own_ptr, 0, sizeof(int) * nptr, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  P.ptr = P.own_ptr;
  P.idx = P.own_idx;
  P.val = P.own_val;
  return KRCN_OK;
}

// Row pointers on the host: n entries of a device array.
static krcn_status host_ptr(const int* dptr, size_t n, hipStream_t s, std::vector<int>* hp) {
  hp->resize(n);
  HIPCHK(hipMemcpyAsync(hp->data(), dptr, sizeof(int) * n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return KRCN_OK;
}

// The stored type of a plan's values: build(TS()) with TS = float on an fp64
// handle storing 4-byte values, else T.
template <typename T, class Build>
static krcn_status with_stored_type(size_t vs, Build&& build) {
  if constexpr (std::is_same<T, double>::value)
    if (vs == 4) return build(float());
  return build(T());
}

// The tile list of a wave or sorted plan (tile_layout) on the device.
static krcn_status build_tiles(PassPlan& P, const TileLayout& tl, hipStream_t s) {
  if (P.kind == KRCN_PLAN_SORTED) {
    CHK(P.own.alloc(&P.tmid, sizeof(int) * tl.tmid.size()));
    HIPCHK(hipMemcpyAsync(P.tmid, tl.tmid.data(), sizeof(int) * tl.tmid.size(), hipMemcpyHostToDevice, s));
  }
  P.ntiles = tl.ntiles;
  CHK(P.own.alloc(&P.tiles, sizeof(TileDesc) * std::max<size_t>(tl.tiles.size(), 1)));
  CHK(P.own.alloc(&P.tbeg, sizeof(int) * tl.tbeg.size()));
  if (!tl.tiles.empty())
    HIPCHK(hipMemcpyAsync(P.tiles, tl.tiles.data(), sizeof(TileDesc) * tl.tiles.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(P.tbeg, tl.tbeg.data(), sizeof(int) * tl.tbeg.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  P.grid = tl.grid;
  P.combine_grid = combine_grid(P.rows);
  return KRCN_OK;
}

// Store the pass's nonzeros sorted by gather index inside every sort segment
// (stable: ties keep CSR order), with their slot in the segment.
template <typename T>
static krcn_status build_sorted(PassPlan& P, const std::vector<int>& segs, const std::vector<int>& segbase,
                               hipStream_t s) {
  const int64_t nnz = P.nnz;
  const int nseg = int(segs.size()) - 1;
  CHK(P.own.alloc(&P.gword, sizeof(unsigned) * std::max<int64_t>(nnz, 1)));
  CHK(P.own.alloc(&P.gval, sizeof(T) * std::max<int64_t>(nnz, 1)));
  if (nnz == 0 || nseg <= 0) return KRCN_OK;
  // (scope exit frees in reverse: the hipCUB scratch, then dsegs, dbase, key, skey, iota, perm)
  DevTmp<int> perm, iota;
  DevTmp<unsigned long long> skey, key;
  DevTmp<int> dbase, dsegs;
  CHK(dsegs.alloc(sizeof(int) * segs.size()));
  HIPCHK(hipMemcpyAsync(dsegs.p, segs.data(), sizeof(int) * segs.size(), hipMemcpyHostToDevice, s));
  CHK(dbase.alloc(sizeof(int) * segbase.size()));
  HIPCHK(hipMemcpyAsync(dbase.p, segbase.data(), sizeof(int) * segbase.size(), hipMemcpyHostToDevice, s));
  CHK(key.alloc(sizeof(unsigned long long) * nnz));
  CHK(skey.alloc(sizeof(unsigned long long) * nnz));
  CHK(iota.alloc(sizeof(int) * nnz));
  CHK(perm.alloc(sizeof(int) * nnz));
  hipLaunchKernelGGL(k_seg_keys, dim3(std::min(nseg, 65535)), dim3(kNT), 0, s, nseg, dsegs.p, P.idx, key.p);
  LAUNCHCHK();
  hipLaunchKernelGGL(k_iota, dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, iota.p);
  LAUNCHCHK();
  int sbits = 1;
  while ((int64_t(1) << sbits) < nseg) ++sbits;
  int slot_bits = 0;
  while ((1 << slot_bits) < P.sort_nt * kSortPerThread) ++slot_bits;
  size_t tmpb = 0;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmpb, key.p, skey.p, iota.p, perm.p, int(nnz), 0, 32 + sbits, s));
  DevTmp<void> tmp;
  CHK(tmp.alloc(tmpb));
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmpb, key.p, skey.p, iota.p, perm.p, int(nnz), 0, 32 + sbits, s));
  hipLaunchKernelGGL((k_sorted_gather<T>), dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, perm.p, skey.p, dsegs.p, dbase.p,
                     static_cast<const T*>(P.val), slot_bits, P.gword, static_cast<T*>(P.gval));
  LAUNCHCHK();
  HIPCHK(hipStreamSynchronize(s));
  // the sorted arrays replace the slice copies (the row pointers stay)
  CHK(P.own.release(&P.own_idx));
  CHK(P.own.release(&P.own_val));
  P.idx = nullptr;
  P.val = nullptr;
  return KRCN_OK;
}

// A/B knob KRCN_PLAN_RELOC (placement): 1 moves a plan's element
// arrays into physically contiguous allocations (hipDeviceMallocContiguous),
// 2 into fresh plain allocations made after the build's temporaries are gone.
static int plan_reloc_env() {
  static const int v = tuning_value("KRCN_PLAN_RELOC", 0);
  return v;
}

static krcn_status plan_reloc(PassPlan& P, void* field, hipStream_t s) {
  const int mode = plan_reloc_env();
  const DevOwner::Slot* sl = P.own.find(field);
  if (mode == 0 || !sl || !*sl->field || sl->bytes == 0) return KRCN_OK;
  void** p = sl->field;
  const size_t bytes = sl->bytes;
  void* q = nullptr;
  if (mode == 1) HIPCHK(hipExtMallocWithFlags(&q, bytes, hipDeviceMallocContiguous));
  else HIPCHK(hipMalloc(&q, bytes));
  HIPCHK(hipMemcpyAsync(q, *p, bytes, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipFree(*p));
  *p = q;
  return KRCN_OK;
}

// The per-block X^T copies of a one-piece window-accum plan (xt_layout, from
// the plan's own 16-bit offsets and stored values) on the device; P.xt stays 0
// when the layout skips them.
template <typename T, typename TS>
static krcn_status build_xt(PassPlan& P, const std::vector<int>& hp, const WinLayout& wl, hipStream_t s) {
  const int64_t nnz = P.nnz;
  std::vector<unsigned short> hidx(size_t(std::max<int64_t>(nnz, 1)));
  std::vector<TS> hval(size_t(std::max<int64_t>(nnz, 1)));
  if (nnz > 0) {
    HIPCHK(hipMemcpy(hidx.data(), P.widx, sizeof(unsigned short) * size_t(nnz), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hval.data(), P.val, sizeof(TS) * size_t(nnz), hipMemcpyDeviceToHost));
  }
  const XtLayout<T> x = xt_layout<T, TS>(P.rows, P.R, int(P.cols), hidx.data(), hval.data(), hp.data(), wl.cut, wl.grid);
  if (x.skipped) return KRCN_OK;
  const size_t ne = x.xr.size();
  CHK(P.own.alloc(&P.xcp, sizeof(int) * x.cp.size()));
  CHK(P.own.alloc(&P.xrow, sizeof(unsigned short) * ne));
  CHK(P.own.alloc(&P.xval, sizeof(T) * ne));
  CHK(P.own.alloc(&P.xpart, sizeof(T) * size_t(wl.grid) * size_t(P.cols)));
  HIPCHK(hipMemcpyAsync(P.xcp, x.cp.data(), sizeof(int) * x.cp.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(P.xrow, x.xr.data(), sizeof(unsigned short) * ne, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(P.xval, x.xv.data(), sizeof(T) * ne, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  P.xt = 1;
  return KRCN_OK;
}

// An LDS-window plan (win_shape, win_layout).  TS: the stored type of the
// values.  The geometry (slices, tiles, segments, grids) is T's whatever TS is:
// only the element type of own_val changes.
template <typename T, typename TS>
static krcn_status build_window_as(PassPlan& P, const int* ptr, const int* idx, const T* val, int accum,
                                   hipStream_t s) {
  const WinShape sh = win_shape<T>(P.cols, accum);
  P.vbytes = int(sizeof(TS));
  const int rows = P.rows, S = sh.S;
  const int64_t nnz = P.nnz;
  P.S = S;
  P.W = sh.W;
  P.kind = sh.kind;
  P.L = 1;
  P.groups = 1;
  CHK((build_slices<T, TS>(P, ptr, idx, val, s, &sh.bounds, kWinPad)));
  CHK(P.own.alloc(&P.widx, sizeof(unsigned short) * size_t(nnz + kWinPad)));
  HIPCHK(hipMemsetAsync(P.widx, 0, sizeof(unsigned short) * size_t(nnz + kWinPad), s));
  if (nnz > 0) {
    hipLaunchKernelGGL(k_local_u16, dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, P.own_idx, sh.W, P.widx);
    LAUNCHCHK();
  }
  HIPCHK(hipStreamSynchronize(s));
  CHK(P.own.release(&P.own_idx));
  P.idx = nullptr;
  std::vector<int> hp;   // slice-major
  CHK(host_ptr(P.ptr, size_t(S) * rows + 1, s, &hp));
  const WinLayout wl = win_layout(sh, rows, nnz, hp.data());
  if (wl.refused != KRCN_OK) return wl.refused;
  P.R = wl.R;
  CHK(plan_reloc(P, &P.widx, s));
  CHK(plan_reloc(P, &P.own_val, s));
  P.val = P.own_val;
  CHK(P.own.alloc(&P.tb, sizeof(int) * size_t(S) * (accum ? 1 : 2) * (wl.ntiles + 1)));
  CHK(P.own.alloc(&P.ro, sizeof(unsigned short) * std::max<size_t>(size_t(S) * rows, 1)));
  std::vector<int> tbr;   // (outlives the copy)
  if (accum) {
    hipLaunchKernelGGL(k_compact_rows, dim3(vec_grid(int64_t(S) * rows)), dim3(kNT), 0, s, S, rows, wl.R, wl.ntiles,
                       P.ptr, P.tb, P.ro);
  } else {
    // the tiles are the layout's (fixed or data-cut): per slice the tiles' bases, then their row starts
    const size_t n1 = size_t(wl.ntiles) + 1;
    tbr.resize(size_t(S) * 2 * n1);
    for (int sl = 0; sl < S; ++sl)
      for (size_t t = 0; t < n1; ++t) {
        const int r = wl.trow[size_t(sl) * n1 + t];
        tbr[size_t(sl) * 2 * n1 + t] = hp[size_t(sl) * rows + r];
        tbr[size_t(sl) * 2 * n1 + n1 + t] = r;
      }
    HIPCHK(hipMemcpyAsync(P.tb, tbr.data(), sizeof(int) * tbr.size(), hipMemcpyHostToDevice, s));
    if (wl.ntiles > 0)
      hipLaunchKernelGGL(k_compact_tiles, dim3(vec_grid(int64_t(S) * wl.ntiles)), dim3(kNT), 0, s, S, rows, wl.ntiles,
                         P.ptr, P.tb, P.ro);
  }
  LAUNCHCHK();
  HIPCHK(hipStreamSynchronize(s));
  // the kernels read the compact form only
  CHK(P.own.release(&P.own_ptr));
  P.ptr = nullptr;
  P.stride = wl.stride;
  P.grid = wl.grid;
  P.kpb = wl.kpb;
  if (accum) {
    if (S == 1 && P.cols <= kWinNT) CHK((build_xt<T, TS>(P, hp, wl, s)));
  } else {
    CHK(P.own.alloc(&P.part, sizeof(T) * size_t(S) * std::max(rows, 1)));
    P.combine_grid = combine_grid(rows);
  }
  P.nseg = int(wl.segs.size());
  P.ntiles = wl.ntiles;
  CHK(P.own.alloc(&P.segs, sizeof(WinSeg) * std::max<size_t>(wl.segs.size(), 1)));
  if (!wl.segs.empty())
    HIPCHK(hipMemcpy(P.segs, wl.segs.data(), sizeof(WinSeg) * wl.segs.size(), hipMemcpyHostToDevice));
  return KRCN_OK;
}

// ------------------------------------------------------ jagged plans
// The long rows of a single-window plan (JagLayout's lrows / ltask / lbeg / lcut / tasks) on the
// device, their elements apart from the units'.
template <typename T, typename TS>
static krcn_status build_jag_long(PassPlan& P, const JagLayout& J, const int* ptr, const int* idx, const T* val,
                                  hipStream_t s) {
  const int nl = int(J.lrows.size()), W = J.W;
  const size_t lsz = size_t(J.lbeg[nl]) + kJagPad;
  CHK(P.own.alloc(&P.jlcut, sizeof(int) * J.lcut.size()));
  CHK(P.own.alloc(&P.jlrow, sizeof(int) * size_t(nl)));
  CHK(P.own.alloc(&P.jltask, sizeof(int) * J.ltask.size()));
  CHK(P.own.alloc(&P.jtask, sizeof(int) * J.tasks.size()));
  CHK(P.own.alloc(&P.jlidx, sizeof(unsigned short) * lsz));
  CHK(P.own.alloc(&P.jlval, sizeof(TS) * lsz));
  DevTmp<int> lbeg_d;
  CHK(lbeg_d.alloc(sizeof(int) * size_t(nl)));
  HIPCHK(hipMemcpyAsync(P.jlcut, J.lcut.data(), sizeof(int) * J.lcut.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(P.jlrow, J.lrows.data(), sizeof(int) * size_t(nl), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(P.jltask, J.ltask.data(), sizeof(int) * J.ltask.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(P.jtask, J.tasks.data(), sizeof(int) * J.tasks.size(), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(lbeg_d.p, J.lbeg.data(), sizeof(int) * size_t(nl), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(P.jlidx, 0, sizeof(unsigned short) * lsz, s));
  HIPCHK(hipMemsetAsync(P.jlval, 0, sizeof(TS) * lsz, s));
  hipLaunchKernelGGL((k_jag_long_fill<T, TS>), dim3(std::min(nl, 4096)), dim3(kNT), 0, s, nl, W, P.jlrow, lbeg_d.p, ptr,
                     idx, val, P.jlidx, static_cast<TS*>(P.jlval));
  LAUNCHCHK();
  HIPCHK(hipStreamSynchronize(s));
  lbeg_d.reset();
  return KRCN_OK;
}

// 8-bit lane counts: a 32-bit word for the K = 4 accumulate kernel, else 64-bit
static krcn_status build_jag_counts(PassPlan& P, const JagLayout& J, const unsigned char* cnt8, hipStream_t s) {
  const int K = J.K;
  const int64_t nrec = J.nrec;
  const bool w32 = J.S > 1 && K <= 4;
  const size_t cbytes = size_t(nrec) * 64 * (w32 ? 4 : 8);
  CHK(P.own.alloc(&P.jcnt, cbytes));
  if (w32)
    hipLaunchKernelGGL((k_jag_words<unsigned>), dim3(vec_grid(nrec * 64)), dim3(kNT), 0, s, nrec, K, cnt8,
                       reinterpret_cast<unsigned*>(P.jcnt));
  else
    hipLaunchKernelGGL((k_jag_words<unsigned long long>), dim3(vec_grid(nrec * 64)), dim3(kNT), 0, s, nrec, K,
                       cnt8, reinterpret_cast<unsigned long long*>(P.jcnt));
  LAUNCHCHK();
  HIPCHK(hipStreamSynchronize(s));
  return KRCN_OK;
}

// A jagged plan (jag_layout, from the pass's CSR row pointers hp).  TS: the
// stored type of the values (own_val and the long rows' jlval); every choice
// of the layout is T's.  The device scan adds the refusals only it can see:
// descending column indices, more than 255 elements of a row in one slice, a
// unit past kJagSlab.
template <typename T, typename TS>
static krcn_status build_jag_as(PassPlan& P, const int* ptr, const int* idx, const T* val, int pass, bool seq,
                                const std::vector<int>& hp, hipStream_t s) {
  const int rows = P.rows;
  P.vbytes = int(sizeof(TS));
  const int64_t nnz = P.nnz;
  const JagLayout J = jag_layout<T>(rows, P.cols, nnz, pass, seq, hp.data());
  if (J.refused != KRCN_OK) return J.refused;
  const int S = J.S, W = J.W, SG = J.SG, Sg = J.Sg, G = J.G, R = J.R, K = J.K, B = J.B, ubits = J.ubits;
  const int64_t NU = J.NU, nrec = J.nrec;
  const int nl = int(J.lrows.size());
  CHK(P.own.alloc(&P.jgcut, sizeof(int) * (size_t(R) + 1)));
  CHK(P.own.alloc(&P.jumeta, sizeof(int) * size_t(nrec) * 2 * K));
  HIPCHK(hipMemcpyAsync(P.jgcut, J.cut.data(), sizeof(int) * (size_t(R) + 1), hipMemcpyHostToDevice, s));
  if (SG > 1) {   // per-group partial row sums
    CHK(P.own.alloc(&P.part, sizeof(T) * size_t(SG) * size_t(rows)));
    P.combine_grid = combine_grid(rows);
  }

  // (scope exit frees in reverse: gblk_d first, the hipCUB scratch last)
  DevTmp<void> tmp;
  DevTmp<unsigned char> cnt8;
  DevTmp<unsigned long long> keys_out, keys;
  DevTmp<int> pbase, first, usize, perm, iota, flags, gblk_d;
  int hflags[3] = {0, 0, 0};
  // single window: pair-level order, one pad key slot per row after the nonzeros
  const bool pairs = S == 1;
  const int64_t nitems = pairs ? nnz + rows : nnz;
  const unsigned long long sentinel = (1ull << (ubits + 22)) - 1ull;   // unit id >= NU: sorts past every real key
  if (nitems >= (int64_t(1) << 31)) return fail(KRCN_ERR_UNSUPPORTED, "jag plan: too many elements");
  CHK(gblk_d.alloc(sizeof(int) * size_t(G)));
  CHK(flags.alloc(3 * sizeof(int)));
  CHK(iota.alloc(sizeof(int) * size_t(nitems)));
  CHK(perm.alloc(sizeof(int) * size_t(nitems)));
  CHK(keys.alloc(sizeof(unsigned long long) * size_t(nitems)));
  CHK(keys_out.alloc(sizeof(unsigned long long) * size_t(nitems)));
  CHK(cnt8.alloc(size_t(NU) * 64));
  CHK(usize.alloc(sizeof(int) * size_t(NU)));
  CHK(first.alloc(sizeof(int) * size_t(NU)));
  HIPCHK(hipMemsetAsync(first.p, 0, sizeof(int) * size_t(NU), s));
  HIPCHK(hipMemsetAsync(usize.p, 0, sizeof(int) * size_t(NU), s));
  HIPCHK(hipMemcpyAsync(gblk_d.p, J.gblk.data(), sizeof(int) * size_t(G), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(flags.p, 0, 3 * sizeof(int), s));
  HIPCHK(hipMemsetAsync(cnt8.p, 0, size_t(NU) * 64, s));
  hipLaunchKernelGGL(k_jag_keys, dim3(vec_grid(rows)), dim3(kNT), 0, s, rows, Sg, SG, W, K, pairs ? 0 : 1, nnz,
                     sentinel, nl > 0 ? J.lthr : 0, ptr, idx, P.jgcut, gblk_d.p, keys.p, cnt8.p, usize.p, flags.p);
  LAUNCHCHK();
  HIPCHK(hipMemcpyAsync(hflags, flags.p, 3 * sizeof(int), hipMemcpyDeviceToHost, s));
  std::vector<int> hsz(S > 1 ? size_t(NU) : 0);
  if (S > 1) HIPCHK(hipMemcpyAsync(hsz.data(), usize.p, sizeof(int) * size_t(NU), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (hflags[0]) return fail(KRCN_ERR_UNSUPPORTED, "jag plan: rows with descending column indices");
  if (hflags[1] > 255) return fail(KRCN_ERR_UNSUPPORTED, "jag plan: %d elements of a row in one slice (max 255)", hflags[1]);
  const int umax = hsz.empty() ? 0 : *std::max_element(hsz.begin(), hsz.end());
  if (umax > kJagSlab)
    return fail(KRCN_ERR_UNSUPPORTED, "jag plan: a group holds %d elements of one slice (accumulate mode: max %d)",
                umax, kJagSlab);
  hipLaunchKernelGGL(k_iota, dim3(vec_grid(nitems)), dim3(kNT), 0, s, nitems, iota.p);
  LAUNCHCHK();
  size_t tb = 0;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, keys.p, keys_out.p, iota.p, perm.p, int(nitems), 0, ubits + 22, s));
  CHK(tmp.alloc(tb));
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, keys.p, keys_out.p, iota.p, perm.p, int(nitems), 0, ubits + 22, s));
  hipLaunchKernelGGL(k_jag_firsts, dim3(vec_grid(nitems)), dim3(kNT), 0, s, nitems, NU, keys_out.p, first.p);
  LAUNCHCHK();
  // single window: the nonzeros and their pads in sorted (pair-level) order
  // (long rows' elements sort past them, as sentinels); accumulate layout:
  // every unit padded to an even count (two elements a lane)
  int64_t total = (pairs ? nnz + hflags[2] : nnz) - J.lnnz;
  if (S > 1) {
    CHK(pbase.alloc(sizeof(int) * size_t(NU)));
    hipLaunchKernelGGL(k_jag_pad2, dim3(vec_grid(NU)), dim3(kNT), 0, s, NU, usize.p, first.p);   // first := padded sizes
    LAUNCHCHK();
    HIPCHK(hipStreamSynchronize(s));
    tmp.reset();
    size_t tb2 = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, first.p, pbase.p, int(NU), s));
    CHK(tmp.alloc(tb2));
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tb2, first.p, pbase.p, int(NU), s));
    int last[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&last[0], pbase.p + NU - 1, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&last[1], first.p + NU - 1, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    total = int64_t(last[0]) + last[1];
    hipLaunchKernelGGL(k_jag_firsts, dim3(vec_grid(nnz)), dim3(kNT), 0, s, nnz, NU, keys_out.p, first.p);   // restore
    LAUNCHCHK();
  }
  CHK(P.own.alloc(&P.widx, sizeof(unsigned short) * size_t(total + kJagPad)));
  CHK(P.own.alloc(&P.own_val, sizeof(TS) * size_t(total + kJagPad)));
  HIPCHK(hipMemsetAsync(P.widx, 0, sizeof(unsigned short) * size_t(total + kJagPad), s));
  HIPCHK(hipMemsetAsync(P.own_val, 0, sizeof(TS) * size_t(total + kJagPad), s));
  hipLaunchKernelGGL((k_jag_gather<T, TS>), dim3(vec_grid(pairs ? total : nnz)), dim3(kNT), 0, s, pairs ? total : nnz,
                     nnz, W, perm.p, idx, val, keys_out.p, first.p, pbase.p, P.widx, static_cast<TS*>(P.own_val));
  LAUNCHCHK();
  hipLaunchKernelGGL(k_jag_umeta, dim3(vec_grid(nrec * 2 * K)), dim3(kNT), 0, s, nrec, K, pbase.p ? pbase.p : first.p,
                     usize.p, P.jumeta);
  LAUNCHCHK();
  CHK(plan_reloc(P, &P.widx, s));
  CHK(plan_reloc(P, &P.own_val, s));
  if (nl > 0) CHK((build_jag_long<T, TS>(P, J, ptr, idx, val, s)));
  CHK(build_jag_counts(P, J, cnt8.p, s));
  P.kind = KRCN_PLAN_JAG;
  P.jlong = nl;
  P.jlpiece = J.lpiece;
  P.jK = K;
  P.jG = SG;
  P.jSg = Sg;
  P.S = S;
  P.W = W;
  P.L = 1;
  P.groups = 1;
  P.grid = B;
  P.ntiles = G;
  P.val = P.own_val;
  return KRCN_OK;
}

// ----------------------------------------------------------- dense format
// The image of one pass (krcn_dense.hpp): zero fill plus a scatter of the CSR
// on the build stream; the slice partials when the geometry slices the pass.
// TS is the stored type of the image's values: T, or float on an fp64 handle
// under KRCN_VALUES_F32 (the geometry is then that of an fp32 image).
template <typename T, typename TS>
static krcn_status build_dense_as(PassPlan& P, const int* ptr, const int* idx, const T* val, int lanes, int slicing,
                                  hipStream_t s) {
  const DenseGeom g = dense_geometry(P.rows, P.cols, sizeof(TS), lanes, slicing);
  CHK(P.own.alloc(&P.own_val, size_t(g.bytes)));
  HIPCHK(hipMemsetAsync(P.own_val, 0, size_t(g.bytes), s));
  if (P.nnz > 0) {
    const int64_t blocks = (int64_t(P.rows) + kDenseNT / 64 - 1) / (kDenseNT / 64);
    hipLaunchKernelGGL((k_dense_scatter<T, TS>), dim3(unsigned(std::min<int64_t>(blocks, 65536))), dim3(kDenseNT), 0,
                       s, P.rows, ptr, idx, val, g.ld, static_cast<TS*>(P.own_val));
    LAUNCHCHK();
  }
  if (g.S > 1) CHK(P.own.alloc(&P.part, sizeof(T) * size_t(g.S) * size_t(std::max(P.rows, 1))));
  HIPCHK(hipStreamSynchronize(s));
  P.kind = KRCN_PLAN_DENSE;
  P.dld = g.ld;
  P.vbytes = int(sizeof(TS));
  P.S = g.S;
  P.L = g.L;
  P.ntiles = int(g.groups);
  P.grid = g.grid;
  P.combine_grid = combine_grid(P.rows);
  P.val = P.own_val;
  return KRCN_OK;
}

// KRCN_VALUES_F32_EXACT: *flag |= 1 when some value does not survive the round
// trip through fp32 (a NaN never does).
__global__ __launch_bounds__(256) void k_values_f32_exact(const double* __restrict__ val, int64_t nnz,
                                                          int* __restrict__ flag) {
  bool bad = false;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < nnz; i += int64_t(gridDim.x) * blockDim.x) {
    const double v = val[i];
    bad |= !(double(static_cast<float>(v)) == v);
  }
  if (bad) atomicOr(flag, 1);
}

// Bytes per stored value of the passes a plan build may narrow (dense, window
// and jagged plans): the handle's policy (krcn_csr_set_value_storage), decided
// once per build.
template <typename T>
static krcn_status stored_value_bytes(const krcn_csr* h, hipStream_t s, size_t* vs) {
  *vs = sizeof(T);
  if (sizeof(T) == 4 || h->values == KRCN_VALUES_FULL) return KRCN_OK;
  if (h->values == KRCN_VALUES_F32_EXACT && h->nnz > 0) {
    DevTmp<int> flag;
    CHK(flag.alloc(sizeof(int)));
    HIPCHK(hipMemsetAsync(flag.p, 0, sizeof(int), s));
    const int64_t blocks = (h->nnz + 255) / 256;
    hipLaunchKernelGGL(k_values_f32_exact, dim3(unsigned(std::min<int64_t>(blocks, 4096))), dim3(256), 0, s,
                       static_cast<const double*>(h->val), h->nnz, flag.p);
    LAUNCHCHK();
    int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (bad) return KRCN_OK;
  }
  *vs = 4;
  return KRCN_OK;
}

// The format policy of one pass: krcn_csr_set_pass_format over
// krcn_csr_set_format, under the A/B knobs KRCN_FMT1 / KRCN_FMT2 (KRCN_FORMAT_*
// values; unset keeps the handle's).
static int pass_format(const krcn_csr* h, int pass) {
  int fmt = h->format_pass[pass - 1] >= 0 ? h->format_pass[pass - 1] : h->format;
  static const int f1 = tuning_value("KRCN_FMT1", -1);
  static const int f2 = tuning_value("KRCN_FMT2", -1);
  const int f = pass == 2 ? f2 : f1;
  if (f >= KRCN_FORMAT_AUTO && f <= KRCN_FORMAT_DENSE) fmt = f;
  return fmt;
}

extern "C" krcn_status krcn_dense_geometry(int64_t rows, int64_t cols, int dtype, int lanes, int slicing,
                                           int64_t* out_host) {
  if (!out_host) return fail(KRCN_ERR_INVALID, "krcn_dense_geometry: null argument");
  if (rows < 0 || cols < 0 || rows > INT32_MAX || cols > INT32_MAX || (dtype != KRCN_F64 && dtype != KRCN_F32))
    return fail(KRCN_ERR_INVALID, "krcn_dense_geometry: expected 0 <= rows, cols < 2^31 and a KRCN_F64 / KRCN_F32 dtype");
  const bool lanes_ok = lanes == KRCN_LANES_AUTO || lanes == KRCN_LANES_SEQUENTIAL ||
                        (lanes >= 2 && lanes <= 64 && (lanes & (lanes - 1)) == 0);
  const bool slicing_ok = slicing == KRCN_SLICING_AUTO || slicing == KRCN_SLICING_OFF || (slicing >= 8 && slicing % 8 == 0);
  if (!lanes_ok || !slicing_ok)
    return fail(KRCN_ERR_INVALID, "krcn_dense_geometry: lanes and slicing as krcn_csr_set_lanes / krcn_csr_set_slicing take them");
  const DenseGeom g = dense_geometry(rows, cols, dtype == KRCN_F64 ? 8 : 4, lanes, slicing);
  out_host[0] = g.ld;
  out_host[1] = g.L;
  out_host[2] = g.S;
  out_host[3] = g.width;
  out_host[4] = g.groups;
  out_host[5] = g.grid;
  out_host[6] = g.bytes;
  out_host[7] = g.nvec;
  return KRCN_OK;
}

template <typename T>
static krcn_status build_plan(krcn_csr* h, int pass, int rows, int64_t cols, int64_t nnz, const int* ptr,
                              const int* idx, const T* val, int lanes, size_t csr_vs, hipStream_t s) {
  // csr_vs: bytes per stored value of a window or jagged plan (build_plans:
  // sizeof(T), or the build's stored width when the other pass narrows too)
  PassPlan& P = pass == 2 ? h->p2 : h->p1;
  reset_plan(P, rows, cols, nnz, sizeof(T));
  const bool seq = lanes == KRCN_LANES_SEQUENTIAL;
  const int fmt = pass_format(h, pass);
  if (fmt == KRCN_FORMAT_DENSE) {
    if (h->shard != KRCN_SHARD_NONE)
      return fail(KRCN_ERR_UNSUPPORTED, "the dense format does not run on a sharded handle");
    return with_stored_type<T>(h->store_vs, [&](auto ts) {
      return build_dense_as<T, decltype(ts)>(P, ptr, idx, val, lanes, h->slicing, s);
    });
  }
  // the pass's CSR row pointers, once for every layout below
  std::vector<int> hp;
  CHK(host_ptr(ptr, size_t(rows) + 1, s, &hp));
  // jagged format: forced, or by the auto policy (its summation order is
  // scipy's, so the sequential lane policy may use it too)
  if (fmt == KRCN_FORMAT_JAG ||
      (fmt == KRCN_FORMAT_AUTO && h->slicing == KRCN_SLICING_AUTO && jag_choice<T>(rows, cols, nnz, pass))) {
    const krcn_status r = with_stored_type<T>(csr_vs, [&](auto ts) {
      return build_jag_as<T, decltype(ts)>(P, ptr, idx, val, pass, seq, hp, s);
    });
    if (r != KRCN_ERR_UNSUPPORTED || fmt == KRCN_FORMAT_JAG) return r;
    reset_plan(P, rows, cols, nnz, sizeof(T));
  }
  // LDS-window format: forced, or by the auto policy (never under the
  // sequential lane policy, whose sliced passes must stay unsliced)
  {
    int wc = 0;
    if (fmt == KRCN_FORMAT_WINDOW) {
      wc = window_forced<T>(cols);
    } else if (fmt == KRCN_FORMAT_AUTO && !seq && h->slicing == KRCN_SLICING_AUTO) {
      wc = window_choice(rows, cols, nnz, sizeof(T));
    }
    if (wc) {
      const krcn_status r = with_stored_type<T>(csr_vs, [&](auto ts) {
        return build_window_as<T, decltype(ts)>(P, ptr, idx, val, wc == 1, s);
      });
      if (r != KRCN_ERR_UNSUPPORTED || fmt == KRCN_FORMAT_WINDOW) return r;
      reset_plan(P, rows, cols, nnz, sizeof(T));   // not applicable to this matrix: fall through to the other formats
    }
  }
  // wave or sorted tiles
  const TilePolicy tp = tile_policy(rows, cols, nnz,
                                    TilePolicyIn{fmt, pass, lanes, h->slicing, h->sort_nt, h->shard != KRCN_SHARD_NONE,
                                                 h->p1_unsliced, sizeof(T)},
                                    hp.data());
  P.S = tp.S;
  P.kind = tp.sorted ? KRCN_PLAN_SORTED : KRCN_PLAN_WAVE;
  P.sort_nt = tp.sort_nt;
  P.groups = tp.groups;
  P.L = tp.L;
  if (P.S == 1) {
    P.ptr = ptr;
    P.idx = idx;
    P.val = val;
  } else {
    CHK(build_slices<T>(P, ptr, idx, val, s));
    CHK(P.own.alloc(&P.part, sizeof(T) * size_t(P.S) * std::max(rows, 1)));
    CHK(host_ptr(P.ptr, size_t(P.S) * rows + 1, s, &hp));   // slice-major from here on
  }
  const TileLayout tl = tile_layout(rows, cols, tp, hp.data());
  CHK(build_tiles(P, tl, s));
  if (tp.sorted) CHK(build_sorted<T>(P, tl.segs, tl.segbase, s));
  return KRCN_OK;
}

template <typename T>
static krcn_status build_plans(krcn_csr* h, bool lz2, hipStream_t s) {
  h->store_vs = sizeof(T);
  if (h->shard == KRCN_SHARD_NONE) CHK(stored_value_bytes<T>(h, s, &h->store_vs));   // (one scan per build)
  // dense passes: the images must fit the device's free memory (with what the
  // plans about to be replaced give back), checked before anything is
  // allocated or freed so that a refusal leaves the handle as it was
  {
    const bool dn[2] = {pass_format(h, 1) == KRCN_FORMAT_DENSE, pass_format(h, 2) == KRCN_FORMAT_DENSE};
    if ((dn[0] || dn[1]) && h->shard == KRCN_SHARD_NONE) {
      const int64_t b1 = dn[0] ? dense_geometry(h->n, h->d, h->store_vs, h->lanes_x, h->slicing).bytes : 0;
      const int64_t b2 = dn[1] ? dense_geometry(h->d, h->n, h->store_vs, h->lanes_xt, h->slicing).bytes : 0;
      const int64_t need = b1 > INT64_MAX - b2 ? INT64_MAX : b1 + b2;
      size_t mfree = 0, mtotal = 0;
      HIPCHK(hipMemGetInfo(&mfree, &mtotal));
      const size_t avail = mfree + h->p1.own.bytes() + h->p2.own.bytes();
      if (uint64_t(need) > uint64_t(avail))
        return fail(KRCN_ERR_UNSUPPORTED, "the dense format needs %lld bytes of images for this %lld x %lld matrix, "
                    "the device has %lld bytes free", (long long)need, (long long)h->n, (long long)h->d,
                    (long long)avail);
      free_plan(h->p1);   // (both before either image is allocated: the peak holds no old plan)
      free_plan(h->p2);
    }
  }
  // One matrix per operator: a window or jagged pass narrows only beside a
  // pass that narrows too (dense, window or jagged), so no plan pair computes
  // A32^T diag(w) A.  Pass 2 is built first at the build's stored width; pass
  // 1 takes that width when pass 2 came out a narrowing kind, and pass 2 is
  // rebuilt at full width when pass 1 did not (an AUTO plan like rcv1's:
  // sorted pass 1, jagged pass 2).  The formats' choices do not depend on the
  // width, so the rebuilt plan has the same kind and geometry.  (A dense image
  // narrows whatever its partner is: the dense + wave mix keeps that.)
  auto pass2 = [&](size_t vs) {
    return build_plan<T>(h, 2, int(h->d), h->n, h->nnz, h->tptr, h->tidx, static_cast<const T*>(h->tval), h->lanes_xt,
                         vs, s);
  };
  CHK(pass2(h->store_vs));
  h->p1_unsliced = lz2 && h->p2.kind == KRCN_PLAN_JAG && h->p2.S == 1 && h->shard == KRCN_SHARD_NONE;
  CHK(build_plan<T>(h, 1, int(h->n), h->d, h->nnz, h->ptr, h->idx, static_cast<const T*>(h->val), h->lanes_x,
                    plan_narrows(h->p2.kind) ? h->store_vs : sizeof(T), s));
  if (h->p2.vbytes != int(sizeof(T)) && h->p2.kind != KRCN_PLAN_DENSE && !plan_narrows(h->p1.kind)) CHK(pass2(sizeof(T)));
  return KRCN_OK;
}

krcn_status ensure_plans(krcn_csr* h) {
  if (h->plans_ready) return KRCN_OK;
  std::lock_guard<std::mutex> lk(build_mutex());
  h->rows_pq = -1;   // new plans: row shards agree again (agree_rows)
  lzp_abort(h);      // (and the Lanczos-call placement search starts over)
  h->lzp_best = -1;
  h->lzp_ran = 0;
  hipStream_t s = nullptr;
  HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  // pass 2 first: whether it is a single-window jagged plan may decide pass
  // 1's slicing.  Off by default: unslicing rcv1's sorted pass 1 for the
  // two-launch step ran 33.4-34.1 k HVP/s against 43.3-44.2 k for the sliced
  // pass + combine (pass 1 16 against 10 us, pass 2 13.7 against 10.3 us;
  // profiles/r04_rcv1_lz2.txt).  A/B knob KRCN_LZ2=1 turns it on (the step
  // itself reads the same knob the other way round: krcn_lzstep.hpp LzKnobs::lz2).
  static const bool lz2_env = tuning_off("KRCN_LZ2");
  krcn_status r = h->dtype == KRCN_F64 ? build_plans<double>(h, lz2_env, s) : build_plans<float>(h, lz2_env, s);
  (void)hipStreamDestroy(s);
  CHK(r);
  // size the partials buffers to the plans' largest reducing grid (an
  // accumulate-mode window plan over a tall X^T can run up to 64 x 256 blocks)
  int64_t need = kMaxPartials;
  for (const PassPlan* P : {&h->p1, &h->p2}) need = std::max<int64_t>(need, std::max(P->grid, P->combine_grid));
  if (need > h->pcap) {
    for (double** b : {&h->pa, &h->pb, &h->pz, &h->pq}) {
      CHK(h->own.release(b));
      CHK(dalloc(h, b, size_t(need)));
    }
    h->pcap = need;
  } else if (!h->pz) {   // the fused step B's ||z||^2 (early-alpha step: z.v) and the combine's alpha partials
    CHK(dalloc(h, &h->pz, size_t(h->pcap)));
    CHK(dalloc(h, &h->pq, size_t(h->pcap)));
  }
  h->p1.pcap = h->p2.pcap = h->pcap;
#if KRCN_FOLD
  CHK(h->own.release(&h->fcnt));
  if (h->p1.kind == KRCN_PLAN_WINDOW_SLICES && h->p1.ntiles > 0) {   // tickets (ntiles), then the per-block won lists
    const size_t cnt = size_t(h->p1.ntiles) * size_t(kFoldPad + h->p1.grid);
    CHK(h->own.alloc(&h->fcnt, sizeof(int) * cnt));
    HIPCHK(hipMemset(h->fcnt, 0, sizeof(int) * cnt));
  }
#endif
  h->plans_ready = true;
  ++h->ws_gen;   // a recorded Lanczos graph points into the old plans
  return tune_placement(h);
}

krcn_status reserve_reorth(krcn_csr* h, int m) {
  // dot partials: k_cgs_rowdots (chunks x rows, <= kCgsRdParts + rows) in
  // pr, k_cgs_update_dots ((column slabs) x rows) in pr2
  if (m <= h->reorth_m) return KRCN_OK;
  std::lock_guard<std::mutex> lk(build_mutex());
  const int64_t cap = ((h->d + kCgsUpdCols - 1) / kCgsUpdCols) * int64_t(m);
  CHK(h->own.release(&h->pr));
  CHK(h->own.release(&h->pr2));
  h->pr_cap = 0;
  h->prv_cap = 0;
  h->reorth_m = 0;
  // chunk partials of either path: the batched k_cgs_rowdots (C k <= kCgsRdPartsV)
  // and k_cgs_rowdots_v (C k, C = the 1 KiB-piece chunks of a row: past
  // 16 x 16 x 256 vectors a row takes more than kCgsRdChunksV of them)
  const int64_t nv = h->d / int64_t(16 / h->vs);
  const int64_t cv = std::max<int64_t>(kCgsRdChunksV, nv > 0 ? cgs_rdv_chunks_of(nv) : 0);
  const int64_t prv = std::max<int64_t>(kCgsRdPartsV, cv * m) + 4 * int64_t(m);
  CHK(dalloc(h, &h->pr, size_t(prv)));
  h->prv_cap = prv;
  CHK(dalloc(h, &h->pr2, size_t(cap)));
  // k_cgs_colsweep: the row ranges of a sweep over up to m - 1 rows (one range
  // needs no partials), V^T h partials of each, and one arrival counter per
  // 64-vector column group; not allocated where the 1 KiB-piece path never
  // runs (column shards, rows not whole 16-byte vectors)
  CHK(h->own.release(&h->cy));
  CHK(h->own.release(&h->ccnt));
  h->cy_q = 0;
  const int q = cgs_col_ranges(m);
  if (q > 1 && h->shard != KRCN_SHARD_COLS && h->d % int64_t(16 / h->vs) == 0) {
    const int64_t ncg = (h->d + 63) / 64;   // >= the column groups of either dtype
    CHK(dalloc(h, &h->cy, size_t(q) * size_t(h->d)));
    CHK(dalloc(h, &h->ccnt, size_t(ncg)));
    HIPCHK(hipMemsetAsync(h->ccnt, 0, sizeof(int) * size_t(ncg), nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));   // zero before any stream of the handle counts on it
    h->cy_q = q;
  }
  h->pr_cap = cap;
  h->reorth_m = m;
  ++h->ws_gen;
  return KRCN_OK;
}

extern "C" krcn_status krcn_csr_reserve(krcn_csr* h, int m_max, int reorth) {
  if (!h) return fail(KRCN_ERR_INVALID, "krcn_csr_reserve: null handle");
  if (m_max < 1 || m_max > kLzMaxM) return fail(KRCN_ERR_INVALID, "krcn_csr_reserve: m_max must be 1..%d", kLzMaxM);
  CHK(set_device(h));
  CHK(ensure_plans(h));
  CHK(agree_rows(h));   // (outside the build lock: virtual ranks are threads of one process)
  if (reorth) CHK(reserve_reorth(h, m_max));
  if (h->shard == KRCN_SHARD_NONE) CHK(ensure_crn_ws(h));   // krcn_crn_step's state and subproblem vectors
  return KRCN_OK;
}
