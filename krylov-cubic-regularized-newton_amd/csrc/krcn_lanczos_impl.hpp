// krcn_lanczos_impl.hpp — the device Lanczos recurrence of cubic.py:77-111
// (included once per dtype by krcn_lanczos_f64.hip / krcn_lanczos_f32.hip).
// Which step a handle runs is decided in krcn_lzstep.hpp (lanczos_step); this
// file holds one launch sequence per step and the loop that enqueues them.
#pragma once
#include "krcn_internal.hpp"

// ------------------------------------------------------------- Lanczos
// The recurrence allocates nothing: the alphas | betas | state block and the
// CGS2 coefficients exist from krcn_csr_create (m <= kLzMaxM), the CGS2 dot
// partials from krcn_csr_reserve (reserve_reorth, krcn_plan.hip).  An
// unsharded handle reserves them on its first reorthogonalised call; a handle
// of a multi-rank communicator must have reserved them before the collectives.
static krcn_status check_lanczos_ws(krcn_csr* h, int m, int reorth) {
  if (m > h->mcap) return fail(KRCN_ERR_UNSUPPORTED, "krcn_lanczos: m = %d exceeds %d", m, h->mcap);
  if (!reorth || m <= h->reorth_m) return KRCN_OK;
  if (h->comm && h->comm->nranks > 1)
    return fail(KRCN_ERR_INVALID, "krcn_lanczos: reorthogonalisation workspace reserved for m <= %d, not %d: call "
                "krcn_csr_reserve(h, m, 1) before the recurrence on a sharded handle", h->reorth_m, m);
  return reserve_reorth(h, m);
}

// step B operands for the fused first sweep (k_cgs_rowdots_vb)
template <typename T> struct CgsStepB {
  const T* W; const double* pa; int Pa;
};

// The 1 KiB-piece CGS2 path applies: unsharded, rows of whole 16-byte
// vectors, aligned, at most pcap column groups, the k_cgs_rowdots_v chunk
// partials of a k-row sweep within pr and its row ranges within cy (both
// sized by reserve_reorth; tuning knob KRCN_CGS_1K=0 keeps the batched
// round-3 kernels for A/B).
template <typename T>
static bool cgs_vec_ok(const krcn_csr* h, const T* V, const T* z, bool over_ranks, int k) {
  static const bool env = tuning_on("KRCN_CGS_1K");
  constexpr int E = Vec16<T>::E;
  const int64_t d = h->d;
  const int64_t ncg = (d / E + 63) / 64;
  if (!env || over_ranks || d % E != 0 || ncg > h->pcap) return false;
  if (int64_t(cgs_rdv_chunks_of(d / E)) * k + 4 * int64_t(k) > h->prv_cap) return false;
  const int q = cgs_col_ranges(k);
  if (q > 1 && (q > h->cy_q || !h->cy || !h->ccnt)) return false;
  return reinterpret_cast<uintptr_t>(V) % 16 == 0 && reinterpret_cast<uintptr_t>(z) % 16 == 0;
}

// The three sweeps of the 1 KiB-piece path: row dots over C chunks of S
// steps, the column sweep over ncg column groups, both again with the norm.
template <typename T>
static void cgs_colsweeps(krcn_csr* h, const T* V, int k, T* z, int C, int S, int ncg, const CgsStepB<T>* sb,
                          hipStream_t s) {
  const int64_t d = h->d;
  // a colsweep block walks NB batches of 4 U rows (default 8 x 32 = 256-row
  // ranges: profiles/r04_cgs2_ab.txt; tuning knob KRCN_CGS_NB = 1, 2, 4, 8, 16)
  const int U = cgs_col_unroll(k, cgs_umax()), NB = cgs_nb();
  const int Q = (k + 4 * U * NB - 1) / (4 * U * NB);   // = cgs_col_ranges(k) (cgs_vec_ok checked cy holds them)
  auto rowdots = [&](const T* zz) {
    with_pow2(S, [&](auto sc) {
      hipLaunchKernelGGL((k_cgs_rowdots_v<T, decltype(sc)::value>), dim3(C, k), dim3(kNT), 0, s, d, k, V, zz, h->pr,
                         h->st);
    });
  };
  if (sb) {   // z = V[k] is formed (step B) by the first sweep itself
    with_pow2(S, [&](auto sc) {
      hipLaunchKernelGGL((k_cgs_rowdots_vb<T, decltype(sc)::value>), dim3(C, k), dim3(kNT), 0, s, d, k,
                         const_cast<T*>(V), sb->W, sb->pa, sb->Pa, h->alphas_dev, h->pr, h->st);
    });
  } else {
    rowdots(z);
  }
  auto colsweep = [&](auto norm) {
    with_pow2(U, [&](auto uc) {
      with_pow2(NB, [&](auto nb) {
        hipLaunchKernelGGL((k_cgs_colsweep<T, decltype(uc)::value, decltype(norm)::value, decltype(nb)::value>),
                           dim3(ncg, Q), dim3(kNT), 0, s, d, k, V, static_cast<const double*>(h->pr), C, z, h->cy,
                           h->ccnt, h->pb, h->st);
      });
    });
  };
  colsweep(std::false_type{});
  rowdots(z);
  colsweep(std::true_type{});
}

// CGS2 of z against V[0..k) (krcn_cgs2.hpp): three sweeps over V; the
// ||z||^2 partials land in h->pb, their count in *Pnorm.
template <typename T>
static krcn_status reorth_cgs2(krcn_csr* h, const T* V, int k, T* z, bool over_ranks, int* Pnorm, hipStream_t s,
                               const CgsStepB<T>* sb = nullptr) {
  const int64_t d = h->d;
  const int n3 = int((d + kCgsUpdCols - 1) / kCgsUpdCols);
  const int cgrid = (k + kCgsHPad + kCgsCoefRows - 1) / kCgsCoefRows;
  if (k > kCgsKMax) return fail(KRCN_ERR_UNSUPPORTED, "CGS2: more than 2048 basis vectors");
  constexpr int E = Vec16<T>::E;
  const int64_t ncg = (d / E + 63) / 64;   // k_cgs_colsweep column groups: one ||z||^2 partial each
  const bool vec_ok = cgs_vec_ok<T>(h, V, z, over_ranks, k);
  if (sb && !vec_ok) return fail(KRCN_ERR_UNSUPPORTED, "CGS2: step B fused into a sweep the path does not run");
  if (vec_ok) {
    const int64_t nv = d / E;
    const int S = cgs_rdv_steps(nv, k);
    *Pnorm = int(ncg);
    cgs_colsweeps<T>(h, V, k, z, cgs_rdv_chunks(nv, S), S, int(ncg), sb, s);
    LAUNCHCHK();
    return KRCN_OK;
  }
  const int C = cgs_rd_chunks(d, k);
  {
    const int64_t cw = (d + C - 1) / C;
    hipLaunchKernelGGL((k_cgs_rowdots<T>), dim3(C, (k + kCgsRdRows - 1) / kCgsRdRows), dim3(kCgsRdNT), 0, s, d, k,
                       cw, V, static_cast<const T*>(z), h->pr, h->st);
  }
  LAUNCHCHK();
  if (over_ranks) {
    // the chunk partials are per rank: sum them to h1 first, all-reduce, and
    // hand the update the global h1 as a single chunk
    hipLaunchKernelGGL(k_cgs_coeffs, dim3(cgrid), dim3(kCgsCoefNT), 0, s, h->pr, C, k, h->hcoef, h->st);
    LAUNCHCHK();
    CHK(allreduce(h, h->hcoef, k, KRCN_F64, s));
    HIPCHK(hipMemcpyAsync(h->pr, h->hcoef, size_t(k) * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  const int Cu = over_ranks ? 1 : C;
  const bool cached = int64_t(k) * kCgsSlabLd * int64_t(sizeof(T)) <= kCgsCacheBytes;
  const int gn = int(std::min<int64_t>((d + kCgsNormCols - 1) / kCgsNormCols, kMaxPartials));
  *Pnorm = gn;
  const double* h1 = static_cast<const double*>(h->pr);
  with_pow2(cgs_unroll(k), [&](auto uc) {
    constexpr int U = decltype(uc)::value;
    const size_t lds = cgs_upd_lds<T>(k, U, Cu, cached);
    if (cached)
      hipLaunchKernelGGL((k_cgs_update_dots<T, true, U>), dim3(n3), dim3(kCgsUpdNT), lds, s, d, k, V, h1, Cu, z,
                         h->pr2, h->st);
    else
      hipLaunchKernelGGL((k_cgs_update_dots<T, false, U>), dim3(n3), dim3(kCgsUpdNT), lds, s, d, k, V, h1, Cu, z,
                         h->pr2, h->st);
  });
  LAUNCHCHK();
  hipLaunchKernelGGL(k_cgs_coeffs, dim3(cgrid), dim3(kCgsCoefNT), 0, s, h->pr2, n3, k, h->hcoef, h->st);
  LAUNCHCHK();
  if (over_ranks) CHK(allreduce(h, h->hcoef, k, KRCN_F64, s));
  with_pow2(cgs_norm_unroll(k), [&](auto uc) {
    hipLaunchKernelGGL((k_cgs_update_norm<T, decltype(uc)::value>), dim3(gn), dim3(kCgsUpdNT), 0, s, d, k, V,
                       static_cast<const double*>(h->hcoef), z, h->pb, h->st);
  });
  LAUNCHCHK();
  return KRCN_OK;
}

// Make the partials `*p` (*P entries) global across ranks when the reduced
// space is sharded: collapse them to one scalar in h->scal[slot], all-reduce
// it there, and point the consumer at it (*p = that slot, *P = 1).
static krcn_status globalise(krcn_csr* h, double** p, int* P, int slot, hipStream_t s) {
  hipLaunchKernelGGL((k_finish<0>), dim3(1), dim3(kNT), 0, s, *p, *P, h->scal + slot);
  LAUNCHCHK();
  CHK(allreduce(h, h->scal + slot, 1, KRCN_F64, s));
  *p = h->scal + slot;
  *P = 1;
  return KRCN_OK;
}

// ----------------------------------------------------- one recurrence
// What the steps of one recurrence share.
template <typename T> struct LzRun {
  krcn_csr* h;
  hipStream_t s;
  LzStepChoice ch;
  LzCtl<T> c;             // c.j: the step; c.pnorm / c.Pnorm: the ||z_j||^2 partials the next consumer reads
  const T* w;
  T *W, *u;
  T tn, tl2;              // n_global and l2 as the epilogues take them
  double l2;
  int reorth;
  int Pa_prev = 0;        // partials of the previous step's pass 2 (v.w; early steps: z.v)
  double* pa_g = nullptr; // v.w partials as the consumers read them (globalise may redirect)
  bool packed = false;    // u[n] holds this rank's ||z_j||^2 for the coming step (LzStepChoice::pack)

  T* vj(int j) const { return c.V + int64_t(j) * c.ld; }
  double* unorm() const { return static_cast<double*>(h->u) + h->n; }   // the packed d-space sums past u's n rows
  bool cols() const { return h->shard == KRCN_SHARD_COLS; }             // d-space dots need a rank sum
};

// The pass-2 epilogue of a step: step A (EpiLz2, w into W), or the early
// steps' step A + B (EpiLz2E, their z.v partials into part2).
template <class E, typename T>
static E lz_epi2(const LzRun<T>& r, double* part2 = nullptr) {
  E e{};
  e.c = r.c;
  e.n = r.tn;
  e.l2 = r.tl2;
  if constexpr (std::is_same<E, EpiLz2<T>>::value) e.W = r.W;
  else e.part2 = part2;
  return e;
}

// One step between its profiling events: e0, pass1(record), e1, pass2(), e2
// (run_pass records em between pass 1's main launch and its combine).
template <typename T, class P1, class P2>
static krcn_status lz_profiled(LzRun<T>& r, P1&& pass1, P2&& pass2) {
  ProfRec* pr = prof_next(r.h);
  if (pr) HIPCHK(hipEventRecord(pr->e0, r.s));
  CHK(pass1(pr));
  if (pr) HIPCHK(hipEventRecord(pr->e1, r.s));
  CHK(pass2());
  if (pr) HIPCHK(hipEventRecord(pr->e2, r.s));
  return KRCN_OK;
}

// generic: one HVP + step A on the step's vector (mode 0: loop step j, 1: the
// final quotient); partials of v.w land in h->pa.
template <typename T>
static krcn_status step_generic(LzRun<T>& r, int mode, int* Pa) {
  krcn_csr* h = r.h;
  hipStream_t s = r.s;
  LzCtl<T>& c = r.c;
  const int64_t n = h->n, d = h->d;
  T* u = r.u;
  c.mode = mode;
  const SrcLzState<T> later{c, {}};
  const SrcGuard<T> src2{u, h->st, mode};
  CHK(lz_profiled(r, [&](ProfRec* pr) -> krcn_status {
    const EpiLz1<T> e1{r.w, u, T(1)};
    if (r.cols() && mode == 0 && r.packed) {
      // Column shards, packed norm: pass 1 gathers z unnormalised without the
      // beta prologue (SrcGuard), and the row apply after the all-reduce runs
      // it (SrcLzStep: beta, the breakdown test, the state) from u[n]
      const SrcGuard<T> zsrc{r.vj(c.j), h->st, 0};
      CHK(run_pass<T>(h->p1, zsrc, zsrc, EpiStore<T>{u}, nullptr, nullptr, s, pr));
      CHK(allreduce(h, u, n + 1, h->dtype, s));
      LzCtl<T> cp = c;
      cp.pnorm = r.unorm();
      cp.Pnorm = 1;
      hipLaunchKernelGGL((k_rows_apply<T, SrcLzStep<T>, EpiLz1<T>>), dim3(apply_grid(n)), dim3(kNT), 0, s, int(n),
                         static_cast<const T*>(u), SrcLzStep<T>{cp, {}}, e1, static_cast<double*>(nullptr));
      LAUNCHCHK();
    } else if (r.cols()) {
      // raw X_p z_p, all-reduced, then u = w (t / div)
      if (mode == 0) CHK(run_pass<T>(h->p1, SrcLzStep<T>{c, {}}, later, EpiStore<T>{u}, nullptr, nullptr, s, pr));
      else CHK(run_pass<T>(h->p1, later, later, EpiStore<T>{u}, nullptr, nullptr, s, pr));
      CHK(allreduce(h, u, n, h->dtype, s));
      hipLaunchKernelGGL((k_rows_apply<T, SrcLzState<T>, EpiLz1<T>>), dim3(apply_grid(n)), dim3(kNT), 0, s, int(n),
                         static_cast<const T*>(u), later, e1, static_cast<double*>(nullptr));
      LAUNCHCHK();
    } else if (mode == 0) {
      CHK(run_pass<T>(h->p1, SrcLzStep<T>{c, {}}, later, e1, nullptr, nullptr, s, pr));
    } else {
      CHK(run_pass<T>(h->p1, later, later, e1, nullptr, nullptr, s, pr));
    }
    return KRCN_OK;
  }, [&]() -> krcn_status {
    const EpiLz2<T> e2 = lz_epi2<EpiLz2<T>>(r);
    if (h->shard != KRCN_SHARD_ROWS) return run_pass<T>(h->p2, src2, src2, e2, h->pa, Pa, s);
    // the raw X_p^T u_p partial is all-reduced before step A runs
    T* raw = static_cast<T*>(h->td);
    CHK(run_pass<T>(h->p2, src2, src2, EpiStore<T>{raw}, nullptr, nullptr, s));
    CHK(allreduce(h, raw, d, h->dtype, s));
    *Pa = apply_grid(d);
    hipLaunchKernelGGL((k_rows_apply<T, SrcGuard<T>, EpiLz2<T>>), dim3(*Pa), dim3(kNT), 0, s, int(d),
                       static_cast<const T*>(raw), src2, e2, h->pa);
    LAUNCHCHK();
    return KRCN_OK;
  }));
  r.pa_g = h->pa;
  if (r.cols()) CHK(globalise(h, &r.pa_g, Pa, 2, s));
  return KRCN_OK;
}

// early (window-slices or sliced sorted-tile pass 1; krcn_kernels.hpp
// EpiLz2E): pass 1 (SrcLzBeta: block 0 settles beta_{j-1} from pass 2's
// ||z_j||^2 partials, the breakdown test) gathers the stored z_j alone, its
// combine also forms the partials of (X v_j).(w X v_j), pass 2 settles
// alpha_j from them in its prologue and runs step B in its epilogue (v_j,
// z_{j+1} into V[j+1], their partials).  The z.v partials alternate between
// pa and pz: pass 2 of step j reads step j-1's while it writes.
template <typename T>
static krcn_status step_early(LzRun<T>& r) {
  krcn_csr* h = r.h;
  LzCtl<T>& c = r.c;
  const int j = c.j;
  c.mode = 0;
  int Pq = 0, Pa = 0;
  CHK(lz_profiled(r, [&](ProfRec* pr) -> krcn_status {
#if KRCN_FOLD
    if (std::is_same<T, double>::value && fold_ok(h)) {   // the slice combine folded into pass 1
      EpiSliceFold<T> ef{static_cast<T*>(h->p1.part), int64_t(h->p1.rows), h->fcnt, h->fcnt + int64_t(h->p1.ntiles) * kFoldPad,
                         nullptr, h->p1.ntiles, h->pq, r.w, r.u, c, h->p1.S};
      Pq = h->p1.ntiles;
      return run_fold_pass1<T>(h, SrcLzBeta<T>{c, {}}, ef, r.s);
    }
#endif
    return run_pass<T>(h->p1, SrcLzBeta<T>{c, {}}, SrcLzState<T>{c, {}}, EpiLz1A<T>{r.w, r.u, T(1)}, h->pq, &Pq, r.s, pr);
  }, [&]() -> krcn_status {
    const double* zv_in = (j & 1) ? h->pa : h->pz;
    const SrcLzAlpha<T> asrc{r.u, h->st, h->pq, Pq, zv_in, r.Pa_prev, h->alphas_dev, j, double(h->n_global), r.l2};
    return run_pass<T>(h->p2, asrc, asrc, lz_epi2<EpiLz2E<T>>(r, (j & 1) ? h->pz : h->pa), h->pb, &Pa, r.s);
  }));
  r.Pa_prev = Pa;
  c.pnorm = h->pb;   // ||z_{j+1}||^2: the next pass 1, or the final check
  c.Pnorm = Pa;
  return KRCN_OK;
}

// early-cols (news20 on 8 GPUs), fp64: one collective per step.  The row
// sums t = X z_j are all-reduced with this rank's ||z_p||^2 and z_p . v_p
// packed as elements n and n + 1; the row apply (replicated over n on every
// rank) settles beta and forms u with the partials of u.q, which are then
// the same on every rank — so pass 2 settles alpha_j in its prologue
// (SrcLzAlpha) and runs steps A and B in its epilogue (EpiLz2E) with no
// scalar all-reduce and no step-B launch.
template <typename T>
static krcn_status step_early_cols(LzRun<T>& r) {
  krcn_csr* h = r.h;
  hipStream_t s = r.s;
  LzCtl<T>& c = r.c;
  const int j = c.j;
  const int64_t n = h->n;
  c.mode = 0;
  const int Pr = apply_grid(n);
  int Pa = 0;
  CHK(lz_profiled(r, [&](ProfRec* pr) -> krcn_status {
    // (j = 0 runs unguarded: the state still holds the previous call's
    // flag until the row apply's prologue resets it)
    const SrcGuard<T> zsrc{j == 0 ? c.g : r.vj(j), h->st, j == 0 ? 1 : 0};
    if (j == 0) {
      CHK(run_pass<T>(h->p1, zsrc, zsrc, EpiStore<T>{r.u}, nullptr, nullptr, s, pr));
    } else {
      const SrcGuardPack<T> psrc{r.vj(j), h->st, h->pb, h->pz, r.Pa_prev, r.unorm()};
      CHK(run_pass<T>(h->p1, psrc, zsrc, EpiStore<T>{r.u}, nullptr, nullptr, s, pr));
    }
    // u[n] = ||z_p||^2, u[n + 1] = z_p . v_{p,j-1}: packed by pass 1's block 0
    // from the previous pass 2's partials (j = 0: ||g||^2 is already global)
    CHK(allreduce(h, r.u, n + (j == 0 ? 0 : 2), h->dtype, s));
    LzCtl<T> cp = c;
    if (j > 0) {
      cp.pnorm = r.unorm();
      cp.Pnorm = 1;
    }
    hipLaunchKernelGGL((k_rows_apply<T, SrcLzStep<T>, EpiLz1A<T>>), dim3(Pr), dim3(kNT), 0, s, int(n),
                       static_cast<const T*>(r.u), SrcLzStep<T>{cp, {}}, EpiLz1A<T>{r.w, r.u, T(1)}, h->pq);
    LAUNCHCHK();
    return KRCN_OK;
  }, [&]() -> krcn_status {
    const SrcLzAlpha<T> asrc{r.u, h->st, h->pq, Pr, r.unorm() + 1, 1, h->alphas_dev, j, double(h->n_global), r.l2};
    return run_pass<T>(h->p2, asrc, asrc, lz_epi2<EpiLz2E<T>>(r, h->pz), h->pb, &Pa, s);
  }));
  if (j + 2 < c.m) {   // the next pass 1 packs the next all-reduce's two d-space sums
    c.pnorm = r.unorm();
    c.Pnorm = 1;
  } else {   // the final check reads ||z_{m-1}||^2 as a global sum
    double* pbp = h->pb;
    int Pb = Pa;
    CHK(globalise(h, &pbp, &Pb, 3, s));
    c.pnorm = pbp;
    c.Pnorm = Pb;
  }
  r.Pa_prev = Pa;
  return KRCN_OK;
}

// early-rows (synth on 8 GPUs), fp64: the same early alpha with the d-vector
// all-reduce carrying the rank's partials of (X v_j).(w X v_j) past element
// d (td holds d + kMaxPartials), so the row apply after it settles alpha_j
// and runs steps A and B in one launch (EpiLz2E: v_j, z_{j+1}, their
// partials) — no k_lz_step_b and no W round trip.  The z_j . v_{j-1}
// partials are d-space, replicated on every rank.
template <typename T>
static krcn_status step_early_rows(LzRun<T>& r) {
  krcn_csr* h = r.h;
  hipStream_t s = r.s;
  LzCtl<T>& c = r.c;
  const int j = c.j, Pc = r.ch.Pc, pq_local = pass_partials(h->p1);
  const int64_t d = h->d;
  c.mode = 0;
  T* raw = static_cast<T*>(h->td);
  double* rq = reinterpret_cast<double*>(raw + d);
  const int Pe = apply_grid(d);
  CHK(lz_profiled(r, [&](ProfRec* pr) -> krcn_status {
    int Pq = 0;
    CHK(run_pass<T>(h->p1, SrcLzStep<T>{c, {}}, SrcLzState<T>{c, {}}, EpiLz1A<T>{r.w, r.u, T(1)}, rq, &Pq, s, pr));
    if (Pq != pq_local)
      return fail(KRCN_ERR_INVALID, "krcn_lanczos: pass 1 wrote %d partials, the plan promised %d", Pq, pq_local);
    return KRCN_OK;
  }, [&]() -> krcn_status {
    // slots [pq_local, Pc) hold the previous all-reduce's sums on this rank: zero them
    if (Pc > pq_local) HIPCHK(hipMemsetAsync(rq + pq_local, 0, sizeof(double) * size_t(Pc - pq_local), s));
    const SrcGuard<T> src2{r.u, h->st, 0};
    CHK(run_pass<T>(h->p2, src2, src2, EpiStore<T>{raw}, nullptr, nullptr, s));
    CHK(allreduce(h, raw, d + Pc, h->dtype, s));
    const double* zv_in = (j & 1) ? h->pa : h->pz;
    const SrcLzAlpha<T> asrc{r.u, h->st, rq, Pc, zv_in, r.Pa_prev, h->alphas_dev, j, double(h->n_global), r.l2};
    hipLaunchKernelGGL((k_rows_apply<T, SrcLzAlpha<T>, EpiLz2E<T>>), dim3(Pe), dim3(kNT), 0, s, int(d),
                       static_cast<const T*>(raw), asrc, lz_epi2<EpiLz2E<T>>(r, (j & 1) ? h->pz : h->pa), h->pb);
    LAUNCHCHK();
    return KRCN_OK;
  }));
  r.Pa_prev = Pe;
  c.pnorm = h->pb;   // ||z_{j+1}||^2: the next pass 1, or the final check
  c.Pnorm = Pe;
  return KRCN_OK;
}

// The control block of a fused pass 2 / combine that settles beta_{j-1}: from
// step 1 on, z_j's norm partials are those of the pass-1 blocks that stored it.
template <typename T>
static LzCtl<T> lz_beta_ctl(const LzRun<T>& r, int writers) {
  LzCtl<T> cb = r.c;
  if (r.c.j > 0) {
    cb.pnorm = r.h->pz;
    cb.Pnorm = writers;
  }
  return cb;
}

// two-launch: pass 1 with step B fused stores u' = w (.) X z_j, and pass 2
// settles beta in every block's prologue and gathers u = u' / beta (SrcLzU),
// where the plain path would run a separate step B.
template <typename T>
static krcn_status step_two_launch(LzRun<T>& r, int* Pa) {
  krcn_csr* h = r.h;
  r.c.mode = 0;
  return lz_profiled(r, [&](ProfRec* pr) -> krcn_status {
    const SrcLzZ<T> zsrc{r.c, static_cast<const T*>(r.W), h->pa, r.Pa_prev, h->alphas_dev, h->pz, T(0), 1};
    return run_pass<T>(h->p1, zsrc, zsrc, EpiWeighted<T>{r.w, r.u}, nullptr, nullptr, r.s, pr);
  }, [&]() -> krcn_status {
    const SrcLzU<T> usrc{lz_beta_ctl(r, std::min(h->p1.grid, kNT)), r.u, {}};
    return run_pass<T>(h->p2, usrc, usrc, lz_epi2<EpiLz2<T>>(r), h->pa, Pa, r.s);
  });
}

// fused-window, fused-sorted, fused-small, fused-small-xt: step B fused into
// pass 1.  Pass 1 of step j builds z_j = w - alpha_{j-1} v_{j-1} in its
// windows or gathers (SrcLzZ; one-piece plans: SrcLzSmall, every block forms
// all of z and beta), the slice combine settles beta_{j-1}.
template <typename T>
static krcn_status step_fused(LzRun<T>& r, int* Pa) {
  krcn_csr* h = r.h;
  hipStream_t s = r.s;
  const LzCtl<T>& c = r.c;
  const LzStep step = r.ch.step;
  const bool xt = step == LZ_FUSED_SMALL_XT;
  const T* Wc = static_cast<const T*>(r.W);
  r.c.mode = 0;
  return lz_profiled(r, [&](ProfRec* pr) -> krcn_status {
    const EpiLz1<T> e1{r.w, r.u, T(1)};
    if (step == LZ_FUSED_WINDOW || step == LZ_FUSED_SORTED) {
      // z writers: every block of the window pass, the first kNT of the sorted one.
      // zw: the window-slices pass 1 stores no z_j, pass 2 re-forms it (EpiLz2::zw)
      const int writers = step == LZ_FUSED_WINDOW ? h->p1.grid : std::min(h->p1.grid, kNT);
      const SrcLzZ<T> zsrc{c, Wc, h->pa, r.Pa_prev, h->alphas_dev, h->pz, T(0), r.ch.zw ? 0 : 1};
      return run_pass<T>(h->p1, zsrc, SrcLzStep<T>{lz_beta_ctl(r, writers), {}}, e1, nullptr, nullptr, s, pr);
    }
    const SrcLzSmall<T> zs{c, Wc, h->pa, r.Pa_prev, h->alphas_dev, {}};
    if (!xt) return run_pass<T>(h->p1, zs, zs, e1, nullptr, nullptr, s, pr);
    // pass 1 also forms the blocks' shares of X^T u (EpiLz1X)
    const EpiLz1X<T> ex{r.w, T(1), h->p1.xcp, h->p1.xrow, static_cast<const T*>(h->p1.xval),
                        static_cast<T*>(h->p1.xpart), int(h->d), nullptr, 0};
    return run_pass<T>(h->p1, zs, zs, ex, nullptr, nullptr, s, pr);
  }, [&]() -> krcn_status {
    const SrcGuard<T> src2{r.u, h->st, 0};
    EpiLz2<T> e2 = lz_epi2<EpiLz2<T>>(r);
    if (r.ch.zw) {
      e2.alphas = h->alphas_dev;
      e2.zw = 1;
    }
    // fused-small-xt: pass 2 = the blocks' X^T u partials added in a fixed order, with step A in the epilogue
    if (xt) return run_xt_combine<T>(h->p1, lz_knobs().xt_comb ? lz_knobs().xt_rb : 0, src2, e2, h->pa, Pa, s);
    return run_pass<T>(h->p2, src2, src2, e2, h->pa, Pa, s);
  });
}

// The separate step B after a step that did not fuse it (and after every
// step's last loop iteration but the early ones': k_lz_final_check and the
// final quotient read its z_{m-1} and norm partials): k_lz_step_b, CGS2 when
// reorthogonalising, then the norm partials packed or made global.
template <typename T>
static krcn_status separate_step_b(LzRun<T>& r, int Pa) {
  krcn_csr* h = r.h;
  hipStream_t s = r.s;
  LzCtl<T>& c = r.c;
  const int j = c.j;
  const int64_t d = h->d;
  c.mode = 0;
  int Pb = vec_grid(d);
  T* zn = r.vj(j + 1);
  // a reorthogonalised step on the 1 KiB-piece CGS2 path forms step B inside
  // its first sweep (k_cgs_rowdots_vb): no k_lz_step_b launch
  const bool fuse_b = r.reorth && lz_knobs().cgs_fuseb && cgs_vec_ok<T>(h, c.V, zn, r.cols(), j + 1);
  if (!fuse_b) {
    hipLaunchKernelGGL((k_lz_step_b<T>), dim3(Pb), dim3(kNT), 0, s, d, static_cast<const T*>(r.W), c, r.pa_g, Pa,
                       h->alphas_dev, h->pb);
    LAUNCHCHK();
  }
  if (r.reorth) {
    const CgsStepB<T> sb{static_cast<const T*>(r.W), r.pa_g, Pa};
    CHK(reorth_cgs2<T>(h, c.V, j + 1, zn, r.cols(), &Pb, s, fuse_b ? &sb : nullptr));
  }
  // Column shards, fp64, no reorthogonalisation (LzStepChoice::pack):
  // ||z_{j+1}||^2 travels as element n of the next row-sum all-reduce instead
  // of an all-reduce of its own (2 collectives per step instead of 3).  The
  // last loop step keeps the scalar all-reduce: k_lz_final_check reads that norm.
  r.packed = false;
  double* pbp = h->pb;
  if (r.ch.pack && j + 2 < c.m) {
    hipLaunchKernelGGL((k_finish<0>), dim3(1), dim3(kNT), 0, s, h->pb, Pb, r.unorm());
    LAUNCHCHK();
    r.packed = true;
  } else if (r.cols()) {
    CHK(globalise(h, &pbp, &Pb, 3, s));
  }
  c.pnorm = pbp;
  c.Pnorm = Pb;
  return KRCN_OK;
}

// krcn_csr_set_graph(h, 1) replays repeated Lanczos calls as a hipGraph.
// Off by default: interleaved A/B on the box (profiles/
// r02_graph_ab.txt) measured rcv1 and rcv1_stress equal, w8a within its noise
// and news20 7-8 % slower under replay than the eager stream launches.
static uint64_t bits(double x) {
  uint64_t b;
  std::memcpy(&b, &x, sizeof(b));
  return b;
}

// Submit one call's launch sequence, enqueue(stream).  It depends only on the
// arguments (`key`), the plans and the handle's buffers, so with `graph` a
// call replays it as one hipGraph: recorded on the handle's private stream
// the second time the same key arrives, launched on the caller's stream from
// then on (one submission per call instead of 2-4 dependent launches per
// Lanczos step).  Eager calls run inside the placement search
// (krcn_place.hip lzp_*): *lzp_timed says whether this one was timed.
template <class F>
static krcn_status lz_submit(krcn_csr* h, bool graph, const uint64_t* key, int m, hipStream_t s_call, F&& enqueue,
                             bool* lzp_timed) {
  constexpr int K = krcn_csr::kGraphKey;
  bool replay = false, capture = false;
  if (graph) {
    replay = h->gexec && std::equal(key, key + K, h->gkey);
    capture = !replay && std::equal(key, key + K, h->glast);
    std::copy(key, key + K, h->glast);
  }
  if (replay) {
    HIPCHK(hipGraphLaunch(h->gexec, s_call));
  } else if (capture) {
    if (!h->gstream) HIPCHK(hipStreamCreateWithFlags(&h->gstream, hipStreamNonBlocking));
    HIPCHK(hipStreamBeginCapture(h->gstream, hipStreamCaptureModeThreadLocal));
    const krcn_status r = enqueue(h->gstream);
    hipGraph_t gr = nullptr;
    const hipError_t e = hipStreamEndCapture(h->gstream, &gr);
    if (r != KRCN_OK || e != hipSuccess) {
      if (gr) (void)hipGraphDestroy(gr);
      CHK(r);
      HIPCHK(e);
    }
    if (h->gexec) (void)hipGraphExecDestroy(h->gexec);
    h->gexec = nullptr;
    const hipError_t ei = hipGraphInstantiate(&h->gexec, gr, nullptr, nullptr, 0);
    (void)hipGraphDestroy(gr);
    if (ei != hipSuccess) h->gexec = nullptr;
    HIPCHK(ei);
    std::copy(key, key + K, h->gkey);
    HIPCHK(hipGraphLaunch(h->gexec, s_call));
  } else {
    bool timed = false;
    CHK(lzp_begin(h, m, s_call, &timed));
    CHK(enqueue(s_call));
    CHK(lzp_end(h, s_call, timed));
    *lzp_timed = timed;
  }
  return KRCN_OK;
}

template <typename T>
static krcn_status lanczos_impl(krcn_csr* h, const T* w, const T* g, int m, int reorth, double tol,
                                double l2, T* V, double* alphas_host, double* betas_host,
                                krcn_lanczos_info* info, hipStream_t s_call, bool enqueue_only) {
  const int64_t d = h->d;
  CHK(plans_for_compute(h));
  CHK(check_lanczos_ws(h, m, reorth));
  const LzStepChoice ch = lanczos_step(lz_step_in(h, reorth));
  CHK(ch.refusal);

  // every hot buffer (W, u, the partials) is read in here, after lz_submit's lzp_begin has applied the
  // placement this call runs and times
  auto enqueue = [&](hipStream_t s) -> krcn_status {
    LzRun<T> r{h, s, ch, LzCtl<T>{V, g, d, m, 0, 0, h->st, h->betas_dev, h->pb, 0, tol}, w, static_cast<T*>(h->W),
               static_cast<T*>(h->u), T(h->n_global), T(l2), l2, reorth};
    LzCtl<T>& c = r.c;
    // start (cubic.py:85): zero alphas / betas, partials of ||g||^2 (pass 1 or
    // the combine of step 0 finishes the norm)
    int Pn = vec_grid(d);
    hipLaunchKernelGGL((k_lz_begin<T>), dim3(Pn), dim3(kNT), 0, s, d, g, m, h->alphas_dev, h->betas_dev, h->pb);
    LAUNCHCHK();
    double* pn = h->pb;
    if (r.cols()) CHK(globalise(h, &pn, &Pn, 1, s));
    c.pnorm = pn;
    c.Pnorm = Pn;
    r.pa_g = h->pa;
    for (int j = 0; j + 1 < m; ++j) {
      c.j = j;
      int Pa = 0;
      switch (ch.step) {
        case LZ_EARLY: CHK(step_early(r)); continue;
        case LZ_EARLY_COLS: CHK(step_early_cols(r)); continue;
        case LZ_EARLY_ROWS: CHK(step_early_rows(r)); continue;
        case LZ_TWO_LAUNCH: CHK(step_two_launch(r, &Pa)); break;
        case LZ_GENERIC: CHK(step_generic(r, 0, &Pa)); break;
        default: CHK(step_fused(r, &Pa)); break;   // the four fused steps
      }
      r.Pa_prev = Pa;
      // the fused steps' next pass 1 runs step B; their last loop step keeps the separate one
      if (ch.step != LZ_GENERIC && j + 2 < m) continue;
      CHK(separate_step_b(r, Pa));
    }
    c.mode = 1;
    hipLaunchKernelGGL((k_lz_final_check<T>), dim3(1), dim3(kNT), 0, s, c);
    LAUNCHCHK();
    int Pa = 0;
    CHK(step_generic(r, 1, &Pa));
    hipLaunchKernelGGL((k_lz_final<T>), dim3(vec_grid(d)), dim3(kNT), 0, s, r.pa_g, Pa, c, h->alphas_dev,
                       h->hostres_dev);
    LAUNCHCHK();
    return KRCN_OK;
  };
  // krcn_crn_step: the launches alone, eager and outside the placement search;
  // the caller synchronises and reads the results block (lanczos_results)
  if (enqueue_only) return enqueue(s_call);
  // unsharded, unprofiled calls may replay (a replaying handle is outside the placement search, so W stays put)
  const bool graph = h->graph && h->shard == KRCN_SHARD_NONE && !h->prof;
  const uint64_t key[krcn_csr::kGraphKey] = {uint64_t(uintptr_t(w)), uint64_t(uintptr_t(g)), uint64_t(uintptr_t(V)),
                                             uint64_t(uintptr_t(h->W)), uint64_t(m), uint64_t(reorth), bits(tol),
                                             bits(l2), h->ws_gen, uint64_t(sizeof(T))};
  bool lzp_timed = false;
  CHK(lz_submit(h, graph, key, m, s_call, enqueue, &lzp_timed));
  // the recurrence results: k_lz_final packed the state, alphas[0..m) and
  // betas[0..m-1) straight into the mapped host block (no copy launch)
  if (2 * m + 3 > kLzOut) return fail(KRCN_ERR_UNSUPPORTED, "krcn_lanczos: m > 2044 not supported");
  HIPCHK(hipStreamSynchronize(s_call));
  CHK(lzp_done(h, lzp_timed));
  lanczos_results(h, m, alphas_host, betas_host, info);
  return KRCN_OK;
}

// krcn_cgs2: reorth_cgs2 on a caller's z and the first k rows of a caller's V,
// outside any recurrence.  The workspace is an unsharded krcn_lanczos's for
// m = k + 1 (the step that sweeps k rows); the state flag, which a recurrence
// that broke down leaves set and every sweep obeys, is cleared as an m = 1
// recurrence clears it (k_lz_final_check; no norm partials: gnorm = 0).  The
// ||z2||^2 partials are summed as the next step's prologue sums them
// (sum_partials, by k_finish).
template <typename T>
static krcn_status cgs2_impl(krcn_csr* h, int k, const T* V, T* z, double* norm2_host, int* path_host,
                             hipStream_t s) {
  CHK(reserve_reorth(h, k + 1));
  const LzCtl<T> c{const_cast<T*>(V), z, h->d, 1, 0, 1, h->st, h->betas_dev, h->pb, 0, 0.0};
  hipLaunchKernelGGL((k_lz_final_check<T>), dim3(1), dim3(kNT), 0, s, c);
  LAUNCHCHK();
  const bool vec = cgs_vec_ok<T>(h, V, z, false, k);
  int P = 0;
  CHK(reorth_cgs2<T>(h, V, k, z, false, &P, s));
  hipLaunchKernelGGL((k_finish<0>), dim3(1), dim3(kNT), 0, s, static_cast<const double*>(h->pb), P, h->scal + 5);
  LAUNCHCHK();
  HIPCHK(hipMemcpyAsync(h->hostbuf, h->scal + 5, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (norm2_host) *norm2_host = h->hostbuf[0];
  if (path_host) *path_host = vec ? 1 : 0;
  return KRCN_OK;
}
