// krcn_pass.hpp — the pass launcher: the shape of a pass (does a slice combine
// follow its main launch, over how many partial arrays, on what grid), one
// main-launch helper per plan kind, and run_pass, which the kernels of every
// translation unit are instantiated through.  Included at the end of
// krcn_internal.hpp (it needs the handle layout and the error macros).
#pragma once

template <typename F>
inline void with_lanes(int L, F&& f) {
  switch (L) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 64>{}); break;
  }
}

// 1, 2, 4, 8 or 16 (the CGS2 unrolls, steps and batches, krcn_lanczos_impl.hpp)
template <typename F>
inline void with_pow2(int v, F&& f) {
  switch (v) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: f(std::integral_constant<int, 16>{}); break;
  }
}

template <class F>
inline void with_sort_nt(int nt, F&& f) {
  switch (nt) {
    case 512: f(std::integral_constant<int, 512>{}); break;
    case 1024: f(std::integral_constant<int, 1024>{}); break;
    default: f(std::integral_constant<int, 256>{}); break;
  }
}

// ------------------------------------------------------- the shape of a pass
// How many partial arrays (P.part) the slice combine sums after the main
// launch; 0: no combine, the main launch runs the epilogue itself.
inline int combine_arrays(const PassPlan& P) {
  switch (P.kind) {
    case KRCN_PLAN_JAG: return P.S > 1 && P.jG > 1 ? P.jG : 0;   // accumulate over jG slice groups
    case KRCN_PLAN_WINDOW_SLICES: return P.S;
    case KRCN_PLAN_WINDOW_ACCUM: return 0;
    default: return P.S > 1 ? P.S : 0;   // wave, sorted and dense plans
  }
}

// A/B knob KRCN_COMBINE_W=1: slices combine with 16-byte loads (k_slice_combine_w).
inline bool combine_w_env() {
  static const bool v = tuning_off("KRCN_COMBINE_W");
  return v;
}

// The combine kernel over A partial arrays and the grid it is launched on
// (vw: rows per 16-byte vector, CombW<T>::VW).
enum class Combine { Small, Wide, Plain };
struct CombineShape {
  Combine kernel;
  int grid;
};
inline CombineShape combine_shape(const PassPlan& P, int A, int vw) {
  if (A <= kCombineSmallS) return {Combine::Small, combine_small_grid(P.rows)};
  if (combine_w_env() && A >= 32 && P.rows % vw == 0 && combine_w_grid(P.rows, vw) <= P.pcap)
    return {Combine::Wide, combine_w_grid(P.rows, vw)};
  return {Combine::Plain, P.combine_grid};
}

// The number of partials run_pass writes for plan P when its epilogue
// reduces (the *Pout of a non-fused launch): the combine's grid for sliced
// plans, the main launch's otherwise.  Row shards agree on its maximum over
// ranks before the collectives (krcn_handle.hip agree_rows).
inline int pass_partials(const PassPlan& P) {
  const int A = combine_arrays(P);
  return A ? combine_shape(P, A, 2).grid : P.grid;   // (fp64 rows: CombW<double>::VW = 2; row shards are fp64)
}

// The slice combine of a sliced pass over its A partial arrays (P.part).
template <typename T, class Src2, class Epi>
inline krcn_status run_combine(PassPlan& P, int A, const Src2& rest, const Epi& epi, double* partials, int* Pout,
                               hipStream_t s) {
  const CombineShape c = combine_shape(P, A, CombW<T>::VW);
  const T* pp = static_cast<const T*>(P.part);
  if (c.kernel == Combine::Small) {
    const int nt = combine_small_nt(P.rows);
    auto go = [&](auto sm, auto ntc) {
      hipLaunchKernelGGL((k_slice_combine_small<T, Src2, Epi, decltype(sm)::value, decltype(ntc)::value>),
                         dim3(c.grid), dim3(decltype(ntc)::value), 0, s, P.rows, A, pp, rest, epi, partials);
    };
    auto by_s = [&](auto ntc) {
      if (A <= 2) go(std::integral_constant<int, 2>{}, ntc);
      else if (A <= 4) go(std::integral_constant<int, 4>{}, ntc);
      else if (A <= 8) go(std::integral_constant<int, 8>{}, ntc);
      else go(std::integral_constant<int, 16>{}, ntc);
    };
    if (nt == 256) by_s(std::integral_constant<int, 256>{});
    else by_s(std::integral_constant<int, kCombineNT>{});
  } else if (c.kernel == Combine::Wide) {
    hipLaunchKernelGGL((k_slice_combine_w<T, Src2, Epi>), dim3(c.grid), dim3(kCombineNT), 0, s, P.rows, A, pp, rest,
                       epi, partials);
  } else {
    hipLaunchKernelGGL((k_slice_combine<T, Src2, Epi>), dim3(c.grid), dim3(kCombineNT), 0, s, P.rows, A,
                       combine_rows(P.rows), pp, rest, epi, partials);
  }
  LAUNCHCHK();
  if (Pout) *Pout = c.grid;
  return KRCN_OK;
}

// The pass 2 of a one-piece plan with per-block X^T copies (pass 1's EpiLz1X
// left the blocks' shares of X^T u in P.xpart): their sum in a fixed order
// with the epilogue, by k_xt_combine on blocks of rb = 16 / 32 / 64 rows, or
// (rb = 0) by k_slice_combine.
template <typename T, class Src2, class Epi>
inline krcn_status run_xt_combine(PassPlan& P, int rb, const Src2& rest, const Epi& epi, double* partials, int* Pout,
                                  hipStream_t s) {
  const int d = int(P.cols);
  const T* xp = static_cast<const T*>(P.xpart);
  const int cg = rb ? (d + rb - 1) / rb : combine_grid(d);
  auto xt = [&](auto rc) {
    hipLaunchKernelGGL((k_xt_combine<T, Src2, Epi, decltype(rc)::value>), dim3(cg), dim3(kCombineNT), 0, s, d, P.grid,
                       xp, rest, epi, partials);
  };
  if (rb == 16) xt(std::integral_constant<int, 16>{});
  else if (rb == 64) xt(std::integral_constant<int, 64>{});
  else if (rb) xt(std::integral_constant<int, 32>{});
  else
    hipLaunchKernelGGL((k_slice_combine<T, Src2, Epi>), dim3(cg), dim3(kCombineNT), 0, s, d, P.grid, combine_rows(d),
                       xp, rest, epi, partials);
  LAUNCHCHK();
  *Pout = cg;
  return KRCN_OK;
}

// ------------------------------------------- the main launch of each plan kind
// Each takes the epilogue it is handed: the caller's (with its partials), or
// EpiSlicePart<T> into P.part when a combine follows.  The tiled kernels walk
// P.groups XCD groups of slices (one group when unsliced).
template <typename T, class Src, class E>
inline void launch_wave(const PassPlan& P, const Src& first, const E& ep, double* parts, hipStream_t s) {
  with_lanes(P.L, [&](auto lc) {
    hipLaunchKernelGGL((k_tiled_pass<T, decltype(lc)::value, Src, E>), dim3(P.grid), dim3(kNT), 0, s, P.rows,
                       P.S == 1 ? 1 : P.groups, P.ptr, P.idx, static_cast<const T*>(P.val), P.tiles, P.tbeg, first,
                       ep, parts);
  });
}

template <typename T, class Src, class E>
inline void launch_sorted(const PassPlan& P, const Src& first, const E& ep, double* parts, hipStream_t s) {
  with_lanes(P.L, [&](auto lc) {
    constexpr int LL = decltype(lc)::value;
    with_sort_nt(P.sort_nt, [&](auto nc) {
      constexpr int NT = decltype(nc)::value;
      hipLaunchKernelGGL((k_sorted_pass<T, LL, NT, Src, E>), dim3(P.grid), dim3(NT), 0, s, P.rows,
                         P.S == 1 ? 1 : P.groups, P.ptr, P.gword, static_cast<const T*>(P.gval), P.tiles, P.tbeg,
                         P.tmid, first, ep, parts);
    });
  });
}

// f(a value of the plan's stored value type): T, or float for a narrowed plan
// of an fp64 handle (PassPlan::vbytes == 4).  Only T = double gets the second
// instantiation.
template <typename T, class F>
inline void with_stored(const PassPlan& P, F&& f) {
  if constexpr (std::is_same<T, double>::value) {
    if (P.vbytes == 4) {
      f(0.0f);
      return;
    }
  }
  f(T(0));
}

// Both window kinds: the slices kernel writes per-slice partials (mode 0; the
// fused step B of an IsLzZ source: mode 2), the accumulate kernel (mode 1)
// runs the caller's epilogue.
template <typename T, class Src, class E>
inline void launch_window(const PassPlan& P, const Src& first, const E& ep, double* parts, hipStream_t s) {
  constexpr bool accum = !std::is_same<E, EpiSlicePart<T>>::value;
  WinArgs wa{P.rows, P.W, P.stride, P.S, IsLzZ<Src>::value ? 2 : (accum ? 1 : 0), P.ntiles, P.cols,
             P.tb, P.ro, P.widx, P.val, P.segs};
  wa.kpb = P.kpb;
  with_stored<T>(P, [&](auto ts) {
    using TS = decltype(ts);
    auto launch = [&](auto rc) {
      hipLaunchKernelGGL((k_window_pass<T, TS, decltype(rc)::value, Src, E, accum>), dim3(P.grid), dim3(kWinNT), 0, s,
                         wa, first, ep, parts);
    };
    // slices mode: the tiles' rows are plan data (they follow the bases in P.tb), one kernel with a lane cap of 64 whatever P.R
    if constexpr (accum) {
      if (P.R == 16) return launch(std::integral_constant<int, 16>{});
      if (P.R == 32) return launch(std::integral_constant<int, 32>{});
    }
    launch(std::integral_constant<int, 64>{});
  });
}

// Single window (S == 1): k_jag_pass.  Accumulate over jG slice groups:
// k_jag_acc, with per-group partial row sums when jG > 1 (k_slice_combine
// adds them in group order and runs the epilogue).
template <typename T, class Src, class E>
inline void launch_jag(const PassPlan& P, const Src& first, const E& ep, double* parts, hipStream_t s) {
  JagArgs ja{P.rows, P.S == 1 ? 1 : P.jSg, P.W, P.jG, P.cols, P.jgcut, P.jumeta, P.jcnt, P.widx, P.val};
  ja.xmap = P.S == 1 && KRCN_JAG_XMAP;
  if (P.jlong > 0) {
    ja.nlong = P.jlong;
    ja.lpiece = P.jlpiece;
    ja.lcut = P.jlcut;
    ja.tcut = P.jlcut + P.grid + 1;
    ja.lrow = P.jlrow;
    ja.ltask = P.jltask;
    ja.task = P.jtask;
    ja.lidx = P.jlidx;
    ja.lval = P.jlval;
  }
  with_stored<T>(P, [&](auto ts) {
    using TS = decltype(ts);
    if constexpr (!std::is_same<E, EpiSlicePart<T>>::value) {
      if (P.S == 1) {
        auto one = [&](auto kc) {
          constexpr int K = decltype(kc)::value;
          hipLaunchKernelGGL((k_jag_pass<T, TS, K, jag_cpg(K), 8, Src, E>), dim3(P.grid), dim3(kJagNT), 0, s, ja, first,
                             ep, parts);
        };
        if (P.jK == 1) one(std::integral_constant<int, 1>{});
        else if (P.jK == 2) one(std::integral_constant<int, 2>{});
        else if (P.jK == 3) one(std::integral_constant<int, 3>{});
        else one(std::integral_constant<int, kJagK1>{});
        return;
      }
    }
    if (P.jK == 4)
      hipLaunchKernelGGL((k_jag_acc<T, TS, 4, Src, E>), dim3(P.grid), dim3(kJagNT), 0, s, ja, first, ep, parts);
    else
      hipLaunchKernelGGL((k_jag_acc<T, TS, kJagK2, Src, E>), dim3(P.grid), dim3(kJagNT), 0, s, ja, first, ep, parts);
  });
}

template <typename T, class Src, class E>
inline void launch_dense(const PassPlan& P, const Src& first, const E& ep, double* parts, hipStream_t s) {
  DenseArgs da{P.rows, P.S, P.ntiles, P.cols, P.dld, P.dld / int64_t(16 / P.vbytes), P.val};
  auto launch = [&](auto ts) {   // ts: a value of the image's stored type
    using TS = decltype(ts);
    with_lanes(P.L, [&](auto lc) {
      hipLaunchKernelGGL((k_dense_pass<T, TS, decltype(lc)::value, Src, E>), dim3(P.grid), dim3(kDenseNT), 0, s, da,
                         first, ep, parts);
    });
  };
  if (P.vbytes == int(sizeof(T))) launch(T(0));
  else launch(0.0f);   // fp32 values under fp64 arithmetic (KRCN_VALUES_F32)
}

// Which launches exist: a source `Src` with the caller's epilogue `Epi`
// (part = false) or with EpiSlicePart ahead of a combine (part = true) over a
// plan of `kind`.  The fused Lanczos sources have kernels over few kinds only
// (run_pass refuses the rest), and no other pair is instantiated.
template <typename T, class Src, class Epi>
constexpr bool pass_has_kernel(int kind, bool part) {
  constexpr bool z = IsLzZ<Src>::value, u = IsLzU<Src>::value;
  if (IsLzSmall<Src>::value) return kind == KRCN_PLAN_WINDOW_ACCUM && !part;
  switch (kind) {
    case KRCN_PLAN_WINDOW_SLICES: return part;
    case KRCN_PLAN_WINDOW_ACCUM: return !part && !z;
    case KRCN_PLAN_JAG: return !z;
    case KRCN_PLAN_DENSE: return !z && !u;
    // fused step B over sorted tiles: the two-launch step's EpiWeighted runs
    // in the main launch, every other epilogue in the combine
    case KRCN_PLAN_SORTED: return !z || part != std::is_same<Epi, EpiWeighted<T>>::value;
    default: return !z;   // wave tiles
  }
}

// One SpMV pass: `first` is the source of the main launch, `rest` of the
// slice-combine launch (sliced plans); partial sums of a reducing epilogue land
// in `partials` (*Pout entries).
// `mid` (profiling): its em event is recorded between the main launch and
// the slice combine.
template <typename T, class Src, class Src2, class Epi>
inline krcn_status run_pass(PassPlan& P, const Src& first, const Src2& rest, const Epi& epi, double* partials,
                            int* Pout, hipStream_t s, ProfRec* mid = nullptr) {
  constexpr bool z = IsLzZ<Src>::value, u = IsLzU<Src>::value, small = IsLzSmall<Src>::value;
  constexpr bool weighted = std::is_same<Epi, EpiWeighted<T>>::value;
  const int kind = P.kind;
  // 1. the source and the plan kind must have a kernel between them
  if constexpr (small) {
    if (kind != KRCN_PLAN_WINDOW_ACCUM || P.S != 1 || P.cols > kWinNT)
      return fail(KRCN_ERR_UNSUPPORTED, "fused small-vector Lanczos pass 1 needs a one-piece window-accum plan");
  }
  if (kind == KRCN_PLAN_DENSE) {
    // dense plans run the generic step only: the sources of the fused steps
    // are never selected for one (krcn_lzstep.hpp lanczos_step)
    if (z || u) return fail(KRCN_ERR_UNSUPPORTED, "fused Lanczos steps do not run over a dense plan");
  }
  // the stored width of the plan's values: the arithmetic's, or fp32 under
  // fp64 arithmetic in the kinds that narrow (with_stored, launch_dense)
  if (P.vbytes != int(sizeof(T)) &&
      (P.vbytes != 4 || kind == KRCN_PLAN_WAVE || kind == KRCN_PLAN_SORTED))
    return fail(KRCN_ERR_INVALID, "run_pass: a plan of kind %d with %d-byte values under %d-byte arithmetic", kind,
                P.vbytes, int(sizeof(T)));
  if constexpr (u) {
    if (kind != KRCN_PLAN_JAG || P.S != 1)
      return fail(KRCN_ERR_UNSUPPORTED, "the two-launch Lanczos pass 2 needs a single-window jagged plan");
  }
  if constexpr (z) {
    // fused step B: over window slices (the combine settles beta), or over
    // sorted tiles — unsliced under the two-launch step's EpiWeighted (pass
    // 2's SrcLzU settles beta), else through the combine
    if (kind == KRCN_PLAN_JAG || kind == KRCN_PLAN_WINDOW_ACCUM)
      return fail(KRCN_ERR_UNSUPPORTED, "fused Lanczos pass 1 needs an LDS-window slices plan");
    if (weighted && kind != KRCN_PLAN_WINDOW_SLICES && (kind != KRCN_PLAN_SORTED || P.S != 1))
      return fail(KRCN_ERR_UNSUPPORTED, "the two-launch Lanczos pass 1 needs an unsliced sorted-tile plan");
    if (kind == KRCN_PLAN_WAVE)
      return fail(KRCN_ERR_UNSUPPORTED, "fused Lanczos pass 1 needs an LDS-window or sorted-tile plan");
  }
  // partial arrays the combine sums (a fused step B over sorted tiles always
  // ends in it, whatever S is: only EpiWeighted runs in the main launch.
  // krcn_lzstep.hpp lanczos_step takes that step for sliced plans only,
  // fused-sorted: an unsliced plan owns no P.part)
  const int A = z && !weighted && kind == KRCN_PLAN_SORTED ? P.S : combine_arrays(P);
  // a reducing launch writes one partial per block, the combine's when one
  // follows: the buffer must hold them.  This is the grid run_combine will
  // launch, not P.combine_grid; for every plan the builders make the outcome
  // is the same, since the small and plain combine grids are at most
  // kCombineSpread (256 < kMaxPartials <= pcap) and the 16-byte combine's
  // is taken only when it fits pcap (combine_shape).
  const int reducer_grid = A ? combine_shape(P, A, CombW<T>::VW).grid : P.grid;
  if (partials && reducer_grid > P.pcap)
    return fail(KRCN_ERR_INVALID, "run_pass: %d partials exceed the %lld-entry buffer", reducer_grid,
                (long long)P.pcap);
  // 2. the main launch: into P.part when a combine follows, else the
  // caller's epilogue.  The if constexpr keeps the pairs step 1 refused (and
  // the kinds' kernels a fused source has none for) out of the build.
  auto main_launch = [&](auto part, const auto& ep, double* parts) {
    constexpr bool pt = decltype(part)::value;
    constexpr auto has = &pass_has_kernel<T, Src, Epi>;
    switch (kind) {
      case KRCN_PLAN_WINDOW_SLICES:
      case KRCN_PLAN_WINDOW_ACCUM:   // (slices exactly when a combine follows)
        if constexpr (has(pt ? KRCN_PLAN_WINDOW_SLICES : KRCN_PLAN_WINDOW_ACCUM, pt))
          launch_window<T>(P, first, ep, parts, s);
        break;
      case KRCN_PLAN_JAG:
        if constexpr (has(KRCN_PLAN_JAG, pt)) launch_jag<T>(P, first, ep, parts, s);
        break;
      case KRCN_PLAN_DENSE:
        if constexpr (has(KRCN_PLAN_DENSE, pt)) launch_dense<T>(P, first, ep, parts, s);
        break;
      case KRCN_PLAN_SORTED:
        if constexpr (has(KRCN_PLAN_SORTED, pt)) launch_sorted<T>(P, first, ep, parts, s);
        break;
      default:
        if constexpr (has(KRCN_PLAN_WAVE, pt)) launch_wave<T>(P, first, ep, parts, s);
        break;
    }
  };
  if (A) main_launch(std::true_type{}, EpiSlicePart<T>{static_cast<T*>(P.part), int64_t(P.rows)},
                     static_cast<double*>(nullptr));
  else main_launch(std::false_type{}, epi, partials);
  // 3. the tail
  LAUNCHCHK();
  if constexpr (!small) {   // (no combine follows a one-piece window-accum pass)
    if (A) {
      if (mid) {
        HIPCHK(hipEventRecord(mid->em, s));
        mid->mid = true;
      }
      return run_combine<T>(P, A, rest, epi, partials, Pout, s);
    }
  }
  if (Pout) *Pout = P.grid;
  return KRCN_OK;
}

// What lanczos_step (krcn_lzstep.hpp) reads of a handle as it stands: the
// recurrence and krcn_csr_lanczos_step both choose the step from this.
inline LzStepIn lz_step_in(const krcn_csr* h, int reorth) {
  LzStepIn in;
  in.shard = h->shard;
  in.multi = h->comm && h->comm->nranks > 1;
  in.f64 = h->dtype == KRCN_F64;
  in.reorth = reorth != 0;
  in.n = h->n, in.d = h->d, in.pcap = h->pcap;
  in.p1_kind = h->p1.kind, in.p1_S = h->p1.S, in.p1_grid = h->p1.grid, in.p1_combine_grid = h->p1.combine_grid;
  in.p1_xt = h->p1.xt;
  in.p2_kind = h->p2.kind, in.p2_S = h->p2.S, in.p2_jG = h->p2.jG;
  in.pq = h->pq != nullptr;
  in.pq_local = pass_partials(h->p1);
  in.rows_pq = h->rows_pq, in.rows_early = h->rows_early;
  in.knobs = lz_knobs();
  return in;
}

#if KRCN_FOLD
// The early-alpha pass 1 of a window-slices plan with its slice combine
// folded in (krcn_window.hpp EpiSliceFold; tuning builds).
inline bool fold_ok(const krcn_csr* h) {
  const PassPlan& P = h->p1;
  // (uniform 32-row tiles only — the tile index is r0 / 32; a data-cut plan has R = 64 — and full-width plans)
  return h->fcnt && P.kind == KRCN_PLAN_WINDOW_SLICES && P.R == 32 && P.S <= 96 && P.ntiles <= h->pcap &&
         P.vbytes == int(h->vs);
}
template <typename T>
inline krcn_status run_fold_pass1(krcn_csr* h, const SrcLzBeta<T>& src, const EpiSliceFold<T>& epi, hipStream_t s) {
  PassPlan& P = h->p1;
  WinArgs wa{P.rows, P.W, P.stride, P.S, 0, P.ntiles, P.cols, P.tb, P.ro, P.widx, P.val, P.segs};
  wa.kpb = P.kpb;
  hipLaunchKernelGGL((k_window_pass<T, T, 32, SrcLzBeta<T>, EpiSliceFold<T>, false>), dim3(P.grid), dim3(kWinNT), 0, s,
                     wa, src, epi, static_cast<double*>(nullptr));
  LAUNCHCHK();
  return KRCN_OK;
}
#endif

// Pass over X (rows) / X^T with a plain gathered vector.
template <typename T, class Epi>
inline krcn_status launch_rows_x(krcn_csr* h, const T* x, const Epi& epi, double* partials, int* P,
                                 hipStream_t s) {
  CHK(plans_for_compute(h));
  return run_pass<T>(h->p1, SrcPlain<T>{x}, SrcPlain<T>{x}, epi, partials, P, s);
}

template <typename T, class Epi>
inline krcn_status launch_rows_xt(krcn_csr* h, const T* u, const Epi& epi, double* partials, int* P,
                                  hipStream_t s) {
  CHK(plans_for_compute(h));
  return run_pass<T>(h->p2, SrcPlain<T>{u}, SrcPlain<T>{u}, epi, partials, P, s);
}
