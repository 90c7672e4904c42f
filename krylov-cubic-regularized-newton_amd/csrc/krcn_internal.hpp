// krcn_internal.hpp — shared host-side internals of libkrcn.so (not part of the ABI).
//
// The library is split into translation units that compile in parallel:
//   krcn_handle.hip      error recorder, handle lifecycle, transposed CSR, setters / getters, profiling
//   krcn_plan.hip        the pass plans on the device (layouts: krcn_layout.hpp), ensure_plans, the reorth workspace
//   krcn_place.hip       the placement probe and the placement search over Lanczos calls
//   krcn_comm.hip        the RCCL communicator and the virtual communicator
//   krcn_ops.hip         objective pieces (Ax, X^T u, weights, HVP, gradient, loss, dots)
//   krcn_coord.hip       coordinate blocks of SSCN (gradient, Hessian block, Ax update)
//   krcn_block.hip       block products: k vectors per pass over the matrix (X V, X^T U / n, the block HVP)
//   krcn_lanczos_block.hip  the batched Lanczos: k recurrences in lockstep over the block HVP (krcn_blz.hpp;
//                        its per-column state rule, krcn_blz_state.hpp, is host-only like the three below)
//   krcn_crn.hip         the device cubic subproblem and the one-call Krylov-CRN step (krcn_cubic.hpp; the host
//                        side of its trial chain, krcn_crn_chain.hpp, is also the SSCN steps')
//   krcn_sscn.hip        the dense cubic subproblem and the Cholesky route of the one-call SSCN step
//                        (krcn_cubic_dense.hpp; the step and its entry checks, krcn_sscn_step.hpp, over the
//                        host-only selection rule, krcn_sscn_sel.hpp)
//   krcn_sytd.hip        the tridiagonal reduction and the tridiagonal route of the same step (krcn_sytd.hpp)
//   krcn_cubic_cg.hip    the full-space cubic subproblem, Newton over CG in one call (krcn_cgn.hpp; its
//                        state rule, krcn_cgn_state.hpp, is host-only like the three below)
//   krcn_gram.hip        the dense Hessian as a Gram product over the dense X^T image, fp64 MFMA (krcn_gram.hpp;
//                        its cut of the work, krcn_gram_geom.hpp, is host-only like the three below)
//   krcn_lanczos_f64.hip / krcn_lanczos_f32.hip
//                        the device Lanczos recurrence (krcn_lanczos_impl.hpp), one dtype each
// Three host-only headers (plain C++17, no HIP header: they also build with g++
// under the host sanitizers, tests/native/layout_check.cpp and lzstep_check.cpp):
//   krcn_geom.hpp        the constants and small structs host and device agree through (block
//                        shapes, tile caps, LDS geometry, TileDesc / WinSeg, the lane rule, the
//                        tuning-knob readers); the kernel headers include it
//   krcn_layout.hpp      the format policy and one layout function per format, from host row
//                        pointers to plain structs; krcn_plan.hip materialises them on the device
//   krcn_lzstep.hpp      which Lanczos step a handle runs, from plain scalars (the recurrence's
//                        tuning switches live there); krcn_lanczos_impl.hpp enqueues that step
// This header holds the handle layout, the error macros and the host helpers;
// it ends by including
//   krcn_pass.hpp        the pass launcher (run_pass, run_combine, the shape of a pass) that the
//                        kernels of every unit are instantiated through
#pragma once
#include "krcn.h"
#include "krcn_host.hpp"
#include "krcn_rendezvous.hpp"
#include "krcn_lzstep.hpp"
#include "krcn_kernels.hpp"
#include "krcn_tiled.hpp"
#include "krcn_window.hpp"
#include "krcn_jag.hpp"
#include "krcn_dense.hpp"
#include "krcn_cg.hpp"
#include "krcn_cgs2.hpp"

#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

using namespace krcn;

// CGS2 colsweep shape (krcn_cgs2.hpp k_cgs_colsweep): rows per wave and batch
// past k = 4 U (tuning knob KRCN_CGS_COLU) and batches per block (KRCN_CGS_NB);
// a block's row range is 4 U NB rows (default 8 x 8 x 4 = 256).  The range
// count of a sweep over k rows sizes the row-range partials (reserve_reorth).
inline int cgs_umax() {
  static const int v = [] {
    const int x = tuning_value("KRCN_CGS_COLU", 8);
    return x >= 2 ? x : 8;
  }();
  return v;
}
inline int cgs_nb() {
  static const int v = [] {
    const int x = tuning_value("KRCN_CGS_NB", 8);
    return x == 1 || x == 2 || x == 4 || x == 16 ? x : 8;
  }();
  return v;
}
inline int cgs_col_ranges(int k) {
  const int rows = 4 * cgs_col_unroll(k, cgs_umax()) * cgs_nb();
  return (k + rows - 1) / rows;
}
// chunks of k_cgs_rowdots_v over a row of nv 16-byte vectors
inline int cgs_rdv_chunks_of(int64_t nv) { return cgs_rdv_chunks(nv, cgs_rdv_steps(nv, 0)); }

#define HIPCHK(call)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(KRCN_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #call,            \
                  hipGetErrorString(e_));                                               \
  } while (0)

#define NCCLCHK(call)                                                                   \
  do {                                                                                  \
    ncclResult_t r_ = (call);                                                           \
    if (r_ != ncclSuccess)                                                              \
      return fail(KRCN_ERR_RCCL, "%s:%d %s -> %s", __FILE__, __LINE__, #call,           \
                  ncclGetErrorString(r_));                                              \
  } while (0)

#define CHK(expr)                             \
  do {                                        \
    krcn_status s_ = (expr);                  \
    if (s_ != KRCN_OK) return s_;             \
  } while (0)

#define LAUNCHCHK() HIPCHK(hipGetLastError())

// ----------------------------------------------------------------- handles
struct VirtualGroup;   // krcn_comm.hip: the ranks of a virtual communicator
constexpr int kVirtualMaxRanks = 16;
constexpr int kVirtualTimeoutS = 90;    // a rank that never arrives breaks the group after this (under
                                        // the GPU box's 180 s silence limit: a stall fails, not hangs)
struct VirtualBufs {
  void* p[kVirtualMaxRanks];
};
struct krcn_comm {
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0, device = 0;
  VirtualGroup* vg = nullptr;   // virtual ranks on one device (krcn_comm_create_virtual), else RCCL
  uint64_t seq = 0;             // all-reduces this rank has entered (virtual ranks: the timeout report)
};

// Largest Lanczos m: the alphas | betas | state block is allocated for it in
// krcn_csr_create, and comes back through the 4096-double pinned staging buffer.
constexpr int kLzMaxM = 2044;
// the packed results block k_lz_final writes after alphas | betas | state: the
// state (4 doubles), alphas[0..m), betas[0..m-1) — one D2H of 2 m + 3 doubles
// per call (round 4 copied the whole 2 kLzMaxM + 4: 32 KB per call, the copy
// path of a large transfer, on w8a's 10-HVP calls)
constexpr int kLzOut = 2 * kLzMaxM + 4;

// Handle construction and plan builds hold this process-wide lock: they
// allocate, free temporaries (hipFree synchronises the whole device) and sort
// with hipCUB, and a virtual-rank test builds 8 handles from 8 threads.
std::mutex& build_mutex();

// All-reduce of a virtual communicator: every rank's host thread drains its
// stream, the last to arrive sums the ranks' buffers in rank order on the
// device and writes the sum back to each of them (krcn_comm.hip).
krcn_status virtual_allreduce(krcn_comm* c, void* buf, int64_t count, int dtype, hipStream_t s);

struct ProfRec {
  hipEvent_t e0, e1, e2;
  hipEvent_t em;        // between pass 1's main launch and its slice combine
  bool mid = false;
};

// Owner of persistent device buffers: for every allocation the address of the
// field that holds it and its byte size.  Teardown, owned_bytes and the
// placement slots are all read from this table, so a buffer is named once,
// where it is allocated.  The table holds addresses of its owner's fields:
// it does not copy (a PassPlan resets through free_plan, a handle lives on
// the heap).
struct DevOwner {
  struct Slot {
    void** field;
    size_t bytes;
  };
  std::vector<Slot> slots;
  DevOwner() = default;
  DevOwner(const DevOwner&) = delete;
  DevOwner& operator=(const DevOwner&) = delete;
  template <typename T>
  krcn_status alloc(T** field, size_t bytes) {
    HIPCHK(hipMalloc(reinterpret_cast<void**>(field), bytes));
    slots.push_back(Slot{reinterpret_cast<void**>(field), bytes});
    return KRCN_OK;
  }
  const Slot* find(const void* field) const {
    for (const Slot& s : slots)
      if (s.field == field) return &s;
    return nullptr;
  }
  // frees one field's buffer early and drops its bytes (a field the table does not hold: nothing)
  krcn_status release(void* field) {
    for (size_t i = 0; i < slots.size(); ++i)
      if (slots[i].field == field) {
        void* b = *slots[i].field;
        *slots[i].field = nullptr;
        slots.erase(slots.begin() + long(i));
        if (b) HIPCHK(hipFree(b));
        break;
      }
    return KRCN_OK;
  }
  void free_all() {
    for (const Slot& s : slots) {
      if (*s.field) (void)hipFree(*s.field);
      *s.field = nullptr;
    }
    slots.clear();
  }
  size_t bytes() const {
    size_t b = 0;
    for (const Slot& s : slots) b += s.bytes;
    return b;
  }
};

// A temporary device allocation of a build: freed at scope exit (every early
// return included), or earlier by reset() where a later allocation is meant
// to reuse its space.  No conversion to T*: a kernel launch packs its
// arguments by their own types, so the pointer is always passed as .p.
template <typename T>
struct DevTmp {
  T* p = nullptr;
  DevTmp() = default;
  DevTmp(const DevTmp&) = delete;
  DevTmp& operator=(const DevTmp&) = delete;
  ~DevTmp() { reset(); }
  krcn_status alloc(size_t bytes) {
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&p), bytes));
    return KRCN_OK;
  }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
};

// Execution plan of one SpMV direction (pass 1: X, pass 2: X^T): its fields,
// which free_plan resets to these defaults ...
struct PlanFields {
  int S = 1, groups = 1, L = 1, grid = 1, combine_grid = 1, ntiles = 0;
  int rows = 0;
  int64_t cols = 0, nnz = 0;
  const int* ptr = nullptr;   // flattened slice-major row pointers (S * rows + 1)
  const int* idx = nullptr;
  const void* val = nullptr;
  int* own_ptr = nullptr;     // owned copies when sliced
  int* own_idx = nullptr;
  void* own_val = nullptr;
  TileDesc* tiles = nullptr;
  int* tbeg = nullptr;        // groups + 1 tile offsets
  void* part = nullptr;       // S * rows partial row sums (sliced)
  int kind = KRCN_PLAN_WAVE;  // the format (KRCN_PLAN_*): the one kernel family that runs the plan
  int vbytes = 0;             // bytes per stored matrix value: the handle's value size, or 4 in a dense, window or
                              // jagged plan of an fp64 handle under KRCN_VALUES_F32 (val, own_val, jlval)
  // sorted block tiles (k_sorted_pass) instead of wave tiles
  int sort_nt = 256;          // sorted tiles: threads per block (tile = kSortPerThread x sort_nt nonzeros)
  unsigned* gword = nullptr;  // sorted tiles: (column - tile base) << kSortSlotBits | CSR slot
  void* gval = nullptr;       //               value, same (tile-sorted) order
  int* tmid = nullptr;        // sorted tiles: first single-long-row tile of each group
  // LDS-window formats (k_window_pass; window-accum: every block walks all slices of its tile range, no partials)
  int R = 64;                 //   rows per tile (one lane per row); slices mode with data-cut tiles: the cap, 64
  int W = 0;                  //   slice width (window entries)
  int stride = 1;             //   segment slots per block
  int kpb = 0;                //   slices mode: blocks per slice when not a power of two (0: block = slice + S chunk)
  int nseg = 0;
  unsigned short* widx = nullptr;  // slice-local 16-bit column offsets (slice-major CSR order)
  WinSeg* segs = nullptr;     // per-block segment lists: block b runs segs[b * stride + i]
  int* tb = nullptr;          // compact row pointers: tile bases (S x (ntiles + 1)); slices mode: every slice's
                              //   bases are followed by its tiles' row starts (S x 2 (ntiles + 1); ntiles: the
                              //   largest slice's count)
  unsigned short* ro = nullptr;   //   row ends relative to the tile base (S x rows)
  // jagged lane-per-row format (k_jag_pass; S, W, widx, own_val, grid)
  int jK = 0;                 //   groups per wave (units per wave and slice)
  int jG = 1, jSg = 1;        //   accumulate: slice groups, slices per group
  int* jgcut = nullptr;       //   group cuts per block (grid + 1)
  int* jumeta = nullptr;      //   per (block, slice, wave): K unit bases, K unit sizes
  unsigned char* jcnt = nullptr;  // per unit: lane counts
  int jlong = 0, jlpiece = 0;     //   single window: long rows (JagArgs), LDS piece of their partials
  int* jlcut = nullptr;       //     per block: long rows, then tasks (2 x (grid + 1))
  int* jlrow = nullptr;       //     per long row: row id
  int* jltask = nullptr;      //     per long row: first task (+ 1 end entry)
  int* jtask = nullptr;       //     per task: element start, element count
  unsigned short* jlidx = nullptr;
  void* jlval = nullptr;
  int xt = 0;                 // one-piece window-accum X: per-block X^T copies (EpiLz1X)
  int* xcp = nullptr;         //   per block: cols + 1 absolute column offsets
  unsigned short* xrow = nullptr;  //   row offsets in the block's rows, column-major per block
  void* xval = nullptr;
  void* xpart = nullptr;      //   per block X^T u partials (grid x cols)
  // dense format (k_dense_pass; S, L, grid, ntiles = row groups, own_val = the image)
  int64_t dld = 0;            //   entries per image row
  int64_t pcap = 0;           // entries of the handle's partials buffers (ensure_plans)
};
// ... and the owner of every device buffer those fields point to.
struct PassPlan : PlanFields {
  DevOwner own;
};

struct CoordWs;   // krcn_coord.hip: the workspace of the coordinate calls

struct krcn_csr {
  int device = 0, dtype = KRCN_F64, shard = KRCN_SHARD_NONE;
  size_t vs = 8;
  int64_t n = 0, d = 0, nnz = 0, n_global = 0;
  const int* ptr = nullptr;
  const int* idx = nullptr;
  const void* val = nullptr;
  int* tptr = nullptr;
  int* tidx = nullptr;
  void* tval = nullptr;
  int lanes_x = KRCN_LANES_AUTO, lanes_xt = KRCN_LANES_AUTO;
  int slicing = KRCN_SLICING_AUTO;
  int format = KRCN_FORMAT_AUTO;
  int format_pass[2] = {-1, -1};   // krcn_csr_set_pass_format (-1: the handle's format)
  int values = KRCN_VALUES_FULL;   // krcn_csr_set_value_storage: stored width of the narrowing plans' values
  size_t store_vs = 8;             //   bytes per stored value the current plan build decided on (build_plans)
  int sort_nt = 0;            // sorted-tile block size; 0 = by matrix size
  bool plans_ready = false;
  bool p1_unsliced = false;   // pass 2 took a single-window jagged plan: pass 1's sorted tiles go
                              // unsliced (the two-launch Lanczos step, krcn_lzstep.hpp)
  PassPlan p1, p2;            // pass 1 over X, pass 2 over X^T
  // workspace
  double* pa = nullptr;   // partials of reducing launches (pcap entries)
  double* pb = nullptr;   // second partials buffer
  double* scal = nullptr; // 16 device scalars (all-reduced dots, results)
  LanczosState* st = nullptr;
  void* u = nullptr;      // n-vector (w (.) Xv)
  void* tn = nullptr;     // n-vector scratch (raw partials, residual)
  void* W = nullptr;      // d-vector (Lanczos w)
  void* td = nullptr;     // d-vector scratch (raw partial X^T u)
  double* hostbuf = nullptr;  // pinned host staging
  double* hostres = nullptr;  // pinned host results block k_lz_final writes directly (no D2H copy)
  double* hostres_dev = nullptr;   //   its device-side address
  int mcap = 0;               // Lanczos m the alphas block holds (kLzMaxM, from krcn_csr_create)
  double* alphas_dev = nullptr;
  double* betas_dev = nullptr;
  double* hcoef = nullptr;    // reorth coefficients (mcap)
  double* pz = nullptr;       // per-slice partials of ||z||^2 (fused step B, pcap entries)
  double* pq = nullptr;       // early-alpha step: the combine's partials of (X v).(w (X v)) (pcap entries)
  int* fcnt = nullptr;        // slice-combine fold (KRCN_FOLD builds): per pass-1 tile, tickets drawn
  int64_t pcap = kMaxPartials;   // entries of pa / pb / pz: >= every reducing launch's grid
  double* pr = nullptr;       // CGS2 h1 partials (k_cgs_rowdots: column chunks x rows)
  double* pr2 = nullptr;      // CGS2 h2 partials (k_cgs_update_dots: column slabs x rows)
  double* cy = nullptr;       // CGS2 row-range partials of V^T h (k_cgs_colsweep: ranges x d)
  int* ccnt = nullptr;        //   its per column group arrival counters (zero between launches)
  int64_t pr_cap = 0;
  int64_t prv_cap = 0;        // entries of pr (the 1 KiB-piece path checks its C k chunk partials fit)
  int cy_q = 0;               // row ranges cy holds (0: not allocated; one range needs none)
  int reorth_m = 0;           // CGS2 workspace reserved for Lanczos m <= this (krcn_csr_reserve)
  void* cg_r = nullptr;       // CG vectors r | p | q (3 d-vectors, krcn_cg_solve)
  struct krcn::CgState* cg_st = nullptr;
  void* cgn_z = nullptr;      // krcn_cubic_cg (krcn_cubic_cg.hip): the d-vector z of its solve_y phase
  double* cgn_st = nullptr;   //   the chain state, then the two partial arrays of a turn's sums
  double* cgn_res = nullptr;  //   pinned, mapped host record the turn that ends the chain writes
  double* cgn_res_dev = nullptr;
  double* gram_ws = nullptr;  // krcn_hessian_gram (krcn_gram.hip): the raw tiles of its K splits (grown on demand)
  size_t gram_ws_bytes = 0;
  int gram_split = 0;         // krcn_csr_set_gram_split (0: the rule of krcn_gram_geom.hpp)
  double* crn_ws = nullptr;  // krcn_crn_step / krcn_cubic_tridiag: the chain state, then the subproblem's
                              // alphas | betas | s (three kLzMaxM-vectors; its solves work in LDS)
  double* crn_res = nullptr;  //   pinned, mapped host record the judge kernel writes (krcn_crn.hip)
  double* crn_res_dev = nullptr;
  CoordWs* cw = nullptr;      // coordinate workspace (first krcn_coord_* call; its device block is in own)
  int coord_window = 0;       // krcn_csr_set_coord_window (0: auto)
  char* sscn_ws = nullptr;    // krcn_sscn_step: the selection in both orders, its permutation and the
                              //   coordinate gradient (krcn_sscn.hip; a fixed block, allocated by the first step)
  double* sytd_ws = nullptr;  // the tridiagonal reduction's workspace for blocks of up to sytd_k columns
  int sytd_k = 0;             //   (krcn_sytd.hip; allocated by the first call that needs it, grown when k grows)
  void* blk_u = nullptr;      // krcn_hvp_block: its (n, blk_k) intermediate (krcn_block.hip; grown when k grows)
  int blk_k = 0;
  int* blk_long[2] = {};      // block products: rows of X / X^T above KRCN_BLOCK_LONG_ROW, listed at the
  int blk_nlong[2] = {};      //   first pass over that matrix (null while there is none)
  bool blk_listed[2] = {};
  // krcn_lanczos_block (krcn_lanczos_block.hip): grown when k, or k and m, grow
  void* blz_y = nullptr;      //   (d, blz_k) block: the block HVP's result
  void* blz_op = nullptr;     //   (d, blz_k) block: the final quotient's operand
  int blz_k = 0;
  double* blz_pa = nullptr;   //   per-workgroup partials of the two alpha sums, and of ||z||^2 behind them
  double* blz_res = nullptr;  //   k states | alphas | betas (blz_res_cap doubles)
  double* blz_s = nullptr;    //   krcn_basis_combine_block: the (m, k) coefficients (blz_s_cap doubles)
  size_t blz_res_cap = 0, blz_s_cap = 0;
  double* blz_host = nullptr; //   pinned, mapped host copy of blz_res that the last launch writes
  double* blz_host_dev = nullptr;
  // krcn_crn_step_block and its pieces (krcn_crn_block.hip): the blocks grow when k grows
  void* crnb_g = nullptr;     //   (d, crnb_k) block: the gradients
  void* crnb_w = nullptr;     //   (n, crnb_k) block: the residuals, then the Hessian weights
  double* crnb_sub = nullptr; //   the subproblem's alphas | betas | s: 3 crnb_k kLzMaxM doubles
  int crnb_k = 0;
  double* crnb_st = nullptr;  //   head | KRCN_BLOCK_MAX records | the staged per-column parameters
  double* crnb_pa = nullptr;  //   per-workgroup partials of the loss terms, and of the squared norms behind them
  double* crnb_host = nullptr;   // pinned, mapped host block the judge writes: head | records | k values
  double* crnb_host_dev = nullptr;
  DevOwner own;              // every device buffer above but betas_dev (it aliases alphas_dev)
  krcn_comm* comm = nullptr;
  bool prof = false;
  std::vector<ProfRec> prof_pool;
  ProfRec* prof_cur = nullptr;   // run_pass records its em when set
  size_t prof_used = 0;
  // hipGraph of the Lanczos launch sequence (lanczos_impl): keyed by the call's
  // arguments and ws_gen, which every plan rebuild / workspace realloc bumps
  static constexpr int kGraphKey = 10;
  uint64_t ws_gen = 0;
  bool graph = false;          // krcn_csr_set_graph
  hipStream_t gstream = nullptr;
  hipGraphExec_t gexec = nullptr;
  uint64_t gkey[kGraphKey] = {};    // arguments gexec was recorded with
  uint64_t glast[kGraphKey] = {};   // arguments of the previous call
  // row shards of a multi-rank communicator: what every rank's early-alpha
  // Lanczos step must agree on (krcn_handle.hip agree_rows, after each plan build)
  int rows_pq = -1;            // packed alpha partials = max over ranks of pass_partials(p1); -1: not agreed
  int rows_early = 0;          // every rank's pass-1 grids fit kMaxPartials
  // placement probe of the hot buffers (ensure_plans, krcn_csr_set_placement_trials)
  static constexpr int kPlaceMax = 8;
  int place_trials = -1;       // -1 auto, 0 off, k: k placements probed
  int place_keep = -1;         // -1: the fastest is kept; 0..7: placement min(keep, probed - 1), both searches
                               //   (krcn_csr_set_placement_keep)
  int place_ran = 0;           // placements probed at the last plan build (0: none)
  int place_best = -1;         // the one kept
  float place_us[kPlaceMax] = {};   // probe HVP time of each (us)
  double place_hot_mb = 0.0;   // hot bytes the auto rule saw
  // the placement search over the first Lanczos calls (krcn_place.hip lzp_*)
  int lzp_stage = 0;           // 0: not started; s >= 1: the next call times placement s - 1; -1: done
  int lzp_m = 0;               // the m the timed calls share
  int lzp_ran = 0, lzp_best = -1;
  float lzp_ms[kPlaceMax] = {};
  std::vector<std::vector<void*>> lzp_cand;   // the placements (slot values), [0] the one found
  hipEvent_t lzp_e0 = nullptr, lzp_e1 = nullptr;
};

void free_plan(PassPlan& P);
void coord_free(krcn_csr* h);   // krcn_coord.hip: releases h->cw
krcn_status ensure_plans(krcn_csr* h);
// Row shards agree on the packed alpha partials (krcn_handle.hip; collective).
krcn_status agree_rows(krcn_csr* h);
// The handle's hot buffers as relocatable slots (krcn_place.hip): the plans'
// tables and the handle's u, tn, W, td, pa, pb, pz, pq.
void hot_slots(krcn_csr* h, std::vector<DevOwner::Slot>& out);
// The placement probe of a plan build (krcn_place.hip; ensure_plans ends with it).
krcn_status tune_placement(krcn_csr* h);
// `reps` back-to-back local HVPs (pass 1 and pass 2 of the handle's plans, no
// collective) on the handle's scratch vectors: *us = microseconds per HVP
// (krcn_ops.hip; the placement probe of ensure_plans).
krcn_status placement_probe(krcn_csr* h, hipStream_t s, int reps, float* us);
// The placement search over Lanczos calls (krcn_place.hip): lzp_begin before
// a call's launches (may relocate the hot buffers on stream s and start the
// timing), lzp_end after them, lzp_done after the call's synchronisation.
krcn_status lzp_begin(krcn_csr* h, int m, hipStream_t s, bool* timed);
krcn_status lzp_end(krcn_csr* h, hipStream_t s, bool timed);
krcn_status lzp_done(krcn_csr* h, bool timed);
void lzp_abort(krcn_csr* h);
// CGS2 dot partials for Lanczos m <= m (krcn_plan.hip; frees and reallocates).
krcn_status reserve_reorth(krcn_csr* h, int m);

// A handle whose communicator spans several ranks joins collectives in every
// compute call, so it must not build plans (allocations, device-wide syncs)
// inside one: krcn_csr_attach_comm / krcn_csr_reserve build them up front, and
// a compute call on such a handle without them fails instead.  Other handles
// build their plans on first use.
inline krcn_status plans_for_compute(krcn_csr* h) {
  if (h->plans_ready) return KRCN_OK;
  if (h->comm && h->comm->nranks > 1)
    return fail(KRCN_ERR_INVALID, "a sharded handle with a %d-rank communicator has no plans: call krcn_csr_reserve "
                "(or krcn_csr_attach_comm) after changing its policies, before the collectives", h->comm->nranks);
  return ensure_plans(h);
}

// ---------------------------------------------------------------- helpers
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline int vec_grid(int64_t len) {
  int64_t b = (len + kNT - 1) / kNT;
  if (b < 1) b = 1;
  if (b > 1024) b = 1024;
  return int(b);
}

inline krcn_status set_device(const krcn_csr* h) {
  HIPCHK(hipSetDevice(h->device));
  return KRCN_OK;
}

// count elements (at least one) into a field of the handle
template <typename T>
inline krcn_status dalloc(krcn_csr* h, T** p, size_t count) {
  return h->own.alloc(p, std::max<size_t>(count, 1) * sizeof(T));
}

inline krcn_status nccl_dtype(int dtype, ncclDataType_t* t) {
  *t = dtype == KRCN_F64 ? ncclDouble : ncclFloat;
  return KRCN_OK;
}

// (an RCCL communicator of one rank still runs the collective: the
// rehearsals of bench.py --rehearse-shard time its launch and stream cost)
inline krcn_status allreduce(krcn_csr* h, void* buf, int64_t count, int dtype, hipStream_t s) {
  if (!h->comm || count == 0) return KRCN_OK;
  if (h->comm->vg) return h->comm->nranks == 1 ? KRCN_OK : virtual_allreduce(h->comm, buf, count, dtype, s);
  ncclDataType_t t;
  nccl_dtype(dtype, &t);
  NCCLCHK(ncclAllReduce(buf, buf, size_t(count), t, ncclSum, h->comm->comm, s));
  return KRCN_OK;
}

// ------------------------------------------------------------- profiling
inline ProfRec* prof_next(krcn_csr* h) {
  if (!h->prof) return nullptr;
  if (h->prof_used == h->prof_pool.size()) {
    ProfRec r;
    // timing-only events without the system-scope release fence a default
    // event record carries (they sit between kernels of the timed region)
    const unsigned fl = hipEventDisableSystemFence;
    if (hipEventCreateWithFlags(&r.e0, fl) != hipSuccess || hipEventCreateWithFlags(&r.e1, fl) != hipSuccess ||
        hipEventCreateWithFlags(&r.e2, fl) != hipSuccess || hipEventCreateWithFlags(&r.em, fl) != hipSuccess)
      return nullptr;
    h->prof_pool.push_back(r);
  }
  ProfRec* r = &h->prof_pool[h->prof_used++];
  r->mid = false;
  return r;
}

// Lanczos recurrences, one translation unit per dtype (krcn_lanczos_impl.hpp).
// enqueue_only (krcn_crn_step): the launches alone — no graph replay, no
// placement search, no synchronisation; the host arrays and info are left
// untouched and the caller reads them with lanczos_results after its own sync.
krcn_status lanczos_f64(krcn_csr* h, const double* w, const double* g, int m, int reorth, double tol, double l2,
                        double* V, double* alphas_host, double* betas_host, krcn_lanczos_info* info, hipStream_t s,
                        bool enqueue_only = false);
krcn_status lanczos_f32(krcn_csr* h, const float* w, const float* g, int m, int reorth, double tol, double l2,
                        float* V, double* alphas_host, double* betas_host, krcn_lanczos_info* info, hipStream_t s,
                        bool enqueue_only = false);
// krcn_cgs2 per dtype (arguments already checked): reorth_cgs2 on the caller's V and z, synchronous.
krcn_status cgs2_f64(krcn_csr* h, int k, const double* V, double* z, double* norm2_host, int* path_host,
                     hipStream_t s);
krcn_status cgs2_f32(krcn_csr* h, int k, const float* V, float* z, double* norm2_host, int* path_host,
                     hipStream_t s);

// The results of a recurrence from the mapped block k_lz_final packed (state,
// alphas[0..m), betas[0..m-1)), after the stream has passed it: the
// reference's truncation rule (cubic.py:105-108) and return values.
inline void lanczos_results(const krcn_csr* h, int m, double* alphas_host, double* betas_host,
                            krcn_lanczos_info* info) {
  const double* hb = h->hostres;
  LanczosState stc;
  std::memcpy(&stc, hb, sizeof(LanczosState));
  const bool trunc = stc.done && stc.j_break < m - 2;
  const int m_eff = trunc ? stc.j_break + 1 : m;
  for (int i = 0; i < m; ++i) alphas_host[i] = i < m_eff ? hb[4 + i] : 0.0;
  for (int i = 0; i + 1 < m; ++i) betas_host[i] = i < m_eff - 1 ? hb[4 + m + i] : 0.0;
  info->m_eff = m_eff;
  info->breakdown = stc.done;
  info->j_break = stc.done ? stc.j_break : -1;
  info->hvps = (stc.done ? stc.j_break + 1 : (m - 1)) + 1;
  info->beta_last = stc.beta_last;
  info->gnorm = stc.gnorm;
}

// The workspace of krcn_cubic_tridiag / krcn_crn_step (krcn_crn.hip): allocated
// by krcn_csr_reserve and by the first of those calls.
krcn_status ensure_crn_ws(krcn_csr* h);
// The vectors r | p | q and the state of krcn_cg_solve (krcn_cg.hip): allocated by the
// first krcn_cg_solve or krcn_cubic_cg, which runs its solves in the same vectors.
krcn_status ensure_cg_ws(krcn_csr* h);

// The batched Lanczos in two parts (krcn_lanczos_block.hip): the launches of a
// call alone — arguments as krcn_lanczos_block's, already checked; no
// synchronisation after the recurrence —, and the reading of the mapped results
// block once the stream has passed k_blz_finish (alphas_host / betas_host may
// be null).  krcn_lanczos_block is the first, a synchronisation and the second.
krcn_status lanczos_block_enqueue(krcn_csr* h, int k, const void* w, int w_cols, const void* G, int m, double tol,
                                  const double* l2_host, void* V, hipStream_t s);
void lanczos_block_results(const krcn_csr* h, int k, int m, double* alphas_host, double* betas_host,
                           krcn_lanczos_info* info);

// Block passes behind the batched Krylov-CRN step (krcn_block.hip; arguments
// already checked, no pass plans).  Y = X^T U / n + l2_c Xv[:, c]: the block
// gradient's product, krcn_rmatvec_block's walk with EpiGrad's expression
// (BlkHvpOut's, with the iterate as v).  T = X V for the live columns of a
// trial: a guarded launch that returns at once when the chain has ended.
krcn_status block_rmatvec_l2(krcn_csr* h, int k, const void* U, const void* Xv, const double* l2_host, void* Y,
                             hipStream_t s);
krcn_status block_matvec_live(krcn_csr* h, int k, const void* V, void* Tn, const double* state, hipStream_t s);

#include "krcn_pass.hpp"
