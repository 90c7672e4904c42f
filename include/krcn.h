/*
 * krcn.h — C ABI of the MI355X-native Krylov cubic-regularized-Newton hot path.
 *
 * The hot path is the Lanczos + logistic Hessian-vector-product (HVP) inner loop
 * of Krylov CRN.  Every entry point below replaces one reference (Python/scipy)
 * operation; the reference location it replaces is cited on each declaration.
 * Reference root: Raymond30/Krylov-Cubic-Regularized-Newton (optimizer/loss.py,
 * optimizer/cubic.py).
 *
 * Conventions
 *   - All array arguments are DEVICE pointers (HIP global memory, e.g. the
 *     data_ptr() of a torch tensor) unless the name ends in _host.
 *   - Values are fp64 (KRCN_F64) or fp32 (KRCN_F32), chosen when the matrix
 *     handle is created; every vector passed with that handle has that dtype.
 *     Indices and row pointers are int32 (the reference's scipy CSR downcasts
 *     to int32 whenever nnz < 2^31).
 *   - Calls are asynchronous on `stream` (a hipStream_t, 0 = legacy default)
 *     unless documented as synchronous (they return a scalar to the host).
 *   - The caller owns every buffer it passes.  The library allocates device
 *     memory in krcn_csr_create (transposed CSR, vectors, the Lanczos results
 *     block for m <= 2044), when it builds a handle's pass plans and their
 *     partials (krcn_csr_reserve, krcn_csr_attach_comm of a multi-rank
 *     communicator, the plan queries, or the first compute call of any other
 *     handle), in krcn_csr_reserve(.., reorth = 1) (CGS2 workspace) and in the
 *     first krcn_cg_solve (the first krcn_cubic_cg allocates the same vectors,
 *     one more d-vector and 16,512 bytes), and the workspace of krcn_crn_step / krcn_cubic_tridiag
 *     (about 50 KB) in krcn_csr_reserve of an unsharded handle or the first of
 *     those calls.  krcn_lanczos allocates nothing on a handle that is
 *     reserved for its m.  The coordinate calls (krcn_coord_*) allocate their
 *     own workspace at the first of them and grow it when k grows: the device
 *     cols and delta (k_cap int32 + k_cap doubles) and a k_cap x k_cap fp64
 *     result, cap (12 + 8 cap) device bytes for k_cap = k rounded up to a
 *     multiple of 64, counted by krcn_csr_owned_bytes and freed by
 *     krcn_csr_destroy, plus pinned host memory (the result's mirror and the
 *     staging ring).  The block calls (krcn_matvec_block, krcn_rmatvec_block,
 *     krcn_hvp_block) build no plans.  krcn_hvp_block allocates its (n, k)
 *     intermediate, n * k * sizeof(dtype) device bytes, at its first call and
 *     again when k grows; the first block call that walks X, and the first
 *     that walks X^T, copies that matrix's row pointers to the host once
 *     (synchronising the stream) and keeps the ids of its rows above
 *     KRCN_BLOCK_LONG_ROW on the device, 4 bytes each, nothing when there is
 *     none.  Both are counted by krcn_csr_owned_bytes and freed by
 *     krcn_csr_destroy.  A handle of a multi-rank communicator never builds
 *     or allocates inside a compute call (that call fails instead), so no
 *     rank synchronises the device while its peers wait in a collective.
 *   - Errors: every call returns a krcn_status (0 = OK).  The message of the
 *     last failure on the calling thread is krcn_last_error_string().  No C++
 *     exception crosses this boundary.
 *   - A handle is not thread-safe; one host thread drives one device.
 *   - A handle is single-stream: its scratch (u, w, partials, the Lanczos
 *     state, the pinned staging buffer) lives on the handle, not per call, so
 *     every call on one handle must go to the same stream, or the caller must
 *     order calls on different streams itself (events).  Calls on different
 *     handles are independent.
 *   - Sharded handles (KRCN_SHARD_ROWS / _COLS) must hold at least one row and
 *     one column: every rank joins the collectives of every call, and an empty
 *     block is rejected by krcn_csr_create rather than left to hang its peers.
 */
#ifndef KRCN_H
#define KRCN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int krcn_status;
enum {
  KRCN_OK = 0,
  KRCN_ERR_INVALID = 1,     /* bad argument (null pointer, shape, dtype, m < 1) */
  KRCN_ERR_HIP = 2,         /* a HIP runtime call failed                        */
  KRCN_ERR_RCCL = 3,        /* an RCCL call failed                              */
  KRCN_ERR_UNSUPPORTED = 4  /* valid request this build does not implement      */
};

enum { KRCN_F64 = 0, KRCN_F32 = 1 };

/* How a matrix shard relates to the global X (n_global x d_global).
 * KRCN_SHARD_NONE: the handle holds all of X.
 * KRCN_SHARD_ROWS: the handle holds a contiguous block of rows; d-vectors are
 *                  replicated and the HVP all-reduces its d-length partial.
 * KRCN_SHARD_COLS: the handle holds a contiguous block of columns (local column
 *                  indices); d-vectors are sharded, the HVP all-reduces X_p v_p
 *                  (n-length) and Lanczos dots all-reduce one scalar each. */
enum { KRCN_SHARD_NONE = 0, KRCN_SHARD_ROWS = 1, KRCN_SHARD_COLS = 2 };

/* Row-group width policy of the CSR row kernels (lanes of a 64-wide wave that
 * cooperate on one row).  KRCN_LANES_AUTO picks from the mean row length;
 * KRCN_LANES_SEQUENTIAL (1 lane per row, left-to-right sum, no FMA contraction)
 * reproduces scipy's csr_matvec / csc_matvec summation order bit for bit. */
enum { KRCN_LANES_AUTO = 0, KRCN_LANES_SEQUENTIAL = 1 };

/* Column slicing of the two SpMV passes ("Slices"):
 * KRCN_SLICING_AUTO slices a pass when the vector it gathers exceeds ~3 MiB,
 * KRCN_SLICING_OFF never slices, a value k >= 8 (multiple of 8) forces k. */
enum { KRCN_SLICING_AUTO = 0, KRCN_SLICING_OFF = 1 };

/* Tile format of the SpMV passes ("Sorted tiles", "LDS windows"):
 * KRCN_FORMAT_AUTO picks per pass from a cost model, KRCN_FORMAT_WAVE uses
 * per-wave tiles in CSR order, KRCN_FORMAT_SORTED uses block tiles whose
 * nonzeros are stored sorted by gather index (same results, fewer distinct
 * cache lines per gather), KRCN_FORMAT_WINDOW copies column slices of the
 * gathered vector into LDS and sums each row in one lane (short rows),
 * KRCN_FORMAT_JAG gives every lane a row and stores the elements level by level
 * so that the whole LDS holds the gathered vector (one window, or two
 * double-buffered windows walked by every block; scipy's summation order).
 * KRCN_FORMAT_DENSE (nearly dense matrices) stores no indices:
 *   - Storage: each dense pass owns a row-major image of its own matrix (X for
 *     pass 1, n rows; X^T for pass 2, d rows), rows padded to whole 16-byte
 *     vectors, entries absent from the CSR stored as zeros: rows x ld x
 *     sizeof(dtype) device bytes per pass (krcn_dense_geometry reports them),
 *     about 2 n d sizeof(dtype) for both, counted by krcn_csr_owned_bytes.
 *     The plan build checks that the images fit the device's free memory
 *     before it allocates anything and returns KRCN_ERR_UNSUPPORTED (needed
 *     and free bytes in the message) otherwise, leaving the handle as it was.
 *   - Summation order: a row is summed by L lanes; lane l adds the products
 *     of the row's 16-byte vectors l, l + L, ... left to right, entry by
 *     entry; the L lane sums are combined by an xor butterfly, and the sums
 *     of column slices (few, long rows) are added in slice order.  Under
 *     KRCN_LANES_SEQUENTIAL a row is one left-to-right sum without FMA
 *     contraction: scipy's csr_matvec / csc_matvec bits for finite vectors.
 *   - Non-finite vectors: a dense pass multiplies the stored zeros, so an inf
 *     or nan in the gathered vector reaches every row, not only the rows that
 *     hold a nonzero in that column.  For finite vectors nothing changes.
 *   - Explicit stored zeros and rows with unsorted columns are fine.  Repeated
 *     entries are not supported: krcn_csr_create, and through it the
 *     transposed CSR that the coordinate calls and krcn_csr_get_transpose
 *     use, keep their duplicate-free-input assumption.
 *   - Never picked by KRCN_FORMAT_AUTO; one pass may be dense while the other
 *     keeps a CSR format (krcn_csr_set_pass_format).  Sharded handles return
 *     KRCN_ERR_UNSUPPORTED from the setters. */
enum { KRCN_FORMAT_AUTO = 0, KRCN_FORMAT_WAVE = 1, KRCN_FORMAT_SORTED = 2, KRCN_FORMAT_WINDOW = 3,
       KRCN_FORMAT_JAG = 4, KRCN_FORMAT_DENSE = 5 };

/* Stored width of the matrix values in the pass plans.  Arithmetic, vectors
 * and sums keep the handle's dtype.
 * Scope: on a KRCN_F64 handle KRCN_VALUES_F32 and _F32_EXACT narrow dense,
 * window-slices, window-accum and jagged passes (KRCN_PLAN_DENSE,
 * _WINDOW_SLICES, _WINDOW_ACCUM, _JAG).  Wave and sorted passes keep full
 * width.  krcn_csr_plan_value_bytes reports 4 for a narrowed pass and
 * sizeof(dtype) otherwise.  On a KRCN_F32 handle every policy is a no-op
 * (both passes report 4, results are bitwise the same).  The policy touches
 * the pass plans only: krcn_csr_get_transpose and the coordinate calls
 * (krcn_coord_*) read the handle's transposed CSR, which stays full width.
 * No default picks a narrowed plan.
 * A narrowed window or jagged pass on a KRCN_F64 handle:
 *   - Values: each stored value is static_cast<float>(v), the long-row arrays
 *     of a jagged plan included; it is widened to double when loaded (exact),
 *     and products, the LDS slabs, sums, partials and epilogues stay fp64.
 *     Pads stay zero.
 *   - Summation order: the full-width order of that format.  A narrowed pass
 *     is bitwise the full-width pass of the same plan over A32 =
 *     double(float(A)); wherever the full-width pass is bitwise scipy, the
 *     narrowed pass is bitwise scipy on A32.
 *   - Geometry and choice do not depend on the stored width: the automatic
 *     format choice, slices, tiles, lanes, grids and the jagged long-row rule
 *     are those of the full-width plan; krcn_csr_plan_info and
 *     krcn_csr_plan_format equal the full-width handle's.  Only the element
 *     type of the value arrays changes (10 -> 6 bytes per nonzero).
 *   - One matrix per operator: a window or jagged pass narrows only if the
 *     other pass narrows too (it is dense, window or jagged).  Otherwise both
 *     stay full width: an automatic plan with a sorted pass 1 and a jagged
 *     pass 2 never computes A32^T diag(w) A.  (A dense pass narrows whatever
 *     its partner is: dense + wave computes with A32 in the dense pass only.)
 *   - Internal copies: every copy of the matrix a narrowed plan holds carries
 *     A32.  The per-block X^T copy of a one-piece window-accum plan stores the
 *     widened rounded values at 8 bytes.
 * A narrowed dense pass on a KRCN_F64 handle:
 *   - Values: the image stores static_cast<float>(v) (round to nearest even);
 *     the kernel widens each stored value to double, which is exact, and
 *     products and sums are fp64.  The pass computes with A32 =
 *     double(float(A)) and nothing else.  Values outside fp32's normal range
 *     (overflow to inf, subnormal results, flush to zero) are the caller's
 *     responsibility.
 *   - Geometry: the dense geometry at 4-byte entries, four entries per 16-byte
 *     vector, ld a multiple of 4, lanes and slices from ceil(cols / 4)
 *     vectors: what krcn_dense_geometry(rows, cols, KRCN_F32, lanes, slicing,
 *     ..) returns, and what krcn_csr_plan_info reports.
 *   - Summation order: lane l of L adds the products of the 16-byte vectors
 *     l, l + L, ... of the row's slice, within a vector entry by entry, left
 *     to right (four entries per vector); then the xor butterfly, then the
 *     slices in slice order.  Under KRCN_LANES_SEQUENTIAL a row is one
 *     left-to-right sum without FMA contraction: scipy's csr_matvec /
 *     csc_matvec on A32, bit for bit, for finite vectors.
 *   - Memory: rows x ld x 4 image bytes per pass; the fit check against the
 *     device's free memory and krcn_csr_owned_bytes count the narrowed bytes.
 * KRCN_VALUES_F32_EXACT decides once per plan build, from a device scan of the
 * handle's borrowed CSR data: if every value survives double(float(v)) == v
 * (a NaN does not) the plans are bitwise those of KRCN_VALUES_F32, else
 * bitwise those of KRCN_VALUES_FULL. */
enum { KRCN_VALUES_FULL = 0,       /* the handle's dtype (default)                      */
       KRCN_VALUES_F32 = 1,        /* fp32, each value rounded to nearest even          */
       KRCN_VALUES_F32_EXACT = 2 };/* fp32 only if every value of the CSR survives the
                                      round trip double(float(v)) == v, else FULL       */

/* Formats reported by krcn_csr_plan_format. */
enum { KRCN_PLAN_WAVE = 1, KRCN_PLAN_SORTED = 2, KRCN_PLAN_WINDOW_SLICES = 3, KRCN_PLAN_WINDOW_ACCUM = 4,
       KRCN_PLAN_JAG = 5, KRCN_PLAN_DENSE = 6 };

typedef struct krcn_csr krcn_csr;
typedef struct krcn_comm krcn_comm;
typedef struct krcn_vctx krcn_vctx;

/* Result summary of krcn_lanczos (mirrors the reference's return values and
 * its truncation rule, optimizer/cubic.py:105-111). */
typedef struct {
  int m_eff;         /* number of basis vectors returned (columns of the reference V)   */
  int breakdown;     /* 1 if |beta| < tol ended the recurrence early (cubic.py:98-99)   */
  int j_break;       /* loop index j at which the breakdown happened, -1 if none        */
  int hvps;          /* Hessian-vector products executed (m when there is no breakdown) */
  double beta_last;  /* the reference's 4th return value `beta` (cubic.py:111)          */
  double gnorm;      /* ||g||_2, the normaliser of the first vector (cubic.py:85)       */
} krcn_lanczos_info;

/* Result summary of krcn_cg_solve (scipy.sparse.linalg.cg's return code, plus
 * what it does not report). */
typedef struct {
  int converged;         /* 1 if norm(r) < rtol ||b|| was reached (scipy info = 0) */
  int info;              /* scipy's info: 0 converged, maxiter if not              */
  int iterations;        /* updates of x performed                                 */
  int pad;
  double residual_norm;  /* ||r|| after the last update                            */
} krcn_cg_info;

/* Result record of krcn_crn_step; krcn_cubic_tridiag fills its solver fields
 * (solver_it, solver_status, reg_coef, lam, model_decrease) and zeroes the rest. */
typedef struct {
  int accepted;         /* 1: a trial met value_new <= value - model_decrease           */
  int trials;           /* backtracking trials after the first solve (0..max_trials)   */
  int solver_it;        /* Newton iterations of the last subproblem solve              */
  int solver_status;    /* 0 ok, 1 T + lam I not positive definite, 2 derivative zero,
                           3 it_max reached (root still returned, as root_scalar does) */
  double reg_coef;      /* M of the last solve                                         */
  double lam;           /* its root (the caller's next r0)                             */
  double model_decrease;
  double value_new;     /* f(x_new), l2 term included                                  */
  double dx_norm;       /* ||x_new - x||_2, krcn_diff_norm's bits                      */
  krcn_lanczos_info lanczos;
} krcn_crn_info;

/* ---- library ------------------------------------------------------------ */
const char* krcn_last_error_string(void);
int krcn_version(void);

/* ---- matrix handle ------------------------------------------------------ */
/* Upload-side constructor.  indptr (n+1), indices (nnz), data (nnz) are the
 * caller's device CSR arrays of the local block (borrowed: they must outlive
 * the handle).  The handle builds and owns the transposed CSR (X^T stored
 * explicitly, stable in row order so per-column sums run in the order of the
 * reference's csc_matvec scatter).
 * Replaces: the scipy CSR held by LogisticRegression (optimizer/loss.py:188,211)
 * and the zero-copy CSC view A.T it multiplies by (loss.py:227,302).
 * n_global: the reference's self.n (the 1/n of loss.py:227,302);
 * shard_mode: KRCN_SHARD_* (a COLS shard uses local column indices 0..d-1). */
krcn_status krcn_csr_create(int device, int64_t n, int64_t d, int64_t nnz,
                            const int32_t* indptr, const int32_t* indices,
                            const void* data, int dtype, int64_t n_global,
                            int shard_mode, krcn_csr** out);
krcn_status krcn_csr_destroy(krcn_csr* h);
/* Device bytes the handle holds now (transpose, pass plans, workspace). */
krcn_status krcn_csr_owned_bytes(const krcn_csr* h, int64_t* bytes_host);
/* Row-group policy for X (pass 1) and X^T (pass 2): KRCN_LANES_AUTO,
 * KRCN_LANES_SEQUENTIAL, or an explicit power of two 2..64. */
krcn_status krcn_csr_set_lanes(krcn_csr* h, int lanes_x, int lanes_xt);
/* Slicing policy (KRCN_SLICING_*, or a forced slice count). */
krcn_status krcn_csr_set_slicing(krcn_csr* h, int slicing);
/* Tile format policy (KRCN_FORMAT_*) of both passes. */
krcn_status krcn_csr_set_format(krcn_csr* h, int format);
/* Tile format policy of one pass (1: X, 2: X^T), overriding krcn_csr_set_format
 * for it; -1 returns the pass to the handle's policy. */
krcn_status krcn_csr_set_pass_format(krcn_csr* h, int pass, int format);
/* Stored width of the plans' matrix values (KRCN_VALUES_*; see there).
 * Invalidates the plans as krcn_csr_set_format does.  An unknown value is
 * KRCN_ERR_INVALID; on a sharded handle a value other than KRCN_VALUES_FULL is
 * KRCN_ERR_UNSUPPORTED; the handle is unchanged in both cases. */
krcn_status krcn_csr_set_value_storage(krcn_csr* h, int values);
/* Bytes per stored matrix value of each pass's plan (builds the plans if
 * needed): out2_host = {pass 1, pass 2}. */
krcn_status krcn_csr_plan_value_bytes(krcn_csr* h, int* out2_host);
/* Execution plan summary (builds the plan if needed):
 * out8_host = {slices, lanes, tiles, grid} of pass 1 (X) then pass 2 (X^T);
 * a sorted-tile pass reports its slice count negated; a dense pass reports
 * {slices, lanes, row groups, grid}.  A window plan reports the tiles of one
 * slice: ceil(rows / R) for fixed tiles of R rows; for a window-slices plan
 * whose tiles are cut from the data (as many rows, up to 64, as fill one
 * 256-nonzero chunk; long streams of short rows) the count of the slice with
 * the most tiles. */
krcn_status krcn_csr_plan_info(krcn_csr* h, int* out8_host);
/* Format of each pass's plan (KRCN_PLAN_*): out2_host = {pass 1, pass 2}. */
krcn_status krcn_csr_plan_format(krcn_csr* h, int* out2_host);
/* The step a krcn_lanczos call (with this reorth) would run on the handle as
 * it stands (builds the plans if needed, as krcn_csr_plan_format does):
 * *step_host = KRCN_LZ_*.  Not collective: a handle of a multi-rank
 * communicator without plans, or row shards that have not agreed on them,
 * get the error krcn_lanczos would give. */
enum { KRCN_LZ_GENERIC = 0, KRCN_LZ_FUSED_WINDOW = 1, KRCN_LZ_FUSED_SORTED = 2, KRCN_LZ_FUSED_SMALL = 3,
       KRCN_LZ_FUSED_SMALL_XT = 4, KRCN_LZ_TWO_LAUNCH = 5, KRCN_LZ_EARLY = 6, KRCN_LZ_EARLY_COLS = 7,
       KRCN_LZ_EARLY_ROWS = 8 };
krcn_status krcn_csr_lanczos_step(krcn_csr* h, int reorth, int* step_host);
/* Geometry of a dense pass (KRCN_FORMAT_DENSE) over a rows x cols matrix under
 * a lane and a slicing policy (as krcn_csr_set_lanes / krcn_csr_set_slicing
 * take them).  Host arithmetic only: needs no device.
 * out_host (8 entries) = {ld (entries per image row), lanes, slices, entries
 * of the widest slice, row groups, grid, image bytes (saturating at
 * INT64_MAX), 16-byte vectors per row}. */
krcn_status krcn_dense_geometry(int64_t rows, int64_t cols, int dtype, int lanes, int slicing,
                                int64_t* out_host);
/* Read back the transposed CSR (tests): colptr (d+1), rowidx (nnz), vals (nnz). */
krcn_status krcn_csr_get_transpose(const krcn_csr* h, int32_t* colptr,
                                   int32_t* rowidx, void* vals, void* stream);
/* hipGraph replay of krcn_lanczos (unsharded handles, profiling off): on = 1
 * records the whole launch sequence of a call the second time the same
 * arguments arrive and replays it with one hipGraphLaunch from then on
 * (bitwise the eager sequence).  Off by default: measured no faster on the
 * BASELINE shapes.  Replaces no reference call: the
 * reference's Lanczos loop is Python (optimizer/cubic.py:92-103). */
krcn_status krcn_csr_set_graph(krcn_csr* h, int on);
/* Placement probe of the hot buffers at every plan build (DESIGN.md §5
 * "Placement"): when the handle's per-HVP working set is within reach of the
 * 256 MiB Infinity Cache (96-400 MB), its plan arrays, partials and scratch
 * vectors are copied to trials - 1 further placements, each is timed with the
 * same local HVP (no collective) and the fastest is kept; the rest are freed.
 * Results are bitwise unchanged.  trials: -1 auto (4 in that band, else off;
 * the default), 0 off, 1..8 forced.  Invalidates the plans.  Replaces no
 * reference call (scipy's arrays live in host memory, optimizer/loss.py:188). */
krcn_status krcn_csr_set_placement_trials(krcn_csr* h, int trials);
/* Which of the probed placements is kept: keep = -1 the fastest (the default),
 * 0..7 placement min(keep, probed - 1) whatever the timings say, both at the
 * plan-build probe and after the search over krcn_lanczos calls below.  Every
 * placement is still built and timed.  Pins a placement for A/B timing, and
 * lets a test move the buffers on every run instead of when the timer says so.
 * A change invalidates the plans; a value outside -1..7 is KRCN_ERR_INVALID.
 * krcn_csr_get_placement_keep reads it back (the 24 doubles of
 * krcn_csr_placement_info are all taken).  Replaces no reference call. */
krcn_status krcn_csr_set_placement_keep(krcn_csr* h, int keep);
krcn_status krcn_csr_get_placement_keep(const krcn_csr* h, int* keep_host);
/* The same search continues over the first krcn_lanczos calls of such a
 * handle (unsharded or single-rank, no graph replay, m >= 8): call 1 runs
 * untimed, the next `trials` calls of the same m each run on one placement
 * (the probe's, then fresh copies), timed by events, and the fastest is kept
 * — the recurrence also streams the caller's V, which the plan-build probe
 * cannot see.  Results of every call are unchanged.
 * krcn_csr_placement_info (builds the plans if needed): out24_host =
 * {placements probed at the plan build, the one kept (-1: none), hot set MB,
 * policy, us per probe HVP of each placement (8 slots), Lanczos calls timed,
 * the placement kept after them (-1: not finished), their m, the search
 * stage, ms per timed call (8 slots)}. */
krcn_status krcn_csr_placement_info(krcn_csr* h, double* out24_host);
/* Attach a communicator for sharded operation (ROWS / COLS modes).  With a
 * communicator of more than one rank the pass plans are built here, before
 * any collective, and the call is COLLECTIVE for ROWS handles: every rank
 * calls it (each on its own thread for a virtual communicator), and the ranks
 * agree on the packed length of their one all-reduce per Lanczos step (the
 * pass-1 alpha partials ride past the d-vector; their count depends on the
 * rank's block).  krcn_csr_reserve after a policy change agrees again. */
krcn_status krcn_csr_attach_comm(krcn_csr* h, krcn_comm* comm);
/* Build the pass plans now (if a policy call invalidated them) and reserve
 * the workspace of krcn_lanczos up to m_max (1..2044; reorth = 1 adds the
 * CGS2 partials for m_max), so that later krcn_lanczos calls with m <= m_max
 * allocate and free nothing.  Required on a handle of a multi-rank
 * communicator after a policy change and before reorthogonalised calls.
 * Replaces no reference call (the reference allocates per numpy call). */
krcn_status krcn_csr_reserve(krcn_csr* h, int m_max, int reorth);

/* ---- objective pieces (optimizer/loss.py) -------------------------------- */
/* Ax = X x.                       Replaces LogisticRegression.mat_vec_product,
 *                                 loss.py:266-277 (the A @ x of :270).        */
krcn_status krcn_matvec(krcn_csr* h, const void* x, void* Ax, void* stream);
/* y = (X^T u) / n_global.         Replaces A.T @ u / self.n, loss.py:227,302. */
krcn_status krcn_rmatvec(krcn_csr* h, const void* u, void* y, void* stream);
/* w_i = s(1 - s), s = expit(Ax_i). Replaces loss.py:296-297 (hoisted: it
 *                                 depends on x only, not on v).               */
krcn_status krcn_weights(krcn_csr* h, const void* Ax, void* w, void* stream);
/* y = X^T (w (.) X v) / n + l2 v. Replaces LogisticRegression.hess_vec_prod,
 *                                 loss.py:289-302 (grad_dif=False branch).
 * l2 == 0 stores X^T(..)/n without reading v: the reference's + 0 * v gives
 * the same bits for every finite v, the sign of a zero included — a row sum
 * s is never -0 (it starts from +0; +0 + (-0) and x + (-x) round to +0), so
 * s/n + (+-0) = s/n — and would turn an inf / nan v into nan
 * (tests/test_gpu_hvp.py::test_l2_zero_hvp_signed_zeros). */
krcn_status krcn_hvp(krcn_csr* h, const void* w, const void* v, void* y,
                     double l2, void* stream);
/* grad = X^T (expit(Ax) - b) / n (+ l2 x when l2 != 0).
 *                                 Replaces LogisticRegression.gradient,
 *                                 loss.py:223-232.                            */
krcn_status krcn_gradient(krcn_csr* h, const void* Ax, const void* b,
                          const void* x, double l2, void* grad, void* stream);
/* SYNCHRONOUS.  *out_host = mean((1 - b) Ax - logsig(Ax)) (without the l2
 * term, which the host adds as the reference does).
 *                                 Replaces LogisticRegression._value,
 *                                 loss.py:215-220, and logsig, loss.py:161-176. */
krcn_status krcn_loss_mean(krcn_csr* h, const void* Ax, const void* b,
                           double* out_host, void* stream);

/* SYNCHRONOUS.  out_host[i] = mean((1 - b) X x_i - logsig(X x_i)) for k
 * iterates x_i (device d-vectors; xs_host is a HOST array of k device
 * pointers), without the l2 term — each value bitwise what krcn_matvec +
 * krcn_loss_mean return for that iterate, with all 2k launches in one
 * submission, one all-reduce of the k sums (ROWS) and one D2H.  Uses the
 * handle's n-vector scratch.
 * Replaces the loop `[self.loss.value(x) for x in self.xs]` of
 * Trace.compute_loss_of_iterates, optimizer/opt_trace.py:39-41 (with
 * optimizer.py:164-166), over iterates kept on the device. */
krcn_status krcn_loss_values(krcn_csr* h, int k, const void* const* xs_host, const void* b,
                             double* out_host, void* stream);

/* ---- coordinate blocks (SSCN) --------------------------------------------- */
/* A selection is k column indices cols_host (HOST int32): any order, repeats
 * allowed, 1 <= k <= KRCN_COORD_MAX.  It is validated on the host before
 * anything is launched: an index outside [0, d) or a k outside the range is
 * KRCN_ERR_INVALID with the offending position in the error string; no bad
 * index reaches a kernel.  Unsharded handles only (a sharded handle gets
 * KRCN_ERR_UNSUPPORTED), both dtypes: device vectors have the handle's dtype,
 * sums are accumulated in fp64 in a fixed order, host outputs are double.
 * The calls read the handle's transposed CSR (every column of X a row-sorted
 * list with distinct rows: a CSR without repeated entries), need no pass
 * plans (they never trigger the plan build) and use their own workspace, not
 * the handle's scratch vectors.  n == 0 or nnz == 0: l2 x_I, l2 I and a copy
 * of Ax_in (zeros if it is NULL), without reading the matrix.
 * Staging: cols_host and delta_host may be overwritten as soon as a call
 * returns.  Each call copies them into the next slot of a ring of pinned
 * staging slots (a host memcpy before the call returns) and enqueues the H2D
 * copy from that slot with an event behind it; a slot is refilled only once
 * its event has completed, so back-to-back asynchronous calls never share a
 * slot in flight, and the one device copy is ordered by the handle's stream. */
enum { KRCN_COORD_MAX = 1024 };
/* SYNCHRONOUS. g_host[a] = sum_r X[r,c_a] (expit(Ax_r) - b_r) / n_global (+ l2 x[c_a] when l2 != 0);
 * entry a depends on column c_a alone, not on the rest of the selection.
 * Replaces LogisticRegression.partial_gradient, loss.py:234-247. */
krcn_status krcn_coord_gradient(krcn_csr* h, int k, const int32_t* cols_host, const void* Ax,
                                const void* b, const void* x, double l2, double* g_host, void* stream);
/* SYNCHRONOUS. H_host[a*k+b] = sum_r w_r X[r,c_a] X[r,c_b] / n_global + l2 [a == b],
 * w_r = s(1-s), s = expit(Ax_r), computed in the kernel with krcn_weights' arithmetic.
 * H_host is exactly symmetric, and positions that repeat an index carry the
 * same sums (the kernel runs on the distinct columns; l2 sits on a == b only,
 * as the reference's l2 * eye(k)).  Replaces partial_hessian, loss.py:257-264;
 * with cols = 0..d-1 also hessian, loss.py:249-255. */
krcn_status krcn_coord_hessian(krcn_csr* h, int k, const int32_t* cols_host, const void* Ax,
                               double l2, double* H_host, void* stream);
/* Asynchronous. Ax_out = Ax_in + X[:, cols] delta (Ax_in may be NULL: Ax_out = X[:, cols] delta;
 * Ax_out may alias Ax_in), summed per row column by column in the order of
 * cols, repeats included, product and sum rounded separately: scipy's
 * csc_matvec order, so fp64 is bitwise Ax_in + A.tocsc()[:, cols] @ delta.
 * Replaces update_mat_vec_product, loss.py:279-281. */
krcn_status krcn_coord_update(krcn_csr* h, int k, const int32_t* cols_host, const double* delta_host,
                              const void* Ax_in, void* Ax_out, void* stream);
/* Rows of the LDS window the coordinate kernels walk the samples in: 0 = auto
 * (Hessian: what fits the LDS, 20,416 rows per block; update: 256 rows per
 * wave), otherwise a multiple of 64, clamped to 20,416 (Hessian) and 1,024
 * (update); tests use small values to cross window boundaries on small n.
 * Results of the update do not depend on it. */
krcn_status krcn_csr_set_coord_window(krcn_csr* h, int rows);

/* ---- block products: k vectors per pass over X ----------------------------- */
/* A block of k vectors over a space of length L (n or d) is an (L, k) row-major
 * DEVICE array of the handle's dtype: element (i, j) at i * k + j, a
 * C-contiguous (L, k) torch or numpy array; 1 <= k <= KRCN_BLOCK_MAX, any k.
 * Each call streams the matrix (index + value) once for the whole block and
 * gathers the k contiguous values of a column of the block together; pass 1
 * walks the caller's CSR of X, pass 2 the handle's transposed CSR.  The calls
 * need no pass plans (they never trigger the plan build) and do not use the
 * handle's scratch vectors.  Unsharded handles only (a sharded handle gets
 * KRCN_ERR_UNSUPPORTED); a null handle, a k outside the range, a w_cols that is
 * neither 1 nor k or a null array are KRCN_ERR_INVALID, all before any HIP call.
 * Inputs and outputs must not alias one another.
 * Summation order: entry (r, j) is the left-to-right sum over row r's stored
 * elements of a_e * V[col_e, j], product and sum rounded separately: scipy's
 * csr_matvecs order on X and csc_matvecs order on X^T, bit for bit in fp64,
 * for every row of at most KRCN_BLOCK_LONG_ROW stored elements.  A longer row
 * (of X or of X^T) is cut into 1024 / K contiguous segments of
 * ceil(len / (1024 / K)) elements, K the next power of two >= k; each segment is
 * summed left to right and the segment sums are added in segment order: a
 * fixed order that depends on the row's length and K alone (no atomics;
 * bitwise equal from run to run and whatever the other rows are).
 * n == 0 or nnz == 0: zeros, and l2_j V[:, j] from krcn_hvp_block, without
 * reading the matrix. */
enum { KRCN_BLOCK_MAX = 16, KRCN_BLOCK_LONG_ROW = 512 };
/* T (n,k) = X V (d,k).                      k single krcn_matvec calls */
krcn_status krcn_matvec_block(krcn_csr* h, int k, const void* V, void* T, void* stream);
/* Y (d,k) = X^T U (n,k) / n_global.         k single krcn_rmatvec calls */
krcn_status krcn_rmatvec_block(krcn_csr* h, int k, const void* U, void* Y, void* stream);
/* Y[:,j] = X^T (w_j (.) X V[:,j]) / n + l2_j V[:,j].  w_cols = 1: one n-vector
 * of weights for every column (H V at one x); w_cols = k: an (n,k) block
 * (k problems over one X).  l2_host: k HOST doubles, read before the call
 * returns; NULL = all zero.  A column with l2_j == 0 never reads V in the
 * epilogue, as krcn_hvp.  Replaces hess_vec_prod, loss.py:289-302, k times. */
krcn_status krcn_hvp_block(krcn_csr* h, int k, const void* w, int w_cols, const void* V, void* Y,
                           const double* l2_host, void* stream);

/* ---- Lanczos (optimizer/cubic.py:77-111) -------------------------------- */
/* SYNCHRONOUS on return of alphas/betas/info.  Runs the reference three-term
 * Lanczos on the operator v -> hess_vec_prod(x, v) (w = weights at x), started
 * from g.  V is the caller's device basis of m rows x ld columns (row j = the
 * reference's column V[:, j], contiguous; ld = local d).  alphas_host[m],
 * betas_host[max(m-1,1)] receive the reference's alphas/betas (already
 * truncated to info->m_eff / m_eff-1 entries; entries past that are zero).
 * reorth = 0 reproduces the reference (no reorthogonalisation, the default);
 * reorth = 1 adds classical Gram-Schmidt twice (CGS2) against all previous
 * basis vectors (build-only extension; not in the reference).  An unsharded
 * handle whose V is 16-byte aligned with rows of whole 16-byte vectors
 * (ld * sizeof(T) % 16 == 0) runs the 1 KiB-row-piece sweeps with step B in
 * the first; otherwise the batched sweeps run (the same CGS2, summed in
 * another fixed order).
 * tol is the reference's absolute breakdown threshold (1e-6, cubic.py:98). */
krcn_status krcn_lanczos(krcn_csr* h, const void* w, const void* g, int m,
                         int reorth, double tol, double l2, void* V,
                         double* alphas_host, double* betas_host,
                         krcn_lanczos_info* info_host, void* stream);

/* SYNCHRONOUS.  The reorthogonalisation of krcn_lanczos (reorth = 1) on a
 * caller's basis, outside any recurrence: classical Gram-Schmidt twice,
 *   z1 = z - V_k^T (V_k z),  z2 = z1 - V_k^T (V_k z1),  z <- z2 in place,
 * over the first k rows V_k of the row-major device array V (rows of d = the
 * handle's column count, contiguous).  V need NOT be orthonormal: the call
 * applies the two sweeps as written, whatever V holds, and leaves V untouched.
 * The same launches as a recurrence step that sweeps k rows run: the 1 KiB-row-
 * piece sweeps when V and z are 16-byte aligned and rows are whole 16-byte
 * vectors (d * sizeof(T) % 16 == 0), else the batched sweeps; *path_host
 * receives 1 for the former and 0 for the latter.  *norm2_host receives
 * ||z2||^2 as the recurrence forms the next beta^2: the sweeps' per-block
 * partials (of the rounded, stored z2) added in the recurrence's fixed order.
 * Either out pointer may be NULL.  Products and sums are in double for both
 * dtypes, in a fixed order: bitwise equal from call to call.
 * Workspace: as an unsharded krcn_lanczos(reorth = 1) with m = k + 1 reserves
 * it on its first call (krcn_csr_reserve(h, k + 1, 1) beforehand makes the
 * call allocation-free); builds no pass plans.  The device Lanczos state of
 * the handle is reset, as by a recurrence's start.
 * KRCN_ERR_INVALID before any HIP call: k outside 1..2043, a null handle, a
 * null V or z.  Sharded handles: KRCN_ERR_UNSUPPORTED.
 * What optimizer/cubic.py's Lanczos over a callable A needs for reorth=True
 * (build-only extension; not in the reference). */
krcn_status krcn_cgs2(krcn_csr* h, int k, const void* V, void* z,
                      double* norm2_host, int* path_host, void* stream);

/* ---- batched Lanczos: k recurrences in lockstep over the block HVP --------- */
/* SYNCHRONOUS on return of alphas/betas/info.  k independent recurrences of
 * krcn_lanczos (reorth = 0) over one X, advanced together: every step runs one
 * krcn_hvp_block for all columns (m of them per call: m - 1 loop steps and the
 * final quotient) and at most three vector launches over (d, k) blocks; control
 * stays on the device and the call synchronises once, at its end.  Not a
 * block-Krylov method: column c is the reference's Lanczos(A_c, G[:, c], m)
 * with A_c = v -> X^T (w_c (.) X v) / n + l2_c v, every quirk included, and its
 * results do not depend on what the other columns hold (bitwise), nor on the
 * run.  Per column the outcome is what krcn_lanczos(h, w_c, G[:, c], m, 0, tol,
 * l2_c, ..) defines: the absolute |beta| < tol test, truncation only when
 * j < m - 2, a zero last vector and betas[m - 2] = 0 for a breakdown at
 * j == m - 2, the final alphas[m_eff - 1] = v.A(v) on the column's current v,
 * zeros past m_eff / m_eff - 1, one Rayleigh quotient for m = 1; info_host[c]
 * as krcn_lanczos fills it (hvps: what the single call would report for the
 * column, not the block HVPs run).  The sums run in another fixed order than
 * krcn_lanczos's, so the values agree at the rounding level, not bitwise.
 * A column that has broken down is frozen: its alphas, betas and state stop
 * changing and its v is never divided by the tiny beta.
 * Layouts: G a (d, k) block (element (i, c) at i * k + c); w an n-vector
 * (w_cols = 1) or an (n, k) block (w_cols = k); l2_host k HOST doubles (NULL:
 * all zero); V m slabs of (d, k), element (j, i, c) at (j * d + i) * k + c (a
 * C-contiguous (m, d, k) tensor; slab j is a block-HVP operand);
 * alphas_host[k * m], row c at c * m; betas_host[k * max(m - 1, 1)], row c at
 * c * max(m - 1, 1); info_host[k].  The call writes column c of every slab:
 * its basis vectors, and zeros in every slab that holds none of column c,
 * whatever V held before, so krcn_basis_combine_block may run over all m slabs
 * with s zero-padded.  A zero start column gives NaNs in that column.
 * Both dtypes, scalars in double.  Builds no pass plans and does not touch the
 * handle's scratch vectors or the results block of krcn_lanczos.  Workspace:
 * two (d, k) blocks, 393,216 bytes of partials and a results block of
 * k (2 m + 3 (+ 1 when m = 1)) doubles (with a pinned host mirror), in the
 * handle's owner table, counted by krcn_csr_owned_bytes, grown only when k or
 * the results block grows, freed by krcn_csr_destroy; krcn_hvp_block's (n, k)
 * intermediate as there.  A second call with the same (k, m) allocates nothing.
 * KRCN_ERR_INVALID before any HIP call: k outside 1..KRCN_BLOCK_MAX, m outside
 * 1..2044, w_cols neither 1 nor k, a null handle, a null array.  Sharded
 * handles: KRCN_ERR_UNSUPPORTED.
 * Replaces k calls of Lanczos, cubic.py:77-111 (cubic_newton.py:67-73 runs
 * two problems over one matrix). */
krcn_status krcn_lanczos_block(krcn_csr* h, int k, const void* w, int w_cols, const void* G, int m,
                               double tol, const double* l2_host, void* V,
                               double* alphas_host, double* betas_host,
                               krcn_lanczos_info* info_host, void* stream);
/* Xnew[i, c] = X0[i, c] + sum_j V[j, i, c] * s[j * k + c], j ascending over all
 * m slabs (zero-pad s past a column's m_eff): per column krcn_basis_combine's
 * sum, bit for bit.  s_host: (m, k) HOST doubles, read before the call
 * returns.  X0 and Xnew are (d, k) blocks.  Replaces x + V @ s_new,
 * cubic.py:291,301, k times. */
krcn_status krcn_basis_combine_block(krcn_csr* h, int k, int m, const void* V, const double* s_host,
                                     const void* X0, void* Xnew, void* stream);
/* W = s (1 - s), s = expit(AX), over the n k entries of AX = X xs (an (n, k)
 * block, krcn_matvec_block's result for k iterates): krcn_weights column by
 * column, bit for bit.  Replaces loss.py:296-297, k times. */
krcn_status krcn_weights_block(krcn_csr* h, int k, const void* AX, void* W, void* stream);

/* x_new = x + V^T s over the first m_eff basis rows (the reference's
 * x + V @ s_new, cubic.py:291,301).  V is the handle's basis (m rows x local d),
 * s_host an m_eff-vector on the host; x, x_new are local d-vectors. */
krcn_status krcn_basis_combine(krcn_csr* h, int m_eff, const void* V,
                               const double* s_host, const void* x, void* x_new,
                               void* stream);

/* ---- conjugate gradients on the Hessian (full-space CRN) ---------------- */
/* SYNCHRONOUS.  Solves (H + shift I) x = b, H = X^T diag(w) X / n_global,
 * by unpreconditioned conjugate gradients from x0 = 0 with scipy's loop and
 * stopping rule (scipy.sparse.linalg.cg: stop when ||r|| < rtol ||b||, at most
 * maxiter updates; ||b|| = 0 returns x = 0).  Each iteration is one HVP on the
 * device plus two vector launches; control stays on the device.
 * Replaces the cg(LinearOperator(v -> hess_vec_prod(x, v) + lam v), -g, tol)
 * calls of Cubic_LS.cubic_solver_root_CG, optimizer/cubic.py:152-182 (pass the
 * reference's l2 + lam as shift).  Unsharded handles only. */
krcn_status krcn_cg_solve(krcn_csr* h, const void* w, const void* b, double shift,
                          double rtol, int maxiter, void* x,
                          krcn_cg_info* info_host, void* stream);

/* ---- the Krylov-CRN step on the device ---------------------------------- */
/* SYNCHRONOUS.  argmin_s <g,s> + 1/2 s^T T s + M/3 ||s||^3 for
 * T = tridiag(betas, alphas, betas) (m and m - 1 host entries; betas_host may
 * be NULL when m = 1) and g = gnorm e1, solved by one workgroup on the device
 * in fp64 whatever the handle's dtype: scipy's scalar Newton (root_scalar,
 * method="newton", x0 = r0, xtol = eps, maxiter = it_max) on
 * phi(lam) = lam^2 - M^2 ||s(lam)||^2, each shifted solve an LDL^T of
 * T + lam I by dpttrf's recurrence with dpttrs's substitutions, and the
 * reference's closing expressions.  s_host receives the m entries of s (zeros
 * when the solve failed: solver_status 1 or 2); 1 <= m <= 2044, it_max >= 1.
 * Allocates the step workspace on a handle that was not reserved.
 * Replaces cubic_solver_root on the Krylov subspace model, cubic.py:40-75
 * (called at cubic.py:285-286, :298-299). */
krcn_status krcn_cubic_tridiag(krcn_csr* h, int m, const double* alphas_host, const double* betas_host,
                               double gnorm, double M, double r0, double eps, int it_max,
                               double* s_host, krcn_crn_info* info_host, void* stream);

/* SYNCHRONOUS.  One Krylov-CRN step from x with f(x) = value: Ax = X x if Ax is
 * NULL, the gradient, the Hessian weights, the m-step Lanczos recurrence of
 * krcn_lanczos (same reorth / tol / l2; its alphas, betas and state stay on the
 * device), then the line search: M = reg_coef * ls_beta, trial 0, and while
 * value_new > value - model_decrease and trials < max_trials: M /= ls_beta and
 * the next trial.  A trial is the subproblem of krcn_cubic_tridiag from r0
 * (every trial starts from the caller's r0), x_new = x + V^T s,
 * Ax_new = X x_new, f(x_new) = mean + l2 / 2 * ||x_new||^2, and the test; the
 * decision is taken on the device and the launches of later trials are guarded
 * by it, so x_new / Ax_new hold the accepted trial (the last one at the cap).
 * The host enqueues trials 0 and 1, then batches of four, and synchronises once
 * per batch.  A failed solve (solver_status 1 or 2) ends the chain; x_new and
 * Ax_new are then unspecified.  V is the basis (m rows x d, as krcn_lanczos),
 * x_new a d-vector and Ax_new an n-vector that alias no input; alphas_host[m]
 * and betas_host[max(m-1,1)] receive the recurrence's results as krcn_lanczos
 * returns them and may be NULL.  Graph replay and the Lanczos placement search
 * do not run inside this call.  Unsharded handles only
 * (KRCN_ERR_UNSUPPORTED otherwise); allocates nothing on a reserved handle
 * (krcn_csr_reserve also reserves this call's workspace).
 * Replaces the body of Cubic_Krylov_LS.step, cubic.py:265-309. */
krcn_status krcn_crn_step(krcn_csr* h, const void* x, const void* b, const void* Ax, double value,
                          int m, int reorth, double tol, double l2, double reg_coef, double ls_beta,
                          double r0, double solver_eps, int solver_it_max, int max_trials, void* V,
                          void* x_new, void* Ax_new, double* alphas_host, double* betas_host,
                          krcn_crn_info* info_host, void* stream);

/* ---- the SSCN step on the device ------------------------------------------ */
/* Largest coordinate block of krcn_cubic_dense / krcn_sscn_step (the reference
 * driver's default subspace_dim is 100). */
enum { KRCN_SSCN_MAX = 128 };

/* SYNCHRONOUS.  argmin_s <g,s> + 1/2 s^T H s + M/3 ||s||^3 for a symmetric
 * k x k H (HOST, row-major k * k; only the upper triangle, column >= row, is
 * read, as by the host's solve(assume_a='pos')) and a general g (k HOST
 * doubles), 1 <= k <= KRCN_SSCN_MAX.  Solved by one workgroup on the device in
 * fp64 whatever the handle's dtype: scipy's scalar
 * Newton (root_scalar, method="newton", x0 = r0, xtol = eps, maxiter = it_max)
 * on phi(lam) = lam^2 - M^2 ||s(lam)||^2 — the loop krcn_cubic_tridiag runs —,
 * one Cholesky factorisation of H + lam I per lam shared by phi and dphi (a
 * pivot <= 0 or non-finite is solver_status 1, the host's LinAlgError from
 * solve(assume_a='pos')), two substitution pairs per lam, fixed-order sums and
 * the reference's closing expressions.  Fills the solver fields of info_host
 * (solver_it, solver_status, reg_coef, lam, model_decrease) and zeroes the
 * rest; s_host receives the k entries of s (zeros when the solve failed:
 * solver_status 1 or 2).  Argument errors (null handle or pointer, k outside
 * the range, it_max < 1) are KRCN_ERR_INVALID before any HIP call.  Uses the
 * coordinate workspace and the step workspace (allocated on first use).
 * Replaces cubic_solver_root (dense branch), cubic.py:40-75, as SSCN calls it
 * (cubic.py:373-374, :386-387). */
krcn_status krcn_cubic_dense(krcn_csr* h, int k, const double* H_host, const double* g_host, double M,
                             double r0, double eps, int it_max, double* s_host,
                             krcn_crn_info* info_host, void* stream);

/* SYNCHRONOUS.  One SSCN step from x with f(x) = value over the k DISTINCT
 * columns cols_host (HOST int32, 1 <= k <= KRCN_SSCN_MAX): Ax = X x if Ax is
 * NULL, the coordinate gradient and the coordinate Hessian block
 * (krcn_coord_gradient's and krcn_coord_hessian's kernels; their results stay
 * on the device), x_new = x (one D2D copy), then the line search:
 * M = max(reg_coef * ls_beta, DBL_EPSILON), trial 0, and while
 * value_new > value - model_decrease and trials < max_trials: M /= ls_beta and
 * the next trial.  A trial is the subproblem of krcn_cubic_dense over the block
 * in selection order with l2 on its diagonal (every trial starts from the
 * caller's r0), x_new[c_a] = x[c_a] + s_a, Ax_new = Ax + X[:, cols] s
 * (krcn_coord_update's walk; every trial starts from the same Ax),
 * f(x_new) = mean + l2 / 2 * ||x_new||^2 from krcn_loss_mean's and
 * krcn_diff_norm's partial sums in their order, and the test; the decision is
 * taken on the device and the launches of later trials are guarded by it, so
 * x_new / Ax_new hold the accepted trial (the last one at the cap).  The host
 * enqueues trials 0 and 1, then batches of four, synchronises once per batch
 * and never before the first batch ends.  A failed solve (solver_status 1 or
 * 2) ends the chain; x_new and Ax_new are then unspecified.  info_host: the
 * fields of krcn_crn_step, with dx_norm the solver's ||s|| and `lanczos`
 * zeroed.  x_new (d) and Ax_new (n) alias no input.
 * Refused with KRCN_ERR_INVALID before any launch, the position named: an
 * index outside [0, d), a repeated index, k outside [1, KRCN_SSCN_MAX];
 * sharded handles get KRCN_ERR_UNSUPPORTED.  n == 0 or nnz == 0: the model is
 * the l2 term alone (gradient l2 x_I, Hessian l2 I, Ax_new a copy of Ax), as
 * in the coordinate calls; with n == 0 the mean over no rows counts as 0, so
 * value_new = l2 / 2 * ||x_new||^2 (b, Ax and Ax_new may then be NULL).  Workspace: the coordinate workspace, the step
 * workspace of krcn_crn_step and 2,560 bytes of its own, all in the owner table
 * and counted by krcn_csr_owned_bytes; a second step with the same k allocates
 * nothing.  Builds pass plans only when Ax is NULL (before any scratch buffer
 * is read: the build may move them).
 * Replaces the body of SSCN.step, cubic.py:352-398. */
krcn_status krcn_sscn_step(krcn_csr* h, int k, const int32_t* cols_host, const void* x, const void* b,
                           const void* Ax, double value, double l2, double reg_coef, double ls_beta,
                           double r0, double solver_eps, int solver_it_max, int max_trials, void* x_new,
                           void* Ax_new, krcn_crn_info* info_host, void* stream);

/* ---- the SSCN step over one tridiagonal reduction (k up to 1024) ---------- */
/* Largest coordinate block of krcn_dense_tridiag, krcn_cubic_dense_tridiag and
 * krcn_sscn_step_tridiag (= KRCN_COORD_MAX; the reference's experiment script
 * runs SSCN with subspace dimensions up to 1000). */
enum { KRCN_SSCN_TRIDIAG_MAX = 1024 };

/* The route.  H is the same for every lam of a solve and every trial of a step,
 * so it is reduced once, by Householder reflectors, to T = Q^T H Q tridiagonal
 * with Q's first column along g; the subproblem is then krcn_cubic_tridiag's
 * (g = b_0 e1, O(k) per lam) and s = Q s_T, with ||s|| = ||s_T|| and
 * g.s = b_0 (s_T)_0, so the reference's closing expressions are unchanged.
 * The reduction works in fp64, whatever the handle's dtype, on the bordered
 * matrix B = [[0, g^T], [g, H]] of order K = k + 1 in full storage: its first
 * reflector maps g to b_0 e1 (b_0 = -sign(g_0) ||g||, sign(0) = +) and the later
 * ones leave that direction fixed.  LAPACK dlarfg's conventions without its
 * rescaling of tiny columns; tau = 0 (the identity, no division) when the column
 * below the subdiagonal is already zero, so g = 0, a diagonal H and a decoupled
 * block pass through.  One launch per column j = 0 .. K - 3 with one workgroup
 * per 4 rows of the trailing block, a fill kernel before and a one-workgroup
 * closing kernel after; no workgroup waits on another, no atomics, every sum in
 * a fixed order: the bits depend on k and the data alone.
 * Workspace: B, the reflector rows, two p vectors, tau / alphas / betas, g, s_T
 * and the selection: 8 ld (2 (k + 1) + 9) bytes with ld = k + 1 rounded up to a
 * multiple of 8 (16,999,104 bytes at k = 1024), one buffer of the handle's owner
 * table, counted by krcn_csr_owned_bytes, allocated by the first call that needs
 * it and grown (freed and reallocated) only when a later call has a larger k. */

/* Host arithmetic only: needs no device.  The column launches of a reduction of
 * a k-column block (k - 1 for k >= 2, none for k = 1) and the bytes of its
 * workspace, in 64 bits.  KRCN_ERR_INVALID: k outside
 * [1, KRCN_SSCN_TRIDIAG_MAX], a null pointer. */
krcn_status krcn_dense_tridiag_geometry(int k, int64_t* launches_host, int64_t* workspace_bytes_host);

/* SYNCHRONOUS.  The reduction alone, for a symmetric k x k H (HOST, row-major;
 * only the upper triangle, column >= row, is read, as by krcn_cubic_dense) and
 * g (k HOST doubles), 1 <= k <= KRCN_SSCN_TRIDIAG_MAX.  alphas_host (k): T's
 * diagonal.  betas_host (k): betas[0] = b_0, the signed ||g||; betas[1..k) T's
 * off-diagonal.  Q_host, if not NULL (k x k, row-major): Q, formed by
 * back-transforming the k unit vectors (a test path, one workgroup a column).
 * H = Q T Q^T and g = b_0 Q e1.  Argument errors (null handle or pointer other
 * than Q_host, k outside the range) are KRCN_ERR_INVALID before any HIP call.
 * Replaces nothing of the reference by itself: it is the factorisation that
 * krcn_cubic_dense_tridiag puts in place of the per-lam solves of
 * cubic_solver_root, cubic.py:60-62 (func), :64-67 (grad) and :72. */
krcn_status krcn_dense_tridiag(krcn_csr* h, int k, const double* H_host, const double* g_host,
                               double* alphas_host, double* betas_host, double* Q_host, void* stream);

/* SYNCHRONOUS.  krcn_cubic_dense's contract and result record for
 * 1 <= k <= KRCN_SSCN_TRIDIAG_MAX by the route above: one reduction, then
 * krcn_cubic_tridiag's kernel on (alphas, betas[1..k), gnorm = b_0) — the same
 * scalar Newton loop, one LDL^T of T + lam I per lam — and the back-transform
 * s = Q s_T (reflectors applied last to first).  The solver statuses keep their
 * meaning: a non-positive or non-finite pivot of the LDL^T is solver_status 1
 * (the host's LinAlgError), 2 phi' = 0, 3 it_max reached; s_host is zeroed on 1
 * and 2.  Argument errors (null handle or pointer, k outside the range,
 * it_max < 1) are KRCN_ERR_INVALID before any HIP call.
 * Replaces cubic_solver_root, cubic.py:40-75 (its dense branch :49-52, :56-58
 * and, for a sparse H of 500 or more columns, its spsolve branch :53-55), as
 * SSCN calls it
 * (cubic.py:373-374, :386-387). */
krcn_status krcn_cubic_dense_tridiag(krcn_csr* h, int k, const double* H_host, const double* g_host, double M,
                                     double r0, double eps, int it_max, double* s_host,
                                     krcn_crn_info* info_host, void* stream);

/* SYNCHRONOUS.  krcn_sscn_step's signature and contract with
 * 1 <= k <= KRCN_SSCN_TRIDIAG_MAX.  The chain: Ax = X x if Ax is NULL, the
 * coordinate gradient and Hessian block, the reduction (once per step, before
 * the first trial, whatever the number of trials), x_new = x, the chain's begin
 * with M = max(reg_coef * ls_beta, DBL_EPSILON), gnorm = b_0 and m_eff = k; then
 * the trials, each [tridiagonal solve -> back-transform (writes s and
 * x_new[c_a] = x[c_a] + s_a) -> coordinate update of Ax -> loss and norm
 * partials -> judge], in krcn_sscn_step's batches over the same chain state.
 * info_host as krcn_sscn_step's; dx_norm is ||s_T|| (= ||s||).  The same
 * refusals with the same position-naming messages: an index outside [0, d), a
 * repeated index, k outside the range (KRCN_ERR_INVALID before any launch);
 * sharded handles get KRCN_ERR_UNSUPPORTED.  Workspace: the coordinate
 * workspace, the step workspace of krcn_crn_step and the reduction's; a second
 * step with the same k allocates nothing.  Builds pass plans only when Ax is
 * NULL, before any scratch buffer is read.
 * Replaces the body of SSCN.step, cubic.py:352-398. */
krcn_status krcn_sscn_step_tridiag(krcn_csr* h, int k, const int32_t* cols_host, const void* x, const void* b,
                                   const void* Ax, double value, double l2, double reg_coef, double ls_beta,
                                   double r0, double solver_eps, int solver_it_max, int max_trials, void* x_new,
                                   void* Ax_new, krcn_crn_info* info_host, void* stream);

/* ---- the full-space cubic subproblem on the device: Newton over CG -------- */
/* Result record of krcn_cubic_cg. */
typedef struct {
  int solver_it, solver_status;      /* as krcn_crn_info; status 4: a non-finite lam, rho or p.q ended the chain */
  int cg_solves, cg_unconverged;     /* solves run; solves that ended at cg_maxiter */
  int64_t cg_iterations, ticks;      /* x-updates over all solves; ticks enqueued until the end was seen */
  double reg_coef, lam, model_decrease, s_norm;
} krcn_cubic_cg_info;

/* SYNCHRONOUS.  argmin_s <g,s> + 1/2 s^T H s + M/3 ||s||^3 for
 * H = X^T diag(w) X / n_global + l2 I, never formed: scipy's scalar Newton
 * (root_scalar, method="newton", x0 = r0, xtol = eps, maxiter = it_max) on
 * phi(lam) = lam^2 - M^2 ||s(lam)||^2 — the loop krcn_cubic_tridiag runs —
 * with every (H + lam I)^{-1} applied by krcn_cg_solve's conjugate gradients
 * (shift l2 + lam, rtol cg_rtol, at most cg_maxiter updates, 10 d when
 * cg_maxiter <= 0): y = (H + lam I)^{-1} g for phi, z = (H + lam I)^{-1} y for
 * its derivative, the closing solve at the root, s = -y, and the reference's
 * closing expressions (s_norm = ||s||, krcn_diff_norm's bits; model_decrease
 * with krcn_dot's g.s).  w is the n-vector of Hessian weights, g and s are
 * d-vectors of the handle's dtype that do not alias; scalars, sums and the
 * Newton iteration are double.
 * The host enqueues ticks — one CG iteration (the launches of krcn_cg_solve's)
 * and one single-workgroup turn that takes every decision on the device: has
 * the solve ended, the Newton step, the next solve's shift and tolerance — in
 * batches of 16, synchronises once per batch and reads one mapped record;
 * launches after the end return at once.  A solve that stops at cg_maxiter is
 * counted in cg_unconverged and its iterate used, as the host path does.
 * solver_status: 0 ok; 1 p.q <= 0 with rho > 0 (H + lam I is not positive
 * definite); 2 phi' = 0; 3 it_max reached (the last iterate is the root and
 * the closing solve still runs, as root_scalar returns it); 4 a non-finite
 * lam, rho or p.q.  Statuses 1, 2 and 4 end the chain with s zeroed.
 * KRCN_ERR_INVALID before any HIP call, scalars first: it_max < 1,
 * !(cg_rtol >= 0), M not positive and finite, !(eps >= 0), a null handle or
 * pointer, s == g; sharded handles get KRCN_ERR_UNSUPPORTED; d == 0 returns
 * KRCN_OK with info zeroed.  KRCN_ERR_HIP if the chain has not ended after
 * (2 it_max + 1)(cg_maxiter + 1) ticks.
 * Workspace: krcn_cg_solve's r | p | q, one more d-vector, a state block of
 * 16,512 bytes (all in the owner table, counted by krcn_csr_owned_bytes) and a
 * mapped host record, allocated by the first call; a second call allocates
 * nothing.  Builds pass plans on first use, before any scratch buffer is read.
 * Replaces the root_scalar loop of Cubic_LS.cubic_solver_root_CG,
 * cubic.py:152-182. */
krcn_status krcn_cubic_cg(krcn_csr* h, const void* w, const void* g, double l2, double M, double r0,
                          double eps, int it_max, double cg_rtol, int cg_maxiter /* <= 0: 10 d */,
                          void* s /* d-vector, out */, krcn_cubic_cg_info* info_host, void* stream);

/* ---- the dense Hessian as one Gram product (fp64 MFMA) -------------------- */
/* Asynchronous.  H (DEVICE, d x d doubles, row-major) = X^T diag(w) X / n_global
 * + l2 I, computed as A diag(w) A^T over the dense image A of X^T that a
 * KRCN_PLAN_DENSE pass 2 owns (d rows of ld >= n stored values), with
 * v_mfma_f64_16x16x4_f64.  w: a DEVICE n-vector of the handle's dtype
 * (krcn_weights' output).  The arithmetic is fp64 whatever the handle's dtype
 * and the image's stored width are (stored floats are widened, which is exact):
 * an fp64 handle under KRCN_VALUES_F32 computes with double(float(X)).
 * One workgroup computes one 64 x 64 tile (ta, tb), tb >= ta, of the upper
 * triangle over 32-entry slabs of the summed index r; tiles below one per CU are
 * split along r (krcn_gram_geometry; krcn_csr_set_gram_split forces the split).
 * Sum order of an entry: each w_r x_rb is rounded to fp64 once (the reference's
 * A.T * weights), then the terms x_ra (w_r x_rb) are accumulated by fused
 * multiply-adds, r ascending inside a split; the split sums are added in split
 * order by a second kernel; then s / n_global with a true division, plus l2 on
 * the diagonal, as krcn_hvp's expression.  No atomics: the bits depend on the
 * shape and the split count alone, and two calls return the same bytes.
 * Symmetry: H[a][b] and H[b][a] are written from the same sum, so H is exactly
 * symmetric; every entry of the d x d output is written exactly once, whatever
 * it held before.  w is never read at or past n.
 * n == 0 or nnz == 0: H = l2 I without reading the image.  d == 0: KRCN_OK,
 * nothing launched.  KRCN_ERR_INVALID before any HIP call: a null w, H or
 * handle.  Sharded handles get KRCN_ERR_UNSUPPORTED, and so does a handle whose
 * pass-2 plan is not KRCN_PLAN_DENSE (call krcn_csr_set_pass_format(h, 2,
 * KRCN_FORMAT_DENSE); pass 1 may have any format).  Builds pass plans on first
 * use, before any plan pointer is read.
 * Allocation: with a split above 1 the raw tiles of the splits (tiles x split x
 * 32 KiB) live in one buffer of the handle's owner table, counted by
 * krcn_csr_owned_bytes, allocated by the first call that needs it and grown
 * (freed and reallocated) only when a later call needs more; split 1 allocates
 * nothing.
 * Replaces hessian, loss.py:249-255. */
krcn_status krcn_hessian_gram(krcn_csr* h, const void* w, double l2, double* H, void* stream);
/* Split of krcn_hessian_gram along the summed index: 0 the rule (auto), else
 * 1..256 workgroups per tile, taken as it is (tests force small shapes across
 * splits; a split beyond the slab count leaves some workgroups a zero sum).
 * Builds nothing.  KRCN_ERR_INVALID outside 0..256. */
krcn_status krcn_csr_set_gram_split(krcn_csr* h, int split);
/* The cut of krcn_hessian_gram's work for a d-column, n-row matrix under a
 * split (0: the rule).  Host arithmetic only: needs no device.  out_host (8
 * entries) = {tile edge T, slab entries KS, tiles per side ceil(d / T),
 * upper-triangle tiles, slabs ceil(n / KS), split, grid (tiles x split),
 * workspace bytes of the split partials (0 at split 1)}.  The rule: split 1 when
 * the tiles number at least one per CU (256), else the smallest split that
 * reaches that, while every split keeps 8 slabs and the partials stay within
 * 256 MiB.  KRCN_ERR_INVALID: d outside [0, 2^20], n outside [0, 2^31), split
 * outside 0..256, a null out_host. */
krcn_status krcn_gram_geometry(int64_t d, int64_t n, int split, int64_t* out_host);

/* ---- the batched Krylov-CRN step: k problems over one X per call ---------- */
/* The batch forms of krcn_gradient, the loss value, krcn_cubic_tridiag and
 * krcn_crn_step over the (L, k) blocks of the block products (element (i, c)
 * at i * k + c, 1 <= k <= KRCN_BLOCK_MAX), both dtypes, scalars in double.
 * Unsharded handles only (KRCN_ERR_UNSUPPORTED otherwise).  Argument errors are
 * KRCN_ERR_INVALID before any HIP call, and the scalar ranges (k, m, b_cols,
 * max_trials, ls_beta, solver_it_max, it_max) are checked before the handle is
 * looked at.  Per-column reductions are two-stage in krcn_lanczos_block's fixed
 * order (no atomics): a column's bytes depend on k's lane group (the next
 * power of two >= k) and not on what the other columns hold.  The calls build
 * no pass plans.  Workspace: a (d, k) and an (n, k) block and 3 k 2044 doubles
 * of subproblem vectors, grown only when k grows, and fixed blocks for the
 * state, the partials (262,144 bytes) and a pinned host record block; all in the
 * handle's owner table, counted by krcn_csr_owned_bytes, freed by
 * krcn_csr_destroy, apart from u / tn / W / td, krcn_crn_step's workspace and
 * krcn_lanczos's results block.  A second call with the same (k, m) allocates
 * nothing. */
/* G[:, c] = X^T (expit(AX[:, c]) - b_c) / n + l2_c X[:, c].  b_cols = 1: one
 * label n-vector for every column; b_cols = k: an (n, k) block of 0/1 labels
 * (one-vs-rest).  l2_host: k HOST doubles (NULL: all zero); a column with
 * l2_c == 0 never reads X, which may be NULL when every l2_c is zero.
 * Replaces k calls of gradient, loss.py:223-232. */
krcn_status krcn_gradient_block(krcn_csr* h, int k, const void* AX, const void* b, int b_cols,
                                const void* X, const double* l2_host, void* G, void* stream);
/* SYNCHRONOUS.  values_host[c] = mean_i((1 - b_c) a - logsig(a)) + l2_c / 2 ||X[:, c]||^2
 * over a = AX[:, c].  Replaces k calls of value, loss.py:215-220. */
krcn_status krcn_value_block(krcn_csr* h, int k, const void* AX, const void* b, int b_cols, const void* X,
                             const double* l2_host, double* values_host, void* stream);
/* SYNCHRONOUS.  k subproblems of krcn_cubic_tridiag in one launch, one
 * workgroup per column: column c solves over its first m_eff_host[c] <= m
 * entries (row c of alphas_host / s_host at c * m, of betas_host at
 * c * max(m - 1, 1)) with gnorm_host[c], M_host[c] and r0_host[c]; per column
 * s (zero past m_eff_c, zero when the solve failed) and the solver fields of
 * info_host[c] are bitwise what krcn_cubic_tridiag returns for that column's
 * inputs.  Replaces k calls of cubic_solver_root, cubic.py:40-75. */
krcn_status krcn_cubic_tridiag_block(krcn_csr* h, int k, int m, const int* m_eff_host,
                                     const double* alphas_host, const double* betas_host,
                                     const double* gnorm_host, const double* M_host, const double* r0_host,
                                     double eps, int it_max, double* s_host, krcn_crn_info* info_host,
                                     void* stream);
/* SYNCHRONOUS.  One Krylov-CRN step of k problems over one X.  Column c is what
 * krcn_crn_step(h, X[:, c], b_c, AX[:, c], values_host[c], m, 0, tol, l2_c,
 * reg_coef_host[c], ls_beta, r0_host[c], ..) defines: the same line search
 * (M = reg_coef_c * ls_beta, divided by ls_beta per rejected trial, at most
 * max_trials of them), the same truncation of the subproblem to the column's
 * m_eff and the same krcn_crn_info fields, with `lanczos` as krcn_lanczos_block
 * fills it.  The recurrence is krcn_lanczos_block's, so values agree with the
 * single call at the rounding level, not bitwise.  X (d, k), AX (n, k) or NULL
 * (then X X is formed), V (m, d, k) as krcn_lanczos_block, X_new (d, k) and
 * AX_new (n, k) that alias no input; values_host, reg_coef_host, r0_host: k HOST
 * doubles; l2_host: k doubles or NULL; alphas_host[k * m] and
 * betas_host[k * max(m - 1, 1)] as krcn_lanczos_block returns them, or NULL.
 * active_host (k ints, NULL: all active): a column with active_host[c] == 0
 * starts as done: X_new[:, c] / AX_new[:, c] are byte copies of the inputs
 * (of X X[:, c] when AX is NULL), its info reports accepted = 0, trials = 0,
 * value_new = values_host[c], reg_coef = reg_coef_host[c], dx_norm = 0, and
 * whatever the recurrence computes in that column reaches no other column.
 * A column whose solve fails (solver_status 1 or 2) ends its own chain only;
 * its X_new / AX_new column is unspecified and its dx_norm 0.  The decisions
 * are taken per column on the device; a column that has ended keeps the
 * iterate it accepted (the last trial's at the cap) while the others go on.
 * The host enqueues trials 0 and 1, then batches of four, and synchronises
 * once per batch.  No reorthogonalisation; no graph replay or placement search
 * inside the call.
 * Replaces k calls of Cubic_Krylov_LS.step, cubic.py:265-309
 * (cubic_newton.py:67-73 runs two problems over one matrix). */
krcn_status krcn_crn_step_block(krcn_csr* h, int k, const void* X, const void* b, int b_cols, const void* AX,
                                const double* values_host, const int* active_host, int m, double tol,
                                const double* l2_host, const double* reg_coef_host, double ls_beta,
                                const double* r0_host, double solver_eps, int solver_it_max, int max_trials,
                                void* V, void* X_new, void* AX_new, double* alphas_host, double* betas_host,
                                krcn_crn_info* info_host, void* stream);

/* ---- dense vector helpers (host glue of optimizer.py / utils.py) -------- */
/* Vector spaces of a handle: n-vectors (one entry per sample row) and
 * d-vectors (one entry per feature).  In a sharded handle the helper reduces
 * over all ranks when that space is sharded (ROWS: n, COLS: d). */
enum { KRCN_SPACE_N = 0, KRCN_SPACE_D = 1 };
/* SYNCHRONOUS.  *out_host = sum_i a_i b_i, deterministic tree order
 * (np.dot, cubic.py:94,109). */
krcn_status krcn_dot(krcn_csr* h, int space, const void* a, const void* b,
                     double* out_host, void* stream);
/* SYNCHRONOUS.  *out_host = ||a - b||_2 (b may be NULL for ||a||_2).
 * Replaces loss.norm(x - x_old) of optimizer.py:110 and np.linalg.norm. */
krcn_status krcn_diff_norm(krcn_csr* h, int space, const void* a, const void* b,
                           double* out_host, void* stream);

/* ---- handle-free vector context ------------------------------------------ */
/* Reduction scratch + pinned staging on one device, for vectors of any length
 * and either dtype (no matrix handle needed). */
krcn_status krcn_vctx_create(int device, krcn_vctx** out);
krcn_status krcn_vctx_destroy(krcn_vctx* c);
/* SYNCHRONOUS.  One Lanczos step over an external operator, y = A(v) supplied
 * by the caller: w = y - beta v_pre (w = y when v_pre is NULL), alpha = v.w,
 * z = w - alpha v, beta' = ||z||; z receives the unnormalised next vector,
 * alpha_beta_host = {alpha, beta'}.  Replaces cubic.py:93-97 for Lanczos(A, v, m)
 * with a callable A the fused krcn_lanczos cannot run. */
krcn_status krcn_lz_ext_step(krcn_vctx* c, int dtype, int64_t n, const void* y,
                             const void* v, const void* v_pre, double beta,
                             void* z, double* alpha_beta_host, void* stream);
/* SYNCHRONOUS.  *out_host = a.b (fixed-order tree; np.dot, cubic.py:109). */
krcn_status krcn_vec_dot(krcn_vctx* c, int dtype, int64_t n, const void* a,
                         const void* b, double* out_host, void* stream);
/* out = a / div (the reference's v = w / beta, cubic.py:85,102). */
krcn_status krcn_vec_div(krcn_vctx* c, int dtype, int64_t n, const void* a,
                         double div, void* out, void* stream);
/* out = y + alpha x (x + s of Cubic_LS.step, cubic.py:209; out may alias y). */
krcn_status krcn_vec_axpy(krcn_vctx* c, int dtype, int64_t n, double alpha,
                          const void* x, const void* y, void* out, void* stream);

/* ---- multi-GPU (RCCL over xGMI; one process per GPU) -------------------- */
/* 128-byte RCCL unique id, produced on rank 0 and broadcast by the caller. */
krcn_status krcn_comm_unique_id(void* uid128_host);
krcn_status krcn_comm_create(int nranks, int rank, const void* uid128_host,
                             int device, krcn_comm** out);
krcn_status krcn_comm_destroy(krcn_comm* c);
/* nranks VIRTUAL ranks on one device (tests and rehearsals of a sharded run
 * without nranks GPUs; RCCL refuses two ranks on one device): out[0..nranks)
 * receive one communicator per rank, each to be attached to that rank's
 * handle and driven by its own host thread on its own stream.  Every
 * all-reduce drains the caller's stream and waits for the other ranks; the
 * last to arrive sums the ranks' buffers in rank order on the device.  A rank
 * missing for 90 s breaks the group (every waiting call fails, and the error
 * string lists how many all-reduces each rank has entered, the count of its
 * last one and which ranks were waiting).  Destroy
 * each communicator; the group goes with the last one.  Not in the
 * reference: it has no parallelism ("P virtual shards"). */
krcn_status krcn_comm_create_virtual(int nranks, int device, krcn_comm** out);
/* In-place sum all-reduce of n values of dtype (plumbing for tests/bench). */
krcn_status krcn_comm_allreduce(krcn_comm* c, int dtype, void* buf, int64_t n,
                                void* stream);

/* ---- LIBSVM / svmlight text (host) ---------------------------------------- */
/* Parse svmlight text (text[0..len), not NUL-terminated) on `threads` host
 * threads (<= 0: all cores) into a parsed set: info4_host = {rows, nnz, the
 * largest index, the smallest index (-1 without nonzeros)}.  The grammar and
 * the errors are sklearn.datasets.load_svmlight_file's (comments, blank
 * lines, a leading qid:, correctly rounded decimal floats; a negative index or
 * indices not strictly increasing in a row are KRCN_ERR_INVALID with sklearn's
 * message).  Replaces the reference's load_svmlight_file(path)
 * (cubic_newton.py:52-53). */
typedef struct krcn_svm krcn_svm;
krcn_status krcn_svm_parse(const char* text, int64_t len, int threads, krcn_svm** out,
                           int64_t* info4_host);
/* Copy a parsed set into the caller's HOST arrays: indptr (rows + 1) and
 * indices (nnz) as int32 with every index lowered by `shift` (1 for one-based
 * files), data (nnz) and labels (rows) as float64. */
krcn_status krcn_svm_export(const krcn_svm* p, int64_t shift, int32_t* indptr, int32_t* indices,
                            double* data, double* labels);
krcn_status krcn_svm_destroy(krcn_svm* p);

/* ---- profiling ----------------------------------------------------------- */
/* When enabled, krcn_hvp / krcn_lanczos record HIP events around every
 * pass-1 (X v) and pass-2 (X^T u) launch on the call's stream and accumulate
 * their durations; krcn_prof_read returns {calls, ms} for pass 1 (with its
 * slice combine), pass 2 and the whole HVP (pass 1 start to pass 2 end), then
 * the ms of pass 1's main launch alone and of its slice combine, and resets
 * the counters: out8_host = {c, p1, c, p2, c, hvp, p1_kernel, p1_combine}. */
krcn_status krcn_prof_enable(krcn_csr* h, int on);
krcn_status krcn_prof_read(krcn_csr* h, double* out8_host);

#ifdef __cplusplus
}
#endif
#endif /* KRCN_H */
