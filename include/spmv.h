/*
 * spmv.h — C-ABI of the MI355X (gfx950) fp64 SpMV kernels: y = A·x.
 *
 * This is the drop-in boundary that replaces the reference's
 * "clSetKernelArg ×k → clEnqueueNDRangeKernel" call sites
 * (reference coo.c:163-194, csr.c:170-201, ell.c:242-273,
 *  sigma_c.c:280-311, cmrs.c:195-232) and the five OpenCL kernels
 * (reference kernels/{Coo,Csr,Ell,Sigma_C,Cmrs}.cl).  Everything here is
 * plain C: device pointers, sizes, a hipStream_t passed as `void *`.
 *
 * A caller uses it in two steps:
 *   1. spmv_plan_<fmt>(dims, the format's device arrays, options) looks at
 *      the matrix once and builds everything the measured-best kernel path
 *      for it needs (x windows, head copies, tile plans, workspace);
 *   2. spmv_plan_run(plan, x, y, stream) launches that path.
 * ./bin/{coo,csr,ell,sigma_c,cmrs} (drivers/driver.c) and the Python
 * binding (spmv_amd.to_device) both go through the plans, so the programs
 * run the kernels bench.py measures.  The five spmv_<fmt>_run entry points
 * below are the reference kernels' one-call equivalents (no build step,
 * global x gathers); the individual kernel variants the plans choose
 * between, the compressed formats and the device builders are in
 * spmv_ext.h.
 *
 * Conventions (all entry points):
 *   - Every array argument is a DEVICE pointer on `d.device`, owned by the
 *     caller; a plan keeps pointers to them (they must outlive the plan)
 *     and owns only what it builds.  The library's own scratch
 *     (spmv_flush_cache's buffer) is freed by spmv_release().
 *   - y is FULLY overwritten (rows without entries get 0.0).  The reference
 *     COO relied on fresh device memory being zero (reference coo.c:120);
 *     here no pre-zeroing is required.
 *   - Runs are asynchronous on the given stream (NULL = the device's
 *     default stream).  No hidden device-wide synchronisation and no
 *     allocation inside a run, so a caller may capture runs into a
 *     hipGraph.  Plan creation synchronises d.stream (build time).
 *   - Return value: 0 on success, otherwise a code of spmv_rc.h with the
 *     reference's numeric meaning (reference inc/enums.h:4-11):
 *     1 device error, 2 launch/copy error, 4 bad arguments.
 *     spmv_last_error() returns a human readable message for the last
 *     failure on the calling thread.
 *   - Indices are 0-based.  Column indices are int32 (as the reference);
 *     offsets into the value arrays are int64 (the reference's int32
 *     offsets overflow past 2^31 entries).
 */
#ifndef SPMV_H
#define SPMV_H

#include <stddef.h>
#include <stdint.h>

#include "spmv_rc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spmv_dims {
    int64_t n_rows; /* N: rows of A, length of y            */
    int64_t n_cols; /* M: columns of A, length of x         */
    int64_t nnz;    /* Z: stored entries that are multiplied */
    int device;     /* HIP device ordinal holding the arrays */
    void *stream;   /* hipStream_t (NULL: default stream)    */
} spmv_dims;

/* --------------------------------------------------------------- plans ---
 * One plan per matrix and format.  The arrays are the format's device
 * arrays as the host builders of spmv_host.h (or the device builders of
 * spmv_ext.h) produce them; the plan keeps pointers to them.
 *
 * Options (spmv_plan_opts_init sets the library defaults; every "-1" means
 * "the library's rule for this matrix"):
 *   lanes      CSR lanes per row (2..64, a power of two); 0 = rule
 *   variant    CSR: -1 rule (4 when the longest row exceeds 4,096 entries
 *              and 64x the mean, else the x-window kernel), 1 direct,
 *              2 staged, 3 staged persistent (x windows when xwin), 4
 *              entry-balanced tiles; CMRS: -1 rule, 1 strip runs, 2
 *              entry-balanced tiles
 *   xwin       x windows in LDS: -1 default (CSR, ELL, SELL, CMRS on; COO
 *              off), 0 off, 1 on
 *   xwin_rows  CSR rows per x window; 0 = 128
 *   head       SELL small matrices: the head copy of every wave's first
 *              slot groups; -1 default (on), 0 off
 *   index16    SELL: 1 = SELL16, 16-bit column offsets from each
 *              workgroup's window base (plan-owned copy; C = 64, refused
 *              when a window spans more than 65,536 columns).  CSR
 *              ignores it: an x-window CSR plan builds its 16-bit
 *              window-relative column copy by the library's rule
 *              (SPMV_OPT_CSR_COL16, spmv_ext.h) wherever every window with
 *              entries fits the LDS cap, and spmv_plan_info.index16 says so
 *   coo_pass   COO: -1 the single pass wherever every row ends within 80
 *              entries past its tile, else the carry pass; 0 carry pass;
 *              1 single pass or SPMV_OTHER_ERROR
 *   split      SELL wide slices: -1 rule (spmv_sell_split_auto), 0 off,
 *              T > 0 (a multiple of ki) slot columns per slice in the main
 *              kernel, the rest in chunks
 *   bigplan    tiled CSR: list the rows of tiles owning > 1,024 rows
 *              (runs of empty rows); -1 default (on), 0 off
 *   H          hot-column table for power-law columns (COO, tiled CSR,
 *              SELL, tiled CMRS): the plan renumbers the H most frequent
 *              columns into a compact x table gathered at the start of
 *              every run (spmv_hot_columns, spmv_host.h; plan-owned column
 *              copy); -1 the rule (2^19 columns when n_cols > 2^21 and they
 *              hold half the entries), 0 none (e.g. columns already
 *              relabelled by degree, spmv_column_relabel), > 0 that many  */
enum spmv_fmt {
    SPMV_FMT_COO = 0,
    SPMV_FMT_CSR = 1,
    SPMV_FMT_ELL = 2,
    SPMV_FMT_SELL = 3,
    SPMV_FMT_CMRS = 4,
    SPMV_FMT_BSR = 5 /* block CSR, not one of the reference's five: spmv_plan_bsr */
};

typedef struct spmv_plan_opts {
    int32_t lanes;
    int32_t variant;
    int32_t xwin;
    int32_t xwin_rows;
    int32_t head;
    int32_t index16;
    int32_t coo_pass;
    int32_t split;
    int32_t bigplan;
    int32_t reserved;
    int64_t H;
} spmv_plan_opts;

typedef struct spmv_plan spmv_plan;

/* What a plan runs (spmv_plan_get_info): kernel = the dominant kernel's
 * name as rocprofv3 reports it (without the namespace and template
 * arguments), desc = one line naming the path and its parameters.       */
typedef struct spmv_plan_info {
    int32_t format;      /* enum spmv_fmt */
    int32_t path;        /* internal path id (stable within a build) */
    int32_t lanes;       /* CSR lanes per row */
    int32_t variant;     /* CSR 1-4; CMRS 0 strip runs, 1 tiles */
    int32_t ki;          /* ELL / SELL k-interleave */
    int32_t xcap;        /* LDS x-window entries (0: no window fits / none) */
    int32_t xwin;        /* x windows built */
    int32_t head;        /* SELL head copy built */
    int32_t single_pass; /* COO without the carry kernel */
    int32_t index16;     /* SELL16; CSR: the plan streams its own 16-bit window column offsets */
    int32_t split_T;     /* SELL split width (0: none) */
    int32_t reserved;
    int64_t n_chunks;    /* SELL split chunks */
    int64_t big_tiles;   /* tiled CSR tiles with a listed row plan */
    int64_t head_bytes;
    int64_t ws_bytes;
    int64_t owned_bytes; /* device bytes the plan allocated (index16 copies included: 2 per entry) */
    int64_t H;
    char kernel[64];
    char desc[320];
} spmv_plan_info;

void spmv_plan_opts_init(spmv_plan_opts *o);
/* Replaces the COO launch (reference coo.c:47-48,68-73,163-168,194;
 * kernels/Coo.cl:24).  Entries sorted by row (any order inside a row:
 * spmv_coo_sort_by_row, spmv_host.h).  o = NULL: defaults.                */
int spmv_plan_coo(spmv_dims d, const int32_t *row, const int32_t *col, const double *val,
                  const spmv_plan_opts *o, spmv_plan **out);
/* Replaces the CSR launch (reference csr.c:47-48,170-175,201;
 * kernels/Csr.cl:1).  row_ptr[N+1] int64, col/val[Z].                     */
int spmv_plan_csr(spmv_dims d, const int64_t *row_ptr, const int32_t *col, const double *val,
                  const spmv_plan_opts *o, spmv_plan **out);
/* Replaces the ELL launch (reference ell.c:47-48,242-248,273;
 * kernels/Ell.cl:1).  Layout of spmv_ell_run below.                       */
int spmv_plan_ell(spmv_dims d, int32_t K, int64_t ld, int32_t ki, const int32_t *col, const double *val,
                  const spmv_plan_opts *o, spmv_plan **out);
/* Replaces the SELL-C-sigma launch (reference sigma_c.c:50-51,71-72,
 * 280-285,311; kernels/Sigma_C.cl:1).  Layout of spmv_sell_run below.     */
int spmv_plan_sell(spmv_dims d, int32_t C, int32_t sigma, int32_t ki, int64_t n_slices, const int64_t *slice_ptr,
                   const int32_t *perm, const int32_t *col, const double *val, const spmv_plan_opts *o,
                   spmv_plan **out);
/* Replaces the CMRS launch (reference cmrs.c:51-52,195-205,232;
 * kernels/Cmrs.cl:1).  Layout of spmv_cmrs_run below.                     */
int spmv_plan_cmrs(spmv_dims d, int32_t h, int64_t n_strips, const int64_t *strip_ptr, const uint8_t *row_in_strip,
                   const int32_t *col, const double *val, const spmv_plan_opts *o, spmv_plan **out);
/* Block CSR (BSR) with b x b blocks, b in {2, 3, 4}: one int32 column per
 * block, 8 + 4/b^2 bytes per stored value instead of CSR's 12, for matrices
 * with b unknowns per node (3-dof FEM).  The arrays are those of
 * spmv_bsr_fill (spmv_host.h, which states the layout and THE FILL-IN RULE: a
 * slot without an entry multiplies 0.0 by an x value of its block column):
 * brow_ptr[n_brows + 1] int64, bcol[n_blocks] int32 ascending inside a block
 * row, bval[n_blocks * b * b] row-major inside a block.  d.n_rows and d.n_cols
 * are the scalar sizes, d.nnz the stored values n_blocks * b * b ("the stored
 * entries that are multiplied"); n_brows = ceil(n_rows / b), the last block
 * row and block column may be partial.
 *   - Only opts.lanes is honoured: the lanes per block row, a power of two
 *     2..64; 0 = about one lane per 2 blocks of the mean block row, 8 at
 *     the least (spmv_bsr_auto_lanes).  The other options are ignored.
 *   - The plan builds nothing (owned_bytes = 0).  spmv_plan_run's contract
 *     holds word for word: a partial last block column is guarded, no 16-byte
 *     load of x or store of y, no atomics, the same bits on every run and
 *     under every spmv_set_option switch.  Info: format 5, kernel
 *     "bsr_kernel", desc names b, the lanes and the block count.
 *   - Refused with SPMV_OTHER_ERROR, a message and no plan: b not in
 *     {2, 3, 4}, n_brows != ceil(n_rows / b), d.nnz not a multiple of b*b,
 *     n_cols > INT32_MAX - 8, lanes not 0 or a power of two in 2..64, a NULL
 *     array with blocks present.
 *   - No multi-vector, transposed or symmetric run: spmv_plan_run_multi
 *     refuses, the three *_supported calls answer 0 and the three prepare
 *     calls refuse as for every non-CSR plan.
 * Which to call (the byte model, profiles/bsr/README.md): BSR stores fewer
 * bytes than CSR when fill (stored values / entries) < 12 / (8 + 4/b^2), i.e.
 * 1.33 / 1.42 / 1.45 at b = 2 / 3 / 4; on the cant-like matrix at b = 3 (fill
 * 1.079) it is 0.755 of CSR's bytes, on a truly blocked matrix 0.70.  On an
 * MI355X (cold, b = 3, tools/bsr_bench.py, profiles/bsr/README.md) those
 * bytes turn into time only in part.  One cant-like matrix: SLOWER than the
 * default CSR plan, 12.0 against 10.4 us (1.16x, the same in a second run).
 * The 32-copy cant-like batch: a tie, 0.2104 against 0.2190 ms in one run
 * (0.96x), 0.2301 against 0.2159 on another box (1.07x).  A fill-1.0 matrix
 * of 49,152 rows: FASTER, 4.7 against 6.9 us (0.68x, one run).  Call
 * spmv_plan_bsr for a truly blocked matrix or where the memory matters,
 * spmv_plan_csr for one matrix with fill-in.                              */
int spmv_bsr_auto_lanes(int64_t n_brows, int64_t n_blocks);
int spmv_plan_bsr(spmv_dims d, int32_t b, int64_t n_brows, const int64_t *brow_ptr, const int32_t *bcol,
                  const double *bval, const spmv_plan_opts *o, spmv_plan **out);
/* y = A x on `stream` (NULL = the default stream; the plan's d.stream is
 * used for building only).  x[n_cols], y[n_rows], device pointers.
 *   - y[0 .. n_rows) is FULLY overwritten (rows without entries get 0.0);
 *     NO byte of y outside it is written.
 *   - x and y need 8-byte alignment only: every load of x and store of y is
 *     8 bytes wide (the 16-byte loads are of the matrix arrays and of
 *     plan-owned buffers).
 *   - NO value outside x[0 .. n_cols) enters a result (padding slots
 *     included).
 *   - x and y must not overlap; runs of one plan must be serialised.
 * tests/test_exact_gpu.py (test_forward_memory_contract) holds every format
 * to this with x and y one element into larger buffers.                   */
int spmv_plan_run(const spmv_plan *p, const double *x, double *y, void *stream);
/* Y = A·X for k vectors stored row-major ("vector index fastest"):
 * X[c*ldx + j], c < n_cols, j < k;  Y[i*ldy + j], i < n_rows, j < k.
 * ldx >= k, ldy >= k (leading dimensions in elements), k >= 1.
 *
 * The conventions above hold: device pointers, asynchronous on `stream`,
 * no allocation and no synchronisation inside the call (it can be captured
 * into a graph), codes of spmv_rc.h, a message in spmv_last_error().
 *   - Y[i*ldy + j], j < k, is fully overwritten (rows without entries get
 *     0.0); NO element Y[i*ldy + j] with j >= k is written.
 *   - NO byte outside X[c*ldx .. c*ldx + k) is read for any c: nothing past
 *     the end of the last row when ldx == k, and no 16-byte load straddles
 *     column k-1.
 *   - X and Y need 8-byte alignment only and any ldx, ldy >= k (odd ones
 *     too).  16-byte loads and stores of X / Y rows are used only where
 *     the call has proven them aligned (base address and leading dimension
 *     both 16-byte compatible); otherwise the 8-byte kernels run.
 *   - X and Y must not overlap; runs of one plan must be serialised, as for
 *     spmv_plan_run.
 *   - The matrix is read once per block of up to 8 vectors, ceil(k/8)
 *     times.  The kernels exist for 1, 2, 4 and 8 vectors; a block of r
 *     remaining vectors uses the smallest width >= r, its unused
 *     accumulator columns load column k-1 again and are never stored.
 *   - The bits of output column j depend only on the matrix (and the
 *     plan's format and geometry) and on input column j: not on k, on j's
 *     place in its block, on ldx / ldy or on the 8- or 16-byte kernels.
 *     Column j need not equal spmv_plan_run's bits (that path sums in its
 *     own order); it meets the same 1e-6 per-row criterion.
 *   - SPMV_OTHER_ERROR with a message, before any device work: NULL plan,
 *     k < 1, ldx < k or ldy < k, NULL X with entries present, NULL Y with
 *     rows present, a plan without a multi-vector kernel.
 * Plans that run: CSR (every path), ELL (both paths), SELL (every path but
 * SELL16, any C, ki 1 or 2).  The run reads the caller's arrays (never the
 * plan's hot-renumbered column copy) and gathers X from global memory.
 * Refused: COO and CMRS (no multi-vector kernel), SELL16 (the plan does not
 * require the int32 columns to outlive its creation).                      */
int spmv_plan_run_multi(const spmv_plan *p, int32_t k, const double *X, int64_t ldx,
                        double *Y, int64_t ldy, void *stream);
/* 1 when spmv_plan_run_multi can run this plan, else 0 (also for NULL). */
int spmv_plan_multi_supported(const spmv_plan *p);
/* The balanced mode of spmv_plan_run_multi for CSR matrices with long rows
 * (opt-in, built once like spmv_plan_prepare_transpose).  Without it every
 * row is summed by one group of `lanes` entry lanes, so a hub row of 1e4-1e5
 * entries is walked by a handful of lanes while the rest of the chip waits.
 * SPMV_M_BALANCED splits the rows in two bins:
 *   - rows of at most long_len entries: csr_multi_kernel as before, in the
 *     same order and with the same bits as on a plan that was not prepared;
 *   - longer rows: cut into segments of at most seg_len consecutive entries
 *     (spmv_csr_multi_plan, spmv_host.h), each summed by 16 entry lanes
 *     (csr_multi_long_kernel); a row of several segments gets its partial
 *     sums added in segment order by csr_multi_finish_kernel.
 * No atomics and a fixed order: results stay bitwise reproducible, and the
 * bit rule of spmv_plan_run_multi holds (column j's bits do not depend on k,
 * j's place, ldx / ldy or the access path); the bits of a long row differ
 * from the unprepared run's (another summation order, the same 1e-6
 * criterion and fp64 bound).  A plan without long rows launches nothing
 * extra.
 * Options (spmv_multi_opts_init: both -1 = the library's rule):
 *   long_len   rows longer than this are long; rule 32 x the plan's lanes
 *              per row; >= 0
 *   seg_len    entries per segment; rule 512; >= 1
 * spmv_plan_prepare_multi (build time) may allocate and synchronises the
 * plan's d.stream: it copies row_ptr to the host (the matrix may exist only
 * in device memory), runs the host planner, uploads its tables and
 * allocates the partial workspace (slots x 8 doubles).  The same mode and
 * options again is a no-op; other options rebuild; SPMV_M_NONE frees
 * everything and restores the unprepared run; spmv_plan_destroy frees
 * whatever was built.  CSR plans only (every path, with or without a
 * hot-column table: the caller's col is read, never the hot copy).
 * SPMV_OTHER_ERROR with a message, the plan left as it was: NULL plan, unknown
 * mode, long_len < -1, seg_len < -1 or 0, a plan that is not CSR.
 * With SPMV_T_COPY the mode and options extend to the inner plan over A^T
 * (rule values resolved against the inner plan's own lanes), whichever of
 * spmv_plan_prepare_multi / spmv_plan_prepare_transpose comes first, and
 * end with either; scatter mode is not affected.  With SPMV_S_EXPAND they
 * extend in the same way to the inner plan over A = S + S^T - diag S
 * (spmv_plan_prepare_symmetric, spmv_plan_run_sym_multi), whose balanced state
 * is reported in spmv_symmetric_multi_info; fused mode is not affected.
 * spmv_plan_run_multi itself is unchanged: no allocation, no synchronisation,
 * capturable.  The partial workspace belongs to the plan, so two balanced
 * runs of ONE plan must not overlap in time, on different streams either
 * (the tiled forward run's rule).  The new bytes are reported here only:
 * spmv_plan_get_info, spmv_transpose_info and spmv_transpose_multi_info
 * answer as before.
 * Which to call (MI355X, profiles/spmm/README.md): on the 100,000-row /
 * 1,000,000-entry power-law R-MAT a balanced run took 0.025 / 0.031 / 0.036 ms
 * at k = 2 / 4 / 8 against 0.46 / 0.49 / 0.49 ms unprepared (14 to 18 times
 * faster) and against 0.029 / 0.057 / 0.114 ms for k spmv_plan_run calls
 * (level to 1.15 / 1.8 / 3.2 times faster).  On matrices without long rows
 * (cant-like) nothing extra is launched and the two runs are within 5 % of
 * each other.  The rule was picked by a sweep on that R-MAT (lanes = 2):
 * long_len of 64 and 128 x lanes is 1.5 times slower, 16 x lanes a few
 * microseconds faster there but would make ordinary 64-entry rows long at
 * lanes = 4; seg_len 512 beats 256, 1,024 and 2,048.                      */
enum spmv_multi_mode { SPMV_M_NONE = 0, SPMV_M_BALANCED = 1 };
typedef struct spmv_multi_opts {
    int32_t long_len;
    int32_t seg_len;
} spmv_multi_opts;
typedef struct spmv_multi_info {
    int32_t mode;          /* enum spmv_multi_mode */
    int32_t long_len;      /* resolved thresholds (0 when not prepared) */
    int32_t seg_len;
    int32_t reserved;
    int64_t long_rows;     /* rows of more than long_len entries */
    int64_t segments;
    int64_t slots;         /* partial slots (segments of rows with several) */
    int64_t long_entries;  /* entries of the long rows */
    int64_t owned_bytes;   /* device bytes of the tables and the workspace */
    int64_t t_long_rows;   /* copy mode's inner plan over A^T; 0 without one */
    int64_t t_segments;
    int64_t t_owned_bytes;
    char kernel[64];       /* the long rows' kernel ("" when not prepared) */
} spmv_multi_info;
void spmv_multi_opts_init(spmv_multi_opts *o);
int spmv_plan_prepare_multi(spmv_plan *p, int mode, const spmv_multi_opts *o /* NULL: the rules */);
int spmv_plan_get_multi_info(const spmv_plan *p, spmv_multi_info *info);
/* The transposed product y = A^T x on the same plan: A is n_rows x n_cols,
 * x[n_rows], y[n_cols].  CSR plans only (every path); two modes, built by
 * spmv_plan_prepare_transpose:
 *   SPMV_T_SCATTER  no second copy of the matrix.  One workgroup per block
 *       of 128 rows streams the block's entries once; a block whose columns
 *       span at most `cap` (2,048) entries sums val * x[row] in an LDS
 *       accumulator and adds it to y with one fp64 atomic per touched
 *       column (consecutive lanes, consecutive columns), a wider block adds
 *       every product straight into y with a global fp64 atomic.  The plan
 *       owns 8 bytes per row block.  Results are NOT bitwise reproducible
 *       from run to run (the atomics arrive in any order); they meet the
 *       project's 1e-6 per-row criterion.  y must be ordinary device memory
 *       (hipMalloc, torch): hardware float atomics are not defined on
 *       fine-grained or host memory.
 *   SPMV_T_COPY     A^T built once on the device as CSR
 *       (spmv_dev_csr_transpose, spmv_ext.h; about 12 nnz + 8 (n_cols + 1)
 *       plan-owned bytes) and run by an inner forward CSR plan with default
 *       options, whose rules pick its kernel from A^T's own row lengths.
 *       Bitwise reproducible: the bits of a forward CSR plan with default
 *       options on the same three arrays (prepared by
 *       spmv_plan_prepare_multi as the outer plan is, if it is).
 * spmv_plan_prepare_transpose (build time) runs on the plan's d.stream and
 * synchronises it before returning, so runs may come on any stream.
 * Preparing the mode the plan already has is a no-op; preparing the other
 * mode frees the first mode's buffers; SPMV_T_NONE frees everything;
 * spmv_plan_destroy frees whatever was built.  SPMV_OTHER_ERROR with a
 * message: NULL plan, unknown mode, a plan that is not CSR.
 * spmv_plan_run_t follows the conventions above: asynchronous on `stream`,
 * no allocation and no synchronisation (it can be captured into a graph on
 * one stream), codes of spmv_rc.h.
 *   - y[0 .. n_cols) is FULLY overwritten (columns without entries get
 *     0.0); NO byte of y at or past n_cols is written.
 *   - x and y must not overlap; runs of one plan must be serialised, as for
 *     spmv_plan_run.
 *   - SPMV_OTHER_ERROR with a message, before any device work: NULL plan,
 *     a plan that was not prepared, NULL x with rows present, NULL y with
 *     columns present.
 * The transposed run reads the caller's row_ptr, col and val (never the
 * plan's hot-renumbered column copy).  In scatter mode an entry whose column
 * lies outside [0, n_cols) is dropped (the recorded column ranges leave it
 * out and every add is bounds-checked); copy mode refuses such a matrix at
 * build time with SPMV_OTHER_ERROR.  spmv_plan_get_info and its
 * owned_bytes do not change: the transposed path reports its own bytes in
 * spmv_transpose_info.                                                     */
enum spmv_transpose_mode { SPMV_T_NONE = 0, SPMV_T_SCATTER = 1, SPMV_T_COPY = 2 };
typedef struct spmv_transpose_info {
    int32_t mode;          /* enum spmv_transpose_mode */
    int32_t cap;           /* scatter: LDS accumulator entries per workgroup */
    int64_t blocks;        /* scatter: row blocks */
    int64_t lds_blocks;    /* scatter: row blocks whose column span fits cap */
    int64_t flush_entries; /* scatter: y entries added by window flushes per run (sum of those spans) */
    int64_t owned_bytes;   /* device bytes the transposed path allocated */
    char kernel[64];       /* dominant kernel, as spmv_plan_info.kernel */
} spmv_transpose_info;
/* 1: CSR plans (every path); 0 otherwise and for NULL */
int spmv_plan_transpose_supported(const spmv_plan *p);
int spmv_plan_prepare_transpose(spmv_plan *p, int mode);
int spmv_plan_get_transpose_info(const spmv_plan *p, spmv_transpose_info *info);
int spmv_plan_run_t(const spmv_plan *p, const double *x, double *y, void *stream);
/* Y = A^T·X for k vectors stored row-major, the layout of spmv_plan_run_multi
 * with the roles swapped: X[r*ldx + j], r < n_rows;  Y[c*ldy + j], c < n_cols;
 * j < k;  ldx >= k, ldy >= k (elements), k >= 1.  Needs
 * spmv_plan_prepare_transpose first and runs in whichever mode was prepared.
 *
 * The conventions above hold: device pointers, asynchronous on `stream`, no
 * allocation and no synchronisation inside the call (it can be captured into
 * a graph on one stream), codes of spmv_rc.h, a message in spmv_last_error().
 *   - Y[c*ldy + j], j < k, is fully overwritten (columns of A without
 *     entries get 0.0); NO element with j >= k and nothing at or past row
 *     n_cols is written.
 *   - NO byte outside X[r*ldx .. r*ldx + k) is read for any r.
 *   - X and Y need 8-byte alignment only and any ldx, ldy >= k: every load
 *     of X and every add to Y is 8 bytes wide.
 *   - X and Y must not overlap; runs of one plan must be serialised.
 *   - Reads the caller's row_ptr, col and val, never the plan's
 *     hot-renumbered column copy.
 *   - SPMV_OTHER_ERROR with a message, before any device work: NULL plan, a
 *     plan that was not prepared (every plan that is not CSR: it cannot be),
 *     k < 1, ldx < k or ldy < k, NULL X with rows present, NULL Y with
 *     columns present.
 * SPMV_T_COPY: spmv_plan_run_multi on the inner forward plan over A^T and
 *     nothing else, so its bit rule carries over: the bits of column j are
 *     those of spmv_plan_run_multi on a default forward CSR plan over
 *     spmv_csr_transpose's arrays, independent of k, of j's place in its
 *     block of 8 and of ldx / ldy.  An outer plan prepared with
 *     spmv_plan_prepare_multi runs the inner plan balanced too: the bits of
 *     that forward plan prepared with the same options.
 * SPMV_T_SCATTER: csr_t_multi_kernel<KV>, KV in {1, 2, 4, 8}.  The matrix is
 *     streamed once per block of up to 8 vectors (ceil(k/8) passes, pass b on
 *     X + 8b, Y + 8b); a block of r remaining vectors runs the smallest
 *     KV >= r and neither loads nor adds its unused columns.  Y is zeroed once
 *     before the first pass.  The geometry is spmv_plan_run_t's (one
 *     workgroup per 128 rows, the same recorded column ranges); the LDS
 *     accumulator holds span * KV sums, so a row block sums in LDS when its
 *     column span is at most cap_cols[w] = 8,192 / KV and adds every product
 *     straight into Y (k-wide pieces of 8 * KV bytes) otherwise.  Results are
 *     NOT bitwise reproducible from run to run (the atomics arrive in any
 *     order); Y must be ordinary device memory, as for spmv_plan_run_t.
 * Which to call (MI355X, cold, profiles/transpose/README.md): against k calls
 * of spmv_plan_run_t on the same plan, one call was 1.9 / 2.2-2.8 / 2.2-3.8
 * times faster at k = 2 / 4 / 8 in scatter mode on cant-like matrices, 1.2 /
 * 2.4 / 5.5 times faster in scatter mode on a power-law R-MAT (every product
 * a global atomic either way) and 1.2-1.4 / 1.9-2.1 / 2.3-3.0 times faster in
 * copy mode on cant-like matrices.  In COPY mode on the power-law R-MAT one
 * call on an unprepared plan was 5 to 20 times SLOWER than k calls (the hub
 * rows of A^T are walked by two lanes each): prepare the plan with
 * spmv_plan_prepare_multi(SPMV_M_BALANCED) there, after which one call took
 * 0.036 / 0.040 / 0.046 ms at k = 2 / 4 / 8, 13 to 16 times less than
 * unprepared and 0.84 / 1.5 / 2.6 times the speed of k spmv_plan_run_t calls
 * (at k = 2 the two calls are still the faster way).  One vector belongs to
 * spmv_plan_run_t (k == 1 with ldx == ldy == 1 is that very launch in scatter
 * mode; in copy mode spmv_plan_run_multi at k = 1 is slower than
 * spmv_plan_run).                                                           */
int spmv_plan_run_t_multi(const spmv_plan *p, int32_t k, const double *X, int64_t ldx,
                          double *Y, int64_t ldy, void *stream);
typedef struct spmv_transpose_multi_info {
    int32_t mode;          /* enum spmv_transpose_mode */
    int32_t reserved;
    int32_t cap_cols[4];   /* scatter: widest column span of a row block that is summed in LDS by the
                              kernel of width 1, 2, 4, 8; copy: 0 */
    int64_t lds_blocks[4]; /* scatter: row blocks within that span, per width */
    char kernel[64];       /* dominant kernel; copy: the inner plan's multi-vector kernel */
} spmv_transpose_multi_info;
int spmv_plan_get_transpose_multi_info(const spmv_plan *p, spmv_transpose_multi_info *info);
/* The symmetric product y = (S + S^T - diag S) x on a plan over the STORED
 * HALF S of a symmetric matrix (Matrix Market `symmetric` files list one
 * triangle: SuiteSparse cant.mtx lists 2,034,917 of its 4,007,383 entries).
 * S is square, n x n, of any pattern (lower, upper or mixed); every stored
 * off-diagonal entry (i, j, v) also stands for (j, i, v), diagonal entries
 * count once, duplicates and entries stored on both sides each count as
 * listed: A = the expansion spmv_coo_symmetrize (spmv_host.h) writes.
 * Skew-symmetric (mirror -v) and hermitian complex meanings are out of scope:
 * the reader's `symmetric` flag does not tell the banners apart.
 * CSR plans only (every path), x[n], y[n]; two modes, built by
 * spmv_plan_prepare_symmetric:
 *   SPMV_S_FUSED   one pass over the half storage (12 bytes per stored
 *       entry), no second copy.  One workgroup per block of 128 rows streams
 *       the block's entries once.  The plan records, per block, the union
 *       window {lo, hi} of the block's column range and its own rows: 8 bytes
 *       per block, owned_bytes == 8 * ceil(n / 128) exactly.  A union of at
 *       most `cap` (2,048) columns: x[lo..hi] and an accumulator of the same
 *       span live in LDS, entry (r, c, v) adds v x[c] to acc[r - lo] and,
 *       when c != r, v x[r] to acc[c - lo] (the row products of a wave's 64
 *       consecutive entries are summed per row across the wave and added
 *       once per run, measured faster); the accumulator is added to the
 *       zeroed y with one fp64 atomic per touched entry, consecutive lanes on
 *       consecutive columns.  A wider union: a 128-entry LDS accumulator for
 *       the rows' sums, x[c] gathered from global memory, every mirrored
 *       product added straight into y with a global fp64 atomic.  Every
 *       destination is bounds-checked (against the window or n).  A run is a
 *       memset of y plus one kernel.  Results are NOT bitwise reproducible
 *       from run to run (the atomics arrive in any order); y must be ordinary
 *       device memory (hipMalloc, torch), as for SPMV_T_SCATTER.
 *       flush_entries counts the y entries the flushes address per run: the
 *       window blocks' spans plus the rows of the wide blocks.
 *   SPMV_S_EXPAND  A built once on the device as CSR: the symmetrized COO of
 *       the plan's CSR entries in spmv_coo_symmetrize's order, then
 *       spmv_dev_csr_from_coo (spmv_ext.h), element for element
 *       spmv_csr_from_coo of spmv_coo_symmetrize of the CSR-ordered entries;
 *       run by an inner forward CSR plan with default options.  Bitwise
 *       reproducible: the bits of a default forward CSR plan over those
 *       arrays.  Owned bytes: 12 nnz_A + 8 (n + 1) plus the inner plan's own;
 *       the transient buffers are freed before prepare returns.
 * spmv_plan_prepare_symmetric (build time) runs on the plan's d.stream and
 * synchronises it before returning, so runs may come on any stream.
 * Preparing the mode the plan already has is a no-op; preparing the other
 * mode frees the first mode's buffers (after the new ones are built);
 * SPMV_S_NONE frees everything; spmv_plan_destroy frees whatever was built.
 * On failure the plan is left as it was.  SPMV_OTHER_ERROR with a message:
 * NULL plan, unknown mode, a plan that is not CSR, a matrix that is not
 * square, (expand) a column outside [0, n).  It is independent of
 * spmv_plan_prepare_transpose and spmv_plan_prepare_multi: the three keep
 * separate buffers and separate byte reports, and spmv_plan_get_info is
 * unchanged (a balanced plan's mode extends to expand mode's inner plan, for
 * spmv_plan_run_sym_multi only: spmv_plan_run_sym never uses those tables).
 * spmv_plan_run_sym follows the run conventions: asynchronous on `stream`,
 * no allocation and no synchronisation (it can be captured into a graph on
 * one stream), codes of spmv_rc.h.
 *   - y[0 .. n) is FULLY overwritten (rows and columns without entries get
 *     0.0); NO byte of y at or past n is written.
 *   - NO value outside x[0 .. n) enters a result; x and y need 8-byte
 *     alignment only.
 *   - x and y must not overlap; runs of one plan must be serialised.
 *   - Reads the caller's row_ptr, col and val, never the plan's
 *     hot-renumbered column copy.
 *   - SPMV_OTHER_ERROR with a message, before any device work: NULL plan, a
 *     plan that was not prepared, NULL x or y with n > 0.
 * Which to call (MI355X, cold, profiles/symmetric/README.md; the yardstick is
 * the forward run of a default CSR plan over the host-expanded matrix): on the
 * cant-like lower triangle (2,034,917 stored entries of 4,007,383) the yardstick
 * took 0.0107 ms, SPMV_S_EXPAND 0.0108 ms (1.01 x) and SPMV_S_FUSED 0.0259 ms
 * (2.42 x); on the 32-copy batch 0.2161, 0.2211 (1.02 x) and 0.3019 ms (1.40 x).
 * FUSED is SLOWER than the expanded forward run at both sizes although it
 * streams half the bytes (25.7 against 49.3 MB): call it for memory (3,904
 * plan-owned bytes against 56.6 MB on one matrix, 125 KB against 1.81 GB on
 * the batch) or when the matrix changes too often for A to be rebuilt, and
 * SPMV_S_EXPAND wherever A fits beside the stored half.  Not measured:
 * matrices on the wide path (power-law columns: every mirrored product is a
 * scattered global atomic there), build times, upper-triangle storage.       */
enum spmv_symmetric_mode { SPMV_S_NONE = 0, SPMV_S_FUSED = 1, SPMV_S_EXPAND = 2 };
typedef struct spmv_symmetric_info {
    int32_t mode;          /* enum spmv_symmetric_mode */
    int32_t cap;           /* fused: widest union window (columns) summed in LDS */
    int64_t blocks;        /* fused: row blocks */
    int64_t window_blocks; /* fused: row blocks whose union window fits cap */
    int64_t flush_entries; /* fused: y entries addressed by the flushes per run */
    int64_t nnz_expanded;  /* expand: entries of A */
    int64_t owned_bytes;   /* device bytes the symmetric path allocated */
    char kernel[64];       /* dominant kernel, as spmv_plan_info.kernel */
} spmv_symmetric_info;
/* 1: CSR plans with n_rows == n_cols; 0 otherwise and for NULL */
int spmv_plan_symmetric_supported(const spmv_plan *p);
int spmv_plan_prepare_symmetric(spmv_plan *p, int mode);
int spmv_plan_get_symmetric_info(const spmv_plan *p, spmv_symmetric_info *info);
int spmv_plan_run_sym(const spmv_plan *p, const double *x, double *y, void *stream);
/* SPMV_S_EXPAND only: the plan-owned CSR of A on the device, row_ptr[n + 1],
 * col / val[*nnz]; valid until the mode changes or the plan is destroyed.
 * SPMV_OTHER_ERROR for a NULL argument or a plan in another mode.          */
int spmv_plan_get_symmetric_arrays(const spmv_plan *p, const int64_t **row_ptr, const int32_t **col,
                                   const double **val, int64_t *nnz);
/* Y = (S + S^T - diag S)·X for k vectors stored row-major, the layout of
 * spmv_plan_run_multi: X[c*ldx + j], Y[i*ldy + j], c, i < n;  j < k;
 * ldx >= k, ldy >= k (elements), k >= 1.  Needs spmv_plan_prepare_symmetric
 * first and runs in whichever mode was prepared; there is no further prepare
 * call (spmv_plan_prepare_symmetric builds what this run needs too).
 *
 * The conventions above hold: device pointers, asynchronous on `stream`, no
 * allocation and no synchronisation inside the call (it can be captured into
 * a graph on one stream), codes of spmv_rc.h, a message in spmv_last_error().
 *   - Y[i*ldy + j], j < k, is fully overwritten (rows and columns without
 *     entries get 0.0); NO element with j >= k and nothing at or past row n
 *     is written.
 *   - NO byte outside X[c*ldx .. c*ldx + k) is read for any c.
 *   - X and Y need 8-byte alignment only and any ldx, ldy >= k: every load
 *     of X and every add to Y is 8 bytes wide.
 *   - X and Y must not overlap; runs of one plan must be serialised.
 *   - Reads the caller's row_ptr, col and val, never the plan's
 *     hot-renumbered column copy.  A column outside [0, n) is dropped whole,
 *     as in spmv_plan_run_sym.
 *   - SPMV_OTHER_ERROR with a message, before any device work (Y is left
 *     untouched): NULL plan, a plan that was not prepared (every plan that is
 *     not CSR or not square: it cannot be), k < 1, ldx < k or ldy < k, NULL X
 *     or Y with n > 0.
 * SPMV_S_EXPAND: spmv_plan_run_multi on the inner forward plan over A and
 *     nothing else, so its bit rule carries over: the bits of column j are
 *     those of spmv_plan_run_multi on a default forward CSR plan over the
 *     arrays of spmv_plan_get_symmetric_arrays, independent of k, of j's place
 *     in its block of 8 and of ldx / ldy.  An outer plan prepared with
 *     spmv_plan_prepare_multi(SPMV_M_BALANCED) runs the inner plan balanced
 *     too, whichever of the two prepares comes first (rule values are resolved
 *     against the inner plan's own lanes; SPMV_M_NONE ends it on the inner
 *     plan too): the bits of that forward plan prepared with the same options.
 *     spmv_multi_info is unchanged; the inner plan's balanced state is
 *     reported in spmv_symmetric_multi_info.  spmv_plan_run_sym never uses
 *     the balanced tables.
 * SPMV_S_FUSED: csr_sym_multi_kernel<KV>, KV in {1, 2, 4, 8}, one workgroup
 *     per 128 rows on the window table spmv_plan_run_sym uses (owned_bytes
 *     stays 8 * blocks).  The matrix is streamed once per block of up to 8
 *     vectors (ceil(k/8) passes, pass b on X + 8b, Y + 8b); a block of r
 *     remaining vectors runs the smallest KV >= r and neither loads nor adds
 *     its unused columns.  Y's live columns are zeroed once before the first
 *     pass.  A union window of at most cap_cols[w] = 4,096 / KV columns: LDS
 *     holds X[lo..hi] as span * KV doubles and an accumulator of the same
 *     size (66,576 bytes of LDS at the most, two workgroups per CU); entry
 *     (r, c, v) adds v X[c][j] to acc[r - lo][j] and, when c != r, v X[r][j]
 *     to acc[c - lo][j] (the row products of a wave's consecutive entries are
 *     summed per row across the wave first); the accumulator is added to Y
 *     with one fp64 atomic per non-zero word, consecutive lanes on
 *     consecutive words.  A wider union: LDS holds the block's 128 x KV values
 *     of X and 128 x KV row sums, X[c][j] is gathered from global memory and
 *     every mirrored product is added straight into Y[c][j] with a global
 *     fp64 atomic; the row sums are flushed at the end.  From KV = 4 on KV / 2
 *     lanes share an entry (handed round by DPP), two columns each.  Results
 *     are NOT bitwise reproducible from run to run; Y must be ordinary device
 *     memory.  The k = 1 result need not have spmv_plan_run_sym's bits.
 *     flush_entries[w] counts the rows of Y the flushes of one pass address
 *     (the window blocks' spans plus the rows of the wide blocks).
 * Which to call (MI355X, cold, one run on one box, profiles/symmetric/README.md;
 * the yardstick is k calls of spmv_plan_run_sym on the same plan): one call was
 * 1.50 / 2.29 / 3.60 times faster at k = 2 / 4 / 8 in fused mode on the
 * cant-like lower triangle and 1.16 / 1.33 / 1.95 times on the 32-copy batch;
 * 1.28 / 1.94 / 2.61 and 1.08 / 1.73 / 2.08 times in expand mode.  Fused stays
 * slower than expand in absolute time at every k (0.0551 against 0.0323 ms at
 * k = 8 on one matrix, 1.198 against 0.831 ms on the batch): it is for plans
 * that are fused for memory.  In EXPAND mode on the lower triangle of a
 * power-law R-MAT one call on an unprepared plan was 5 to 20 times SLOWER than
 * k calls (0.58-0.62 ms: the hub rows of A are walked by two lanes each):
 * prepare the plan with spmv_plan_prepare_multi(SPMV_M_BALANCED) there, after
 * which one call took 0.036 / 0.040 / 0.045 ms at k = 2 / 4 / 8, 0.83 / 1.52 /
 * 2.66 times the speed of k calls (at k = 2 the two calls are still the faster
 * way).  One vector belongs to spmv_plan_run_sym.  Not measured: fused mode on
 * the wide path (power-law columns), k > 8, ld > k.                          */
int spmv_plan_run_sym_multi(const spmv_plan *p, int32_t k, const double *X, int64_t ldx,
                            double *Y, int64_t ldy, void *stream);
typedef struct spmv_symmetric_multi_info {
    int32_t mode;             /* enum spmv_symmetric_mode */
    int32_t reserved;
    int32_t cap_cols[4];      /* fused: widest union window (columns) on the window path of the
                                 kernel of width 1, 2, 4, 8; expand: 0 */
    int64_t window_blocks[4]; /* fused: row blocks within that span, per width */
    int64_t flush_entries[4]; /* fused: rows of Y addressed by the flushes of one pass, per width */
    int64_t long_rows;        /* expand: the inner plan's balanced state (spmv_plan_prepare_multi), */
    int64_t segments;         /*   as spmv_multi_info's fields of these names; 0 when not balanced  */
    int64_t multi_owned_bytes;
    char kernel[64];          /* fused: csr_sym_multi_kernel; expand: the inner plan's multi-vector kernel */
} spmv_symmetric_multi_info;
/* An unprepared plan answers all zeros and an empty kernel name. */
int spmv_plan_get_symmetric_multi_info(const spmv_plan *p, spmv_symmetric_multi_info *info);
int spmv_plan_get_info(const spmv_plan *p, spmv_plan_info *info);
/* Frees what the plan allocated (never the caller's arrays). */
int spmv_plan_destroy(spmv_plan *p);

/* ------------------------------------------ the five reference kernels ---
 * One call each, no build step, x gathered from global memory: the
 * direct equivalents of the reference's five kernels.  Plans run these
 * or faster variants of them (spmv_ext.h).                               */

/* COO — kernel `coo(row,col,val,x,y,int Z)` (reference kernels/Coo.cl:24).
 * Entries MUST be sorted by row (any order inside a row).  Wave-level
 * segmented reduction over fixed tiles of entries; rows that straddle
 * tiles are finished by a second, deterministic carry pass — no atomics,
 * bitwise reproducible.  `ws` is device scratch of at least
 * spmv_coo_ws_bytes(nnz) bytes.                                          */
size_t spmv_coo_ws_bytes(int64_t nnz);
int spmv_coo_run(spmv_dims d, const int32_t *row, const int32_t *col,
                 const double *val, const double *x, double *y, void *ws,
                 size_t ws_bytes);

/* CSR — kernel `csr(ptr,col,val,x,y,int N)` (reference kernels/Csr.cl:1).
 * CSR-vector: a group of `lanes_per_row` lanes (2..64, power of two) works
 * on one row; the entry stream is staged in LDS; partial sums are reduced
 * with cross-lane moves.  lanes_per_row = 0 picks from the mean row length
 * (spmv_csr_auto_lanes).                                                 */
int spmv_csr_auto_lanes(int64_t n_rows, int64_t nnz);
int spmv_csr_run(spmv_dims d, const int64_t *row_ptr, const int32_t *col,
                 const double *val, const double *x, double *y,
                 int lanes_per_row);

/* ELL — kernel `ell(val,idx,x,y,int N,int K,__local)` (reference
 * kernels/Ell.cl:1).  Column-major, leading dimension `ld` (>= N, multiple
 * of 64), with a k-interleave `ki` in {1,2}: entry (row i, slot k) lives at
 *     (k / ki) * ld * ki + i * ki + (k % ki)
 * so one lane per row reads 8·ki contiguous bytes per step (ki = 2: 16-byte
 * dwordx4 value loads).  K (a multiple of ki) slots per row; padding slots
 * hold value 0.0 and a column already used by the row.                   */
int spmv_ell_run(spmv_dims d, int32_t K, int64_t ld, int32_t ki,
                 const int32_t *col, const double *val, const double *x,
                 double *y);

/* SELL-C-sigma — kernel `sigma_c(val,idx,x,y,slice_ptr,int C)` (reference
 * kernels/Sigma_C.cl:1).  Slices of C rows (C = 64 = one wave by default),
 * rows sorted by length inside windows of sigma rows (builder only), slice
 * s occupies [slice_ptr[s], slice_ptr[s+1]) with entry (slot r, k) at
 *     slice_ptr[s] + (k / ki) * C * ki + r * ki + (k % ki)
 * perm[s*C + r] is the original row of slot r of slice s (-1 = padding
 * slot); y[perm[.]] is written directly, no un-permute pass.  `sigma` is
 * the sorting window the builder used (1 = none; else a multiple of C):
 * one workgroup covers one window so its scattered y stores merge in one
 * L2.  spmv_sell_auto_ki: the k-interleave the SELL builders should use
 * for an n_rows matrix (2 for matrices small enough for the
 * waves-per-slice kernel, else 1), the default of ./bin/sigma_c and
 * spmv_amd.to_device.                                                     */
int spmv_sell_auto_ki(int64_t n_rows, int32_t C);
int spmv_sell_run(spmv_dims d, int32_t C, int32_t sigma, int32_t ki, int64_t n_slices,
                  const int64_t *slice_ptr, const int32_t *perm,
                  const int32_t *col, const double *val, const double *x,
                  double *y);

/* CMRS — kernel `cmrs(val,idx,strip_ptr,row_in_strip,x,y,N,h,__local)`
 * (reference kernels/Cmrs.cl:1).  Strips of h consecutive rows
 * (1 <= h <= 64); strip s holds entries [strip_ptr[s], strip_ptr[s+1]) in
 * row order and row_in_strip[j] in [0,h) (uint8, the reference used
 * int32).  The strip runs are staged in LDS, each row's slice summed by a
 * lane group; the tail strip is bounds-checked (reference Cmrs.cl:38-42
 * wrote past y).                                                          */
int spmv_cmrs_run(spmv_dims d, int32_t h, int64_t n_strips,
                  const int64_t *strip_ptr, const uint8_t *row_in_strip,
                  const int32_t *col, const double *val, const double *x,
                  double *y);

/* ------------------------------------------------------------ helpers ---
 * Device discovery (replaces reference inc/helper_functions.h:76-129),
 * memory (replaces clCreateBuffer / clEnqueueWriteBuffer /
 * clEnqueueReadBuffer, reference csr.c:123-127,183-186,220), timing.    */
int spmv_device_count(int *count);
int spmv_set_device(int device);
int spmv_device_name(int device, char *buf, size_t len);
int spmv_malloc(void **dptr, size_t bytes);
int spmv_free(void *dptr);
int spmv_memset(void *dptr, int value, size_t bytes, void *stream);
int spmv_upload(void *dptr, const void *host, size_t bytes, void *stream);
int spmv_download(void *host, const void *dptr, size_t bytes, void *stream);
int spmv_stream_create(void **stream);
int spmv_stream_destroy(void *stream);
int spmv_sync(void *stream);
/* Write `bytes` (0 = 512 MiB) of library-owned scratch on `stream` so the
 * 256 MiB Infinity Cache and the per-XCD L2s hold no SpMV operand.      */
int spmv_flush_cache(void *stream, size_t bytes);
/* The same eviction by READING the scratch (the caches then hold clean
 * lines, so the next kernel pays no write-back): bench.py's cold state. */
int spmv_flush_cache_read(void *stream, size_t bytes);
/* Timing events on a stream (hipEvent_t as void *). */
int spmv_event_create(void **ev);
int spmv_event_destroy(void *ev);
int spmv_event_record(void *ev, void *stream);
/* Milliseconds from `start` to `end`; waits for `end` to complete. */
int spmv_event_elapsed(void *start, void *end, double *ms);
/* Time one launch: record an event, call launch(arg), record an event,
 * synchronise, return elapsed milliseconds in *ms.                      */
typedef int (*spmv_launch_fn)(void *arg);
int spmv_time_launch(spmv_launch_fn launch, void *arg, void *stream,
                     double *ms);
/* Frees library-owned scratch on the current device. */
int spmv_release(void);
/* ---------------------------------------------------------- multi-GPU ---
 * Single-process row sharding over several GPUs: the
 * reference creates its OpenCL context over every GPU it finds but uses
 * device 0 only (reference csr.c:107,115; its device loop breaks after the
 * first, csr.c:30,279).  spmv_multi_init builds one RCCL communicator per
 * device with ncclCommInitAll and one non-blocking stream each; the caller
 * cuts contiguous row ranges (spmv_partition_rows), runs every shard's
 * spmv_<fmt>_run on its device's stream writing y_full_d + bounds[d], and
 * spmv_multi_allgatherv completes every device's y_full in place: one
 * ncclBroadcast of each shard's REAL row count from its owner, all in one
 * ncclGroupStart/End (an allgatherv; no padding to the largest shard).  */
typedef struct spmv_multi spmv_multi;
int spmv_multi_init(int n_gpus, const int *devices /* NULL: 0..n_gpus-1 */, spmv_multi **out);
int spmv_multi_free(spmv_multi *m);
int spmv_multi_size(const spmv_multi *m);
int spmv_multi_device(const spmv_multi *m, int i);
void *spmv_multi_stream(const spmv_multi *m, int i);
/* y_full[i]: device i's n-row y (device pointer); bounds[n_gpus + 1]      */
int spmv_multi_allgatherv(spmv_multi *m, double *const *y_full, const int64_t *bounds);
int spmv_multi_sync(spmv_multi *m);
/* Time one launch on every device together: optional flush on each, an
 * event pair around launch(arg, i) on each device's stream, all devices
 * synchronised; ms[i] = device i's elapsed time.                        */
typedef int (*spmv_multi_launch_fn)(void *arg, int i);
int spmv_multi_time(spmv_multi *m, spmv_multi_launch_fn launch, void *arg, int flush, double *ms);

const char *spmv_strerror(int rc);
const char *spmv_last_error(void);
/* Version string of the library build, e.g. "spmv-hip 0.2 gfx950". */
const char *spmv_version(void);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_H */
