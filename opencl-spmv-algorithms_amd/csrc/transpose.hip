// transpose.hip — the transposed product y = A^T x of a CSR plan
// (spmv_plan_prepare_transpose / spmv_plan_run_t, include/spmv.h).
//
// Two modes, chosen at build time:
//   SPMV_T_SCATTER  no second copy of the matrix.  The rows are cut into
//       blocks of 128; one workgroup per block streams its entries once and
//       adds val * x[row] to the entry's column.  Entries of one block share
//       few destinations (the block's column range [lo, hi], recorded at
//       build time), so a block whose range fits 2,048 columns sums in an
//       LDS accumulator (ds_add_f64) and adds the accumulator to y once,
//       consecutive lanes on consecutive columns: 256 contiguous bytes per
//       wave instruction, the shape global float atomics run at full rate
//       (DESIGN.md 4).  A block with a wider range (power-law columns) adds
//       every product straight into y (global_atomic_add_f64).
//   SPMV_T_COPY     A^T built once on the device as CSR (spmv_dev_csr_transpose)
//       and run by a forward CSR plan with default options: forward speed,
//       bitwise reproducible, 12 nnz + 8 (n_cols + 1) bytes more.  The outer
//       plan's balanced multi-vector mode (spmv_plan_prepare_multi, plan.hip)
//       extends to that inner plan, whichever is prepared first.
// Both read the caller's row_ptr / col / val, never the plan's hot-renumbered
// column copy.
//
// The multi-vector run Y = A^T X (spmv_plan_run_t_multi) works in whichever
// mode was prepared: copy is spmv_plan_run_multi on the inner plan; scatter is
// csr_t_multi_kernel<KV>, the window kernel's geometry with KV vectors per
// pass and an LDS accumulator of span * KV sums (below).
//
// Block prologue, entry stream, row search, flush and the lane geometry of the
// multi-vector kernel (t_multi_p, group_bcast): rowblock.h.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "plan.h"
#include "rowblock.h"

namespace spmv {

constexpr int32_t kTCap = 2048;   // LDS accumulator entries per workgroup (16 KiB)

// Column range {lo, hi} of every block of kRbRows rows ({0, -1}: no entry
// inside [0, n_cols)).  A column outside [0, n_cols) is left out here, as in
// csr_sym_range_kernel: the flush adds acc[0 .. span) to y[lo .. hi], so the
// recorded range must lie inside y; the run's bound checks then drop the entry.
__global__ __launch_bounds__(kBlock) void csr_t_range_kernel(int64_t n_rows, int64_t n_cols,
                                                             const int64_t *__restrict__ ptr,
                                                             const int32_t *__restrict__ col, int2 *__restrict__ win)
{
    const int64_t r0 = (int64_t)blockIdx.x * kRbRows;
    const int64_t r1 = r0 + kRbRows < n_rows ? r0 + kRbRows : n_rows;
    int lo = INT32_MAX, hi = INT32_MIN;
    for (int64_t e = ptr[r0] + threadIdx.x, e1 = ptr[r1]; e < e1; e += kBlock) {
        const int c = col[e];
        if (c >= 0 && c < n_cols) {
            lo = c < lo ? c : lo;
            hi = c > hi ? c : hi;
        }
    }
    const int2 r = block_minmax(lo, hi);
    if (threadIdx.x == 0)
        win[blockIdx.x] = r;
}

// The per-entry body of the single-vector scatter over the block's stream
// (rb_stream, per-thread loops); x of the block's rows is staged in LDS.
// LDS = true: val * x[row] is added to acc[col - lo] (ds_add_f64); false:
// straight into y[col] (global_atomic_add_f64, no return).  Every destination
// is bounds-checked against the recorded range (LDS) or n_cols (global): a
// column outside them is dropped, never written.
template <bool LDS>
__device__ __forceinline__ void t_scatter_block(const int64_t *s_ptr, const double *s_x, int nr,
                                                const int32_t *__restrict__ col, const double *__restrict__ val,
                                                double *__restrict__ y, double *acc, int32_t lo, uint32_t bound)
{
    rb_stream<false>(s_ptr, nr, col, val, [&](bool, int64_t e, int32_t c, double v) {
        const double p = v * s_x[rb_row_of(s_ptr, nr, e)];
        if constexpr (LDS) {
            const uint32_t j = (uint32_t)(c - lo);
            if (j < bound)
                atomicAdd(&acc[j], p);
        } else {
            if ((uint32_t)c < bound)
                unsafeAtomicAdd(&y[c], p);
        }
    });
}

// One workgroup per block of kRbRows rows.  LDS: the block's kRbRows + 1 row
// offsets and its kRbRows entries of x, then the accumulator of the block's
// column range when it spans at most `cap` columns.
__global__ __launch_bounds__(kBlock) void csr_t_window_kernel(int64_t n_rows, int64_t n_cols,
                                                              const int64_t *__restrict__ ptr,
                                                              const int32_t *__restrict__ col,
                                                              const double *__restrict__ val,
                                                              const double *__restrict__ x, double *__restrict__ y,
                                                              const int2 *__restrict__ win, int32_t cap)
{
    extern __shared__ double s_mem[];
    int64_t *s_ptr = reinterpret_cast<int64_t *>(s_mem);
    double *s_x = s_mem + kRbPtr;
    double *acc = s_x + kRbRows;
    const int tid = (int)threadIdx.x;
    RowBlock b;
    if (!rb_open(n_rows, ptr, win, s_ptr, &b))
        return;
    const bool lds = b.span <= cap;
    if (tid < b.nr)
        s_x[tid] = x[b.r0 + tid];
    if (lds)
        for (int j = tid; j < b.span; j += kBlock)
            acc[j] = 0.0;
    __syncthreads();
    if (!lds) {
        t_scatter_block<false>(s_ptr, s_x, b.nr, col, val, y, acc, 0, (uint32_t)n_cols);
        return;
    }
    t_scatter_block<true>(s_ptr, s_x, b.nr, col, val, y, acc, b.w.x, (uint32_t)b.span);
    __syncthreads();
    rb_flush(acc, b.span, y, b.w.x);
}

// ------------------------------------------------- multi-vector scatter
// Y = A^T X (spmv_plan_run_t_multi): the geometry of csr_t_window_kernel with
// KV vectors per pass.  The LDS accumulator holds span * KV sums, word
// (c - lo) * KV + j, so a block sums in LDS when span * KV <= kTMultiCap.
#ifndef SPMV_T_MULTI_CAP
#define SPMV_T_MULTI_CAP 8192  // an A/B build may override it (profiles/transpose/README.md)
#endif
constexpr int32_t kTMultiCap = SPMV_T_MULTI_CAP;  // LDS accumulator doubles per workgroup (64 KiB)

// One lane's CPL columns [j0, j0 + CPL) of one entry (column c, value v, block
// row r): v * X[r][j] added to acc[(c - lo) * KV + j] (LDS = true, bound = the
// block's span) or to Y[c * ldy + j] (false, bound = n_cols).  A column
// outside the bound is dropped, never written; columns j >= live (a ragged
// last block of vectors) are neither read nor added.
template <int KV, bool LDS>
__device__ __forceinline__ void t_multi_add(const double *s_x, double *acc, double *__restrict__ Y, int64_t ldy,
                                            int32_t lo, uint32_t bound, int32_t live, int j0, int32_t c, double v,
                                            int r)
{
    constexpr int CPL = KV / t_multi_p<KV>();
    const uint32_t idx = LDS ? (uint32_t)c - (uint32_t)lo : (uint32_t)c;
    if (idx >= bound)
        return;
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        const int j = j0 + i;
        if (j < live) {
            const double p = v * s_x[r * KV + j];
            if constexpr (LDS)
                atomicAdd(&acc[idx * KV + j], p);
            else
                unsafeAtomicAdd(&Y[(int64_t)idx * ldy + j], p);
        }
    }
}

// The P rounds of one step: round Q hands entry Q of every P-lane group (its
// column, value and row, found ONCE by the lane that loaded it) to the group's
// P lanes, which add their CPL columns of it.
template <int KV, bool LDS, int Q = 0>
__device__ __forceinline__ void t_multi_rounds(const double *s_x, double *acc, double *__restrict__ Y, int64_t ldy,
                                               int32_t lo, uint32_t bound, int32_t live, int j0, int32_t c, double v,
                                               int r)
{
    constexpr int P = t_multi_p<KV>();
    if constexpr (P == 1) {
        t_multi_add<KV, LDS>(s_x, acc, Y, ldy, lo, bound, live, j0, c, v, r);
    } else if constexpr (Q < P) {
        t_multi_add<KV, LDS>(s_x, acc, Y, ldy, lo, bound, live, j0, group_bcast<P, Q>(c), group_bcast<P, Q>(v),
                             group_bcast<P, Q>(r));
        t_multi_rounds<KV, LDS, Q + 1>(s_x, acc, Y, ldy, lo, bound, live, j0, c, v, r);
    }
}

// t_scatter_block for KV vectors: the same stream (every lane its own entry,
// so the matrix is loaded once) and the same row search, done once per entry
// by the lane that loaded it.  rb_stream's uniform loops (the DPP moves need
// whole waves): in the last partial step a lane past the end carries column
// -1, which every bound check drops.
template <int KV, bool LDS>
__device__ __forceinline__ void t_multi_block(const int64_t *s_ptr, const double *s_x, int nr,
                                              const int32_t *__restrict__ col, const double *__restrict__ val,
                                              double *__restrict__ Y, int64_t ldy, double *acc, int32_t lo,
                                              uint32_t bound, int32_t live)
{
    constexpr int P = t_multi_p<KV>();
    constexpr int CPL = KV / P;
    const int j0 = ((int)threadIdx.x % P) * CPL;
    rb_stream<true>(s_ptr, nr, col, val, [&](bool mine, int64_t e, int32_t c, double v) {
        const int r = mine ? rb_row_of(s_ptr, nr, e) : 0;
        t_multi_rounds<KV, LDS>(s_x, acc, Y, ldy, lo, bound, live, j0, c, v, r);
    });
}

// One workgroup per block of kRbRows rows, one pass over the block's entries
// for `live` <= KV vectors (X, Y: the pass's first column).  LDS: the block's
// kRbRows + 1 row offsets, its kRbRows x KV values of X (8-byte loads: under 2 %
// of the block's bytes), then the accumulator of span x KV sums when the
// block's column range spans at most `cap` = kTMultiCap / KV columns.
template <int KV>
__global__ __launch_bounds__(kBlock) void csr_t_multi_kernel(int64_t n_rows, int64_t n_cols,
                                                             const int64_t *__restrict__ ptr,
                                                             const int32_t *__restrict__ col,
                                                             const double *__restrict__ val,
                                                             const double *__restrict__ X, int64_t ldx,
                                                             double *__restrict__ Y, int64_t ldy,
                                                             const int2 *__restrict__ win, int32_t cap, int32_t live)
{
    extern __shared__ double s_mem[];
    int64_t *s_ptr = reinterpret_cast<int64_t *>(s_mem);
    double *s_x = s_mem + kRbPtr;
    double *acc = s_x + kRbRows * KV;
    const int tid = (int)threadIdx.x;
    RowBlock b;
    if (!rb_open(n_rows, ptr, win, s_ptr, &b))
        return;
    const int2 w = b.w;
    const int span = b.span, nr = b.nr;
    const int64_t r0 = b.r0;
    const bool lds = span <= cap;
    for (int i = tid; i < nr * KV; i += kBlock) {
        const int j = i % KV;
        if (j < live)
            s_x[i] = X[(r0 + i / KV) * ldx + j];
    }
    if (lds)
        for (int i = tid; i < span * KV; i += kBlock)
            acc[i] = 0.0;
    __syncthreads();
    if (!lds) {
        t_multi_block<KV, false>(s_ptr, s_x, nr, col, val, Y, ldy, acc, 0, (uint32_t)n_cols, live);
        return;
    }
    t_multi_block<KV, true>(s_ptr, s_x, nr, col, val, Y, ldy, acc, w.x, (uint32_t)span, live);
    __syncthreads();
    // the flush: thread t takes accumulator words t, t + 256, ...: with
    // ldy == KV a wave instruction covers 512 contiguous bytes of Y.  Sums
    // still exactly 0.0 add nothing to the zeroed Y.
    for (int i = tid; i < span * KV; i += kBlock) {
        const int j = i % KV;
        const double s = acc[i];
        if (j < live && s != 0.0)
            unsafeAtomicAdd(&Y[(int64_t)(w.x + i / KV) * ldy + j], s);
    }
}

// Y[c*ldy + j] = 0 for c < n_cols, j < k (ldy > k: the gaps are not touched)
__global__ __launch_bounds__(kBlock) void t_zero_cols_kernel(int64_t n_cols, int32_t k, double *__restrict__ Y,
                                                             int64_t ldy)
{
    const int64_t n = n_cols * k;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        Y[i / k * ldy + i % k] = 0.0;
}

namespace {

int t_alloc(TransposeState *t, void **dst, size_t bytes)
{
    return owned_alloc(dst, bytes, &t->owned, "spmv_plan_prepare_transpose");
}

// dynamic LDS bytes of a csr_t_multi_kernel<kv> launch whose widest LDS block
// spans `span` columns, and the most a plan can ask for
constexpr size_t t_multi_lds(int kv, int64_t span)
{
    return (size_t)(kRbPtr + kRbRows * kv + span * kv) * sizeof(double);
}

constexpr size_t t_multi_lds_max(int kv) { return t_multi_lds(kv, kTMultiCap / kv); }

int prepare_scatter(spmv_plan *p)
{
    const spmv_dims &d = p->d;
    TransposeState &t = p->t;
    const hipStream_t st = (hipStream_t)d.stream;
    const int64_t blocks = (d.n_rows + kRbRows - 1) / kRbRows;
    if (blocks > INT32_MAX)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_prepare_transpose: too many row blocks");
    t.blocks = blocks;
    if (blocks == 0 || d.nnz == 0)  // a run only zeroes y
        return SPMV_SUCCESS;
    int rc = t_alloc(&t, &t.win, (size_t)blocks * sizeof(int2));
    if (rc != SPMV_SUCCESS)
        return rc;
    hipLaunchKernelGGL(csr_t_range_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, d.n_rows, d.n_cols, p->ptr,
                       p->col, (int2 *)t.win);
    SPMV_CHECK_LAUNCH("csr_t_range_kernel");
    int2 *h = nullptr;
    if ((rc = windows_download(t.win, blocks, st, &h, "spmv_plan_prepare_transpose")) != SPMV_SUCCESS)
        return rc;
    const WindowTally one = windows_tally(h, blocks, kTCap);
    t.lds_blocks = one.blocks;
    t.flush = one.spans;
    t.xcap = one.widest;
    for (int w = 0; w < 4; ++w) {  // the multi-vector kernels: span * KV sums per block
        const WindowTally multi = windows_tally(h, blocks, kTMultiCap / kTWidths[w]);
        t.mlds[w] = multi.blocks;
        t.mxcap[w] = multi.widest;
    }
    free(h);
    // a launch of the widest fitting span may need more than the default 64 KiB
    // of dynamic LDS: allowed here, once, so that a run only launches
    hipError_t e = hipSuccess;
    with_each_width([&](auto KV) {
        constexpr int kv = decltype(KV)::value;
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(csr_t_multi_kernel<kv>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)t_multi_lds_max(kv));
    });
    if (e != hipSuccess)
        return fail(SPMV_PROGRAM_ERROR, "spmv_plan_prepare_transpose: dynamic LDS of csr_t_multi_kernel", e);
    return SPMV_SUCCESS;
}

int prepare_copy(spmv_plan *p)
{
    const spmv_dims &d = p->d;
    if (d.n_rows > INT32_MAX)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_prepare_transpose: the copy stores row ids as int32");
    TransposeState &t = p->t;
    int rc;
    if ((rc = t_alloc(&t, (void **)&t.ptr, (size_t)(d.n_cols + 1) * sizeof(int64_t))) != SPMV_SUCCESS ||
        (rc = t_alloc(&t, (void **)&t.col, (size_t)d.nnz * sizeof(int32_t))) != SPMV_SUCCESS ||
        (rc = t_alloc(&t, (void **)&t.val, (size_t)d.nnz * sizeof(double))) != SPMV_SUCCESS ||
        (rc = spmv_dev_csr_transpose(d, p->ptr, p->col, p->val, t.ptr, t.col, t.val)) != SPMV_SUCCESS)
        return rc;
    spmv_dims dt = d;
    dt.n_rows = d.n_cols;
    dt.n_cols = d.n_rows;
    if ((rc = spmv_plan_csr(dt, t.ptr, t.col, t.val, nullptr, &t.inner)) != SPMV_SUCCESS)
        return rc;
    // a balanced outer plan (spmv_plan_prepare_multi) extends to the inner one
    return p->m.mode != SPMV_M_NONE ? spmv_plan_prepare_multi(t.inner, p->m.mode, &p->m.req) : SPMV_SUCCESS;
}

int launch_scatter(const spmv_plan *p, const double *x, double *y, hipStream_t st)
{
    const spmv_dims &d = p->d;
    if (d.n_cols > 0) {
        hipError_t e = hipMemsetAsync(y, 0, (size_t)d.n_cols * sizeof(double), st);
        if (e != hipSuccess)
            return fail(SPMV_PROGRAM_ERROR, "spmv_plan_run_t: memset", e);
    }
    if (!p->t.win || d.n_cols == 0)
        return SPMV_SUCCESS;
    const size_t lds = (size_t)(kRbPtr + kRbRows + p->t.xcap) * sizeof(double);
    hipLaunchKernelGGL(csr_t_window_kernel, dim3((unsigned)p->t.blocks), dim3(kBlock), lds, st, d.n_rows, d.n_cols,
                       p->ptr, p->col, p->val, x, y, (const int2 *)p->t.win, kTCap);
    SPMV_CHECK_LAUNCH("csr_t_window_kernel");
    return SPMV_SUCCESS;
}

// Y zeroed once (columns j < k only), then ceil(k/8) passes of the narrowest
// kernel that holds the pass's vectors
int launch_scatter_multi(const spmv_plan *p, int32_t k, const double *X, int64_t ldx, double *Y, int64_t ldy,
                         hipStream_t st)
{
    const spmv_dims &d = p->d;
    if (k == 1 && ldx == 1 && ldy == 1)
        return launch_scatter(p, X, Y, st);
    const int rc = zero_cols(d.n_cols, k, Y, ldy, st, "spmv_plan_run_t_multi");
    if (rc != SPMV_SUCCESS)
        return rc;
    if (!p->t.win || d.n_cols == 0)
        return SPMV_SUCCESS;
    for (int32_t j0 = 0; j0 < k; j0 += 8) {
        const int32_t live = k - j0 < 8 ? k - j0 : 8;
        const int w = live > 4 ? 3 : live > 2 ? 2 : live - 1;  // width kTWidths[w] >= live
        with_int<1, 2, 4, 8>(kTWidths[w], [&](auto KV) {
            constexpr int kv = decltype(KV)::value;
            hipLaunchKernelGGL(csr_t_multi_kernel<kv>, dim3((unsigned)p->t.blocks), dim3(kBlock),
                               t_multi_lds(kv, p->t.mxcap[w]), st, d.n_rows, d.n_cols, p->ptr, p->col, p->val, X + j0,
                               ldx, Y + j0, ldy, (const int2 *)p->t.win, kTMultiCap / kv, live);
        });
        SPMV_CHECK_LAUNCH("csr_t_multi_kernel");
    }
    return SPMV_SUCCESS;
}

}  // namespace

void plan_transpose_free(spmv_plan *p) { mode_state_free(&p->t); }

int zero_cols(int64_t n, int32_t k, double *Y, int64_t ldy, hipStream_t st, const char *who)
{
    if (n <= 0)
        return SPMV_SUCCESS;
    if (ldy == k) {
        const hipError_t e = hipMemsetAsync(Y, 0, (size_t)n * k * sizeof(double), st);
        if (e != hipSuccess)
            return fail(SPMV_PROGRAM_ERROR, who, e);
        return SPMV_SUCCESS;
    }
    const int64_t want = (n * k + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(t_zero_cols_kernel, dim3((unsigned)(want < 65536 ? want : 65536)), dim3(kBlock), 0, st, n, k, Y,
                       ldy);
    SPMV_CHECK_LAUNCH(who);
    return SPMV_SUCCESS;
}

}  // namespace spmv

using namespace spmv;

extern "C" {

int spmv_plan_transpose_supported(const spmv_plan *p) { return p && p->fmt == SPMV_FMT_CSR ? 1 : 0; }

int spmv_plan_prepare_transpose(spmv_plan *p, int mode)
{
    if (!p)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_prepare_transpose: plan is NULL");
    if (mode != SPMV_T_NONE && mode != SPMV_T_SCATTER && mode != SPMV_T_COPY)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_prepare_transpose: unknown mode");
    if (p->fmt != SPMV_FMT_CSR)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_prepare_transpose: only CSR plans have a transposed run");
    if (mode == p->t.mode)
        return SPMV_SUCCESS;
    SPMV_GUARD(p->d);
    const hipStream_t st = (hipStream_t)p->d.stream;
    // a run of the old mode may still be in flight on the build stream
    if (p->t.mode != SPMV_T_NONE && hipStreamSynchronize(st) != hipSuccess)
        return fail_msg(SPMV_PROGRAM_ERROR, "spmv_plan_prepare_transpose: synchronise");
    plan_transpose_free(p);
    if (mode == SPMV_T_NONE)
        return SPMV_SUCCESS;
    int rc = mode == SPMV_T_SCATTER ? prepare_scatter(p) : prepare_copy(p);
    // runs may come on any stream: everything is complete when this returns
    if (rc == SPMV_SUCCESS && hipStreamSynchronize(st) != hipSuccess)
        rc = fail_msg(SPMV_PROGRAM_ERROR, "spmv_plan_prepare_transpose: synchronise");
    if (rc != SPMV_SUCCESS)  // SPMV_T_NONE is left
        return fail_after(rc, [&] { plan_transpose_free(p); });
    p->t.mode = mode;
    return SPMV_SUCCESS;
}

int spmv_plan_get_transpose_info(const spmv_plan *p, spmv_transpose_info *info)
{
    if (!p || !info)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_get_transpose_info: NULL argument");
    memset(info, 0, sizeof *info);
    const TransposeState &t = p->t;
    info->mode = t.mode;
    info->owned_bytes = (int64_t)(t.owned + (t.inner ? t.inner->owned : 0));
    if (t.mode == SPMV_T_SCATTER) {
        info->cap = kTCap;
        info->blocks = t.blocks;
        info->lds_blocks = t.lds_blocks;
        info->flush_entries = t.flush;
        snprintf(info->kernel, sizeof info->kernel, "csr_t_window_kernel");
    } else if (t.inner) {
        snprintf(info->kernel, sizeof info->kernel, "%s", t.inner->kernel);
    }
    return SPMV_SUCCESS;
}

int spmv_plan_run_t(const spmv_plan *p, const double *x, double *y, void *stream)
{
    if (!p)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_t: plan is NULL");
    if (p->t.mode == SPMV_T_NONE)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_t: the plan was not prepared (spmv_plan_prepare_transpose)");
    if ((p->d.n_rows > 0 && !x) || (p->d.n_cols > 0 && !y))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_t: x or y is NULL");
    if (p->t.mode == SPMV_T_COPY)
        return spmv_plan_run(p->t.inner, x, y, stream);
    SPMV_GUARD(p->d);
    return launch_scatter(p, x, y, (hipStream_t)stream);
}

int spmv_plan_get_transpose_multi_info(const spmv_plan *p, spmv_transpose_multi_info *info)
{
    if (!p || !info)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_get_transpose_multi_info: NULL argument");
    memset(info, 0, sizeof *info);
    info->mode = p->t.mode;
    if (p->t.mode == SPMV_T_SCATTER) {
        for (int w = 0; w < 4; ++w) {
            info->cap_cols[w] = kTMultiCap / kTWidths[w];
            info->lds_blocks[w] = p->t.mlds[w];
        }
        snprintf(info->kernel, sizeof info->kernel, "csr_t_multi_kernel");
    } else if (p->t.inner) {
        snprintf(info->kernel, sizeof info->kernel, "csr_multi_kernel");  // every CSR path's multi-vector kernel
    }
    return SPMV_SUCCESS;
}

int spmv_plan_run_t_multi(const spmv_plan *p, int32_t k, const double *X, int64_t ldx, double *Y, int64_t ldy,
                          void *stream)
{
    if (!p)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_t_multi: plan is NULL");
    if (p->t.mode == SPMV_T_NONE)
        return fail_msg(SPMV_OTHER_ERROR,
                        "spmv_plan_run_t_multi: the plan was not prepared (spmv_plan_prepare_transpose)");
    if (k < 1)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_t_multi: k must be at least 1");
    if (ldx < k || ldy < k)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_t_multi: ldx and ldy must be at least k");
    if ((p->d.n_rows > 0 && !X) || (p->d.n_cols > 0 && !Y))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_t_multi: X or Y is NULL");
    if (p->t.mode == SPMV_T_COPY)
        return spmv_plan_run_multi(p->t.inner, k, X, ldx, Y, ldy, stream);
    SPMV_GUARD(p->d);
    return launch_scatter_multi(p, k, X, ldx, Y, ldy, (hipStream_t)stream);
}

}  // extern "C"
