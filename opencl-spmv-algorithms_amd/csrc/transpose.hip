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
//       bitwise reproducible, 12 nnz + 8 (n_cols + 1) bytes more.
// Both read the caller's row_ptr / col / val, never the plan's hot-renumbered
// column copy.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "plan.h"

namespace spmv {

constexpr int kTRows = 128;       // rows per block (the forward x-window default)
constexpr int32_t kTCap = 2048;   // LDS accumulator entries per workgroup (16 KiB)
constexpr int kTPtr = kTRows + 2; // LDS slots of the block's kTRows + 1 row offsets (a 16-byte multiple)
constexpr int kTU = 4;            // entries in flight per thread

// column range {lo, hi} of every block of kTRows rows ({0, -1}: no entries)
__global__ __launch_bounds__(kBlock) void csr_t_range_kernel(int64_t n_rows, const int64_t *__restrict__ ptr,
                                                             const int32_t *__restrict__ col, int2 *__restrict__ win)
{
    const int64_t r0 = (int64_t)blockIdx.x * kTRows;
    const int64_t r1 = r0 + kTRows < n_rows ? r0 + kTRows : n_rows;
    const int2 r = block_col_range(col, ptr[r0], ptr[r1]);
    if (threadIdx.x == 0)
        win[blockIdx.x] = r;
}

// The block's entries [s_ptr[0], s_ptr[nr]) as ONE coalesced stream: thread t
// takes entries t, t + 256, ... with kTU of them in flight, whatever the row
// lengths (a lane group per row waits out one memory round trip per row: 39 us
// instead of 28 on the cant-like matrix, profiles/transpose/README.md).  The
// row of an entry is the last r with s_ptr[r] <= e, a fixed-depth binary
// search of the offsets in LDS; x of the block's rows is staged in LDS too.
// LDS = true: val * x[row] is added to acc[col - lo] (ds_add_f64); false:
// straight into y[col] (global_atomic_add_f64, no return).  Every destination
// is bounds-checked against the recorded range (LDS) or n_cols (global): a
// column outside them is dropped, never written.
template <bool LDS>
__device__ __forceinline__ void t_scatter_block(const int64_t *s_ptr, const double *s_x, int nr,
                                                const int32_t *__restrict__ col, const double *__restrict__ val,
                                                double *__restrict__ y, double *acc, int32_t lo, uint32_t bound)
{
    auto add = [&](int64_t e, int32_t c, double v) {
        int r = 0;  // s_ptr[r] <= e < s_ptr[r + span of the search]
#pragma unroll
        for (int step = kTRows / 2; step > 0; step >>= 1)
            if (r + step < nr && s_ptr[r + step] <= e)
                r += step;
        const double p = v * s_x[r];
        if constexpr (LDS) {
            const uint32_t j = (uint32_t)(c - lo);
            if (j < bound)
                atomicAdd(&acc[j], p);
        } else {
            if ((uint32_t)c < bound)
                unsafeAtomicAdd(&y[c], p);
        }
    };
    const int64_t end = s_ptr[nr];
    int64_t e = s_ptr[0] + (int64_t)threadIdx.x;
    for (; e + (kTU - 1) * kBlock < end; e += kTU * kBlock) {
        int32_t c[kTU];
        double v[kTU];
#pragma unroll
        for (int u = 0; u < kTU; ++u) {
            c[u] = stream_load<true>(col + e + u * kBlock);
            v[u] = stream_load<true>(val + e + u * kBlock);
        }
#pragma unroll
        for (int u = 0; u < kTU; ++u)
            add(e + u * kBlock, c[u], v[u]);
    }
    for (; e < end; e += kBlock)
        add(e, stream_load<true>(col + e), stream_load<true>(val + e));
}

// One workgroup per block of kTRows rows.  LDS: the block's kTRows + 1 row
// offsets and its kTRows entries of x, then the accumulator of the block's
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
    double *s_x = s_mem + kTPtr;
    double *acc = s_x + kTRows;
    const int tid = (int)threadIdx.x;
    const int2 w = win[blockIdx.x];
    const int span = w.y - w.x + 1;             // <= 0: a block without entries
    if (span <= 0)                              // uniform per workgroup
        return;
    const bool lds = span <= cap;
    const int64_t r0 = (int64_t)blockIdx.x * kTRows;
    const int nr = (int)(n_rows - r0 < kTRows ? n_rows - r0 : kTRows);
    for (int i = tid; i <= nr; i += kBlock)
        s_ptr[i] = ptr[r0 + i];
    if (tid < nr)
        s_x[tid] = x[r0 + tid];
    if (lds)
        for (int j = tid; j < span; j += kBlock)
            acc[j] = 0.0;
    __syncthreads();
    if (!lds) {
        t_scatter_block<false>(s_ptr, s_x, nr, col, val, y, acc, 0, (uint32_t)n_cols);
        return;
    }
    t_scatter_block<true>(s_ptr, s_x, nr, col, val, y, acc, w.x, (uint32_t)span);
    __syncthreads();
    // the flush: consecutive lanes, consecutive columns; sums still exactly
    // 0.0 add nothing to the zeroed y
    for (int j = tid; j < span; j += kBlock) {
        const double s = acc[j];
        if (s != 0.0)
            unsafeAtomicAdd(&y[w.x + j], s);
    }
}

namespace {

int t_alloc(spmv_plan *p, void **dst, size_t bytes)
{
    *dst = nullptr;
    hipError_t e = hipMalloc(dst, bytes > 0 ? bytes : 16);
    if (e != hipSuccess)
        return fail(SPMV_PROGRAM_ERROR, "spmv_plan_prepare_transpose: hipMalloc", e);
    p->t_owned += bytes;
    return SPMV_SUCCESS;
}

int prepare_scatter(spmv_plan *p)
{
    const spmv_dims &d = p->d;
    const hipStream_t st = (hipStream_t)d.stream;
    const int64_t blocks = (d.n_rows + kTRows - 1) / kTRows;
    if (blocks > INT32_MAX)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_prepare_transpose: too many row blocks");
    p->t_blocks = blocks;
    if (blocks == 0 || d.nnz == 0)  // a run only zeroes y
        return SPMV_SUCCESS;
    int rc = t_alloc(p, &p->t_win, (size_t)blocks * sizeof(int2));
    if (rc != SPMV_SUCCESS)
        return rc;
    hipLaunchKernelGGL(csr_t_range_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, d.n_rows, p->ptr, p->col,
                       (int2 *)p->t_win);
    SPMV_CHECK_LAUNCH("csr_t_range_kernel");
    int2 *h = nullptr;
    if ((rc = windows_download(p->t_win, blocks, st, &h, "spmv_plan_prepare_transpose")) != SPMV_SUCCESS)
        return rc;
    for (int64_t b = 0; b < blocks; ++b) {
        const int64_t span = (int64_t)h[b].y - h[b].x + 1;
        if (span > 0 && span <= kTCap) {
            p->t_lds_blocks++;
            p->t_flush += span;
            p->t_xcap = span > p->t_xcap ? (int32_t)span : p->t_xcap;
        }
    }
    free(h);
    return SPMV_SUCCESS;
}

int prepare_copy(spmv_plan *p)
{
    const spmv_dims &d = p->d;
    if (d.n_rows > INT32_MAX)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_prepare_transpose: the copy stores row ids as int32");
    int rc;
    if ((rc = t_alloc(p, (void **)&p->t_ptr, (size_t)(d.n_cols + 1) * sizeof(int64_t))) != SPMV_SUCCESS ||
        (rc = t_alloc(p, (void **)&p->t_col, (size_t)d.nnz * sizeof(int32_t))) != SPMV_SUCCESS ||
        (rc = t_alloc(p, (void **)&p->t_val, (size_t)d.nnz * sizeof(double))) != SPMV_SUCCESS ||
        (rc = spmv_dev_csr_transpose(d, p->ptr, p->col, p->val, p->t_ptr, p->t_col, p->t_val)) != SPMV_SUCCESS)
        return rc;
    spmv_dims t = d;
    t.n_rows = d.n_cols;
    t.n_cols = d.n_rows;
    return spmv_plan_csr(t, p->t_ptr, p->t_col, p->t_val, nullptr, &p->t_inner);
}

int launch_scatter(const spmv_plan *p, const double *x, double *y, hipStream_t st)
{
    const spmv_dims &d = p->d;
    if (d.n_cols > 0) {
        hipError_t e = hipMemsetAsync(y, 0, (size_t)d.n_cols * sizeof(double), st);
        if (e != hipSuccess)
            return fail(SPMV_PROGRAM_ERROR, "spmv_plan_run_t: memset", e);
    }
    if (!p->t_win || d.n_cols == 0)
        return SPMV_SUCCESS;
    const size_t lds = (size_t)(kTPtr + kTRows + p->t_xcap) * sizeof(double);
    hipLaunchKernelGGL(csr_t_window_kernel, dim3((unsigned)p->t_blocks), dim3(kBlock), lds, st, d.n_rows, d.n_cols,
                       p->ptr, p->col, p->val, x, y, (const int2 *)p->t_win, kTCap);
    SPMV_CHECK_LAUNCH("csr_t_window_kernel");
    return SPMV_SUCCESS;
}

}  // namespace

void plan_transpose_free(spmv_plan *p)
{
    if (p->t_inner)
        spmv_plan_destroy(p->t_inner);
    for (void *q : {p->t_win, (void *)p->t_ptr, (void *)p->t_col, (void *)p->t_val})
        if (q)
            (void)hipFree(q);
    p->t_inner = nullptr;
    p->t_win = nullptr;
    p->t_ptr = nullptr;
    p->t_col = nullptr;
    p->t_val = nullptr;
    p->t_mode = SPMV_T_NONE;
    p->t_xcap = 0;
    p->t_blocks = p->t_lds_blocks = p->t_flush = 0;
    p->t_owned = 0;
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
    if (mode == p->t_mode)
        return SPMV_SUCCESS;
    SPMV_GUARD(p->d);
    const hipStream_t st = (hipStream_t)p->d.stream;
    // a run of the old mode may still be in flight on the build stream
    if (p->t_mode != SPMV_T_NONE && hipStreamSynchronize(st) != hipSuccess)
        return fail_msg(SPMV_PROGRAM_ERROR, "spmv_plan_prepare_transpose: synchronise");
    plan_transpose_free(p);
    if (mode == SPMV_T_NONE)
        return SPMV_SUCCESS;
    int rc = mode == SPMV_T_SCATTER ? prepare_scatter(p) : prepare_copy(p);
    // runs may come on any stream: everything is complete when this returns
    if (rc == SPMV_SUCCESS && hipStreamSynchronize(st) != hipSuccess)
        rc = fail_msg(SPMV_PROGRAM_ERROR, "spmv_plan_prepare_transpose: synchronise");
    if (rc != SPMV_SUCCESS) {
        char keep[512];
        snprintf(keep, sizeof keep, "%s", spmv_last_error());
        plan_transpose_free(p);
        return fail_msg(rc, keep);
    }
    p->t_mode = mode;
    return SPMV_SUCCESS;
}

int spmv_plan_get_transpose_info(const spmv_plan *p, spmv_transpose_info *info)
{
    if (!p || !info)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_get_transpose_info: NULL argument");
    memset(info, 0, sizeof *info);
    info->mode = p->t_mode;
    info->owned_bytes = (int64_t)(p->t_owned + (p->t_inner ? p->t_inner->owned : 0));
    if (p->t_mode == SPMV_T_SCATTER) {
        info->cap = kTCap;
        info->blocks = p->t_blocks;
        info->lds_blocks = p->t_lds_blocks;
        info->flush_entries = p->t_flush;
        snprintf(info->kernel, sizeof info->kernel, "csr_t_window_kernel");
    } else if (p->t_inner) {
        snprintf(info->kernel, sizeof info->kernel, "%s", p->t_inner->kernel);
    }
    return SPMV_SUCCESS;
}

int spmv_plan_run_t(const spmv_plan *p, const double *x, double *y, void *stream)
{
    if (!p)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_t: plan is NULL");
    if (p->t_mode == SPMV_T_NONE)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_t: the plan was not prepared (spmv_plan_prepare_transpose)");
    if ((p->d.n_rows > 0 && !x) || (p->d.n_cols > 0 && !y))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_t: x or y is NULL");
    if (p->t_mode == SPMV_T_COPY)
        return spmv_plan_run(p->t_inner, x, y, stream);
    SPMV_GUARD(p->d);
    return launch_scatter(p, x, y, (hipStream_t)stream);
}

}  // extern "C"
