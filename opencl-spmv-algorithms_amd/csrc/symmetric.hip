// symmetric.hip — the symmetric product y = (S + S^T - diag S) x of a square
// CSR plan that stores one half of a symmetric matrix
// (spmv_plan_prepare_symmetric / spmv_plan_run_sym, include/spmv.h).
//
// Every stored off-diagonal entry (i, j, v) also stands for (j, i, v); the
// diagonal counts once; duplicates and entries stored on both sides count as
// listed (spmv_coo_symmetrize, spmv_host.h).  Skew-symmetric and hermitian
// meanings are out of scope.  Two modes, chosen at build time:
//   SPMV_S_FUSED   one pass over the half storage, no second copy.  The
//       row-block core (rowblock.h): one workgroup per block of 128 rows
//       streams the block's entries once.  The block's
//       UNION window {lo, hi}, its column range joined with its own rows, is
//       recorded at build time.  A union of at most 2,048 columns: x[lo..hi]
//       is staged in LDS beside an accumulator of the same span; entry
//       (r, c, v) adds v x[c] to acc[r - lo] and, when c != r, v x[r] to
//       acc[c - lo] (ds_add_f64, both x values from LDS; the row products of
//       a wave's consecutive entries are summed per row across the wave first
//       and added once per run); the accumulator is added to the zeroed y
//       once, consecutive lanes on consecutive columns.
//       A wider union (power-law columns): the rows' sums go through a
//       128-entry LDS accumulator, x[c] is gathered from global memory and
//       every mirrored product is added straight into y
//       (global_atomic_add_f64).
//   SPMV_S_EXPAND  A built once on the device as CSR: the symmetrized COO in
//       spmv_coo_symmetrize's order (the plan's CSR entries, then the mirror
//       of every off-diagonal one, placed by a prefix sum of the off-diagonal
//       flags), spmv_dev_csr_from_coo over it, and a forward CSR plan with
//       default options over the result.
// Both read the caller's row_ptr / col / val, never the plan's hot-renumbered
// column copy, and are independent of the transposed mode.
//
// The multi-vector run Y = (S + S^T - diag S) X (spmv_plan_run_sym_multi)
// works in whichever mode was prepared: expand is spmv_plan_run_multi on the
// inner plan (the outer plan's balanced mode, spmv_plan_prepare_multi in
// plan.hip, extends to it, whichever is prepared first); fused is
// csr_sym_multi_kernel<KV>, the window kernel's geometry with KV vectors per
// pass (below).  spmv_plan_prepare_symmetric builds what it needs too.
#include <hipcub/hipcub.hpp>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "plan.h"
#include "rowblock.h"

namespace spmv {

constexpr int32_t kSCap = 2048;   // widest union window summed in LDS (x + accumulator: 32 KiB)

// Union window {lo, hi} of every block of kRbRows rows: the range of its
// columns inside [0, n) joined with its own rows ({0, -1}: no such entry).  A
// column outside [0, n) is left out here and dropped by the run's checks.
__global__ __launch_bounds__(kBlock) void csr_sym_range_kernel(int64_t n, int64_t nnz,
                                                               const int64_t *__restrict__ ptr,
                                                               const int32_t *__restrict__ col,
                                                               int2 *__restrict__ win)
{
    const int64_t r0 = (int64_t)blockIdx.x * kRbRows;
    const int64_t r1 = r0 + kRbRows < n ? r0 + kRbRows : n;
    int lo = INT32_MAX, hi = INT32_MIN;
    if (nnz > 0)
        for (int64_t e = ptr[r0] + threadIdx.x, e1 = ptr[r1]; e < e1; e += kBlock) {
            const int c = col[e];
            if (c >= 0 && c < n) {
                lo = c < lo ? c : lo;
                hi = c > hi ? c : hi;
            }
        }
    int2 r = block_minmax(lo, hi);
    if (threadIdx.x == 0) {
        if (r.y >= r.x) {
            r.x = r0 < r.x ? (int)r0 : r.x;
            r.y = r1 - 1 > r.y ? (int)(r1 - 1) : r.y;
        }
        win[blockIdx.x] = r;
    }
}

// A wave's 64 consecutive entries belong to few rows (32 entries per stored
// cant-like row), so their row products would meet at few accumulator words
// and the LDS adds of one instruction would run one after another.  Each run
// of equal keys (lanes in entry order; -1: nothing to add) is summed across
// the wave by a segmented scan and its last lane alone adds the sum.  The
// scan compares a lane's key with the key `off` lanes below only, so equal
// keys must be contiguous: a lane with nothing to add inside a row keeps the
// row's key and passes p = 0.0; -1 is for the lanes past the stream's end,
// the wave's last.  Called in uniform control flow (every lane of the wave
// active).
__device__ __forceinline__ void wave_run_add(double *acc, int key, double p)
{
    const int lane = (int)threadIdx.x % kWave;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const double t = __shfl_up(p, off);
        const int k = __shfl_up(key, off);
        if (lane >= off && k == key)
            p += t;
    }
    const int next = __shfl_down(key, 1);
    if (key >= 0 && (lane == kWave - 1 || next != key))
        atomicAdd(&acc[key], p);
}

// The per-entry body of the fused run over the block's stream (rb_stream,
// uniform loops: the shuffles need whole waves; in the last partial step a
// lane past the end carries key -1).
// WIN = true: xs = x[lo .. lo + bound) and acc of the same span, both LDS;
// an entry whose row or column lies outside the window is dropped whole.
// WIN = false: xs = x of the block's rows and acc their 128 sums, both LDS;
// x[c] comes from global memory, the mirrored product goes straight into
// y[c]; bound = n, a column outside [0, n) is dropped whole.
// The row products of a wave's 64 consecutive entries are summed per row
// across the wave before they reach the accumulator (wave_run_add); a dropped
// entry stays in its row's run with a product of 0.0, as in sym_multi_add.
template <bool WIN>
__device__ __forceinline__ void sym_block(const int64_t *s_ptr, int nr, int64_t r0, const int32_t *__restrict__ col,
                                          const double *__restrict__ val, const double *__restrict__ x,
                                          double *__restrict__ y, const double *xs, double *acc, int32_t lo,
                                          uint32_t bound)
{
    rb_stream<true>(s_ptr, nr, col, val, [&](bool live, int64_t e, int32_t c, double v) {
        const int r = rb_row_of(s_ptr, nr, e);
        int key = -1;
        double p = 0.0;
        if constexpr (WIN) {
            const uint32_t jr = (uint32_t)(r0 + r) - (uint32_t)lo;
            const uint32_t jc = (uint32_t)c - (uint32_t)lo;
            if (live && jr < bound) {
                key = (int)jr;
                if (jc < bound) {
                    p = v * xs[jc];
                    if (jc != jr)
                        atomicAdd(&acc[jc], v * xs[jr]);
                }
            }
        } else {
            if (live) {
                key = r;
                if ((uint32_t)c < bound) {
                    p = v * x[c];
                    if ((int64_t)c != r0 + r)
                        unsafeAtomicAdd(&y[c], v * xs[r]);
                }
            }
        }
        wave_run_add(acc, key, p);
    });
}

// One workgroup per block of kRbRows rows.  LDS: the block's kRbRows + 1 row
// offsets, then two arrays of the union's span (x window, accumulator) when
// it is at most `cap`, else two arrays of kRbRows (the rows' x, their sums).
// The launch provides kRbPtr + 2 * max(widest fitting span, kRbRows) doubles.
__global__ __launch_bounds__(kBlock) void csr_sym_window_kernel(int64_t n, const int64_t *__restrict__ ptr,
                                                                const int32_t *__restrict__ col,
                                                                const double *__restrict__ val,
                                                                const double *__restrict__ x, double *__restrict__ y,
                                                                const int2 *__restrict__ win, int32_t cap)
{
    extern __shared__ double s_mem[];
    int64_t *s_ptr = reinterpret_cast<int64_t *>(s_mem);
    double *xs = s_mem + kRbPtr;
    const int tid = (int)threadIdx.x;
    RowBlock b;
    if (!rb_open(n, ptr, win, s_ptr, &b))
        return;
    const int2 w = b.w;
    const int span = b.span, nr = b.nr;
    const int64_t r0 = b.r0;
    // a window that does not hold the block's rows or leaves [0, n) is not one
    // this plan recorded: nothing is read or written through it
    if (w.x < 0 || w.y >= n || w.x > r0 || w.y < r0 + nr - 1)
        return;
    if (span <= cap) {
        double *acc = xs + span;
        copy_window(xs, x, w.x, span);
        for (int j = tid; j < span; j += kBlock)
            acc[j] = 0.0;
        __syncthreads();
        sym_block<true>(s_ptr, nr, r0, col, val, x, y, xs, acc, w.x, (uint32_t)span);
        __syncthreads();
        rb_flush(acc, span, y, w.x);
        return;
    }
    double *acc = xs + kRbRows;
    if (tid < nr) {
        xs[tid] = x[r0 + tid];
        acc[tid] = 0.0;
    }
    __syncthreads();
    sym_block<false>(s_ptr, nr, r0, col, val, x, y, xs, acc, 0, (uint32_t)n);
    __syncthreads();
    if (tid < nr) {
        const double s = acc[tid];
        if (s != 0.0)
            unsafeAtomicAdd(&y[r0 + tid], s);
    }
}

// ------------------------------------------------- multi-vector fused run
// Y = (S + S^T - diag S) X (spmv_plan_run_sym_multi): the geometry of
// csr_sym_window_kernel with KV vectors per pass.  The window and the
// accumulator hold span * KV words each, word (c - lo) * KV + j, so a block
// takes the window path when span * KV <= kSMultiCap.
#ifndef SPMV_S_MULTI_CAP
#define SPMV_S_MULTI_CAP 4096  // an A/B build may override it (profiles/symmetric/README.md)
#endif
constexpr int32_t kSMultiCap = SPMV_S_MULTI_CAP;  // doubles per LDS array (2 arrays: 64 KiB)
static_assert(kSMultiCap >= kRbRows * 8, "the wide path's two arrays of kRbRows x KV fit the same LDS");

// wave_run_add for lanes that hold CPL sums each (KV <= 2: every lane its own
// entry, lanes in entry order): the runs of equal keys are summed across the
// wave and the last lane of a run adds its CPL sums to acc[key + i], i < live.
// key = -1: nothing to add (only the lanes past the stream's end, which are
// the wave's last).  Called in uniform control flow.
template <int CPL>
__device__ __forceinline__ void wave_run_add_cols(double *acc, int key, double (&p)[CPL], int32_t live)
{
    const int lane = (int)threadIdx.x % kWave;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int k = __shfl_up(key, off);
        const bool same = lane >= off && k == key;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const double t = __shfl_up(p[i], off);
            if (same)
                p[i] += t;
        }
    }
    const int next = __shfl_down(key, 1);
    if (key >= 0 && (lane == kWave - 1 || next != key)) {
#pragma unroll
        for (int i = 0; i < CPL; ++i)
            if (i < live)
                atomicAdd(&acc[key + i], p[i]);
    }
}

// One lane's CPL columns [j0, j0 + CPL) of one entry (column c, value v, block
// row r; r = -1: a lane past the stream's end).
// WIN = true: xs = X[lo .. lo + bound) x KV and acc of the same shape, both
// LDS; an entry whose row or column lies outside the window is dropped whole.
// WIN = false: xs = X of the block's rows and acc their kRbRows x KV sums,
// both LDS; X[c] comes from global memory, the mirrored products go straight
// into Y[c]; bound = n, a column outside [0, n) is dropped whole.
// Columns j >= live (a ragged last block of vectors) are neither read nor
// added.  The row products: KV <= 2 (one lane per entry) sums them per row
// across the wave first (wave_run_add_cols); from KV = 4 on (P lanes per
// entry) they are plain LDS adds, measured faster there
// (profiles/symmetric/README.md).
template <int KV, bool WIN>
__device__ __forceinline__ void sym_multi_add(const double *xs, double *acc, const double *__restrict__ X,
                                              int64_t ldx, double *__restrict__ Y, int64_t ldy, int64_t r0,
                                              int32_t lo, uint32_t bound, int32_t live, int j0, int32_t c, double v,
                                              int r)
{
    constexpr int P = t_multi_p<KV>();
    constexpr int CPL = KV / P;
    double p[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i)
        p[i] = 0.0;
    int key = -1;
    if constexpr (WIN) {
        const uint32_t jr = (uint32_t)(r0 + r) - (uint32_t)lo;
        const uint32_t jc = (uint32_t)c - (uint32_t)lo;
        if (r >= 0 && jr < bound) {
            key = (int)jr * KV + j0;
            if (jc < bound) {
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    const int j = j0 + i;
                    if (j < live) {
                        p[i] = v * xs[jc * KV + j];
                        if (jc != jr)
                            atomicAdd(&acc[jc * KV + j], v * xs[jr * KV + j]);
                    }
                }
            }
        }
    } else {
        if (r >= 0) {
            key = r * KV + j0;
            if ((uint32_t)c < bound) {
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    const int j = j0 + i;
                    if (j < live) {
                        p[i] = v * X[(int64_t)c * ldx + j];
                        if ((int64_t)c != r0 + r)
                            unsafeAtomicAdd(&Y[(int64_t)c * ldy + j], v * xs[r * KV + j]);
                    }
                }
            }
        }
    }
    if constexpr (P == 1) {
        wave_run_add_cols<CPL>(acc, key, p, live);
    } else if (key >= 0) {
#pragma unroll
        for (int i = 0; i < CPL; ++i)
            if (j0 + i < live)
                atomicAdd(&acc[key + i], p[i]);
    }
}

// The P rounds of one step, as t_multi_rounds (transpose.hip): round Q hands
// entry Q of every P-lane group to the group's P lanes.
template <int KV, bool WIN, int Q = 0>
__device__ __forceinline__ void sym_multi_rounds(const double *xs, double *acc, const double *__restrict__ X,
                                                 int64_t ldx, double *__restrict__ Y, int64_t ldy, int64_t r0,
                                                 int32_t lo, uint32_t bound, int32_t live, int j0, int32_t c,
                                                 double v, int r)
{
    constexpr int P = t_multi_p<KV>();
    if constexpr (P == 1) {
        sym_multi_add<KV, WIN>(xs, acc, X, ldx, Y, ldy, r0, lo, bound, live, j0, c, v, r);
    } else if constexpr (Q < P) {
        sym_multi_add<KV, WIN>(xs, acc, X, ldx, Y, ldy, r0, lo, bound, live, j0, group_bcast<P, Q>(c),
                               group_bcast<P, Q>(v), group_bcast<P, Q>(r));
        sym_multi_rounds<KV, WIN, Q + 1>(xs, acc, X, ldx, Y, ldy, r0, lo, bound, live, j0, c, v, r);
    }
}

// One workgroup per block of kRbRows rows, one pass over the block's entries
// for `live` <= KV vectors (X, Y: the pass's first column).  LDS: the block's
// kRbRows + 1 row offsets, then two arrays of span x KV doubles (X window,
// accumulator) when the union spans at most `cap` = kSMultiCap / KV columns,
// else two arrays of kRbRows x KV (the rows' X, their sums).  Every load of X
// and every add to Y is 8 bytes wide.
template <int KV>
__global__ __launch_bounds__(kBlock) void csr_sym_multi_kernel(int64_t n, const int64_t *__restrict__ ptr,
                                                               const int32_t *__restrict__ col,
                                                               const double *__restrict__ val,
                                                               const double *__restrict__ X, int64_t ldx,
                                                               double *__restrict__ Y, int64_t ldy,
                                                               const int2 *__restrict__ win, int32_t cap, int32_t live)
{
    extern __shared__ double s_mem[];
    int64_t *s_ptr = reinterpret_cast<int64_t *>(s_mem);
    double *xs = s_mem + kRbPtr;
    constexpr int P = t_multi_p<KV>();
    const int tid = (int)threadIdx.x;
    const int j0 = (tid % P) * (KV / P);
    RowBlock b;
    if (!rb_open(n, ptr, win, s_ptr, &b))
        return;
    const int2 w = b.w;
    const int span = b.span, nr = b.nr;
    const int64_t r0 = b.r0;
    // as csr_sym_window_kernel: a window this plan did not record is not used
    if (w.x < 0 || w.y >= n || w.x > r0 || w.y < r0 + nr - 1)
        return;
    const bool window = span <= cap;
    const int words = (window ? span : nr) * KV;
    const int64_t first = window ? (int64_t)w.x : r0;  // the row of X and Y that word 0 stands for
    double *acc = xs + (window ? span : kRbRows) * KV;
    for (int i = tid; i < words; i += kBlock) {
        const int j = i % KV;
        if (j < live)
            xs[i] = X[(first + i / KV) * ldx + j];
        acc[i] = 0.0;
    }
    __syncthreads();
    rb_stream<true>(s_ptr, nr, col, val, [&](bool mine, int64_t e, int32_t c, double v) {
        const int r = mine ? rb_row_of(s_ptr, nr, e) : -1;
        if (window)
            sym_multi_rounds<KV, true>(xs, acc, X, ldx, Y, ldy, r0, w.x, (uint32_t)span, live, j0, c, v, r);
        else
            sym_multi_rounds<KV, false>(xs, acc, X, ldx, Y, ldy, r0, 0, (uint32_t)n, live, j0, c, v, r);
    });
    __syncthreads();
    // the flush: thread t takes accumulator words t, t + 256, ...: with
    // ldy == KV a wave instruction covers 512 contiguous bytes of Y.  Sums
    // still exactly 0.0 add nothing to the zeroed Y.
    for (int i = tid; i < words; i += kBlock) {
        const int j = i % KV;
        const double s = acc[i];
        if (j < live && s != 0.0)
            unsafeAtomicAdd(&Y[(first + i / KV) * ldy + j], s);
    }
}

// ------------------------------------------------------------ expand mode
// Entry e of the CSR: its row (the last r with ptr[r] <= e) and whether it is
// off the diagonal; flag[nnz] = 0 closes the prefix sum.  A column outside
// [0, n) sets *bad.
__global__ void sym_flag_kernel(int64_t nnz, int64_t n, const int64_t *__restrict__ ptr,
                                const int32_t *__restrict__ col, int32_t *__restrict__ rowid,
                                int64_t *__restrict__ flag, int *__restrict__ bad)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= nnz; e += stride) {
        if (e == nnz) {
            flag[e] = 0;
            continue;
        }
        int64_t lo = 0, hi = n;  // ptr[lo] <= e < ptr[hi]
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (ptr[mid] <= e)
                lo = mid;
            else
                hi = mid;
        }
        const int32_t c = col[e];
        if (c < 0 || c >= n)
            *bad = 1;
        rowid[e] = (int32_t)lo;
        flag[e] = c != (int32_t)lo ? 1 : 0;
    }
}

// The symmetrized COO in spmv_coo_symmetrize's order: entry e at e, its mirror
// (off-diagonal entries only) at nnz + pos[e], pos = the exclusive prefix sum
// of the flags.
__global__ void sym_write_kernel(int64_t nnz, const int32_t *__restrict__ rowid, const int32_t *__restrict__ col,
                                 const double *__restrict__ val, const int64_t *__restrict__ pos,
                                 int32_t *__restrict__ row_out, int32_t *__restrict__ col_out,
                                 double *__restrict__ val_out)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride) {
        const int32_t r = rowid[e], c = col[e];
        const double v = val[e];
        row_out[e] = r;
        col_out[e] = c;
        val_out[e] = v;
        if (c != r) {
            const int64_t k = nnz + pos[e];
            row_out[k] = c;
            col_out[k] = r;
            val_out[k] = v;
        }
    }
}

namespace {

unsigned grid_for(int64_t n)
{
    const int64_t g = (n + kBlock - 1) / kBlock;
    return (unsigned)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

// transient device memory of a prepare: freed when it leaves scope (every
// user synchronises the stream first)
struct Scratch {
    void *p = nullptr;
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
    void release()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
    }
    ~Scratch() { release(); }
};

int s_alloc(SymState *s, void **dst, size_t bytes)
{
    return owned_alloc(dst, bytes, &s->owned, "spmv_plan_prepare_symmetric");
}

size_t fused_lds(int32_t xcap)
{
    return (size_t)(kRbPtr + 2 * (xcap > kRbRows ? xcap : kRbRows)) * sizeof(double);
}

// dynamic LDS bytes of a csr_sym_multi_kernel<kv> launch whose widest window
// block spans `span` columns (the wide path needs kRbRows x kv per array)
constexpr size_t sym_multi_lds(int kv, int64_t span)
{
    return (size_t)(kRbPtr + 2 * (span > kRbRows ? span : kRbRows) * kv) * sizeof(double);
}

int prepare_fused(const spmv_plan *p, SymState *s)
{
    const spmv_dims &d = p->d;
    const hipStream_t st = (hipStream_t)d.stream;
    const int64_t blocks = (d.n_rows + kRbRows - 1) / kRbRows;
    s->blocks = blocks;
    if (blocks == 0)  // a run does nothing
        return SPMV_SUCCESS;
    int rc = s_alloc(s, &s->win, (size_t)blocks * sizeof(int2));
    if (rc != SPMV_SUCCESS)
        return rc;
    hipLaunchKernelGGL(csr_sym_range_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, d.n_rows, d.nnz, p->ptr,
                       p->col, (int2 *)s->win);
    SPMV_CHECK_LAUNCH("csr_sym_range_kernel");
    int2 *h = nullptr;
    if ((rc = windows_download(s->win, blocks, st, &h, "spmv_plan_prepare_symmetric")) != SPMV_SUCCESS)
        return rc;
    const WindowTally fit = windows_tally(h, blocks, kSCap);
    s->win_blocks = fit.blocks;
    s->flush = fit.spans;
    s->xcap = fit.widest;
    for (int64_t b = 0; b < blocks; ++b)  // a wider union flushes the sums of the block's rows
        if ((int64_t)h[b].y - h[b].x + 1 > kSCap) {
            const int64_t r0 = b * kRbRows;
            s->flush += d.n_rows - r0 < kRbRows ? d.n_rows - r0 : kRbRows;
        }
    for (int w = 0; w < 4; ++w) {  // the multi-vector kernels: span * KV words per array
        const int32_t cap = kSMultiCap / kTWidths[w];
        const WindowTally multi = windows_tally(h, blocks, cap);
        s->mwin[w] = multi.blocks;
        s->mxcap[w] = multi.widest;
        s->mflush[w] = multi.spans;
        for (int64_t b = 0; b < blocks; ++b)
            if ((int64_t)h[b].y - h[b].x + 1 > cap) {
                const int64_t r0 = b * kRbRows;
                s->mflush[w] += d.n_rows - r0 < kRbRows ? d.n_rows - r0 : kRbRows;
            }
    }
    free(h);
    // a launch of the widest fitting window may need more than the default
    // 64 KiB of dynamic LDS: allowed here, once, so that a run only launches
    hipError_t e = hipSuccess;
    with_each_width([&](auto KV) {
        constexpr int kv = decltype(KV)::value;
        if (e == hipSuccess)
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(csr_sym_multi_kernel<kv>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)sym_multi_lds(kv, kSMultiCap / kv));
    });
    if (e != hipSuccess)
        return fail(SPMV_PROGRAM_ERROR, "spmv_plan_prepare_symmetric: dynamic LDS of csr_sym_multi_kernel", e);
    return SPMV_SUCCESS;
}

int prepare_expand(const spmv_plan *p, SymState *s)
{
    const spmv_dims &d = p->d;
    const hipStream_t st = (hipStream_t)d.stream;
    const int64_t n = d.n_rows, nnz = d.nnz;
    int rc;
    hipError_t e;
    int64_t off = 0;
    Scratch rowid, flag, pos, bad, tmp, c_row, c_col, c_val;
    if (nnz > 0) {
        if ((e = rowid.alloc((size_t)nnz * 4)) != hipSuccess || (e = flag.alloc((size_t)(nnz + 1) * 8)) != hipSuccess ||
            (e = pos.alloc((size_t)(nnz + 1) * 8)) != hipSuccess || (e = bad.alloc(sizeof(int))) != hipSuccess)
            return fail(SPMV_PROGRAM_ERROR, "spmv_plan_prepare_symmetric: scratch", e);
        if ((e = hipMemsetAsync(bad.p, 0, sizeof(int), st)) != hipSuccess)
            return fail(SPMV_PROGRAM_ERROR, "spmv_plan_prepare_symmetric: memset", e);
        hipLaunchKernelGGL(sym_flag_kernel, dim3(grid_for(nnz + 1)), dim3(kBlock), 0, st, nnz, n, p->ptr, p->col,
                           (int32_t *)rowid.p, (int64_t *)flag.p, (int *)bad.p);
        SPMV_CHECK_LAUNCH("sym_flag_kernel");
        size_t tbytes = 0;
        e = hipcub::DeviceScan::ExclusiveSum(nullptr, tbytes, (const int64_t *)flag.p, (int64_t *)pos.p, nnz + 1, st);
        if (e == hipSuccess)
            e = tmp.alloc(tbytes);
        if (e == hipSuccess)
            e = hipcub::DeviceScan::ExclusiveSum(tmp.p, tbytes, (const int64_t *)flag.p, (int64_t *)pos.p, nnz + 1, st);
        if (e != hipSuccess)
            return fail(SPMV_PROGRAM_ERROR, "spmv_plan_prepare_symmetric: prefix sum", e);
        int h_bad = 0;
        if ((e = hipMemcpyAsync(&off, (int64_t *)pos.p + nnz, sizeof off, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipMemcpyAsync(&h_bad, bad.p, sizeof h_bad, hipMemcpyDeviceToHost, st)) != hipSuccess ||
            (e = hipStreamSynchronize(st)) != hipSuccess)
            return fail(SPMV_PROGRAM_ERROR, "spmv_plan_prepare_symmetric: sync", e);
        if (h_bad)
            return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_prepare_symmetric: column index out of range");
        flag.release();  // the stream is idle: only rowid and pos are still needed
        tmp.release();
    }
    const int64_t nnz_a = nnz + off;
    s->nnz_a = nnz_a;
    if ((rc = s_alloc(s, (void **)&s->ptr, (size_t)(n + 1) * sizeof(int64_t))) != SPMV_SUCCESS ||
        (rc = s_alloc(s, (void **)&s->col, (size_t)nnz_a * sizeof(int32_t))) != SPMV_SUCCESS ||
        (rc = s_alloc(s, (void **)&s->val, (size_t)nnz_a * sizeof(double))) != SPMV_SUCCESS)
        return rc;
    spmv_dims da = d;
    da.nnz = nnz_a;
    if (nnz > 0) {
        if ((e = c_row.alloc((size_t)nnz_a * 4)) != hipSuccess || (e = c_col.alloc((size_t)nnz_a * 4)) != hipSuccess ||
            (e = c_val.alloc((size_t)nnz_a * 8)) != hipSuccess)
            return fail(SPMV_PROGRAM_ERROR, "spmv_plan_prepare_symmetric: scratch", e);
        hipLaunchKernelGGL(sym_write_kernel, dim3(grid_for(nnz)), dim3(kBlock), 0, st, nnz, (const int32_t *)rowid.p,
                           p->col, p->val, (const int64_t *)pos.p, (int32_t *)c_row.p, (int32_t *)c_col.p,
                           (double *)c_val.p);
        SPMV_CHECK_LAUNCH("sym_write_kernel");
    }
    // synchronises the stream: the transient buffers are idle when they go
    if ((rc = spmv_dev_csr_from_coo(da, (const int32_t *)c_row.p, (const int32_t *)c_col.p, (const double *)c_val.p,
                                    s->ptr, s->col, s->val)) != SPMV_SUCCESS)
        return rc;
    if ((rc = spmv_plan_csr(da, s->ptr, s->col, s->val, nullptr, &s->inner)) != SPMV_SUCCESS)
        return rc;
    // a balanced outer plan (spmv_plan_prepare_multi) extends to the inner one
    return p->m.mode != SPMV_M_NONE ? spmv_plan_prepare_multi(s->inner, p->m.mode, &p->m.req) : SPMV_SUCCESS;
}

int launch_fused(const spmv_plan *p, const double *x, double *y, hipStream_t st)
{
    const spmv_dims &d = p->d;
    const SymState &s = p->sym;
    if (d.n_rows == 0)
        return SPMV_SUCCESS;
    hipError_t e = hipMemsetAsync(y, 0, (size_t)d.n_rows * sizeof(double), st);
    if (e != hipSuccess)
        return fail(SPMV_PROGRAM_ERROR, "spmv_plan_run_sym: memset", e);
    if (!s.win || d.nnz == 0)
        return SPMV_SUCCESS;
    hipLaunchKernelGGL(csr_sym_window_kernel, dim3((unsigned)s.blocks), dim3(kBlock), fused_lds(s.xcap), st, d.n_rows,
                       p->ptr, p->col, p->val, x, y, (const int2 *)s.win, kSCap);
    SPMV_CHECK_LAUNCH("csr_sym_window_kernel");
    return SPMV_SUCCESS;
}

// Y zeroed once (columns j < k only), then ceil(k/8) passes of the narrowest
// kernel that holds the pass's vectors
int launch_fused_multi(const spmv_plan *p, int32_t k, const double *X, int64_t ldx, double *Y, int64_t ldy,
                       hipStream_t st)
{
    const spmv_dims &d = p->d;
    const SymState &s = p->sym;
    const int rc = zero_cols(d.n_rows, k, Y, ldy, st, "spmv_plan_run_sym_multi");
    if (rc != SPMV_SUCCESS)
        return rc;
    if (!s.win || d.nnz == 0 || d.n_rows == 0)
        return SPMV_SUCCESS;
    for (int32_t j0 = 0; j0 < k; j0 += 8) {
        const int32_t live = k - j0 < 8 ? k - j0 : 8;
        const int w = live > 4 ? 3 : live > 2 ? 2 : live - 1;  // width kTWidths[w] >= live
        with_int<1, 2, 4, 8>(kTWidths[w], [&](auto KV) {
            constexpr int kv = decltype(KV)::value;
            hipLaunchKernelGGL(csr_sym_multi_kernel<kv>, dim3((unsigned)s.blocks), dim3(kBlock),
                               sym_multi_lds(kv, s.mxcap[w]), st, d.n_rows, p->ptr, p->col, p->val, X + j0, ldx,
                               Y + j0, ldy, (const int2 *)s.win, kSMultiCap / kv, live);
        });
        SPMV_CHECK_LAUNCH("csr_sym_multi_kernel");
    }
    return SPMV_SUCCESS;
}

}  // namespace

void plan_symmetric_free(spmv_plan *p) { mode_state_free(&p->sym); }

}  // namespace spmv

using namespace spmv;

extern "C" {

int spmv_plan_symmetric_supported(const spmv_plan *p)
{
    return p && p->fmt == SPMV_FMT_CSR && p->d.n_rows == p->d.n_cols ? 1 : 0;
}

int spmv_plan_prepare_symmetric(spmv_plan *p, int mode)
{
    if (!p)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_prepare_symmetric: plan is NULL");
    if (mode != SPMV_S_NONE && mode != SPMV_S_FUSED && mode != SPMV_S_EXPAND)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_prepare_symmetric: unknown mode");
    if (p->fmt != SPMV_FMT_CSR)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_prepare_symmetric: only CSR plans have a symmetric run");
    if (p->d.n_rows != p->d.n_cols)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_prepare_symmetric: the matrix is not square");
    if (mode == p->sym.mode)
        return SPMV_SUCCESS;
    if (p->d.n_rows > INT32_MAX)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_prepare_symmetric: row ids are int32");
    SPMV_GUARD(p->d);
    const hipStream_t st = (hipStream_t)p->d.stream;
    SymState next;
    int rc = SPMV_SUCCESS;
    if (mode != SPMV_S_NONE) {
        rc = mode == SPMV_S_FUSED ? prepare_fused(p, &next) : prepare_expand(p, &next);
        // runs may come on any stream: everything is complete when this returns
        if (rc == SPMV_SUCCESS && hipStreamSynchronize(st) != hipSuccess)
            rc = fail_msg(SPMV_PROGRAM_ERROR, "spmv_plan_prepare_symmetric: synchronise");
        if (rc != SPMV_SUCCESS)  // the plan stays as it was
            return fail_after(rc, [&] {
                (void)hipStreamSynchronize(st);
                mode_state_free(&next);
            });
        next.mode = mode;
    }
    // a run of the old mode may still be in flight on the build stream
    if (p->sym.mode != SPMV_S_NONE && hipStreamSynchronize(st) != hipSuccess) {
        mode_state_free(&next);
        return fail_msg(SPMV_PROGRAM_ERROR, "spmv_plan_prepare_symmetric: synchronise");
    }
    mode_state_free(&p->sym);
    p->sym = next;
    return SPMV_SUCCESS;
}

int spmv_plan_get_symmetric_info(const spmv_plan *p, spmv_symmetric_info *info)
{
    if (!p || !info)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_get_symmetric_info: NULL argument");
    memset(info, 0, sizeof *info);
    const SymState &s = p->sym;
    info->mode = s.mode;
    info->owned_bytes = (int64_t)(s.owned + (s.inner ? s.inner->owned : 0));
    if (s.mode == SPMV_S_FUSED) {
        info->cap = kSCap;
        info->blocks = s.blocks;
        info->window_blocks = s.win_blocks;
        info->flush_entries = s.flush;
        snprintf(info->kernel, sizeof info->kernel, "csr_sym_window_kernel");
    } else if (s.inner) {
        info->nnz_expanded = s.nnz_a;
        snprintf(info->kernel, sizeof info->kernel, "%s", s.inner->kernel);
    }
    return SPMV_SUCCESS;
}

int spmv_plan_get_symmetric_arrays(const spmv_plan *p, const int64_t **row_ptr, const int32_t **col,
                                   const double **val, int64_t *nnz)
{
    if (!p || !row_ptr || !col || !val || !nnz)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_get_symmetric_arrays: NULL argument");
    if (p->sym.mode != SPMV_S_EXPAND)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_get_symmetric_arrays: the plan is not in SPMV_S_EXPAND mode");
    *row_ptr = p->sym.ptr;
    *col = p->sym.col;
    *val = p->sym.val;
    *nnz = p->sym.nnz_a;
    return SPMV_SUCCESS;
}

int spmv_plan_run_sym(const spmv_plan *p, const double *x, double *y, void *stream)
{
    if (!p)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_sym: plan is NULL");
    if (p->sym.mode == SPMV_S_NONE)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_sym: the plan was not prepared (spmv_plan_prepare_symmetric)");
    if (p->d.n_rows > 0 && (!x || !y))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_sym: x or y is NULL");
    if (p->sym.mode == SPMV_S_EXPAND)
        return spmv_plan_run(p->sym.inner, x, y, stream);
    SPMV_GUARD(p->d);
    return launch_fused(p, x, y, (hipStream_t)stream);
}

int spmv_plan_get_symmetric_multi_info(const spmv_plan *p, spmv_symmetric_multi_info *info)
{
    if (!p || !info)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_get_symmetric_multi_info: NULL argument");
    memset(info, 0, sizeof *info);
    const SymState &s = p->sym;
    info->mode = s.mode;
    if (s.mode == SPMV_S_FUSED) {
        for (int w = 0; w < 4; ++w) {
            info->cap_cols[w] = kSMultiCap / kTWidths[w];
            info->window_blocks[w] = s.mwin[w];
            info->flush_entries[w] = s.mflush[w];
        }
        snprintf(info->kernel, sizeof info->kernel, "csr_sym_multi_kernel");
    } else if (s.inner) {
        const MultiBalance &bal = s.inner->m.bal;
        info->long_rows = bal.n_long;
        info->segments = bal.n_seg;
        info->multi_owned_bytes = (int64_t)s.inner->m.owned;
        snprintf(info->kernel, sizeof info->kernel, "%s", bal.n_seg > 0 ? "csr_multi_long_kernel" : "csr_multi_kernel");
    }
    return SPMV_SUCCESS;
}

int spmv_plan_run_sym_multi(const spmv_plan *p, int32_t k, const double *X, int64_t ldx, double *Y, int64_t ldy,
                            void *stream)
{
    if (!p)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_sym_multi: plan is NULL");
    if (p->sym.mode == SPMV_S_NONE)
        return fail_msg(SPMV_OTHER_ERROR,
                        "spmv_plan_run_sym_multi: the plan was not prepared (spmv_plan_prepare_symmetric)");
    if (k < 1)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_sym_multi: k must be at least 1");
    if (ldx < k || ldy < k)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_sym_multi: ldx and ldy must be at least k");
    if (p->d.n_rows > 0 && (!X || !Y))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_sym_multi: X or Y is NULL");
    if (p->sym.mode == SPMV_S_EXPAND)
        return spmv_plan_run_multi(p->sym.inner, k, X, ldx, Y, ldy, stream);
    SPMV_GUARD(p->d);
    return launch_fused_multi(p, k, X, ldx, Y, ldy, (hipStream_t)stream);
}

}  // extern "C"
