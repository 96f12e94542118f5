// bsr.hip — block CSR (BSR) with 2x2, 3x3 and 4x4 blocks: spmv_plan_bsr's
// kernel and the one-call form spmv_bsr_run (include/spmv.h, spmv_ext.h; the
// layout and the fill-in rule are stated in include/spmv_host.h).
//
// One int32 column per b x b block: 8 + 4/b^2 bytes per stored value instead
// of CSR's 12.  A block is b^2 * 8 bytes (72 at b = 3: neither a power of two
// nor a multiple of 16), so a lane walking its own block by strided 8-byte
// loads would spread every load instruction of a wave over dozens of cache
// lines.  Instead the kernel streams bval and bcol FLAT, as the staged CSR
// kernels stream val and col: a workgroup owns 256/L whole block rows, i.e.
// one contiguous range of blocks, cut into chunks of kBsrChunk blocks; all 256
// lanes load a chunk's values as wave-contiguous 16-byte pairs (and one column
// per lane) into LDS; after one barrier each L-lane group walks its block
// row's blocks of the chunk, lane k taking blocks k, k + L, ..., with the b
// values of x by 8-byte loads from global memory / L2 and b accumulators per
// lane that stay in registers across chunks; at the end group_sum reduces
// each scalar row over the lane group.  No atomics, a fixed summation order.
#include <stdio.h>

#include "common.h"

namespace spmv {

// Blocks per LDS chunk: one block column per lane of the workgroup.  LDS per
// workgroup: 256 * (b^2 [+ 1 pad]) * 8 + 1 KiB of columns + the offsets =
// 11.5 / 19.5 / 36 KiB at b = 2 / 3 / 4.  (tests/test_bsr_gpu.py mirrors it.)
constexpr int kBsrChunk = 256;
// Chunks start on a multiple of kBsrChunkAlign blocks at or before the
// workgroup's first block (up to 31 blocks of the previous workgroup are
// loaded and never summed): the first value's offset c0 * b^2 is then even
// (16-byte pairs) and the 4-byte columns start on a 128-byte line.
constexpr int64_t kBsrChunkAlign = 32;
// The lane rule (spmv_bsr_auto_lanes): about one lane per kBsrBlocksPerLane
// blocks of the mean block row, a power of two in [2, 64].  More lanes mean
// fewer block rows, hence fewer chunks, per workgroup and more workgroups:
// cant-like at b = 3 (23 blocks per block row), cold, one matrix / the 32-copy
// batch: L = 2 60.5 us / 0.349 ms, 4 29.4 / 0.263, 8 17.0 / 0.222, 16 12.2 /
// 0.211 (profiles/bsr/README.md); 2 blocks per lane gives 16 there.  Never
// fewer than kBsrMinLanes: block_congruence(128, 3), 5 blocks per block row,
// 9.9 us at L = 2 (three chunks per workgroup), 5.0 at 8, 7.8 at 32.
constexpr int kBsrBlocksPerLane = 2;
constexpr int kBsrMinLanes = 8;
// temporal matrix loads: 0.2224 vs 0.2320 ms non-temporal on the cant-like
// batch (L = 8, profiles/bsr/README.md), as the staged persistent CSR kernel,
// which also gathers x from global memory / L2 (kCsrStreamNtDefault)
constexpr bool kBsrStreamNtDefault = false;

template <int B, int L, bool NT>
__global__ __launch_bounds__(kBlock) void bsr_kernel(int64_t n_rows, int32_t n_cols, int64_t n_brows, int64_t n_blocks,
                                                     const int64_t *__restrict__ brow_ptr,
                                                     const int32_t *__restrict__ bcol,
                                                     const double *__restrict__ bval, const double *__restrict__ x,
                                                     double *__restrict__ y, int remap)
{
    constexpr int BB = B * B;
    constexpr int RPB = kBlock / L;  // block rows per workgroup
    // even block sizes: one pad double per block, else the lanes of a group
    // read their blocks at a stride of 8 (b = 2) or 32 (b = 4) LDS banks
    constexpr int PAD = B % 2 == 0 ? 1 : 0;
    constexpr int STRIDE = BB + PAD;
    constexpr int PAIRS = kBsrChunk * BB / 2;               // 16-byte pairs of a chunk
    constexpr int ROUNDS = (PAIRS + kBlock - 1) / kBlock;  // pairs per lane
    __shared__ int64_t s_ptr[RPB + 1];
    __shared__ double s_val[kBsrChunk * STRIDE];
    __shared__ int32_t s_col[kBsrChunk];

    const int tid = threadIdx.x;
    const int64_t brow0 = xcd_block(remap) * RPB;
    if (tid <= RPB) {
        const int64_t r = brow0 + tid;
        s_ptr[tid] = brow_ptr[r < n_brows ? r : n_brows];
    }
    __syncthreads();

    const int g = tid / L, lane = tid % L;
    const int64_t beg = s_ptr[g], end = s_ptr[g + 1];  // empty past n_brows
    const int64_t gbeg = s_ptr[0], gend = s_ptr[RPB];
    const int64_t nval = n_blocks * BB;
    double acc[B];
#pragma unroll
    for (int r = 0; r < B; ++r)
        acc[r] = 0.0;

    for (int64_t c0 = gbeg & ~(kBsrChunkAlign - 1); c0 < gend; c0 += kBsrChunk) {
        const int64_t cend = c0 + kBsrChunk < gend ? c0 + kBsrChunk : gend;
        // values [c0 * BB, lim): whole pairs up to the chunk's (even-rounded)
        // end, never past the array; an odd array end is one 8-byte load
        const int64_t e0 = c0 * BB;
        int64_t lim = (cend * BB + 1) & ~(int64_t)1;
        lim = lim < nval ? lim : nval;
        double2 v[ROUNDS];
#pragma unroll
        for (int k = 0; k < ROUNDS; ++k) {
            const int p = tid + k * kBlock;
            const int64_t e = e0 + 2 * (int64_t)p;
            v[k] = double2{0.0, 0.0};
            if (p < PAIRS) {
                if (e + 1 < lim)
                    v[k] = stream_load2<NT>(bval + e);
                else if (e < lim)
                    v[k].x = stream_load<NT>(bval + e);
            }
        }
        const int32_t c = c0 + tid < cend ? stream_load<NT>(bcol + c0 + tid) : 0;
#pragma unroll
        for (int k = 0; k < ROUNDS; ++k) {
            const int p = tid + k * kBlock;
            if (p < PAIRS) {
                const int f0 = 2 * p, f1 = 2 * p + 1;  // chunk-relative value
                s_val[f0 + f0 / BB * PAD] = v[k].x;
                s_val[f1 + f1 / BB * PAD] = v[k].y;
            }
        }
        s_col[tid] = c;
        __syncthreads();

        const int64_t lo = beg > c0 ? beg : c0, hi = end < cend ? end : cend;
        for (int64_t j = lo + lane; j < hi; j += L) {
            const int jj = (int)(j - c0);
            const int32_t col0 = s_col[jj] * B;
            const double *blk = s_val + jj * STRIDE;
            double xv[B];
            // a partial last block column is guarded, never read past the
            // end and never hidden behind its stored 0.0
#pragma unroll
            for (int cc = 0; cc < B; ++cc)
                xv[cc] = col0 + cc < n_cols ? x[col0 + cc] : 0.0;
#pragma unroll
            for (int r = 0; r < B; ++r)
#pragma unroll
                for (int cc = 0; cc < B; ++cc)
                    acc[r] += blk[r * B + cc] * xv[cc];
        }
        __syncthreads();
    }

    const int64_t row0 = (brow0 + g) * B;
#pragma unroll
    for (int r = 0; r < B; ++r) {
        const double s = group_sum<L>(acc[r]);
        if (lane == 0 && row0 + r < n_rows)
            store_y(y + row0 + r, s);
    }
}

static bool bsr_lanes_ok(int L) { return L >= 2 && L <= 64 && (L & (L - 1)) == 0; }

const char *bsr_refusal(const spmv_dims &d, int32_t b, int64_t n_brows, const int64_t *brow_ptr, const int32_t *bcol,
                        const double *bval)
{
    if (d.n_rows < 0 || d.n_cols < 0 || d.nnz < 0 || n_brows < 0)
        return "negative sizes";
    if (b < 2 || b > 4)
        return "the block size b must be 2, 3 or 4";
    if (n_brows != (d.n_rows + b - 1) / b)
        return "n_brows must be ceil(n_rows / b)";
    if (d.nnz % (b * b))
        return "d.nnz (the stored values) must be a multiple of b*b";
    if (d.n_cols > (int64_t)INT32_MAX - 8)
        return "n_cols must be at most INT32_MAX - 8";
    if ((n_brows > 0 && !brow_ptr) || (d.nnz > 0 && (!bcol || !bval)))
        return "NULL array";
    return nullptr;
}

int launch_bsr(const spmv_dims &d, int32_t b, int64_t n_brows, const int64_t *brow_ptr, const int32_t *bcol,
               const double *bval, const double *x, double *y, int L)
{
    if (!bsr_lanes_ok(L))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_bsr_run: lanes must be 0 or a power of two in [2,64]");
    if (n_brows == 0)
        return SPMV_SUCCESS;
    const int64_t rpb = kBlock / L, blocks = (n_brows + rpb - 1) / rpb;
    if (blocks > INT32_MAX)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_bsr_run: too many block rows");
    SPMV_GUARD(d);
    const int64_t n_blocks = d.nnz / (b * b);
    const int remap = xcd_remap_enabled() ? 1 : 0;
    with_int<2, 3, 4>(b, [&](auto Bc) {
        with_int<2, 4, 8, 16, 32, 64>(L, [&](auto Lc) {
            with_bool(stream_nt(kBsrStreamNtDefault), [&](auto Nt) {
                hipLaunchKernelGGL((bsr_kernel<decltype(Bc)::value, decltype(Lc)::value, decltype(Nt)::value>),
                                   dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)d.stream, d.n_rows,
                                   (int32_t)d.n_cols, n_brows, n_blocks, brow_ptr, bcol, bval, x, y, remap);
            });
        });
    });
    SPMV_CHECK_LAUNCH("bsr kernel");
    return SPMV_SUCCESS;
}

}  // namespace spmv

using namespace spmv;

extern "C" int spmv_bsr_auto_lanes(int64_t n_brows, int64_t n_blocks)
{
    const double mean = n_brows > 0 ? (double)n_blocks / (double)n_brows : 0.0;
    int L = kBsrMinLanes;
    while (L < 64 && (double)(2 * L) * kBsrBlocksPerLane <= mean * 1.5)
        L *= 2;
    return L;
}

extern "C" int spmv_bsr_run(spmv_dims d, int32_t b, int64_t n_brows, const int64_t *brow_ptr, const int32_t *bcol,
                            const double *bval, const double *x, double *y, int lanes)
{
    if (const char *why = bsr_refusal(d, b, n_brows, brow_ptr, bcol, bval)) {
        static thread_local char msg[128];
        snprintf(msg, sizeof msg, "spmv_bsr_run: %s", why);
        return fail_msg(SPMV_OTHER_ERROR, msg);
    }
    if ((d.n_rows > 0 && !y) || (d.nnz > 0 && d.n_cols > 0 && !x))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_bsr_run: x or y is NULL");
    const int L = lanes > 0 ? lanes : spmv_bsr_auto_lanes(n_brows, d.nnz / (b * b));
    return launch_bsr(d, b, n_brows, brow_ptr, bcol, bval, x, y, L);
}
