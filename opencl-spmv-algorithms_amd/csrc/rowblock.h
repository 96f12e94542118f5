// rowblock.h — the device core of the runs that work on blocks of 128 CSR
// rows: the transposed scatter kernels (transpose.hip) and the fused symmetric
// kernel (symmetric.hip).  One workgroup per block stages the block's row
// offsets in LDS and streams its entries ONCE, coalesced, whatever the row
// lengths; what is done with an entry (the per-entry body) and the LDS budget
// of each kernel stay in its own file.  The lane geometry the multi-vector
// kernels of both files share (lanes per entry, DPP broadcast) is at the end.
#pragma once

#include <type_traits>

#include "common.h"

namespace spmv {

constexpr int kRbRows = 128;         // rows per block (the forward x-window default)
constexpr int kRbPtr = kRbRows + 2;  // LDS slots of the block's kRbRows + 1 row offsets (a 16-byte multiple)
constexpr int kRbU = 4;              // entries in flight per thread

// What a workgroup knows of its block after rb_open.
struct RowBlock {
    int2 w;      // the recorded window {lo, hi} of the block
    int span;    // hi - lo + 1
    int64_t r0;  // first row
    int nr;      // rows (kRbRows but for the last block)
};

// The block prologue: reads the block's window, returns false (uniform per
// workgroup) for a block without entries (span <= 0), else fills *b and copies
// the block's nr + 1 row offsets into s_ptr.  No barrier: the caller stages
// its own arrays first.
__device__ __forceinline__ bool rb_open(int64_t n_rows, const int64_t *__restrict__ ptr,
                                        const int2 *__restrict__ win, int64_t *s_ptr, RowBlock *b)
{
    b->w = win[blockIdx.x];
    b->span = b->w.y - b->w.x + 1;
    if (b->span <= 0)
        return false;
    b->r0 = (int64_t)blockIdx.x * kRbRows;
    b->nr = (int)(n_rows - b->r0 < kRbRows ? n_rows - b->r0 : kRbRows);
    for (int i = (int)threadIdx.x; i <= b->nr; i += kBlock)
        s_ptr[i] = ptr[b->r0 + i];
    return true;
}

// The block row of entry e: the last r with s_ptr[r] <= e, a fixed-depth
// (7-step) binary search of the offsets in LDS.
__device__ __forceinline__ int rb_row_of(const int64_t *s_ptr, int nr, int64_t e)
{
    int r = 0;
#pragma unroll
    for (int step = kRbRows / 2; step > 0; step >>= 1)
        if (r + step < nr && s_ptr[r + step] <= e)
            r += step;
    return r;
}

// The block's entries [s_ptr[0], s_ptr[nr]) as ONE coalesced non-temporal
// stream: thread t takes entries t, t + 256, ... with kRbU col/val loads in
// flight (a lane group per row waits out one memory round trip per row: 39 us
// instead of 28 on the cant-like matrix, profiles/transpose/README.md), then a
// tail of single steps.  Every entry is handed to body(live, e, c, v).
// UNIFORM = false: per-thread loops; a thread leaves when its entries end and
// live is always true.
// UNIFORM = true: the loops are uniform over the workgroup, for bodies that
// move data across lanes (wave shuffles, DPP) and need whole waves: in the
// last partial step a lane past the end calls body(false, e, -1, 0.0).
template <bool UNIFORM, typename Body>
__device__ __forceinline__ void rb_stream(const int64_t *s_ptr, int nr, const int32_t *__restrict__ col,
                                          const double *__restrict__ val, Body &&body)
{
    const int64_t end = s_ptr[nr];
    if constexpr (UNIFORM) {
        int64_t e0 = s_ptr[0];  // uniform
        for (; e0 + kRbU * kBlock <= end; e0 += kRbU * kBlock) {
            const int64_t e = e0 + (int64_t)threadIdx.x;
            int32_t c[kRbU];
            double v[kRbU];
#pragma unroll
            for (int u = 0; u < kRbU; ++u) {
                c[u] = stream_load<true>(col + e + u * kBlock);
                v[u] = stream_load<true>(val + e + u * kBlock);
            }
#pragma unroll
            for (int u = 0; u < kRbU; ++u)
                body(true, e + u * kBlock, c[u], v[u]);
        }
        for (; e0 < end; e0 += kBlock) {
            const int64_t e = e0 + (int64_t)threadIdx.x;
            const bool live = e < end;
            int32_t c = -1;
            double v = 0.0;
            if (live) {
                c = stream_load<true>(col + e);
                v = stream_load<true>(val + e);
            }
            body(live, e, c, v);
        }
    } else {
        int64_t e = s_ptr[0] + (int64_t)threadIdx.x;
        for (; e + (kRbU - 1) * kBlock < end; e += kRbU * kBlock) {
            int32_t c[kRbU];
            double v[kRbU];
#pragma unroll
            for (int u = 0; u < kRbU; ++u) {
                c[u] = stream_load<true>(col + e + u * kBlock);
                v[u] = stream_load<true>(val + e + u * kBlock);
            }
#pragma unroll
            for (int u = 0; u < kRbU; ++u)
                body(true, e + u * kBlock, c[u], v[u]);
        }
        for (; e < end; e += kBlock)
            body(true, e, stream_load<true>(col + e), stream_load<true>(val + e));
    }
}

// The flush of a single-vector LDS accumulator: acc[0 .. span) added to the
// zeroed y[lo .. lo + span), consecutive lanes on consecutive columns (256
// contiguous bytes per wave instruction, the shape global float atomics run at
// full rate); sums still exactly 0.0 add nothing.
__device__ __forceinline__ void rb_flush(const double *acc, int span, double *__restrict__ y, int32_t lo)
{
    for (int j = (int)threadIdx.x; j < span; j += kBlock) {
        const double s = acc[j];
        if (s != 0.0)
            unsafeAtomicAdd(&y[lo + j], s);
    }
}

// ---- the lane geometry of the multi-vector kernels on this core
// (csr_t_multi_kernel<KV>, csr_sym_multi_kernel<KV>; KV = vectors per pass)
constexpr int kTWidths[4] = {1, 2, 4, 8};

// lanes that share one entry: two columns per lane from KV = 4 on, as
// csr_multi_kernel; the P lanes of an entry are neighbours inside one quad
template <int KV>
constexpr int t_multi_p()
{
    return KV >= 4 ? KV / 2 : 1;
}

// The value of lane Q of every P-lane group (P = 2 or 4, groups aligned inside
// a quad) by a DPP quad_perm move: a VALU operand modifier, no LDS traffic.
// Called in uniform control flow only (every lane of the wave active).
template <int P, int Q>
constexpr int group_bcast_ctrl()
{
    static_assert((P == 2 || P == 4) && Q < P, "groups inside one quad");
    return P == 4 ? Q * 0x55 : (Q | Q << 2 | (2 + Q) << 4 | (2 + Q) << 6);
}

template <int P, int Q>
__device__ __forceinline__ int group_bcast(int v)
{
    return __builtin_amdgcn_mov_dpp(v, group_bcast_ctrl<P, Q>(), 0xF, 0xF, false);
}

template <int P, int Q>
__device__ __forceinline__ double group_bcast(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = group_bcast<P, Q>((int)b);
    const int hi = group_bcast<P, Q>((int)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

template <typename F>
inline void with_each_width(F &&f)
{
    f(std::integral_constant<int, 1>{});
    f(std::integral_constant<int, 2>{});
    f(std::integral_constant<int, 4>{});
    f(std::integral_constant<int, 8>{});
}

}  // namespace spmv
