// spmm.hip — multi-vector SpMV Y = A·X for gfx950 (spmv_plan_run_multi,
// include/spmv.h): k vectors stored row-major, X[c*ldx + j], Y[i*ldy + j].
//
// Every SpMV kernel here is bound by the matrix stream, so k separate runs
// read val/col k times.  These kernels read each entry ONCE per block of up
// to 8 vectors and gather the KV values of X row `col` (KV·8 contiguous
// bytes instead of one scattered double).  Kernels exist for KV = 1, 2, 4,
// 8; a block of r < KV remaining vectors clamps the loads of its unused
// accumulator columns to the block's last live column and never stores them.
//
// Lane layout: P neighbouring lanes share one entry (CSR: one of the row's L
// entry lanes; SELL/ELL: one row slot) and own CPL = KV / P columns each, two
// where the wave has room (P = KV / 2), so a wave's load instruction reads
// each X row as ONE contiguous piece (16 bytes per lane) instead of KV/2
// instructions that each touch every row: the X gathers, not HBM, bound
// these kernels.  The P lanes load the same val/col (one address, merged).
//
// The bit rule: column j's sum is one accumulator per entry lane, fed by
// explicit fma()s in entry order, then (CSR) the xor butterfly over the L
// entry lanes.  That order does not depend on KV, P, j's place in the block
// or the access path, so output column j has the same bits for every k, ldx,
// ldy and alignment.  The loops below only batch LOADS (E entries in
// flight); the fma order per column is always entry by entry.
//
// Balanced mode (spmv_plan_prepare_multi, CSR): csr_multi_kernel<.., BAL> leaves
// the rows of more than long_len entries to csr_multi_long_kernel (16 entry
// lanes per segment of at most seg_len entries, the same per-lane fma order
// and butterfly) and csr_multi_finish_kernel (a split row's partial sums,
// added in segment order).  No atomics: the order is fixed by the plan, so the
// bit rule holds there too; rows up to long_len keep the unprepared bits.
//
// Access paths (VEC): 16-byte loads of X rows and stores of Y rows are used
// only for a full block (r == KV >= 2) whose X (and, where Y is stored in
// pairs, Y) rows the host has proven 16-byte aligned (base address and
// leading dimension); everything else runs the 8-byte path, which also
// clamps the masked columns.
#include <stdio.h>

#include "common.h"

namespace spmv {

// lanes that share one entry: KV / 2 (two columns per lane), at most MAXP
template <int KV, int MAXP>
constexpr int multi_p()
{
    constexpr int p = KV / 2 > 0 ? KV / 2 : 1;
    return p < MAXP ? p : MAXP;
}

// entries a lane keeps in flight (loads issued before the first fma): the
// x values of E entries are E·CPL doubles of registers
template <int CPL>
constexpr int multi_inflight()
{
    return CPL >= 8 ? 2 : CPL >= 4 ? 4 : 8;
}

// A lane's CPL columns [j0, j0 + CPL) of one X row (xr = X + c*ldx, block
// relative).  VEC: aligned 16-byte pairs of a full block.  Otherwise 8-byte
// loads, column j >= r clamped to r-1 (the block's last live column: nothing
// outside the row's k values is read).
template <int CPL, bool VEC>
__device__ __forceinline__ void load_xcols(const double *__restrict__ xr, int j0, int32_t r, double (&x)[CPL])
{
    if constexpr (VEC) {
        static_assert(CPL % 2 == 0, "16-byte path needs whole pairs");
#pragma unroll
        for (int i = 0; i < CPL; i += 2) {
            const v2f64 v = *reinterpret_cast<const v2f64 *>(xr + j0 + i);
            x[i] = v.x;
            x[i + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < CPL; ++i)
            x[i] = xr[j0 + i < r ? j0 + i : r - 1];
    }
}

// group_sum<L> over entry lanes that sit P lanes apart (lane = l*P + p): the
// same xor butterfly, offsets L/2 ... 1 in l, hence the same bits for every P.
template <int L, int P>
__device__ __forceinline__ double entry_lane_sum(double v)
{
    if constexpr (P == 1) {
        return group_sum<L>(v);
    } else {
#pragma unroll
        for (int off = L / 2; off > 0; off >>= 1)
            v += __shfl_xor(v, off * P);
        return v;
    }
}

// The sums of one lane group over the entries e, e + L, ... < end (e = the
// group's first entry + the entry lane l): one accumulator per column, fed by
// one fma per entry in that order, E entries' loads in flight; then the
// butterfly over the L entry lanes.  Whole waves call it (the butterfly moves
// data between lanes); a group without work passes e >= end.  Shared by the
// row kernel (L from the plan) and the segment kernel (L = 16).  The pointers
// are the kernels' __restrict__ arguments; they are NOT qualified again here:
// a second noalias scope changes the schedule of the instantiations with one
// wave per row (unprepared lanes = 64 runs measured 7-11 % slower with it).
template <int L, int KV, bool VEC>
__device__ __forceinline__ void multi_group_sums(int64_t e, int64_t end, const int32_t *col, const double *val,
                                                 const double *X, int64_t ldx, int j0, int32_t r,
                                                 double (&acc)[KV / multi_p<KV, kWave / L>()])
{
    constexpr int P = multi_p<KV, kWave / L>();
    constexpr int CPL = KV / P;
    constexpr int E = multi_inflight<CPL>();
#pragma unroll
    for (int i = 0; i < CPL; ++i)
        acc[i] = 0.0;

    for (; e + (int64_t)(E - 1) * L < end; e += (int64_t)E * L) {
        double v[E];
        int32_t c[E];
        double x[E][CPL];
#pragma unroll
        for (int u = 0; u < E; ++u) {
            v[u] = val[e + u * L];
            c[u] = col[e + u * L];
        }
#pragma unroll
        for (int u = 0; u < E; ++u)
            load_xcols<CPL, VEC>(X + (int64_t)c[u] * ldx, j0, r, x[u]);
#pragma unroll
        for (int u = 0; u < E; ++u) {
#pragma unroll
            for (int i = 0; i < CPL; ++i)
                acc[i] = fma(v[u], x[u][i], acc[i]);
        }
    }
    for (; e < end; e += L) {
        const double v = val[e];
        double x[CPL];
        load_xcols<CPL, VEC>(X + (int64_t)col[e] * ldx, j0, r, x);
#pragma unroll
        for (int i = 0; i < CPL; ++i)
            acc[i] = fma(v, x[i], acc[i]);
    }

    // every lane of the workgroup gets here: whole waves run the butterfly
#pragma unroll
    for (int i = 0; i < CPL; ++i)
        acc[i] = entry_lane_sum<L, P>(acc[i]);
}

// CSR: L entry lanes own one row (as csr_vector_kernel); entry lane l takes
// entries beg+l, beg+l+L, ... in that order; each entry lane is P lanes with
// CPL columns each (L·P <= 64).  The sums are reduced over the entry lanes;
// entry lane 0's P lanes store the row.  BAL (a plan prepared with
// SPMV_M_BALANCED): a row of more than long_len entries belongs to
// csr_multi_long_kernel; this kernel sums nothing for it and stores nothing.
template <int L, int KV, bool VEC, bool BAL>
__global__ __launch_bounds__(kBlock) void csr_multi_kernel(
    int64_t n_rows, const int64_t *__restrict__ row_ptr, const int32_t *__restrict__ col,
    const double *__restrict__ val, const double *__restrict__ X, int64_t ldx, double *__restrict__ Y,
    int64_t ldy, int32_t r, int32_t long_len)
{
    constexpr int P = multi_p<KV, kWave / L>();
    constexpr int CPL = KV / P;      // columns per lane
    constexpr int G = L * P;         // lanes per row
    constexpr int RPB = kBlock / G;  // rows per workgroup
    __shared__ int64_t s_ptr[RPB + 1];

    const int64_t row0 = (int64_t)blockIdx.x * RPB;
    if (threadIdx.x <= RPB) {
        const int64_t rr = row0 + threadIdx.x;
        s_ptr[threadIdx.x] = row_ptr[rr < n_rows ? rr : n_rows];
    }
    __syncthreads();

    const int g = threadIdx.x / G;
    const int l = (threadIdx.x % G) / P;
    const int j0 = (threadIdx.x % P) * CPL;
    const int64_t row = row0 + g;
    const int64_t beg = s_ptr[g];
    int64_t end = s_ptr[g + 1];  // rows past n_rows are empty
    bool mine = true;
    if constexpr (BAL) {
        if (end - beg > long_len) {
            mine = false;
            end = beg;
        }
    }

    double acc[CPL];
    multi_group_sums<L, KV, VEC>(beg + l, end, col, val, X, ldx, j0, r, acc);
    if (row < n_rows && l == 0 && mine) {
        double *yr = Y + row * ldy;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            if (j0 + i < r)
                yr[j0 + i] = acc[i];
        }
    }
}

// The long rows of a balanced plan (spmv_csr_multi_plan, spmv_host.h): one
// group of 16 entry lanes x P lanes per SEGMENT of at most seg_len consecutive
// entries of one row, summed exactly as a row of csr_multi_kernel<16, KV>.
// The entry-lane count is 16 for every KV, so a column's bits do not depend on
// the width of its block.  dest >= 0: the segment is its row's only one and
// the sums are Y[dest]; dest < 0: the sums go to partial slot ~dest (8 doubles,
// column j at word j) for csr_multi_finish_kernel.  Every table value is
// checked against the counts before it is used as an index.
constexpr int kMultiLongL = 16;

template <int KV, bool VEC>
__global__ __launch_bounds__(kBlock) void csr_multi_long_kernel(
    int64_t n_rows, int64_t nnz, int64_t n_seg, int64_t n_slots, const int64_t *__restrict__ seg_beg,
    const int32_t *__restrict__ seg_cnt, const int32_t *__restrict__ seg_dest, const int32_t *__restrict__ col,
    const double *__restrict__ val, const double *__restrict__ X, int64_t ldx, double *__restrict__ Y,
    int64_t ldy, double *__restrict__ part, int32_t r)
{
    constexpr int L = kMultiLongL;
    constexpr int P = multi_p<KV, kWave / L>();
    constexpr int CPL = KV / P;
    constexpr int G = L * P;         // lanes per segment
    constexpr int SPB = kBlock / G;  // segments per workgroup

    const int64_t seg = (int64_t)blockIdx.x * SPB + threadIdx.x / G;
    const int l = (threadIdx.x % G) / P;
    const int j0 = (threadIdx.x % P) * CPL;
    int64_t beg = 0, cnt = 0, dest = 0;
    bool own = false;
    if (seg < n_seg) {
        beg = seg_beg[seg];
        cnt = seg_cnt[seg];
        dest = seg_dest[seg];
        own = beg >= 0 && cnt >= 0 && beg <= nnz - cnt && (dest >= 0 ? dest < n_rows : ~dest < n_slots);
    }
    if (!own)
        cnt = 0;

    double acc[CPL];
    multi_group_sums<L, KV, VEC>(beg + l, beg + cnt, col, val, X, ldx, j0, r, acc);
    if (own && l == 0) {
        double *out = dest >= 0 ? Y + dest * ldy : part + ~dest * 8;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            if (j0 + i < r)
                out[j0 + i] = acc[i];
        }
    }
}

// Y[row] of every split long row: slot0 + slot1 + ... in segment order, one
// thread per (row, column j < r).  Always overwrites Y, stores nothing for
// j >= r; a table entry outside the counts is skipped.
template <int KV>
__global__ __launch_bounds__(kBlock) void csr_multi_finish_kernel(
    int64_t n_rows, int64_t n_long, int64_t n_slots, const int32_t *__restrict__ long_row,
    const int32_t *__restrict__ long_first, const double *__restrict__ part, double *__restrict__ Y, int64_t ldy,
    int32_t r)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t i = t / KV;
    const int j = (int)(t % KV);
    if (i >= n_long || j >= r)
        return;
    const int64_t row = long_row[i];
    const int64_t first = long_first[i], last = long_first[i + 1];
    if (row < 0 || row >= n_rows || first < 0 || last > n_slots || first >= last)
        return;
    double s = part[first * 8 + j];
    for (int64_t q = first + 1; q < last; ++q)
        s += part[q * 8 + j];
    Y[row * ldy + j] = s;
}

// One KI-group of a slot-per-lane row: KI values and columns, non-temporal
// (each is read once; X is what the caches should keep).
template <int KI>
struct MultiGroup;

template <>
struct MultiGroup<1> {
    double v[1];
    int32_t c[1];
    __device__ __forceinline__ void load(const double *vp, const int32_t *cp)
    {
        v[0] = stream_load<true>(vp);
        c[0] = stream_load<true>(cp);
    }
};

template <>
struct MultiGroup<2> {
    double v[2];
    int32_t c[2];
    __device__ __forceinline__ void load(const double *vp, const int32_t *cp)
    {
        const double2 vv = stream_load2<true>(vp);
        const int2 cc = stream_load2<true>(cp);
        v[0] = vv.x;
        v[1] = vv.y;
        c[0] = cc.x;
        c[1] = cc.y;
    }
};

// lanes per row slot and slots per workgroup of slot_multi_kernel
template <int KV>
constexpr int slot_multi_p()
{
    return multi_p<KV, 4>();
}

// SELL and ELL: P lanes per row slot (one for KV <= 2, as sell_kernel /
// ell_kernel) with CPL columns each, walking the slot columns in order with
// the formats' layout formulas: entry (slot r, k) at
// base + (k / KI)*step + r*KI + (k % KI).  Padding slots hold 0.0 and a valid
// column, as for the single-vector kernels.  SELL walks the full slice width
// of slice_ptr (a split plan does not matter here) and writes row
// perm[slot] >= 0; ELL writes row i.
template <int KI, int KV, bool VEC, bool SELL>
__global__ __launch_bounds__(kBlock) void slot_multi_kernel(
    int64_t n_rows, int32_t C, int64_t n_slices, const int64_t *__restrict__ slice_ptr,
    const int32_t *__restrict__ perm, int32_t K, int64_t ld, const int32_t *__restrict__ col,
    const double *__restrict__ val, const double *__restrict__ X, int64_t ldx, double *__restrict__ Y,
    int64_t ldy, int32_t r)
{
    constexpr int P = slot_multi_p<KV>();
    constexpr int CPL = KV / P;
    constexpr int U = multi_inflight<CPL>() / KI;  // groups in flight
    const int64_t slot = (int64_t)blockIdx.x * (kBlock / P) + threadIdx.x / P;
    const int j0 = (threadIdx.x % P) * CPL;
    int64_t off, groups, step, row;
    if constexpr (SELL) {
        const int64_t s = slot / C;
        if (s >= n_slices)
            return;
        const int64_t base = slice_ptr[s];
        groups = (slice_ptr[s + 1] - base) / C / KI;
        off = base + (slot - s * C) * KI;
        step = (int64_t)C * KI;
        row = perm[slot];
    } else {
        if (slot >= n_rows)
            return;
        groups = K / KI;
        off = slot * KI;
        step = ld * KI;
        row = slot;
    }
    const double *vp = val + off;
    const int32_t *cp = col + off;

    double acc[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i)
        acc[i] = 0.0;

    int64_t g = 0;
    for (; g + U <= groups; g += U) {
        MultiGroup<KI> m[U];
        double x[U][KI][CPL];
#pragma unroll
        for (int u = 0; u < U; ++u)
            m[u].load(vp + (g + u) * step, cp + (g + u) * step);
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int q = 0; q < KI; ++q)
                load_xcols<CPL, VEC>(X + (int64_t)m[u].c[q] * ldx, j0, r, x[u][q]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int q = 0; q < KI; ++q) {
#pragma unroll
                for (int i = 0; i < CPL; ++i)
                    acc[i] = fma(m[u].v[q], x[u][q][i], acc[i]);
            }
        }
    }
    for (; g < groups; ++g) {
        MultiGroup<KI> m;
        double x[KI][CPL];
        m.load(vp + g * step, cp + g * step);
#pragma unroll
        for (int q = 0; q < KI; ++q)
            load_xcols<CPL, VEC>(X + (int64_t)m.c[q] * ldx, j0, r, x[q]);
#pragma unroll
        for (int q = 0; q < KI; ++q) {
#pragma unroll
            for (int i = 0; i < CPL; ++i)
                acc[i] = fma(m.v[q], x[q][i], acc[i]);
        }
    }

    if (row < 0)  // SELL padding slot
        return;
    double *yr = Y + row * ldy;
    if constexpr (VEC) {
#pragma unroll
        for (int i = 0; i < CPL; i += 2) {
            v2f64 o;
            o.x = acc[i];
            o.y = acc[i + 1];
            *reinterpret_cast<v2f64 *>(yr + j0 + i) = o;
        }
    } else {
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            if (j0 + i < r)
                yr[j0 + i] = acc[i];
        }
    }
}

namespace {

// One block of vectors [j0, j0 + r), r <= 8: the kernel width and whether
// the 16-byte path is proven for it.
struct MultiBlock {
    int32_t r;   // live vectors
    int kv;      // kernel width: smallest of 1, 2, 4, 8 >= r
    bool vec;    // full block with 16-byte aligned X and Y rows
    const double *X;
    double *Y;
};

// vec_y: the kernel stores Y rows as 16-byte pairs (the slot kernels; the CSR
// kernel's lanes store single columns), so Y must be proven aligned too
MultiBlock multi_block(int32_t k, int32_t j0, const double *X, int64_t ldx, double *Y, int64_t ldy, bool vec_y)
{
    MultiBlock b;
    b.r = k - j0 < 8 ? k - j0 : 8;
    b.kv = b.r > 4 ? 8 : b.r > 2 ? 4 : b.r;
    b.X = X ? X + j0 : X;
    b.Y = Y ? Y + j0 : Y;
    // rows start at base + row*ld*8 bytes: 16-byte aligned for every row iff
    // the block's base is and ld is even
    const bool aligned = (uintptr_t)b.X % 16 == 0 && ldx % 2 == 0 &&
                         (!vec_y || ((uintptr_t)b.Y % 16 == 0 && ldy % 2 == 0));
    b.vec = b.kv >= 2 && b.r == b.kv && aligned;
    return b;
}

template <int L, int KV>
void launch_csr_multi_kv(const spmv_dims &d, const int64_t *row_ptr, const int32_t *col, const double *val,
                         const MultiBlock &b, int64_t ldx, int64_t ldy, const MultiBalance *bal)
{
    constexpr int RPB = kBlock / (L * multi_p<KV, kWave / L>());  // rows per workgroup, >= 4
    const int64_t blocks = (d.n_rows + RPB - 1) / RPB;
    with_bool(bal != nullptr, [&](auto BAL) {
        constexpr bool bl = decltype(BAL)::value;
        auto kern = csr_multi_kernel<L, KV, false, bl>;
        if constexpr (KV >= 2) {
            if (b.vec)
                kern = csr_multi_kernel<L, KV, true, bl>;
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)d.stream, d.n_rows, row_ptr,
                           col, val, b.X, ldx, b.Y, ldy, b.r, bal ? bal->long_len : 0);
    });
}

// the long rows of a balanced plan: their segments, then the split rows' sums
template <int KV>
void launch_csr_multi_long_kv(const spmv_dims &d, const int32_t *col, const double *val, const MultiBlock &b,
                              int64_t ldx, int64_t ldy, const MultiBalance &m)
{
    constexpr int SPB = kBlock / (kMultiLongL * multi_p<KV, kWave / kMultiLongL>());  // segments per workgroup
    const hipStream_t st = (hipStream_t)d.stream;
    auto kern = csr_multi_long_kernel<KV, false>;
    if constexpr (KV >= 2) {
        if (b.vec)
            kern = csr_multi_long_kernel<KV, true>;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)((m.n_seg + SPB - 1) / SPB)), dim3(kBlock), 0, st, d.n_rows, d.nnz,
                       m.n_seg, m.n_slots, m.seg_beg, m.seg_cnt, m.seg_dest, col, val, b.X, ldx, b.Y, ldy, m.part,
                       b.r);
    if (m.n_slots > 0)
        hipLaunchKernelGGL(csr_multi_finish_kernel<KV>, dim3((unsigned)((m.n_long * KV + kBlock - 1) / kBlock)),
                           dim3(kBlock), 0, st, d.n_rows, m.n_long, m.n_slots, m.long_row, m.long_first, m.part, b.Y,
                           ldy, b.r);
}

template <int KI, int KV, bool SELL>
void launch_slot_multi_kv(const spmv_dims &d, int64_t slots, int32_t C, int64_t n_slices, const int64_t *slice_ptr,
                          const int32_t *perm, int32_t K, int64_t ld, const int32_t *col, const double *val,
                          const MultiBlock &b, int64_t ldx, int64_t ldy)
{
    constexpr int SPB = kBlock / slot_multi_p<KV>();  // slots per workgroup
    const int64_t blocks = (slots + SPB - 1) / SPB;
    auto kern = slot_multi_kernel<KI, KV, false, SELL>;
    if constexpr (KV >= 2) {
        if (b.vec)
            kern = slot_multi_kernel<KI, KV, true, SELL>;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)d.stream, d.n_rows, C, n_slices,
                       slice_ptr, perm, K, ld, col, val, b.X, ldx, b.Y, ldy, b.r);
}

}  // namespace

int launch_csr_multi(const spmv_dims &d, int L, const int64_t *row_ptr, const int32_t *col, const double *val,
                     int32_t k, const double *X, int64_t ldx, double *Y, int64_t ldy, const MultiBalance *bal)
{
    if (L < 2 || L > 64 || (L & (L - 1)))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_multi: CSR lanes per row must be a power of two in [2,64]");
    if (d.n_rows == 0)
        return SPMV_SUCCESS;
    if ((d.n_rows + 3) / 4 > INT32_MAX)  // at least 4 rows per workgroup
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_multi: too many rows");
    SPMV_GUARD(d);
    for (int32_t j0 = 0; j0 < k; j0 += 8) {
        const MultiBlock b = multi_block(k, j0, X, ldx, Y, ldy, false);
        with_int<2, 4, 8, 16, 32, 64>(L, [&](auto Lc) {
            with_int<1, 2, 4, 8>(b.kv, [&](auto KV) {
                launch_csr_multi_kv<decltype(Lc)::value, decltype(KV)::value>(d, row_ptr, col, val, b, ldx, ldy, bal);
            });
        });
        SPMV_CHECK_LAUNCH("csr_multi_kernel");
        if (bal && bal->n_seg > 0) {  // a plan without long rows launches nothing more
            with_int<1, 2, 4, 8>(b.kv, [&](auto KV) {
                launch_csr_multi_long_kv<decltype(KV)::value>(d, col, val, b, ldx, ldy, *bal);
            });
            SPMV_CHECK_LAUNCH("csr_multi_long_kernel");
        }
    }
    return SPMV_SUCCESS;
}

int launch_slot_multi(const spmv_dims &d, bool sell, int32_t ki, int32_t C, int64_t n_slices, const int64_t *slice_ptr,
                      const int32_t *perm, int32_t K, int64_t ld, const int32_t *col, const double *val, int32_t k,
                      const double *X, int64_t ldx, double *Y, int64_t ldy)
{
    if (ki != 1 && ki != 2)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_multi: ki must be 1 or 2");
    if (d.n_rows == 0 || (sell && n_slices == 0))
        return SPMV_SUCCESS;
    const int64_t slots = sell ? n_slices * C : d.n_rows;
    if ((slots + 63) / 64 > INT32_MAX)  // at least 64 slots per workgroup
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_run_multi: grid too large");
    SPMV_GUARD(d);
    for (int32_t j0 = 0; j0 < k; j0 += 8) {
        const MultiBlock b = multi_block(k, j0, X, ldx, Y, ldy, true);
        with_bool(sell, [&](auto SELL) {
            with_int<2, 1>(ki, [&](auto KI) {
                with_int<1, 2, 4, 8>(b.kv, [&](auto KV) {
                    launch_slot_multi_kv<decltype(KI)::value, decltype(KV)::value, decltype(SELL)::value>(
                        d, slots, C, n_slices, slice_ptr, perm, K, ld, col, val, b, ldx, ldy);
                });
            });
        });
        SPMV_CHECK_LAUNCH("slot_multi_kernel");
    }
    return SPMV_SUCCESS;
}

}  // namespace spmv
