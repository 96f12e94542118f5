// csr.hip — CSR-vector SpMV for gfx950.
//
// Replaces the reference's scalar CSR kernel (reference kernels/Csr.cl:1-17:
// one work-item per row, 8192 work-items total, reference csr.c:47-48).
// Here a group of L lanes (L | 64) owns one row.  Variants (the `variant`
// argument of spmv_csr_run_variant):
//   1 = direct: every L-lane group walks its own row with 16-byte pair loads
//       and reduces with a __shfl_xor butterfly;
//   2 = staged: the row group's entry range is streamed through LDS by all
//       256 lanes like a copy kernel, then each L-lane group sums its row;
//   3 = staged, persistent workgroups with the next group's offsets
//       fetched ahead (default; spmv_csr_run_xwin adds the LDS x windows,
//       load schedule MODE 0 or 3 of csr_xwin_kernel);
//   4 = entry-balanced tiles for skewed rows (spmv_csr_run_tiled, staged.hip).
// Bytes per row: 12·len + 8 (row_ptr) + 8 (y), plus x gathers.
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>

#include "common.h"

namespace spmv {

// One L-lane group's row [beg, end) with 16-byte pair loads: the lane
// reads the aligned pair (p, p+1); entries of the pair outside [beg, end)
// are zeroed by value (their column is a valid neighbour column, so the
// gather stays in bounds).  The last pair of the row is loaded as a
// scalar when p+1 == end, so nothing past val[nnz-1] is ever read.
template <int L, typename XS>
__device__ __forceinline__ double row_dot_pairs(int64_t beg, int64_t end, int lane,
                                                const int32_t *__restrict__ col,
                                                const double *__restrict__ val, const XS &xs)
{
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int64_t p = (beg & ~(int64_t)1) + 2 * lane;
    for (; p + 1 + 2 * L < end; p += 4 * L) {
        const double2 va = *reinterpret_cast<const double2 *>(val + p);
        const int2 ca = *reinterpret_cast<const int2 *>(col + p);
        const double2 vb = *reinterpret_cast<const double2 *>(val + p + 2 * L);
        const int2 cb = *reinterpret_cast<const int2 *>(col + p + 2 * L);
        s0 += (p >= beg ? va.x : 0.0) * xs(ca.x);
        s1 += va.y * xs(ca.y);
        s2 += vb.x * xs(cb.x);
        s3 += vb.y * xs(cb.y);
    }
    for (; p < end; p += 2 * L) {
        if (p + 1 < end) {
            const double2 va = *reinterpret_cast<const double2 *>(val + p);
            const int2 ca = *reinterpret_cast<const int2 *>(col + p);
            s0 += (p >= beg ? va.x : 0.0) * xs(ca.x);
            s1 += va.y * xs(ca.y);
        } else if (p >= beg) {
            s0 += val[p] * xs(col[p]);
        }
    }
    return group_sum<L>((s0 + s1) + (s2 + s3));
}

// Variant 1: the workgroup's 256/L + 1 row offsets staged in LDS, then
// every L-lane group walks its row (row_dot_pairs).
template <int L>
__global__ __launch_bounds__(kBlock) void csr_vector_kernel(
    int64_t n_rows, const int64_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const double *__restrict__ val,
    const double *__restrict__ x, double *__restrict__ y, int remap)
{
    constexpr int RPB = kBlock / L;  // rows per workgroup
    __shared__ int64_t s_ptr[RPB + 1];

    const int64_t row0 = xcd_block(remap) * RPB;
    if (threadIdx.x <= RPB) {
        int64_t r = row0 + threadIdx.x;
        s_ptr[threadIdx.x] = row_ptr[r < n_rows ? r : n_rows];
    }
    __syncthreads();

    const int g = threadIdx.x / L;
    const int lane = threadIdx.x % L;
    const int64_t row = row0 + g;
    const int64_t beg = s_ptr[g], end = s_ptr[g + 1];  // empty past n_rows
    const double sum = row_dot_pairs<L>(beg, end, lane, col, val, XGlobal{x});
    if (lane == 0 && row < n_rows)
        store_y(y + (row), sum);
}

// CSR-vector with the entry stream staged through LDS ("staged" variants).
// The workgroup's rows occupy one contiguous range of entries
// [ptr[row0], ptr[row0+RPB]).  Instead of every L-lane group walking its
// own row (ragged trip counts, loads that straddle row ends), all 256
// lanes stream that range like a copy kernel — aligned 16-byte value
// pairs + 8-byte column pairs, R pairs per lane in flight — and store the
// products a·x in LDS.  After one barrier each L-lane group sums its row's
// slice of the products (conflict-free ds_read_b64, stride 1 across lanes)
// and reduces with the same shuffle butterfly.  Ranges longer than the LDS
// chunk are processed in chunks; a row's partial sum stays in its lanes'
// registers across chunks.
constexpr int kStageRoundsDefault = 3;  // pairs per lane per chunk: 1536 products, 12 KiB
// (round 1, persistent kernel: R = 3 0.3008 ms, R = 4 0.3013, R = 5 and
// R = 8 slower; round 2, x-window kernel MODE 3: R = 3 0.2591-0.2607 ms,
// R = 4 0.2639-0.2642 — one rule for every staged CSR kernel keeps their
// chunk boundaries, hence their bits, identical)
// Chunks of the staged kernels start on a kChunkAlign-entry boundary at or
// before the row group's first entry (up to 31 entries of the previous group
// are loaded and never summed), so a wave's 64 value pairs (1 KiB) and column
// pairs (512 B) cover whole 128-B lines, 8 + 4 instead of 9 + 5: the
// CSR-shaped stream probe reads 6.81 TB/s from aligned tiles and 6.47 TB/s
// from tiles that start on any even entry (tools/bw_probe,
// csr_prologue_dep1[_unaligned]).  Every staged CSR kernel cuts the same
// chunks, so their sums stay bit-identical to each other.
constexpr int64_t kChunkAlign = 32;
__host__ __device__ __forceinline__ int64_t chunk_start(int64_t e) { return e & ~(kChunkAlign - 1); }
constexpr bool kCsrStreamNtDefault = false;  // SPMV_STREAM_NT overrides
// the x-window kernel (x gathers from LDS) streams faster non-temporal:
// 0.2991 vs 0.3077 ms on the cant-like batch
constexpr bool kCsrXwinNtDefault = true;

// Column sources of the staged kernels: where the column of entry p comes
// from.  Col32 = the CSR int32 array.  Col16 = compressed 16-bit indices
// (SURVEY.md §8f row 4): entry p's column is base[p/64] + off[p] when the
// 64-entry block's columns span < 65536, else the block is stored whole in
// esc (base = -1 - slot).  10.06 instead of 12 bytes per entry; the
// columns, hence products and sums, are exactly CSR's.
// Two-phase form for the pipelined kernels: raw(p) only issues loads (no
// load depends on another), decode(raw, p) turns them into the column pair
// (CSR16's escaped blocks load their int32 columns there, a second round
// trip for those blocks only).
// kWindowRelative: the source yields offsets into the running x window, not
// columns (ColWin16 below); the x-window kernel then gathers with XWindowRel.
template <bool NT>
struct Col32 {
    static constexpr bool kWindowRelative = false;
    const int32_t *__restrict__ col;
    using Raw = int2;
    __device__ __forceinline__ int2 pair(int64_t p) const { return stream_load2<NT>(col + p); }
    __device__ __forceinline__ int32_t one(int64_t p) const { return stream_load<NT>(col + p); }
    __device__ __forceinline__ Raw raw(int64_t p) const { return stream_load2<NT>(col + p); }
    __device__ __forceinline__ int2 decode(Raw r, int64_t) const { return r; }
};

template <bool NT>
struct Col16 {
    static constexpr bool kWindowRelative = false;
    const int32_t *__restrict__ base;
    const uint16_t *__restrict__ off;
    const int32_t *__restrict__ esc;
    // p even: entries p, p+1 share a 64-entry block and a 4-byte word
    __device__ __forceinline__ int2 pair(int64_t p) const
    {
        const int32_t b = base[p >> 6];
        if (b >= 0) {
            const uint32_t w = stream_load<NT>(reinterpret_cast<const uint32_t *>(off + p));
            return int2{b + (int32_t)(w & 0xffffu), b + (int32_t)(w >> 16)};
        }
        return stream_load2<NT>(esc + (int64_t)(-1 - b) * 64 + (p & 63));
    }
    __device__ __forceinline__ int32_t one(int64_t p) const
    {
        const int32_t b = base[p >> 6];
        return b >= 0 ? b + (int32_t)stream_load<NT>(off + p) : esc[(int64_t)(-1 - b) * 64 + (p & 63)];
    }
    struct Raw {
        int32_t b;   // the block's base, or -1 - escape slot
        uint32_t w;  // the pair's two 16-bit offsets
    };
    __device__ __forceinline__ Raw raw(int64_t p) const
    {
        return Raw{base[p >> 6], stream_load<NT>(reinterpret_cast<const uint32_t *>(off + p))};
    }
    __device__ __forceinline__ int2 decode(Raw r, int64_t p) const
    {
        if (r.b >= 0)
            return int2{r.b + (int32_t)(r.w & 0xffffu), r.b + (int32_t)(r.w >> 16)};
        return stream_load2<NT>(esc + (int64_t)(-1 - r.b) * 64 + (p & 63));
    }
};

// ColWin16 = the plan-owned window-relative copy (csr_col16_kernel, built
// once per plan): off[p] = col[p] - win[w].x for the x window w that holds
// entry p's row, so an offset indexes the LDS window directly.  10 bytes per
// entry, no base array, no escapes and no subtraction in the run; a plan has
// the copy only when every window with entries fits the LDS cap.  The values
// gathered for the summed entries are exactly Col32's, hence the same bits.
template <bool NT>
struct ColWin16 {
    static constexpr bool kWindowRelative = true;
    const uint16_t *__restrict__ off;
    using Raw = uint32_t;
    // p even: one aligned 4-byte word holds the offsets of entries p, p+1
    __device__ __forceinline__ Raw raw(int64_t p) const
    {
        return stream_load<NT>(reinterpret_cast<const uint32_t *>(off + p));
    }
    __device__ __forceinline__ int2 decode(Raw w, int64_t) const
    {
        return int2{(int32_t)(w & 0xffffu), (int32_t)(w >> 16)};
    }
    __device__ __forceinline__ int2 pair(int64_t p) const { return decode(raw(p), p); }
    __device__ __forceinline__ int32_t one(int64_t p) const { return (int32_t)stream_load<NT>(off + p); }
};

// x source of ColWin16: s[o] for an offset o of the running window, no base
// subtraction.  A window also LOADS entries of its neighbours (the lead-in
// entries before its first chunk, the partner of a pair that straddles its
// range end, the spare pair); those are never summed, but their offsets are
// relative to another window's base and may be anything in [0, 65535], so
// every gather is bounded to the window's last entry, hi = span - 1
// (unsigned: o >= 0).
struct XWindowRel {
    const double *s;  // LDS
    uint32_t hi;
    __device__ __forceinline__ double operator()(int32_t o) const
    {
        const uint32_t u = (uint32_t)o;
        return s[u < hi ? u : hi];
    }
};

// One row group (RPB = 256/L rows) of the staged scheme; s_ptr holds the
// group's RPB+1 row offsets.  Ends with a barrier, so the caller may
// overwrite s_ptr / s_prod afterwards.  Per-round guarded loads (the batched
// schedule measured 0.350 against 0.313 ms here: 76 VGPRs, 6 waves/SIMD).
template <int L, int R, bool NT, typename Cols = Col32<NT>, typename XS = XGlobal, typename V = double>
__device__ __forceinline__ void staged_group(
    int64_t row, const int64_t *s_ptr, double2 *s_prod,
    const Cols cols, const V *__restrict__ val,
    const XS xs, double *__restrict__ y, int64_t n_rows)
{
    constexpr int RPB = kBlock / L;
    constexpr int CH = 2 * kBlock * R;  // products per chunk
    const int g = threadIdx.x / L;
    const int lane = threadIdx.x % L;
    const int64_t beg = s_ptr[g], end = s_ptr[g + 1];
    const int64_t blk_end = s_ptr[RPB];
    const double *prod = reinterpret_cast<const double *>(s_prod);

    double acc = 0.0;
    // chunks start on a kChunkAlign boundary (whole cache lines per wave);
    // entries before the group's range are loaded but never summed.
    for (int64_t cb = chunk_start(s_ptr[0]); cb < blk_end; cb += CH) {
        const int64_t ce = cb + CH < blk_end ? cb + CH : blk_end;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int t = threadIdx.x + k * kBlock;
            const int64_t p = cb + 2 * (int64_t)t;
            double2 pr = {0.0, 0.0};
            if (p + 1 < ce) {
                const double2 v = vpair<NT>(val + p);
                const int2 c = cols.pair(p);
                pr.x = v.x * xs(c.x);
                pr.y = v.y * xs(c.y);
            } else if (p < ce) {
                pr.x = vone<NT>(val + p) * xs(cols.one(p));
            }
            s_prod[t] = pr;
        }
        __syncthreads();
        acc += slice_sum<L>(prod, beg > cb ? beg - cb : 0, (end < ce ? end : ce) - cb, lane);
        __syncthreads();
    }
    acc = group_sum<L>(acc);
    if (lane == 0 && row < n_rows)
        store_y(y + (row), acc);
    __syncthreads();
}

// One lane's share of a staged chunk in flight: R value pairs and R column
// pairs, loaded branch-free (pairs past the chunk load the chunk's first
// pair again and are never summed), so all 2R loads are outstanding
// together and can stay in flight across a barrier while the previous chunk
// is reduced.  (With the guarded loads inside per-round branches the
// compiler serialised the rounds: one round's loads in flight at a time.)
template <int R, bool NT, typename V, typename Cols = Col32<NT>>
struct StreamRegs {
    double2 v[R];
    typename Cols::Raw c[R];
    int64_t q[R];  // the pair each lane loaded (decode needs it for escaped blocks only)

    __device__ __forceinline__ void issue(int64_t cb, int64_t ce, int64_t nz, const Cols &cols,
                                          const V *__restrict__ val)
    {
        if (nz < 2) {  // uniform; a 0/1-entry array has no pair 0 (its entry: products()), nothing is loaded
#pragma unroll
            for (int k = 0; k < R; ++k) {
                v[k] = double2{0.0, 0.0};
                c[k] = typename Cols::Raw{};
                q[k] = 0;
            }
            return;
        }
        const int64_t spare = cb + 1 < nz ? cb : (nz - 2) & ~(int64_t)1;  // this chunk's first pair
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int64_t p = cb + 2 * (int64_t)(threadIdx.x + k * kBlock);
            q[k] = (p < ce && p + 1 < nz) ? p : spare;
            v[k] = vpair<NT>(val + q[k]);
            c[k] = cols.raw(q[k]);
        }
    }

    // products of the issued chunk [cb, ce) into s_prod
    template <typename XS>
    __device__ __forceinline__ void products(int64_t cb, int64_t ce, int64_t nz, const Cols &cols,
                                             const V *__restrict__ val, const XS &xs, double2 *s_prod) const
    {
        if (nz >= 2) {  // uniform (no gathers for a 0/1-entry array: x may be empty)
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int2 cc = cols.decode(c[k], q[k]);
                s_prod[threadIdx.x + k * kBlock] = double2{v[k].x * xs(cc.x), v[k].y * xs(cc.y)};
            }
        } else {
#pragma unroll
            for (int k = 0; k < R; ++k)
                s_prod[threadIdx.x + k * kBlock] = double2{0.0, 0.0};
        }
        const int64_t tail = nz - 1 - cb;  // the array's odd last entry
        if ((nz & 1) && nz - 1 < ce && tail >= 0 && tail < 2 * R * kBlock && (tail >> 1) % kBlock == threadIdx.x) {
            const int64_t p = nz - 1;
            s_prod[tail >> 1].x = vone<NT>(val + p) * xs(cols.one(p));
        }
    }
};

// The row groups of one x window, software-pipelined (csr_xwin_kernel
// MODE 3): the loads of the NEXT chunk — of this row group or of the
// window's next group — are issued right after the current chunk's
// products are in LDS, so they are in flight during the barrier and the
// L-lane reduction instead of after it.  s_off holds the window's
// ngroups·RPB + 1 row offsets.  Chunks and per-row sums are exactly those
// of staged_group (same boundaries, same order): the same bits.
// CSR_STAMP(k): per-wave phase hooks, no-ops in the product; a lab build
// (tools/build_variant.sh stamps_csr) injects tools/lab_stamps_csr.h
#ifndef CSR_STAMP
#define CSR_STAMP(k) \
    do {             \
    } while (0)
#endif
template <int L, int R, bool NT, typename XS, typename V, typename Cols = Col32<NT>>
__device__ __forceinline__ void staged_window_pipelined(int64_t row0, int ngroups, const int64_t *s_off,
                                                        double2 *s_prod, const Cols cols,
                                                        const V *__restrict__ val, const XS xs,
                                                        double *__restrict__ y, int64_t n_rows, int64_t nz)
{
    constexpr int RPB = kBlock / L;
    constexpr int CH = 2 * kBlock * R;
    const int g = threadIdx.x / L;
    const int lane = threadIdx.x % L;
    const double *prod = reinterpret_cast<const double *>(s_prod);
    // first group at or after `from` that has a chunk (staged_group's loop
    // runs a chunk iff chunk_start(start) < end); ngroups when none
    auto next_group = [&](int from) {
        int j = from;
        while (j < ngroups && chunk_start(s_off[j * RPB]) >= s_off[(j + 1) * RPB])
            ++j;
        return j;
    };
    StreamRegs<R, NT, V, Cols> st;  // the chunk loads in flight
    int jn = next_group(0);
    if (jn < ngroups) {
        const int64_t b = chunk_start(s_off[jn * RPB]), e = s_off[(jn + 1) * RPB];
        st.issue(b, b + CH < e ? b + CH : e, nz, cols, val);
    }
    int nchunk = 0;
    (void)nchunk;
    for (int gi = 0; gi < ngroups; ++gi) {
        const int64_t *gp = s_off + gi * RPB;
        const int64_t beg = gp[g], end = gp[g + 1];
        const int64_t blk_end = gp[RPB];
        double acc = 0.0;
        for (int64_t cb = chunk_start(gp[0]); cb < blk_end; cb += CH) {
            const int64_t ce = cb + CH < blk_end ? cb + CH : blk_end;
            st.products(cb, ce, nz, cols, val, xs, s_prod);
            CSR_STAMP(nchunk == 0 ? 2 : 5 + nchunk);  // 2: chunk 0's products; 6, 7: chunks 1, 2
            ++nchunk;
            // the next chunk: this group's, else the next group's first
            if (cb + CH < blk_end) {
                const int64_t nb = cb + CH;
                st.issue(nb, nb + CH < blk_end ? nb + CH : blk_end, nz, cols, val);
            } else if ((jn = next_group(gi + 1)) < ngroups) {
                const int64_t b = chunk_start(s_off[jn * RPB]), e = s_off[(jn + 1) * RPB];
                st.issue(b, b + CH < e ? b + CH : e, nz, cols, val);
            }
            __syncthreads();
            if (nchunk == 1)
                CSR_STAMP(3);  // chunk 0: products published
            acc += slice_sum<L>(prod, beg > cb ? beg - cb : 0, (end < ce ? end : ce) - cb, lane);
            if (nchunk == 1)
                CSR_STAMP(4);  // chunk 0: row sums read
            __syncthreads();
            if (nchunk == 1)
                CSR_STAMP(5);  // chunk 0: second barrier
        }
        acc = group_sum<L>(acc);
        const int64_t row = row0 + (int64_t)gi * RPB + g;
        // (the window's y staged in LDS and stored once at its end measured
        // the same: 0.2481 vs 0.2478 ms, profiles/round2/ab_ystage.log)
        if (lane == 0 && row < n_rows)
            store_y(y + (row), acc);
    }
}

// Variant 2: one workgroup per row group.
template <int L, int R>
__global__ __launch_bounds__(kBlock) void csr_staged_kernel(
    int64_t n_rows, const int64_t *__restrict__ row_ptr,
    const int32_t *__restrict__ col, const double *__restrict__ val,
    const double *__restrict__ x, double *__restrict__ y, int remap)
{
    constexpr int RPB = kBlock / L;
    __shared__ int64_t s_ptr[RPB + 1];
    __shared__ double2 s_prod[kBlock * R];
    const int64_t row0 = xcd_block(remap) * RPB;
    if (threadIdx.x <= RPB) {
        int64_t r = row0 + threadIdx.x;
        s_ptr[threadIdx.x] = row_ptr[r < n_rows ? r : n_rows];
    }
    __syncthreads();
    staged_group<L, R, false>(row0 + threadIdx.x / L, s_ptr, s_prod, Col32<false>{col}, val, XGlobal{x}, y, n_rows);
}

// Variant 3: persistent workgroups (a few per CU) walk the row groups
// grid-stride and PREFETCH the next group's row offsets into registers
// while the current group streams, so a group no longer starts with a
// dependent round trip for its offsets.  Cols = Col32 (CSR) or Col16
// (compressed column indices, spmv_csr16_run).
template <int L, int R, bool NT, typename Cols>
__global__ __launch_bounds__(kBlock) void csr_staged_persistent_kernel(
    int64_t n_rows, int64_t n_groups, const int64_t *__restrict__ row_ptr,
    const Cols cols, const double *__restrict__ val,
    const double *__restrict__ x, double *__restrict__ y)
{
    constexpr int RPB = kBlock / L;
    __shared__ int64_t s_ptr[RPB + 1];
    __shared__ double2 s_prod[kBlock * R];
    int64_t grp = blockIdx.x;
    int64_t next = 0;
    if (threadIdx.x <= RPB) {
        int64_t r = grp * RPB + threadIdx.x;
        next = row_ptr[r < n_rows ? r : n_rows];
    }
    for (; grp < n_groups; grp += gridDim.x) {
        if (threadIdx.x <= RPB)
            s_ptr[threadIdx.x] = next;
        __syncthreads();
        const int64_t g2 = grp + gridDim.x;
        if (threadIdx.x <= RPB && g2 < n_groups) {
            int64_t r = g2 * RPB + threadIdx.x;
            next = row_ptr[r < n_rows ? r : n_rows];
        }
        staged_group<L, R, NT, Cols>(grp * RPB + threadIdx.x / L, s_ptr, s_prod, cols, val, XGlobal{x}, y, n_rows);
    }
}

// Column window of every x window (rpb rows): [min, max] column over every
// entry a staged kernel LOADS for those rows — from two entries before the
// first chunk's 32-entry-aligned start (the lead-in entries of the previous
// rows, and the spare pair of a chunk starting at the array's last entry) to
// one past the rows' last entry (the partner of a pair that straddles the
// range end).  Those entries are never summed, but their gathers read LDS,
// so every one of them must lie inside the window.  One pass over col,
// build time.
__global__ __launch_bounds__(kBlock) void csr_window_kernel(int64_t n_rows, int64_t rpb,
                                                            const int64_t *__restrict__ row_ptr,
                                                            const int32_t *__restrict__ col,
                                                            int2 *__restrict__ win)
{
    const int64_t g = blockIdx.x;
    const int64_t r1 = (g + 1) * rpb < n_rows ? (g + 1) * rpb : n_rows;
    const int64_t nz = row_ptr[n_rows];
    const int64_t b = row_ptr[g * rpb], e = row_ptr[r1];
    int2 r = {0, -1};
    if (b < e) {  // uniform: rows without entries load nothing
        const int64_t lo = chunk_start(b) >= 2 ? chunk_start(b) - 2 : 0;
        const int64_t hi = e + 1 < nz ? e + 1 : nz;
        r = block_col_range(col, lo, hi);
    }
    if (threadIdx.x == 0)
        win[g] = r;
}

// The window-relative 16-bit column copy (ColWin16) of a plan whose windows
// all fit the LDS cap: off[e] = col[e] - win[w].x for the entries e of window
// w's rows (win[w].x is at most every column the window loads, its own
// entries included, and the window spans at most 2,048 columns, so the
// difference fits 11 bits).  Two zero entries pad the array's end.  One pass
// over row_ptr, col and win, build time.
__global__ __launch_bounds__(kBlock) void csr_col16_kernel(int64_t n_rows, int64_t nnz, int64_t rpb,
                                                           const int64_t *__restrict__ row_ptr,
                                                           const int32_t *__restrict__ col,
                                                           const int2 *__restrict__ win,
                                                           uint16_t *__restrict__ off)
{
    const int64_t g = blockIdx.x;
    const int64_t r1 = (g + 1) * rpb < n_rows ? (g + 1) * rpb : n_rows;
    const int64_t b = row_ptr[g * rpb];
    const int64_t e = row_ptr[r1] < nnz ? row_ptr[r1] : nnz;  // off holds nnz + 2 entries
    const int32_t lo = win[g].x;
    for (int64_t p = b + threadIdx.x; p < e; p += kBlock)
        off[p] = (uint16_t)(col[p] - lo);
    if (g == 0 && threadIdx.x < 2)
        off[nnz + threadIdx.x] = 0;
}

// base[byte_off / sizeof(T)] for a wave-uniform base and a per-lane 32-bit
// byte offset: the compiler keeps the base in SGPRs and emits the load's
// scalar-base form (global_load … v_off, s[base]), no 64-bit VALU address.
template <typename T>
__device__ __forceinline__ T load_at(const T *base, uint32_t byte_off)
{
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + byte_off);
}

// The staged kernel with x windows in LDS.  A window covers gpw consecutive
// row groups (rows_per_window = gpw * 256/L rows), one workgroup per window:
// the workgroup copies x[win.x .. win.y] into LDS (dynamic, xcap entries)
// once and then streams the gpw groups, whose products gather from LDS
// instead of global memory — the limiter of the staged kernel (TA busy,
// requests well below the DRAM credit limit: profiles/round1/pmc_stalls.json).
// A window wider than xcap gathers from global memory.  Same products, same
// order: y is bit-identical to variant 3.
// MODE (load schedule; products, sums and y are the same bits in both):
//   0 = window copied by a strided loop, each group's offsets staged in LDS
//       before it, each stream round's loads waited for before the next;
//   3 = the window's row offsets (all its groups, in dynamic LDS behind the
//       x range) and its x range loaded together, 8 loads in flight per
//       thread, before ONE barrier; the chunks software-pipelined: the next
//       chunk's loads are issued before the current chunk's barrier and
//       reduction (staged_window_pipelined).
// (Modes 1/2/4/5-7, a persistent streaming kernel with an x ring and a
// per-entry-range flat schedule were measured slower or equal and removed:
// profiles/round2/ab_csr_xwin*.log, ab_csr_flat.log, ab_xstream.log; so was
// the later MODE 4, MODE 3 with the window's first chunk issued in the
// prologue behind the x-range and offset loads: 15.6 against 14.8 us cold on
// one cant-like matrix, 90 against 72 VGPRs, profiles/round6/csr_prefetch_ab.md.)
// The MODE 3 prologue, cold, is a chain of memory round trips in front of
// the first chunk's loads; what it waits for, in order:
//   1. nothing for the arguments it needs: the library is built with kernarg
//      preload (Makefile KERNARG_PRELOAD), which delivers the first 14 dwords
//      of the arguments in SGPRs at wave launch.  Hence the parameter ORDER:
//      win, row_ptr, n_rows, gpw, n_groups, x, xcap and remap_windows are
//      those 14 dwords; val, y and the by-value column source follow (a
//      by-value struct ends the preloaded run, so it stands last) and are
//      fetched by one s_load beside step 2's.  remap_windows is the grid
//      size itself (0: no remap): gridDim is a hidden argument behind all of
//      these, one more load in front of win[wi].  (Firmware that does not
//      preload runs the s_loads the compiler keeps in front of the entry.)
//   2. win[wi] and row_ptr[n_rows], two scalar loads; the first U·256 row
//      offsets are requested before the wait for them (their addresses need
//      only arguments), the x window right after it;
//   3. the offsets and the window (2 + 8 loads per thread, each a scalar
//      base plus a 32-bit lane offset), all requested before the first LDS
//      store, then ONE barrier.
// profiles/round8/ab_csr_prologue.md has the ISA checks and the figures.
template <int L, int R, bool NT, typename V, int MODE, typename Cols>
__global__ __launch_bounds__(kBlock) void csr_xwin_kernel(
    const int2 *__restrict__ win, const int64_t *__restrict__ row_ptr, int64_t n_rows, int64_t gpw,
    int64_t n_groups, const double *__restrict__ x, int32_t xcap, uint32_t remap_windows,
    const V *__restrict__ val, double *__restrict__ y, const Cols cols)
{
    static_assert(MODE == 0 || MODE == 3, "csr_xwin_kernel: MODE 0 or 3");
    CSR_STAMP(0);
    constexpr int RPB = kBlock / L;
    extern __shared__ double s_x[];
    __shared__ int64_t s_ptr[MODE == 3 ? 1 : RPB + 1];
    __shared__ double2 s_prod[kBlock * R];
    int64_t *s_off = reinterpret_cast<int64_t *>(s_x + xcap);  // MODE 3: the window's offsets
    const int64_t nz = row_ptr[n_rows];
    // remap: consecutive windows on one XCD, so the overlapping x ranges of
    // neighbouring windows are copied from that XCD's L2
    const int64_t wi = xcd_block_of(remap_windows);
    const int64_t g_beg = wi * gpw;
    const int64_t g_end = (wi + 1) * gpw < n_groups ? (wi + 1) * gpw : n_groups;
    const int2 wnd = win[wi];
    if constexpr (MODE == 3) {
        // win[wi] is requested above this line and first used below the next
        // such line, behind the offsets' loads: left alone, the scheduler
        // either waits for it in front of them or requests it behind them
        __builtin_amdgcn_sched_barrier(0);
        // offsets r0 .. r0 + nr of the window's rows (clamped past n_rows),
        // then the x range: every load issued before the stores
        const int64_t r0 = g_beg * RPB;
        const int32_t nr = (int32_t)((g_end - g_beg) * RPB) + 1;
        constexpr int U = 2;  // offsets per thread per pass (nr <= U·256 in one pass)
        constexpr int XU = 8;  // window entries per thread (copy_window's default)
        // First pass, branch-free: the first U·256 offsets' and the window's
        // loads all go out before the first store (inside a loop over the
        // passes the compiler waited for the offsets before requesting the
        // window).  Addresses: a wave-uniform 64-bit base (SGPRs) plus a
        // 32-bit byte offset per lane, one or two VALU instructions per
        // load.  The offsets' addresses need the kernel arguments alone (row
        // min(r0 + i, n_rows), i <= 511), so they stand in front of the
        // first use of win[wi]; the window's need wnd on top (entry
        // min(i, xl), xl <= 2,047 in a window the branch-free copy holds).
        int64_t o[U];
        const int64_t *rbase = row_ptr + (r0 < n_rows ? r0 : n_rows);
        const int64_t rleft = n_rows - r0;  // rows from r0 to the clamp
        const uint32_t rl8 = rleft >= U * kBlock ? U * kBlock * 8u : rleft > 0 ? (uint32_t)rleft * 8u : 0u;
        const uint32_t t8 = threadIdx.x * 8u;
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const uint32_t i8 = t8 + k * kBlock * 8u;
            o[k] = load_at(rbase, i8 < rl8 ? i8 : rl8);
        }
        __builtin_amdgcn_sched_barrier(0);  // win[wi] is first used below
        const int32_t span = wnd.y - wnd.x + 1;
        const bool staged = span > 0 && span <= xcap;  // uniform per workgroup
        auto store_offsets = [&] {
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const int32_t i = (int32_t)threadIdx.x + k * kBlock;
                if (i < nr)
                    s_off[i] = o[k];
            }
        };
        // (the two cases share no registers past this branch: where the
        // window's values lived across its end, the compiler waited for the
        // offsets before it requested the window)
        if (span <= XU * kBlock) {  // uniform: the branch-free copy holds the window
            double xv[XU];
            const uint32_t xl8 = span > 0 ? (uint32_t)(span - 1) * 8u : 0u;  // clamped (loaded, never stored past span)
            const double *xbase = x + wnd.x;
#pragma unroll
            for (int k = 0; k < XU; ++k) {
                const uint32_t i8 = t8 + k * kBlock * 8u;
                xv[k] = load_at(xbase, i8 < xl8 ? i8 : xl8);
            }
            store_offsets();
            if (staged) {
#pragma unroll
                for (int k = 0; k < XU; ++k) {
                    const int32_t i = (int32_t)threadIdx.x + k * kBlock;
                    if (i < span)
                        s_x[i] = xv[k];
                }
            }
        } else {
            if (staged)
                copy_window(s_x, x, wnd.x, span);
            store_offsets();
            // vmcnt(0): nothing of this case is in flight where the cases
            // join, or the compiler guards the other case's registers by
            // waiting for the offsets before it requests the window
            __builtin_amdgcn_s_waitcnt(0x0f70);
        }
        // the further passes of a window of more than U·256 - 1 rows
        for (int32_t b = U * kBlock; b < nr; b += U * kBlock) {
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const int64_t r = r0 + b + threadIdx.x + k * kBlock;
                o[k] = row_ptr[r < n_rows ? r : n_rows];
            }
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const int32_t i = b + (int32_t)threadIdx.x + k * kBlock;
                if (i < nr)
                    s_off[i] = o[k];
            }
        }
        __syncthreads();  // window and offsets visible
        CSR_STAMP(1);
        // window-relative columns: every window with entries is staged (the
        // plan's rule); a window without entries sums nothing and its
        // never-summed gathers read s_x[0] (xcap >= 1)
        if constexpr (Cols::kWindowRelative)
            staged_window_pipelined<L, R, NT, XWindowRel, V, Cols>(r0, (int)(g_end - g_beg), s_off, s_prod, cols,
                                                                  val, XWindowRel{s_x, staged ? (uint32_t)span - 1 : 0u},
                                                                  y, n_rows, nz);
        else if (staged)
            staged_window_pipelined<L, R, NT, XWindow, V, Cols>(r0, (int)(g_end - g_beg), s_off, s_prod, cols, val,
                                                               XWindow{s_x, wnd.x}, y, n_rows, nz);
        else
            staged_window_pipelined<L, R, NT, XGlobal, V, Cols>(r0, (int)(g_end - g_beg), s_off, s_prod, cols, val,
                                                               XGlobal{x}, y, n_rows, nz);
        return;
    }
    const int32_t span = wnd.y - wnd.x + 1;
    const bool staged = span > 0 && span <= xcap;  // uniform per workgroup
    if (staged)
        for (int32_t i = threadIdx.x; i < span; i += kBlock)
            s_x[i] = x[wnd.x + i];
    for (int64_t grp = g_beg; grp < g_end; ++grp) {
        if (threadIdx.x <= RPB) {
            const int64_t r = grp * RPB + threadIdx.x;
            s_ptr[threadIdx.x] = row_ptr[r < n_rows ? r : n_rows];
        }
        __syncthreads();  // offsets (and, for the first group, the window) visible
        const int64_t row = grp * RPB + threadIdx.x / L;
        if constexpr (Cols::kWindowRelative)
            staged_group<L, R, NT, Cols, XWindowRel, V>(row, s_ptr, s_prod, cols, val,
                                                        XWindowRel{s_x, staged ? (uint32_t)span - 1 : 0u}, y, n_rows);
        else if (staged)
            staged_group<L, R, NT, Cols, XWindow, V>(row, s_ptr, s_prod, cols, val, XWindow{s_x, wnd.x}, y, n_rows);
        else
            staged_group<L, R, NT, Cols, XGlobal, V>(row, s_ptr, s_prod, cols, val, XGlobal{x}, y, n_rows);
    }
}

// (Round 6, one cant-like matrix cold, events: R = 2 / 5 / 6 pairs per lane
// 15.5 / 14.9 / 15.6 us against 15.0 us for R = 3, profiles/round6/ab_csr_r.md.)
// Chunk size of the staged CSR kernels for a matrix: R = 3 (1,536-entry
// chunks) unless R = 4 (2,048) cuts a row group of 256/L rows of the mean
// length into FEWER chunks — every chunk is a memory round trip and two
// barriers.  Cant-like (L = 4, 64 rows x 64.2 = 4,107 entries): 3 chunks
// either way, R = 3 (measured 0.2591 vs 0.2639 ms).  Banded (L = 2, 128
// rows x 16 = 2,048): 1 chunk with R = 4 against 2 with R = 3 (configs[4]
// measured 4.50 ms with R = 3).  Every staged CSR path uses this rule, so
// their chunk boundaries, hence their bits, stay identical.
static int csr_stage_rounds(int64_t n_rows, int64_t nnz, int L)
{
    if (n_rows <= 0 || L <= 0)
        return kStageRoundsDefault;
    const double eg = (double)(kBlock / L) * ((double)nnz / (double)n_rows);
    const int64_t c3 = (int64_t)((eg + 1535.0) / 1536.0), c4 = (int64_t)((eg + 2047.0) / 2048.0);
    return c4 < c3 ? 4 : 3;
}

static int cu_count()
{
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
        n = 256;
    return n;
}

// Resident workgroups per CU for a persistent kernel, from the occupancy
// calculator (VGPRs, LDS and the wave limit together), at most 8.  Sizing
// the grid by hand once launched 8 per CU of a kernel that fit only 7,
// and the 256 stragglers ran as a second wave.
template <typename K>
static int64_t persistent_grid(K kernel, int64_t groups, size_t dyn_lds = 0)
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, dyn_lds) != hipSuccess ||
        per_cu <= 0)
        per_cu = 1;
    if (per_cu > 8)
        per_cu = 8;
    const int64_t grid = (int64_t)cu_count() * per_cu;
    return grid < groups ? grid : groups;
}

template <int L, int R, bool NT, typename Cols>
static void launch_persistent(const spmv_dims &d, const int64_t *row_ptr, const Cols cols, const double *val,
                              const double *x, double *y, int64_t groups)
{
    static const int64_t per = persistent_grid(csr_staged_persistent_kernel<L, R, NT, Cols>, INT64_MAX);
    const int64_t grid = per < groups ? per : groups;
    hipLaunchKernelGGL((csr_staged_persistent_kernel<L, R, NT, Cols>), dim3((unsigned)grid), dim3(kBlock), 0,
                       (hipStream_t)d.stream, d.n_rows, groups, row_ptr, cols, val, x, y);
}

// compressed-index CSR: the persistent staged kernel with Col16 columns
template <int L, bool NT>
static void launch_csr16(const spmv_dims &d, const int64_t *row_ptr, const Col16<NT> cols,
                         const double *val, const double *x, double *y)
{
    constexpr int RPB = kBlock / L;
    const int64_t groups = (d.n_rows + RPB - 1) / RPB;
    if (csr_stage_rounds(d.n_rows, d.nnz, L) == 4)
        launch_persistent<L, 4, NT, Col16<NT>>(d, row_ptr, cols, val, x, y, groups);
    else
        launch_persistent<L, 3, NT, Col16<NT>>(d, row_ptr, cols, val, x, y, groups);
}

template <int L, int R>
static void launch_staged(const spmv_dims &d, const int64_t *row_ptr, const int32_t *col,
                          const double *val, const double *x, double *y, int variant)
{
    constexpr int RPB = kBlock / L;
    const int64_t groups = (d.n_rows + RPB - 1) / RPB;
    if (variant == 3) {
        if (stream_nt(kCsrStreamNtDefault))
            launch_persistent<L, R, true>(d, row_ptr, Col32<true>{col}, val, x, y, groups);
        else
            launch_persistent<L, R, false>(d, row_ptr, Col32<false>{col}, val, x, y, groups);
    } else {
        hipLaunchKernelGGL((csr_staged_kernel<L, R>), dim3((unsigned)groups), dim3(kBlock), 0,
                           (hipStream_t)d.stream, d.n_rows, row_ptr, col, val, x, y,
                           xcd_remap_enabled() ? 1 : 0);
    }
}

// the lanes per row the CSR kernels are instantiated for
static bool lanes_ok(int L)
{
    return L >= 2 && L <= 64 && (L & (L - 1)) == 0;
}

template <int L>
static void launch_csr(const spmv_dims &d, const int64_t *row_ptr,
                       const int32_t *col, const double *val, const double *x,
                       double *y, int variant)
{
    constexpr int RPB = kBlock / L;
    const int64_t blocks = (d.n_rows + RPB - 1) / RPB;
    if (variant >= 2) {
        if (csr_stage_rounds(d.n_rows, d.nnz, L) == 4)
            launch_staged<L, 4>(d, row_ptr, col, val, x, y, variant);
        else
            launch_staged<L, 3>(d, row_ptr, col, val, x, y, variant);
    } else {
        hipLaunchKernelGGL((csr_vector_kernel<L>), dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)d.stream,
                           d.n_rows, row_ptr, col, val, x, y, xcd_remap_enabled() ? 1 : 0);
    }
}

}  // namespace spmv

using namespace spmv;

extern "C" int spmv_csr_auto_lanes(int64_t n_rows, int64_t nnz)
{
    // Lanes per row for the default (staged) variant: about one lane per 16
    // entries of the mean row, a power of two in [2, 64].  The reduction
    // reads LDS, so a few lanes per row suffice, and more rows per group
    // amortise the group's offset fetch (mean 64 -> L = 4: 0.320 ms vs
    // 0.328 ms at L = 8 on the cant-like batch, profiles/round1_sweep.md).
    // The direct variant uses twice this (L = 8: 0.353 ms vs 0.383 at 16).
    double mean = n_rows > 0 ? (double)nnz / (double)n_rows : 0.0;
    int L = 2;
    while (L < 64 && (double)(2 * L) * 16.0 <= mean * 1.5)
        L *= 2;
    return L;
}

extern "C" int spmv_csr_run_variant(spmv_dims d, const int64_t *row_ptr,
                                    const int32_t *col, const double *val,
                                    const double *x, double *y, int lanes_per_row,
                                    int variant)
{
    if (d.n_rows < 0 || d.n_cols < 0 || d.nnz < 0)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_run: negative size");
    if (variant < 0 || variant > 3)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_run: variant must be 0..3 (4 = spmv_csr_run_tiled)");
    if (d.n_rows == 0)
        return SPMV_SUCCESS;
    if ((d.n_rows + 1) / 2 > (int64_t)INT32_MAX * 64)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_run: too many rows");
    SPMV_GUARD(d);
    const int v = variant ? variant : 3;
    int L = lanes_per_row;
    if (L <= 0) {
        L = spmv_csr_auto_lanes(d.n_rows, d.nnz);
        if (v == 1 && L < 64)
            L *= 2;
    }
    if (!lanes_ok(L))
        return fail_msg(SPMV_OTHER_ERROR,
                        "spmv_csr_run: lanes_per_row must be 0 or a power of two in [2,64]");
    with_int<2, 4, 8, 16, 32, 64>(L, [&](auto Lc) { launch_csr<decltype(Lc)::value>(d, row_ptr, col, val, x, y, v); });
    SPMV_CHECK_LAUNCH("csr kernel");
    return SPMV_SUCCESS;
}

extern "C" int spmv_csr_run(spmv_dims d, const int64_t *row_ptr,
                            const int32_t *col, const double *val,
                            const double *x, double *y, int lanes_per_row)
{
    return spmv_csr_run_variant(d, row_ptr, col, val, x, y, lanes_per_row, 0);
}

namespace spmv {

constexpr int32_t kCsrXwinCap = 2048;  // 16 KiB of LDS: 32 KiB per workgroup with the stage
constexpr int32_t kCsrXwinRows = 128;  // rows per x window (rows_per_window = 0): 0.2836 ms vs 0.2907 (64), 0.2938 (256), 0.2964 (512), 0.3397 (1024)

// Load schedule of csr_xwin_kernel: MODE 3 when a window's entries make
// more than one chunk (there is a next chunk to pipeline: cant-like, 128
// rows x 64.2 = 8,214 entries in 1,536-entry chunks), else MODE 0 — a
// one-chunk window gains nothing from the pipeline and its 86 instead of 64
// VGPRs cost workgroups per CU (banded, 128 rows x 16 = one 2,048-entry
// chunk: 0.765 ms MODE 0 vs 0.815 ms MODE 3, profiles/round2/ab_banded.log).
// MODE 3 with XCD-contiguous windows: 0.2644 ms vs 0.2678 (MODE 3, round
// robin), 0.2701 (MODE 0, remap) and 0.2717 (MODE 0, round robin), five
// interleaved rounds on one box (profiles/round2/ab_csr_xwin.log).
static int csr_xwin_mode(int64_t n_rows, int64_t nnz, int64_t rows_per_window, int R)
{
    const double ew = n_rows > 0 ? (double)rows_per_window * ((double)nnz / (double)n_rows) : 0.0;
    return ew > 2.0 * kBlock * R ? 3 : 0;
}

// XCD-contiguous windows pay when neighbouring windows share x lines: the
// widest window spans several times its rows (cant-like: 678 columns for 128
// rows; on), not when each row reads a narrow band (banded: 143 columns for
// 128 rows; 0.765 vs 0.782 ms with remap, off).  SPMV_XWIN_REMAP forces it
// (placement only: same bits).
// Round 5: only for grids of many rounds on the chip (>= 8 windows per CU).
// On ONE cant-like matrix (488 windows, one round, all windows resident at
// once) the round-robin placement ran 1.5 % faster in three interleaved A/Bs
// (12.08 / 11.98 vs 12.18 / 12.26 us cold, profiles/round5/ab_remap_staged.md;
// 12.12 vs 12.20-12.30 in round 4, profiles/round4/ab_csr_single.md T).
static bool csr_xwin_remap_rule(int32_t xcap, int64_t rows_per_window, int64_t n_windows)
{
    return xwin_remap((int64_t)xcap > 2 * rows_per_window && n_windows >= 8 * 256);
}

// dynamic LDS of csr_xwin_kernel: the x window, and in MODE 3 the window's
// row offsets behind it
static size_t csr_xwin_lds(int mode, int32_t xcap, int64_t gpw, int rpb)
{
    return ((size_t)xcap + (mode == 3 ? (size_t)(gpw * rpb + 1) : 0)) * sizeof(double);
}

// rows per x window: a multiple of the row group (256/L rows), default
// kCsrXwinRows but at least two groups, so a window whose groups are one
// chunk each still has a next chunk to pipeline (MODE 3): the banded matrix
// (L = 2, 128-row groups of 2,048 entries) 0.7534 ms with one-group windows
// (MODE 0) against 0.7261 ms with two (profiles/round2/ab_banded3.log);
// explicit rows_per_window: at least one group.  Same chunks, same bits.
// A small matrix (fewer than 4 default windows per CU) gets one-group
// windows instead, twice the workgroups to spread over the CUs: one
// cant-like matrix (488 windows of 128 rows) 13.28 vs 13.74 us cold, 10.5 vs
// 12.1 us warm (rocprof, profiles/round3/cant_single_csr_windows.log).
static int64_t csr_xwin_gpw(int L, int32_t rows_per_window, int64_t n_rows)
{
    const int64_t rpb = kBlock / L;
    if (rows_per_window > 0) {
        const int64_t g = (rows_per_window + rpb - 1) / rpb;
        return g < 1 ? 1 : g;
    }
    int64_t g = (kCsrXwinRows + rpb - 1) / rpb;
    g = g < 2 ? 2 : g;
    // the MI355X's 256 CUs as a constant, not the current device's count:
    // the window table (spmv_csr_xwin_build) bakes this choice in, so it
    // must not change with the device a matrix is later run on
    if (n_rows < 4 * (int64_t)256 * g * rpb)
        g = 1;
    return g;
}

// the window table's geometry for a valid L and n_rows > 0: rows per x window
// (whole row groups) and the number of windows
struct XwinGeom {
    int64_t rpw, n_win;
};
static XwinGeom csr_xwin_geom(int L, int32_t rows_per_window, int64_t n_rows)
{
    const int64_t rpw = csr_xwin_gpw(L, rows_per_window, n_rows) * (kBlock / L);
    return {rpw, (n_rows + rpw - 1) / rpw};
}

template <int L, int R, bool NT, typename Cols, typename V = double>
static void launch_csr_xwin(const spmv_dims &d, const int64_t *row_ptr, const Cols cols,
                            const V *val, const double *x, double *y, const int2 *win, int32_t xcap,
                            int64_t gpw)
{
    constexpr int RPB = kBlock / L;
    const int64_t groups = (d.n_rows + RPB - 1) / RPB;
    const int64_t n_win = (groups + gpw - 1) / gpw;
    int mode = csr_xwin_mode(d.n_rows, d.nnz, gpw * RPB, R);
    // a very tall window's offsets would not fit beside the x range in the
    // 64 KiB of dynamic LDS: MODE 0 stages them per row group instead
    if (mode == 3 && csr_xwin_lds(mode, xcap, gpw, RPB) + sizeof(double2) * kBlock * R * 2 > 64 * 1024)
        mode = 0;
    const size_t lds = csr_xwin_lds(mode, xcap, gpw, RPB);
    // the kernel's remap argument is the grid size itself (0: round robin)
    const uint32_t remap_windows = csr_xwin_remap_rule(xcap, gpw * RPB, n_win) ? (uint32_t)n_win : 0u;
    const hipStream_t st = (hipStream_t)d.stream;
    with_int<3, 0>(mode, [&](auto M) {
        hipLaunchKernelGGL((csr_xwin_kernel<L, R, NT, V, decltype(M)::value, Cols>), dim3((unsigned)n_win),
                           dim3(kBlock), lds, st, win, row_ptr, d.n_rows, gpw, groups, x, xcap, remap_windows, val, y,
                           cols);
    });
}

struct MakeCol32 {
    const int32_t *col;
    template <bool NT>
    Col32<NT> get() const { return Col32<NT>{col}; }
};

struct MakeCol16 {
    const int32_t *base;
    const uint16_t *off;
    const int32_t *esc;
    template <bool NT>
    Col16<NT> get() const { return Col16<NT>{base, off, esc}; }
};

struct MakeColWin16 {
    const uint16_t *off;
    template <bool NT>
    ColWin16<NT> get() const { return ColWin16<NT>{off}; }
};

// One launcher per column source / value type: L as asked, R (3 or 4) and the
// load policy from the rules above.
template <typename V, typename MakeCols>
static int launch_xwin_any(const spmv_dims &d, int L, const int64_t *row_ptr, MakeCols mk, const V *val,
                           const double *x, double *y, const int2 *w, int32_t xcap, int64_t gpw)
{
    if (!lanes_ok(L))
        return fail_msg(SPMV_OTHER_ERROR, "csr x-window run: lanes_per_row must be 0 or a power of two in [2,64]");
    const bool nt = stream_nt(kCsrXwinNtDefault);
    with_int<2, 4, 8, 16, 32, 64>(L, [&](auto Lc) {
        with_int<4, 3>(csr_stage_rounds(d.n_rows, d.nnz, decltype(Lc)::value), [&](auto Rc) {
            with_bool(nt, [&](auto NT) {
                launch_csr_xwin<decltype(Lc)::value, decltype(Rc)::value, decltype(NT)::value>(
                    d, row_ptr, mk.template get<decltype(NT)::value>(), val, x, y, w, xcap, gpw);
            });
        });
    });
    return SPMV_SUCCESS;
}

}  // namespace spmv

extern "C" size_t spmv_csr_xwin_bytes(int64_t n_rows, int64_t nnz, int lanes_per_row, int32_t rows_per_window)
{
    const int L = lanes_per_row > 0 ? lanes_per_row : spmv_csr_auto_lanes(n_rows, nnz);
    if (!lanes_ok(L) || n_rows <= 0 || rows_per_window < 0)
        return 0;
    return (size_t)csr_xwin_geom(L, rows_per_window, n_rows).n_win * sizeof(int2);
}

extern "C" int spmv_csr_xwin_build(spmv_dims d, const int64_t *row_ptr, const int32_t *col,
                                   int lanes_per_row, int32_t rows_per_window, void *win, size_t win_bytes,
                                   int32_t *xcap)
{
    if (d.n_rows < 0 || d.nnz < 0 || !xcap || rows_per_window < 0)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_xwin_build: bad arguments");
    *xcap = 0;
    if (d.n_rows == 0)
        return SPMV_SUCCESS;
    const int L = lanes_per_row > 0 ? lanes_per_row : spmv_csr_auto_lanes(d.n_rows, d.nnz);
    if (!lanes_ok(L))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_xwin_build: lanes_per_row must be 0 or a power of two in [2,64]");
    const XwinGeom g = csr_xwin_geom(L, rows_per_window, d.n_rows);
    if (!win || win_bytes < (size_t)g.n_win * sizeof(int2))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_xwin_build: window buffer too small");
    SPMV_GUARD(d);
    const hipStream_t st = (hipStream_t)d.stream;
    hipLaunchKernelGGL(csr_window_kernel, dim3((unsigned)g.n_win), dim3(kBlock), 0, st, d.n_rows, g.rpw, row_ptr,
                       col, (int2 *)win);
    SPMV_CHECK_LAUNCH("csr_window_kernel");
    return windows_xcap(win, g.n_win, kCsrXwinCap, st, xcap, "spmv_csr_xwin_build");
}

// argument checks of the x-window runs; *L = lanes per row, *gpw = row
// groups per window (a grid of one workgroup per window)
static int xwin_args(spmv_dims d, int32_t rows_per_window, const void *win, int32_t xcap, int lanes_per_row,
                     int *L, int64_t *gpw, const char *who)
{
    static thread_local char msg[160];
    if (d.n_rows < 0 || d.n_cols < 0 || d.nnz < 0 || rows_per_window < 0) {
        snprintf(msg, sizeof msg, "%s: bad sizes", who);
        return fail_msg(SPMV_OTHER_ERROR, msg);
    }
    if (d.n_rows > 0 && (!win || xcap < 0 || xcap > kCsrXwinCap)) {
        snprintf(msg, sizeof msg, "%s: bad window arguments", who);
        return fail_msg(SPMV_OTHER_ERROR, msg);
    }
    *L = lanes_per_row > 0 ? lanes_per_row : spmv_csr_auto_lanes(d.n_rows, d.nnz);
    if (!lanes_ok(*L)) {
        snprintf(msg, sizeof msg, "%s: lanes_per_row must be 0 or a power of two in [2,64]", who);
        return fail_msg(SPMV_OTHER_ERROR, msg);
    }
    *gpw = csr_xwin_gpw(*L, rows_per_window, d.n_rows);
    const int64_t groups = (d.n_rows + kBlock / *L - 1) / (kBlock / *L);
    if ((groups + *gpw - 1) / *gpw > INT32_MAX) {
        snprintf(msg, sizeof msg, "%s: grid too large", who);
        return fail_msg(SPMV_OTHER_ERROR, msg);
    }
    return SPMV_SUCCESS;
}

// The tail of every x-window run: the shared argument checks, nothing to do
// for a matrix without rows, then the entry point's own check, then the
// launch on d's device.  mk = the column source, who = the entry point's name
// for the shared error texts, own_err = the text of the entry point's own
// argument error (tested by the caller; null = none), kernel = the launch's
// name in a launch error.
template <typename V, typename MakeCols>
static int run_xwin(spmv_dims d, const int64_t *row_ptr, MakeCols mk, const V *val, const double *x, double *y,
                    int lanes_per_row, int32_t rows_per_window, const void *win, int32_t xcap, const char *who,
                    const char *own_err, const char *kernel)
{
    int L = 0;
    int64_t gpw = 0;
    int rc = xwin_args(d, rows_per_window, win, xcap, lanes_per_row, &L, &gpw, who);
    if (rc != SPMV_SUCCESS || d.n_rows == 0)
        return rc;
    if (own_err)
        return fail_msg(SPMV_OTHER_ERROR, own_err);
    SPMV_GUARD(d);
    rc = launch_xwin_any(d, L, row_ptr, mk, val, x, y, (const int2 *)win, xcap, gpw);
    if (rc != SPMV_SUCCESS)
        return rc;
    SPMV_CHECK_LAUNCH(kernel);
    return SPMV_SUCCESS;
}

extern "C" int spmv_csr_run_xwin(spmv_dims d, const int64_t *row_ptr, const int32_t *col, const double *val,
                                 const double *x, double *y, int lanes_per_row, int32_t rows_per_window,
                                 const void *win, int32_t xcap)
{
    return run_xwin(d, row_ptr, MakeCol32{col}, val, x, y, lanes_per_row, rows_per_window, win, xcap,
                    "spmv_csr_run_xwin", nullptr, "csr_xwin_kernel");
}

// ---- the plan's window-relative 16-bit column copy (ColWin16; plan.hip)
size_t spmv::csr_col16_bytes(int64_t nnz)
{
    return ((size_t)2 * (size_t)(nnz + 2) + 3) & ~(size_t)3;
}

// *fits = every window with entries spans at most xcap columns (a window
// without entries is {0, -1}); one synchronising copy of the window table
int spmv::csr_col16_fits(const spmv_dims &d, int lanes_per_row, int32_t rows_per_window, const void *win,
                         int32_t xcap, bool *fits)
{
    *fits = false;
    const int64_t n_win = (int64_t)(spmv_csr_xwin_bytes(d.n_rows, d.nnz, lanes_per_row, rows_per_window) / sizeof(int2));
    if (d.nnz < 2 || n_win <= 0 || !win || xcap < 1 || xcap > kCsrXwinCap)
        return SPMV_SUCCESS;
    int2 *h = nullptr;
    const int rc = windows_download(win, n_win, (hipStream_t)d.stream, &h, "spmv_plan_csr");
    if (rc != SPMV_SUCCESS)
        return rc;
    bool ok = true;
    for (int64_t w = 0; w < n_win && ok; ++w) {
        const int64_t span = (int64_t)h[w].y - h[w].x + 1;
        ok = span == 0 || (span > 0 && span <= xcap);
    }
    free(h);
    *fits = ok;
    return SPMV_SUCCESS;
}

// fills off (csr_col16_bytes(d.nnz) bytes) on d.stream; not synchronised
int spmv::csr_col16_fill(const spmv_dims &d, const int64_t *row_ptr, const int32_t *col, int lanes_per_row,
                         int32_t rows_per_window, const void *win, uint16_t *off)
{
    const int L = lanes_per_row > 0 ? lanes_per_row : spmv_csr_auto_lanes(d.n_rows, d.nnz);
    if (!lanes_ok(L) || d.n_rows <= 0 || !win || !off)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_plan_csr: 16-bit column copy: bad arguments");
    const XwinGeom g = csr_xwin_geom(L, rows_per_window, d.n_rows);
    hipLaunchKernelGGL(csr_col16_kernel, dim3((unsigned)g.n_win), dim3(kBlock), 0, (hipStream_t)d.stream, d.n_rows,
                       d.nnz, g.rpw, row_ptr, col, (const int2 *)win, off);
    SPMV_CHECK_LAUNCH("csr_col16_kernel");
    return SPMV_SUCCESS;
}

// spmv_csr_run_xwin with the columns read from the plan's copy: the same
// kernel, load schedule, chunks and sums, hence the same bits
int spmv::csr_run_xwin_col16(spmv_dims d, const int64_t *row_ptr, const uint16_t *off, const double *val,
                             const double *x, double *y, int lanes_per_row, int32_t rows_per_window,
                             const void *win, int32_t xcap)
{
    const bool corrupt = !off || xcap < 1 || d.nnz < 2;
    return run_xwin(d, row_ptr, MakeColWin16{off}, val, x, y, lanes_per_row, rows_per_window, win, xcap,
                    "spmv_plan_run", corrupt ? "spmv_plan_run: corrupt 16-bit column copy" : nullptr,
                    "csr_xwin_kernel (16-bit window offsets)");
}

extern "C" int spmv_csr16_run(spmv_dims d, const int64_t *row_ptr, const int32_t *blk_base,
                              const uint16_t *col_off, const int32_t *col_esc, const double *val,
                              const double *x, double *y, int lanes_per_row)
{
    if (d.n_rows < 0 || d.n_cols < 0 || d.nnz < 0)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr16_run: negative size");
    if (d.n_rows == 0)
        return SPMV_SUCCESS;
    if (d.nnz > 0 && (!blk_base || !col_off))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr16_run: missing index arrays");
    SPMV_GUARD(d);
    const int L = lanes_per_row > 0 ? lanes_per_row : spmv_csr_auto_lanes(d.n_rows, d.nnz);
    const bool nt = stream_nt(kCsrStreamNtDefault);
    if (!lanes_ok(L))
        return fail_msg(SPMV_OTHER_ERROR,
                        "spmv_csr16_run: lanes_per_row must be 0 or a power of two in [2,64]");
    with_int<2, 4, 8, 16, 32, 64>(L, [&](auto Lc) {
        with_bool(nt, [&](auto NT) {
            launch_csr16<decltype(Lc)::value, decltype(NT)::value>(
                d, row_ptr, Col16<decltype(NT)::value>{blk_base, col_off, col_esc}, val, x, y);
        });
    });
    SPMV_CHECK_LAUNCH("csr16 kernel");
    return SPMV_SUCCESS;
}

// CSR16 on the x-window pipeline: the same kernel, load schedule and chunks
// as spmv_csr_run_xwin with the columns decoded from the 16-bit offsets
// (escaped blocks from their int32 copy), so y is bit-identical to it.
// Windows from spmv_csr_xwin_build over the CSR's int32 columns (the same
// column values) with the same lanes_per_row and rows_per_window.
extern "C" int spmv_csr16_run_xwin(spmv_dims d, const int64_t *row_ptr, const int32_t *blk_base,
                                   const uint16_t *col_off, const int32_t *col_esc, const double *val,
                                   const double *x, double *y, int lanes_per_row, int32_t rows_per_window,
                                   const void *win, int32_t xcap)
{
    const bool missing = d.nnz > 0 && (!blk_base || !col_off);
    return run_xwin(d, row_ptr, MakeCol16{blk_base, col_off, col_esc}, val, x, y, lanes_per_row, rows_per_window,
                    win, xcap, "spmv_csr16_run_xwin",
                    missing ? "spmv_csr16_run_xwin: missing index arrays" : nullptr,
                    "csr_xwin_kernel (16-bit columns)");
}

// CSR with fp32 values (8 bytes per entry instead of
// 12): the x-window kernel widens each value to fp64 before the product
// and sums in fp64, so y equals spmv_csr_run_xwin's on the fp32-rounded
// values bit for bit.  Windows from spmv_csr_xwin_build on the same
// row_ptr/col with the same lanes_per_row and rows_per_window.
extern "C" int spmv_csr_f32v_run_xwin(spmv_dims d, const int64_t *row_ptr, const int32_t *col, const float *val,
                                      const double *x, double *y, int lanes_per_row, int32_t rows_per_window,
                                      const void *win, int32_t xcap)
{
    return run_xwin(d, row_ptr, MakeCol32{col}, val, x, y, lanes_per_row, rows_per_window, win, xcap,
                    "spmv_csr_f32v_run_xwin", nullptr, "csr_xwin_kernel (fp32 values)");
}

extern "C" size_t spmv_csr_tiled_ws_bytes(int64_t n_rows, int64_t nnz)
{
    (void)n_rows;
    // sized for the smallest tile the run may pick
    const int64_t tiles = nnz > 0 ? (nnz + csr_tiled_tile_min() - 1) / csr_tiled_tile_min() : 0;
    // carry_val[tiles] f64, own_lo[tiles+1] i32, carry_row[tiles] i32
    return (size_t)(8 * tiles + 4 * (tiles + 1) + 4 * tiles + 16);
}

extern "C" int spmv_csr_run_tiled(spmv_dims d, const int64_t *row_ptr, const int32_t *col,
                                  const double *val, const double *x, double *y, void *ws,
                                  size_t ws_bytes)
{
    if (d.n_rows < 0 || d.n_cols < 0 || d.nnz < 0 || d.n_rows > INT32_MAX)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_run_tiled: bad sizes");
    if (d.n_rows == 0)
        return SPMV_SUCCESS;
    SPMV_GUARD(d);
    if (d.nnz == 0) {
        hipError_t e = hipMemsetAsync(y, 0, (size_t)d.n_rows * sizeof(double), (hipStream_t)d.stream);
        return e == hipSuccess ? SPMV_SUCCESS : fail(SPMV_PROGRAM_ERROR, "memset y", e);
    }
    if (!ws || ws_bytes < spmv_csr_tiled_ws_bytes(d.n_rows, d.nnz))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_run_tiled: workspace too small");
    const int64_t tiles = (d.nnz + csr_tiled_tile(d.n_rows, d.nnz) - 1) / csr_tiled_tile(d.n_rows, d.nnz);
    if (tiles > INT32_MAX)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_run_tiled: grid too large");
    double *carry_val = (double *)ws;
    int32_t *own_lo = (int32_t *)(carry_val + tiles);
    int32_t *carry_row = own_lo + tiles + 1;
    int rc = launch_csr_tiled(d, row_ptr, col, val, x, y, own_lo, carry_row, carry_val);
    if (rc != SPMV_SUCCESS)
        return rc;
    return launch_carry(tiles, carry_row, carry_val, y, (hipStream_t)d.stream);
}

extern "C" size_t spmv_csr_hot_ws_bytes(int64_t n_rows, int64_t nnz, int64_t H)
{
    return (size_t)(H > 0 ? H : 0) * sizeof(double) + spmv_csr_tiled_ws_bytes(n_rows, nnz);
}

// Entry-balanced CSR whose column ids >= n_cols name the hot-column table
// (host spmv_hot_columns): xh[i] = x[hot[i]] is gathered first, then the
// tiled kernel reads the H hottest x values from that compact, L2-resident
// table.  Same products in the same order as spmv_csr_run_tiled on the
// un-renumbered columns, so y is bit-identical to it.
template <typename V>
static int run_tiled_hot(spmv_dims d, const int64_t *row_ptr, const int32_t *col_hot, const V *val,
                         const double *x, double *y, int64_t H, const int32_t *hot, const int32_t *own_lo_plan,
                         void *ws, const char *who)
{
    static thread_local char msg[160];
    const int64_t tiles = (d.nnz + csr_tiled_tile(d.n_rows, d.nnz) - 1) / csr_tiled_tile(d.n_rows, d.nnz);
    if (tiles > INT32_MAX) {
        snprintf(msg, sizeof msg, "%s: grid too large", who);
        return fail_msg(SPMV_OTHER_ERROR, msg);
    }
    double *xh = (double *)ws;
    double *carry_val = xh + H;
    int32_t *own_lo = (int32_t *)(carry_val + tiles);
    int32_t *carry_row = own_lo + tiles + 1;
    return launch_csr_tiled_hot(d, row_ptr, col_hot, val, x, y, H, hot, xh, own_lo_plan, own_lo, carry_row,
                                carry_val);
}

extern "C" int spmv_csr_run_tiled_hot(spmv_dims d, const int64_t *row_ptr, const int32_t *col_hot,
                                      const double *val, const double *x, double *y, int64_t H,
                                      const int32_t *hot, const int32_t *own_lo_plan, void *ws,
                                      size_t ws_bytes)
{
    if (d.n_rows < 0 || d.n_cols < 0 || d.nnz < 0 || d.n_rows > INT32_MAX || H < 0 ||
        d.n_cols + H > INT32_MAX)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_run_tiled_hot: bad sizes");
    if (d.n_rows == 0 || d.nnz == 0 || (H == 0 && !own_lo_plan))
        return spmv_csr_run_tiled(d, row_ptr, col_hot, val, x, y, ws, ws_bytes);
    if ((H > 0 && !hot) || !ws || ws_bytes < spmv_csr_hot_ws_bytes(d.n_rows, d.nnz, H))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_run_tiled_hot: hot list or workspace missing");
    SPMV_GUARD(d);
    return run_tiled_hot(d, row_ptr, col_hot, val, x, y, H, hot, own_lo_plan, ws,
                         "spmv_csr_run_tiled_hot");
}

extern "C" int64_t spmv_csr_tiled_tile(int64_t n_rows, int64_t nnz)
{
    return csr_tiled_tile(n_rows, nnz);
}

// spmv_csr_run_tiled_hot with the big-tile plan of the host builder
// spmv_csr_tiled_bigplan (uploaded; built for tile = spmv_csr_tiled_tile):
// tiles owning more than 1,024 rows write their rows without entries as
// zeros and sum only the listed ones, instead of reading every owned row's
// offsets from global memory.  big = NULL: spmv_csr_run_tiled_hot.
extern "C" int spmv_csr_run_tiled_plan(spmv_dims d, const int64_t *row_ptr, const int32_t *col_hot,
                                       const double *val, const double *x, double *y, int64_t H,
                                       const int32_t *hot, const int32_t *own_lo_plan, const int32_t *big,
                                       int64_t big_len, int64_t big_tile, void *ws, size_t ws_bytes)
{
    if (!big)
        return spmv_csr_run_tiled_hot(d, row_ptr, col_hot, val, x, y, H, hot, own_lo_plan, ws, ws_bytes);
    // the plan must be this matrix's: built for the tile the run cuts, and
    // at least as long as its tile index (the kernel bounds-checks the rest)
    if (big_tile != csr_tiled_tile(d.n_rows, d.nnz) || big_tile != csr_tiled_tile_min())
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_run_tiled_plan: plan built for another tile size");
    if (d.nnz > 0 && big_len < (d.nnz + big_tile - 1) / big_tile + 1)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_run_tiled_plan: plan shorter than its tile index");
    if (d.n_rows < 0 || d.n_cols < 0 || d.nnz < 0 || d.n_rows > INT32_MAX || H < 0 ||
        d.n_cols + H > INT32_MAX)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_run_tiled_plan: bad sizes");
    if (d.n_rows == 0 || d.nnz == 0)
        return spmv_csr_run_tiled(d, row_ptr, col_hot, val, x, y, ws, ws_bytes);
    if (!own_lo_plan || (H > 0 && !hot) || !ws || ws_bytes < spmv_csr_hot_ws_bytes(d.n_rows, d.nnz, H))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_run_tiled_plan: tile plan, hot list or workspace missing");
    SPMV_GUARD(d);
    const int64_t tiles = (d.nnz + csr_tiled_tile(d.n_rows, d.nnz) - 1) / csr_tiled_tile(d.n_rows, d.nnz);
    if (tiles > INT32_MAX)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_run_tiled_plan: grid too large");
    double *xh = (double *)ws;
    double *carry_val = xh + H;
    int32_t *own_lo = (int32_t *)(carry_val + tiles);
    int32_t *carry_row = own_lo + tiles + 1;
    return launch_csr_tiled_hot(d, row_ptr, col_hot, val, x, y, H, hot, xh, own_lo_plan, own_lo, carry_row,
                                carry_val, big, big_len);
}

// fp32 values, entry-balanced tiles (+ hot-column table, build-once tile
// plan), as spmv_csr_run_tiled_hot: bit-identical to it on the fp32-rounded
// values.  own_lo_plan from spmv_csr_tiled_plan, or NULL.
extern "C" int spmv_csr_f32v_run_tiled_hot(spmv_dims d, const int64_t *row_ptr, const int32_t *col_hot,
                                           const float *val, const double *x, double *y, int64_t H,
                                           const int32_t *hot, const int32_t *own_lo_plan, void *ws,
                                           size_t ws_bytes)
{
    if (d.n_rows < 0 || d.n_cols < 0 || d.nnz < 0 || d.n_rows > INT32_MAX || H < 0 ||
        d.n_cols + H > INT32_MAX)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_f32v_run_tiled_hot: bad sizes");
    if (d.n_rows == 0)
        return SPMV_SUCCESS;
    SPMV_GUARD(d);
    if (d.nnz == 0) {
        hipError_t e = hipMemsetAsync(y, 0, (size_t)d.n_rows * sizeof(double), (hipStream_t)d.stream);
        return e == hipSuccess ? SPMV_SUCCESS : fail(SPMV_PROGRAM_ERROR, "memset y", e);
    }
    if ((H > 0 && !hot) || !ws || ws_bytes < spmv_csr_hot_ws_bytes(d.n_rows, d.nnz, H))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csr_f32v_run_tiled_hot: hot list or workspace missing");
    return run_tiled_hot(d, row_ptr, col_hot, val, x, y, H, hot, own_lo_plan, ws,
                         "spmv_csr_f32v_run_tiled_hot");
}

// ------------------------------------------------- column-grouped CSR (CSRG)
// Power-law matrices (R-MAT, configs[3]) are bound by their x gathers: a
// cold column fills a whole 128-byte L2 line for 8 bytes, and the R-MAT's
// ~4 M used columns (33 MB of x lines) do not fit one XCD's 4 MiB L2, so
// the tiled kernel moved 3.46x bytes_alg (profiles/traffic_rmat.json).
// CSRG (host spmv_csrg_fill) stores the entries group after group, each
// group owning the x lines of 1/G of the columns; the tiled kernel runs the
// (row, group) pairs in that order, so the tiles in flight gather from one
// group's lines (~5 MB at G = 16) and mostly hit L2.  Each pair's sum goes
// to yp; csrg_reduce_kernel then adds a row block's pair sums in group order
// in LDS: every group's pairs of the block are one contiguous run of yp
// (blk_off), read as a stream.  Deterministic; the row sums are grouped
// differently from CSR's, so y agrees with it to the parity rule.
__global__ __launch_bounds__(kBlock) void csrg_reduce_kernel(int64_t n_rows, int32_t groups, int64_t nb,
                                                             const int32_t *__restrict__ blk_off,
                                                             const uint16_t *__restrict__ pair_row,
                                                             const double *__restrict__ yp, double *__restrict__ y)
{
    constexpr int B = SPMV_CSRG_ROWS;
    __shared__ double s_y[B];
    const int64_t b = blockIdx.x;
    for (int i = threadIdx.x; i < B; i += kBlock)
        s_y[i] = 0.0;
    __syncthreads();
    for (int32_t g = 0; g < groups; ++g) {  // group order: a row's pair sums added g = 0, 1, ...
        const int32_t p0 = blk_off[(int64_t)g * (nb + 1) + b], p1 = blk_off[(int64_t)g * (nb + 1) + b + 1];
        for (int32_t p = p0 + (int32_t)threadIdx.x; p < p1; p += 4 * kBlock) {
            double v[4];
            int r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {  // 4 loads in flight; a row appears once per group
                const int32_t pk = p + k * kBlock;
                r[k] = pk < p1 ? (int)pair_row[pk] : -1;
                v[k] = pk < p1 ? yp[pk] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (r[k] >= 0)
                    s_y[r[k]] += v[k];
        }
        __syncthreads();
    }
    const int64_t r0 = b * B;
    for (int i = threadIdx.x; i < B; i += kBlock)
        if (r0 + i < n_rows)
            store_y(y + r0 + i, s_y[i]);
}

extern "C" size_t spmv_csrg_ws_bytes(int64_t n_pairs, int64_t nnz)
{
    return (size_t)(n_pairs > 0 ? n_pairs : 0) * sizeof(double) + spmv_csr_tiled_ws_bytes(n_pairs, nnz);
}

extern "C" int spmv_csrg_run(spmv_dims d, int32_t groups, int64_t n_pairs, const int64_t *pair_ptr,
                             const int32_t *col_g, const double *val_g, const int32_t *own_lo_plan,
                             const int32_t *blk_off, const uint16_t *pair_row, const double *x, double *y,
                             void *ws, size_t ws_bytes)
{
    if (d.n_rows < 0 || d.n_cols < 0 || d.nnz < 0 || d.n_rows > INT32_MAX || n_pairs < 0 ||
        n_pairs > INT32_MAX || n_pairs > d.nnz || (d.nnz > 0 && n_pairs == 0) || groups < 1 || groups > 64)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csrg_run: bad sizes");
    if (d.n_rows == 0)
        return SPMV_SUCCESS;
    SPMV_GUARD(d);
    if (d.nnz == 0) {
        hipError_t e = hipMemsetAsync(y, 0, (size_t)d.n_rows * sizeof(double), (hipStream_t)d.stream);
        return e == hipSuccess ? SPMV_SUCCESS : fail(SPMV_PROGRAM_ERROR, "memset y", e);
    }
    if (!pair_ptr || !col_g || !val_g || !blk_off || !pair_row || !ws ||
        ws_bytes < spmv_csrg_ws_bytes(n_pairs, d.nnz))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_csrg_run: arrays or workspace missing");
    double *yp = (double *)ws;
    spmv_dims pd = d;  // the pair CSR: one "row" per (row, group) pair
    pd.n_rows = n_pairs;
    int rc = run_tiled_hot(pd, pair_ptr, col_g, val_g, x, yp, 0, nullptr, own_lo_plan, yp + n_pairs,
                           "spmv_csrg_run");
    if (rc != SPMV_SUCCESS)
        return rc;
    const int64_t nb = (d.n_rows + SPMV_CSRG_ROWS - 1) / SPMV_CSRG_ROWS;
    hipLaunchKernelGGL(csrg_reduce_kernel, dim3((unsigned)nb), dim3(kBlock), 0, (hipStream_t)d.stream, d.n_rows,
                       groups, nb, blk_off, pair_row, yp, y);
    SPMV_CHECK_LAUNCH("csrg_reduce_kernel");
    return SPMV_SUCCESS;
}
