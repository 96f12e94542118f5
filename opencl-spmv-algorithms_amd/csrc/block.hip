// block.hip — the two fp64 BLOCK kernels of the LOBPCG eigensolver
// (iterate.lobpcg), on vec_multi.hip's layout (row-major, V[i*ld + j],
// j < k <= ld, 8-byte alignment): all pairwise inner products of two
// tall-skinny blocks in one pass (spmv_gram_multi) and a tall-skinny block
// times a small host matrix (spmv_block_combine_multi).  The reference has no
// counterpart (it runs one SpMV and stops, reference csr.c:198-236).
//
// Gram.  A thread owns a ROW, kGramTile adjacent columns of A and kGramTile of
// B: blockIdx.y picks the tile of A's columns, blockIdx.z that of B's, and the
// thread carries the tile's TA x TB accumulator pairs.  Pair (a, b) is
// "column" a*kb + b of spmv_dot_multi's tree: the rows of a workgroup, the
// accumulator a row feeds, dot_partial_store and dot_multi_final_kernel are
// vec_multi's, so out[a*kb + b] has the bits of spmv_dot_multi(n, 1, A + a,
// lda, B + b, ldb).  A block is read once per tile of the OTHER block's
// columns (k = 8: twice) instead of once per column.
//
// Combine.  A thread owns a row of Y: it walks the row of S = [A0 A1 A2] from
// left to right and feeds kc fma chains, C arriving by value in the kernel
// arguments (nothing is uploaded).
#include "vec_multi.h"

namespace spmv {

// 4 x 4 pairs, two accumulators each: 32 doubles of accumulators and 16 of
// operands for the two rows in flight (profiles/lobpcg/README.md has the
// compiler's register figures for this and the larger tiles)
constexpr int kGramTile = 4;
constexpr int kGramMax = 24;  // three blocks of 8: LOBPCG's whole basis

template <int TA, int TB, bool VA, bool VB>
__global__ __launch_bounds__(kBlock) void gram_partial_kernel(int64_t n, int32_t a0, int32_t b0, int32_t kb,
                                                              const double *__restrict__ A, int64_t lda,
                                                              const double *__restrict__ B, int64_t ldb,
                                                              double *__restrict__ partial)
{
    __shared__ double s_warp[TA][TB][kBlock / kWave];
    const int32_t ja = a0 + TA * (int32_t)blockIdx.y, jb = b0 + TB * (int32_t)blockIdx.z;
    A += ja;
    B += jb;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double s0[TA][TB], s1[TA][TB];
#pragma unroll
    for (int a = 0; a < TA; ++a)
#pragma unroll
        for (int b = 0; b < TB; ++b)
            s0[a][b] = s1[a][b] = 0.0;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + stride < n; i += 2 * stride) {
        double x0[TA], y0[TB], x1[TA], y1[TB];
        load_cols<TA, VA>(A + i * lda, x0);
        load_cols<TB, VB>(B + i * ldb, y0);
        load_cols<TA, VA>(A + (i + stride) * lda, x1);
        load_cols<TB, VB>(B + (i + stride) * ldb, y1);
#pragma unroll
        for (int a = 0; a < TA; ++a)
#pragma unroll
            for (int b = 0; b < TB; ++b) {
                s0[a][b] = fma(x0[a], y0[b], s0[a][b]);
                s1[a][b] = fma(x1[a], y1[b], s1[a][b]);
            }
    }
    if (i < n) {
        double x0[TA], y0[TB];
        load_cols<TA, VA>(A + i * lda, x0);
        load_cols<TB, VB>(B + i * ldb, y0);
#pragma unroll
        for (int a = 0; a < TA; ++a)
#pragma unroll
            for (int b = 0; b < TB; ++b)
                s0[a][b] = fma(x0[a], y0[b], s0[a][b]);
    }
    // row a of the tile: TB adjacent "columns" of the tree, each row of pairs
    // through its own slice of s_warp (no barrier between the rows)
#pragma unroll
    for (int a = 0; a < TA; ++a)
        dot_partial_store<TB>(s0[a], s1[a], s_warp[a], (int64_t)(ja + a) * kb + jb, partial);
}

// f(T, j0, tiles) for the whole tiles of kGramTile columns, then for the
// k % kGramTile columns left
template <typename F>
inline void for_gram_tiles(int32_t k, F &&f)
{
    const int32_t whole = k / kGramTile, rest = k % kGramTile;
    if (whole > 0)
        f(std::integral_constant<int, kGramTile>{}, 0, whole);
    if (rest > 0)
        with_int<1, 2, 3>(rest, [&](auto T) { f(T, whole * kGramTile, 1); });
}
static_assert(kGramTile == 4, "for_gram_tiles lists the widths below the tile");

constexpr int kCombineMax = 8;         // widest operand and widest Y
constexpr int kCombineRows = 2;        // rows a thread has in flight
constexpr int kCombineGridCap = 4096;  // workgroups; more rows: more steps per thread

// C of spmv_block_combine_multi, by value: row r of S times column c of Y at
// c[r * KC + c]
struct CombineMatrix {
    double c[3 * kCombineMax * kCombineMax];
};

struct CombineOperands {
    const double *p[3];
    int64_t ld[3];
    int32_t k[3];
};

// s[c] = fma(row[r], C[(r0 + r) * KC + c], s[c]) for r = 0 .. ka - 1, in that
// order for every c; VEC: row is 16-byte aligned, columns are read in pairs
template <int KC, bool VEC>
__device__ __forceinline__ void combine_row(const double *__restrict__ row, int32_t ka, const double *crow,
                                            double (&s)[KC])
{
    int32_t r = 0;
    if constexpr (VEC) {
        for (; r + 1 < ka; r += 2) {
            const double2 t = *reinterpret_cast<const double2 *>(row + r);
#pragma unroll
            for (int c = 0; c < KC; ++c)
                s[c] = fma(t.x, crow[r * KC + c], s[c]);
#pragma unroll
            for (int c = 0; c < KC; ++c)
                s[c] = fma(t.y, crow[(r + 1) * KC + c], s[c]);
        }
    }
    for (; r < ka; ++r) {
        const double t = row[r];
#pragma unroll
        for (int c = 0; c < KC; ++c)
            s[c] = fma(t, crow[r * KC + c], s[c]);
    }
}

template <int KC, bool VEC>
__device__ __forceinline__ void combine_rows_of(const CombineOperands &o, const CombineMatrix &m, int64_t i,
                                                double (&s)[KC])
{
#pragma unroll
    for (int c = 0; c < KC; ++c)
        s[c] = 0.0;
    int32_t r0 = 0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        if (o.k[q] > 0)
            combine_row<KC, VEC>(o.p[q] + i * o.ld[q], o.k[q], m.c + r0 * KC, s);
        r0 += o.k[q];
    }
}

// VIN: every operand present is 16-byte aligned with an even ld; VOUT: so is
// Y, and KC is even
template <int KC, bool VIN, bool VOUT>
__global__ __launch_bounds__(kBlock) void block_combine_kernel(int64_t n, CombineOperands o, CombineMatrix m,
                                                               double *__restrict__ Y, int64_t ldy)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + (kCombineRows - 1) * stride < n; i += kCombineRows * stride) {
        double s[kCombineRows][KC];
#pragma unroll
        for (int u = 0; u < kCombineRows; ++u)
            combine_rows_of<KC, VIN>(o, m, i + u * stride, s[u]);
#pragma unroll
        for (int u = 0; u < kCombineRows; ++u)
            store_cols<KC, VOUT>(Y + (i + u * stride) * ldy, s[u]);
    }
    for (; i < n; i += stride) {
        double s[KC];
        combine_rows_of<KC, VIN>(o, m, i, s);
        store_cols<KC, VOUT>(Y + i * ldy, s);
    }
}

static unsigned combine_grid(int64_t n)
{
    const int64_t per = (int64_t)kBlock * kCombineRows;
    const int64_t g = (n + per - 1) / per;
    return (unsigned)(g < 1 ? 1 : (g > kCombineGridCap ? kCombineGridCap : g));
}

// the pair loads of combine_row: a 16-byte base and an even ld (any width: an
// odd last column is read alone)
static bool pair_ok(const double *p, int64_t ld)
{
    return ld % 2 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

}  // namespace spmv

using namespace spmv;

static bool gram_widths_ok(int32_t ka, int32_t kb)
{
    return ka >= 1 && ka <= kGramMax && kb >= 1 && kb <= kGramMax;
}

extern "C" size_t spmv_gram_multi_ws_bytes(int64_t n, int32_t ka, int32_t kb)
{
    const size_t pairs = gram_widths_ok(ka, kb) ? (size_t)ka * (size_t)kb : 1;
    return (size_t)dot_multi_blocks(n) * pairs * sizeof(double);
}

extern "C" int spmv_gram_multi(int64_t n, int32_t ka, const double *A, int64_t lda, int32_t kb, const double *B,
                               int64_t ldb, double *out, void *ws, size_t ws_bytes, int device, void *stream)
{
    if (n < 0 || !gram_widths_ok(ka, kb) || !out || lda < ka || ldb < kb || (n > 0 && (!A || !B)))
        return fail_msg(SPMV_OTHER_ERROR,
                        "spmv_gram_multi: bad arguments (n >= 0, ka and kb in 1..24, lda >= ka, ldb >= kb)");
    const int g = dot_multi_blocks(n);
    if (!ws || ws_bytes < (size_t)g * (size_t)ka * (size_t)kb * sizeof(double))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_gram_multi: workspace too small (spmv_gram_multi_ws_bytes)");
    DeviceGuard guard(device);
    if (guard.rc() != SPMV_SUCCESS)
        return guard.rc();
    const hipStream_t st = (hipStream_t)stream;
    for_gram_tiles(ka, [&](auto Ta, int32_t a0, int32_t tiles_a) {
        constexpr int TA = decltype(Ta)::value;
        with_bool(vec_ok(A, lda, a0, TA), [&](auto Va) {
            constexpr bool VA = decltype(Va)::value && TA % 2 == 0;
            for_gram_tiles(kb, [&](auto Tb, int32_t b0, int32_t tiles_b) {
                constexpr int TB = decltype(Tb)::value;
                with_bool(vec_ok(B, ldb, b0, TB), [&](auto Vb) {
                    constexpr bool VB = decltype(Vb)::value && TB % 2 == 0;
                    hipLaunchKernelGGL((gram_partial_kernel<TA, TB, VA, VB>),
                                       dim3(g, (unsigned)tiles_a, (unsigned)tiles_b), dim3(kBlock), 0, st, n, a0, b0,
                                       kb, A, lda, B, ldb, (double *)ws);
                });
            });
        });
    });
    hipLaunchKernelGGL(dot_multi_final_kernel, dim3((unsigned)(ka * kb)), dim3(1024), 0, st, g, (const double *)ws,
                       out);
    SPMV_CHECK_LAUNCH("gram_multi kernels");
    return SPMV_SUCCESS;
}

extern "C" int spmv_block_combine_multi(int64_t n, int32_t kc, const double *C, int32_t ka0, const double *A0,
                                        int64_t lda0, int32_t ka1, const double *A1, int64_t lda1, int32_t ka2,
                                        const double *A2, int64_t lda2, double *Y, int64_t ldy, int device,
                                        void *stream)
{
    const int32_t ka[3] = {ka0, ka1, ka2};
    const double *const p[3] = {A0, A1, A2};
    const int64_t ld[3] = {lda0, lda1, lda2};
    bool ok = n >= 0 && kc >= 1 && kc <= kCombineMax && C && ldy >= kc && (n == 0 || Y);
    int32_t total = 0;
    for (int q = 0; q < 3 && ok; ++q) {
        ok = ka[q] >= 0 && ka[q] <= kCombineMax && (ka[q] == 0 || (ld[q] >= ka[q] && (n == 0 || p[q])));
        total += ok ? ka[q] : 0;
    }
    if (!ok || total < 1)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_block_combine_multi: bad arguments (n >= 0, kc in 1..8, every ka in "
                                          "0..8 and one above 0, lda >= ka, ldy >= kc)");
    if (n == 0)
        return SPMV_SUCCESS;
    DeviceGuard guard(device);
    if (guard.rc() != SPMV_SUCCESS)
        return guard.rc();
    CombineOperands o;
    CombineMatrix m;
    bool vin = true;
    for (int q = 0; q < 3; ++q) {
        o.p[q] = ka[q] > 0 ? p[q] : nullptr;
        o.ld[q] = ka[q] > 0 ? ld[q] : 0;
        o.k[q] = ka[q];
        vin = vin && (ka[q] == 0 || pair_ok(p[q], ld[q]));
    }
    for (int32_t e = 0; e < total * kc; ++e)
        m.c[e] = C[e];
    for (int32_t e = total * kc; e < 3 * kCombineMax * kCombineMax; ++e)
        m.c[e] = 0.0;
    const unsigned g = combine_grid(n);
    with_int<1, 2, 3, 4, 5, 6, 7, 8>(kc, [&](auto Kc) {
        constexpr int KC = decltype(Kc)::value;
        with_bool(vin, [&](auto Vi) {
            with_bool(vec_ok(Y, ldy, 0, KC), [&](auto Vo) {
                constexpr bool VOUT = decltype(Vo)::value && KC % 2 == 0;
                hipLaunchKernelGGL((block_combine_kernel<KC, decltype(Vi)::value, VOUT>), dim3(g), dim3(kBlock), 0,
                                   (hipStream_t)stream, n, o, m, Y, ldy);
            });
        });
    });
    SPMV_CHECK_LAUNCH("block_combine_kernel");
    return SPMV_SUCCESS;
}
