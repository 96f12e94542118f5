// vec_multi.hip — the fp64 BLOCK vector kernels of multi-right-hand-side CG
// (iterate.cg_multi): vec.hip's dot product and ratio updates on k vectors
// at once, stored as spmv_plan_run_multi stores them (row-major,
// V[i*ld + j], j < k <= ld, 8-byte alignment).  The reference has no
// counterpart (it runs one SpMV and stops, reference csr.c:198-236).
//
// One lane shape for all three kernels: a thread owns a ROW and up to
// kVecW = 8 adjacent columns of it, blockIdx.y picks the block of 8 columns.
// With ld == k <= 8 the 64 rows of a wave are 64*k contiguous doubles, so
// the wave's loads together cover whole lines; a host check of base and ld
// (VEC) turns the per-row loads into 16-byte ones.  k > 8 reads the same
// lines once per block of 8 columns (a second launch handles k % 8).
//
// Bit rules.  Row i of the dot product belongs to workgroup, thread and
// step (i / 256) % G, i % 256, i / (256 G), with G a function of n alone,
// and column j has its own accumulator pair fed by fma() in row order: out[j]
// depends on n and on column j of A and B, not on k, ld, alignment or VEC.
// The updates are one fma per element with c_j computed the same way by
// every thread.
#include "vec_multi.h"

namespace spmv {

// stage 1: columns j0 + W*blockIdx.y + [0, W); workgroup b sums rows
// b*256 + t + s*G*256 (even steps s into s0, odd into s1) and writes
// partial[column * G + b]
template <int W, bool VEC>
__global__ __launch_bounds__(kBlock) void dot_multi_partial_kernel(int64_t n, int32_t j0,
                                                                   const double *__restrict__ A, int64_t lda,
                                                                   const double *__restrict__ B, int64_t ldb,
                                                                   double *__restrict__ partial)
{
    __shared__ double s_warp[W][kBlock / kWave];
    const int32_t j = j0 + W * (int32_t)blockIdx.y;
    A += j;
    B += j;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double s0[W], s1[W];
#pragma unroll
    for (int c = 0; c < W; ++c)
        s0[c] = s1[c] = 0.0;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + stride < n; i += 2 * stride) {
        double a0[W], b0[W], a1[W], b1[W];
        load_cols<W, VEC>(A + i * lda, a0);
        load_cols<W, VEC>(B + i * ldb, b0);
        load_cols<W, VEC>(A + (i + stride) * lda, a1);
        load_cols<W, VEC>(B + (i + stride) * ldb, b1);
#pragma unroll
        for (int c = 0; c < W; ++c) {
            s0[c] = fma(a0[c], b0[c], s0[c]);
            s1[c] = fma(a1[c], b1[c], s1[c]);
        }
    }
    if (i < n) {
        double a0[W], b0[W];
        load_cols<W, VEC>(A + i * lda, a0);
        load_cols<W, VEC>(B + i * ldb, b0);
#pragma unroll
        for (int c = 0; c < W; ++c)
            s0[c] = fma(a0[c], b0[c], s0[c]);
    }
    dot_partial_store<W>(s0, s1, s_warp, j, partial);
}

// stage 2: workgroup j folds column j's G partials in a fixed order
__global__ __launch_bounds__(1024) void dot_multi_final_kernel(int g, const double *__restrict__ partial,
                                                               double *__restrict__ out)
{
    __shared__ double s_warp[1024 / kWave];
    const double *p = partial + (int64_t)blockIdx.x * g;
    double v = (int)threadIdx.x < g ? p[threadIdx.x] : 0.0;
    v = group_sum<kWave>(v);
    if (threadIdx.x % kWave == 0)
        s_warp[threadIdx.x / kWave] = v;
    __syncthreads();
    if (threadIdx.x < kWave) {
        double t = threadIdx.x < 1024 / kWave ? s_warp[threadIdx.x] : 0.0;
        t = group_sum<kWave>(t);
        if (threadIdx.x == 0)
            out[blockIdx.x] = t;
    }
}

// XPAY = false: Y = fma(c_j, X, Y), c_j = sign * (num[j] / den[j])
// XPAY = true:  Y = fma(c_j, Y, X), c_j = num[j] / den[j]
// den[j] == 0 gives c_j = 0 (the header has the reason).  U rows per step
// are loaded before the first store.
template <int W, bool VEC, bool XPAY>
__global__ __launch_bounds__(kBlock) void update_multi_kernel(int64_t n, int32_t j0, const double *__restrict__ num,
                                                              const double *__restrict__ den, double sign,
                                                              const double *__restrict__ X, int64_t ldx,
                                                              double *__restrict__ Y, int64_t ldy)
{
    constexpr int U = W >= 4 ? 2 : 4;
    const int32_t j = j0 + W * (int32_t)blockIdx.y;
    double c[W];
#pragma unroll
    for (int q = 0; q < W; ++q) {
        const double d = den[j + q];
        const double r = num[j + q] / d;
        c[q] = d == 0.0 ? 0.0 : (XPAY ? r : sign * r);
    }
    X += j;
    Y += j;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + (U - 1) * stride < n; i += U * stride) {
        double x[U][W], y[U][W];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            load_cols<W, VEC>(X + (i + u * stride) * ldx, x[u]);
            load_cols<W, VEC>(Y + (i + u * stride) * ldy, y[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int q = 0; q < W; ++q)
                y[u][q] = XPAY ? fma(c[q], y[u][q], x[u][q]) : fma(c[q], x[u][q], y[u][q]);
            store_cols<W, VEC>(Y + (i + u * stride) * ldy, y[u]);
        }
    }
    for (; i < n; i += stride) {
        double x[W], y[W];
        load_cols<W, VEC>(X + i * ldx, x);
        load_cols<W, VEC>(Y + i * ldy, y);
#pragma unroll
        for (int q = 0; q < W; ++q)
            y[q] = XPAY ? fma(c[q], y[q], x[q]) : fma(c[q], x[q], y[q]);
        store_cols<W, VEC>(Y + i * ldy, y);
    }
}

static unsigned update_multi_grid(int64_t n)
{
    const int64_t g = (n + kBlock * 4 - 1) / (kBlock * 4);
    return (unsigned)(g < 1 ? 1 : (g > 256 * 16 ? 256 * 16 : g));
}

template <bool XPAY>
static int update_multi(const char *who, int64_t n, int32_t k, const double *num, const double *den, double sign,
                        const double *X, int64_t ldx, double *Y, int64_t ldy, int device, void *stream)
{
    if (n < 0 || k < 1 || !num || !den || ldx < k || ldy < k || (n > 0 && (!X || !Y)))
        return fail_msg(SPMV_OTHER_ERROR, who);
    if (n == 0)
        return SPMV_SUCCESS;
    DeviceGuard guard(device);
    if (guard.rc() != SPMV_SUCCESS)
        return guard.rc();
    const unsigned g = update_multi_grid(n);
    for_column_blocks(k, X, ldx, Y, ldy, [&](auto Wc, auto V, int32_t j0, int32_t chunks) {
        constexpr int W = decltype(Wc)::value;
        constexpr bool VEC = decltype(V)::value && W % 2 == 0;
        hipLaunchKernelGGL((update_multi_kernel<W, VEC, XPAY>), dim3(g, (unsigned)chunks), dim3(kBlock), 0,
                           (hipStream_t)stream, n, j0, num, den, sign, X, ldx, Y, ldy);
    });
    SPMV_CHECK_LAUNCH("update_multi_kernel");
    return SPMV_SUCCESS;
}

}  // namespace spmv

using namespace spmv;

extern "C" size_t spmv_dot_multi_ws_bytes(int64_t n, int32_t k)
{
    return (size_t)dot_multi_blocks(n) * (size_t)(k < 1 ? 1 : k) * sizeof(double);
}

extern "C" int spmv_dot_multi(int64_t n, int32_t k, const double *A, int64_t lda, const double *B, int64_t ldb,
                              double *out, void *ws, size_t ws_bytes, int device, void *stream)
{
    if (n < 0 || k < 1 || !out || lda < k || ldb < k || (n > 0 && (!A || !B)))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_dot_multi: bad arguments (n >= 0, k >= 1, lda and ldb >= k)");
    const int g = dot_multi_blocks(n);
    if (!ws || ws_bytes < (size_t)g * (size_t)k * sizeof(double))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_dot_multi: workspace too small");
    DeviceGuard guard(device);
    if (guard.rc() != SPMV_SUCCESS)
        return guard.rc();
    const hipStream_t st = (hipStream_t)stream;
    for_column_blocks(k, A, lda, B, ldb, [&](auto Wc, auto V, int32_t j0, int32_t chunks) {
        constexpr int W = decltype(Wc)::value;
        constexpr bool VEC = decltype(V)::value && W % 2 == 0;
        hipLaunchKernelGGL((dot_multi_partial_kernel<W, VEC>), dim3(g, (unsigned)chunks), dim3(kBlock), 0, st, n, j0,
                           A, lda, B, ldb, (double *)ws);
    });
    hipLaunchKernelGGL(dot_multi_final_kernel, dim3((unsigned)k), dim3(1024), 0, st, g, (const double *)ws, out);
    SPMV_CHECK_LAUNCH("dot_multi kernels");
    return SPMV_SUCCESS;
}

extern "C" int spmv_axpy_ratio_multi(int64_t n, int32_t k, const double *num, const double *den, double sign,
                                     const double *X, int64_t ldx, double *Y, int64_t ldy, int device, void *stream)
{
    return update_multi<false>("spmv_axpy_ratio_multi: bad arguments (n >= 0, k >= 1, ldx and ldy >= k)", n, k, num,
                               den, sign, X, ldx, Y, ldy, device, stream);
}

extern "C" int spmv_xpay_ratio_multi(int64_t n, int32_t k, const double *num, const double *den, const double *X,
                                     int64_t ldx, double *Y, int64_t ldy, int device, void *stream)
{
    return update_multi<true>("spmv_xpay_ratio_multi: bad arguments (n >= 0, k >= 1, ldx and ldy >= k)", n, k, num,
                              den, 1.0, X, ldx, Y, ldy, device, stream);
}
