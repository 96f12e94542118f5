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

// stage 1 of spmv_dot2_multi: dot_multi_partial_kernel with a second right
// operand, so that A is read once.  Columns j (A.B) and k + j (A.C) of
// `partial`; SAME: C is A itself and is not loaded.  Rows, accumulators and
// fold are dot_multi_partial_kernel's, hence so are the bits of both sums.
template <int W, bool VEC, bool SAME>
__global__ __launch_bounds__(kBlock) void dot2_multi_partial_kernel(int64_t n, int32_t j0, int32_t k,
                                                                    const double *__restrict__ A, int64_t lda,
                                                                    const double *__restrict__ B, int64_t ldb,
                                                                    const double *__restrict__ C, int64_t ldc,
                                                                    double *__restrict__ partial)
{
    __shared__ double s_ab[W][kBlock / kWave], s_ac[W][kBlock / kWave];
    const int32_t j = j0 + W * (int32_t)blockIdx.y;
    A += j;
    B += j;
    C += j;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double ab0[W], ab1[W], ac0[W], ac1[W];
#pragma unroll
    for (int c = 0; c < W; ++c)
        ab0[c] = ab1[c] = ac0[c] = ac1[c] = 0.0;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + stride < n; i += 2 * stride) {
        double a0[W], b0[W], c0[W], a1[W], b1[W], c1[W];
        load_cols<W, VEC>(A + i * lda, a0);
        load_cols<W, VEC>(B + i * ldb, b0);
        load_cols<W, VEC>(A + (i + stride) * lda, a1);
        load_cols<W, VEC>(B + (i + stride) * ldb, b1);
        if constexpr (!SAME) {
            load_cols<W, VEC>(C + i * ldc, c0);
            load_cols<W, VEC>(C + (i + stride) * ldc, c1);
        }
#pragma unroll
        for (int c = 0; c < W; ++c) {
            ab0[c] = fma(a0[c], b0[c], ab0[c]);
            ab1[c] = fma(a1[c], b1[c], ab1[c]);
            ac0[c] = fma(a0[c], SAME ? a0[c] : c0[c], ac0[c]);
            ac1[c] = fma(a1[c], SAME ? a1[c] : c1[c], ac1[c]);
        }
    }
    if (i < n) {
        double a0[W], b0[W], c0[W];
        load_cols<W, VEC>(A + i * lda, a0);
        load_cols<W, VEC>(B + i * ldb, b0);
        if constexpr (!SAME)
            load_cols<W, VEC>(C + i * ldc, c0);
#pragma unroll
        for (int c = 0; c < W; ++c) {
            ab0[c] = fma(a0[c], b0[c], ab0[c]);
            ac0[c] = fma(a0[c], SAME ? a0[c] : c0[c], ac0[c]);
        }
    }
    dot_partial_store<W>(ab0, ab1, s_ab, j, partial);
    dot_partial_store<W>(ac0, ac1, s_ac, (int64_t)k + j, partial);
}

// c = num / den, and 0 when den == 0: the rule of update_multi_kernel
__device__ __forceinline__ double guarded_ratio(double num, double den)
{
    const double r = num / den;
    return den == 0.0 ? 0.0 : r;
}

// the operands of spmv_bicgstab_update_dot_multi, already moved to a launch's
// first column
struct BicgstabOperands {
    const double *Ph;
    int64_t ldph;
    const double *Sh;  // never read when Sh is R (SR)
    int64_t ldsh;
    const double *T;
    int64_t ldt;
    const double *R0;
    int64_t ldr0;
    double *X;
    int64_t ldx;
    double *R;
    int64_t ldr;
};

template <int W>
struct BicgstabRow {
    double ph[W], sh[W], t[W], r0[W], x[W], r[W];
};

template <int W, bool VEC, bool SR>
__device__ __forceinline__ void bicgstab_row_load(const BicgstabOperands &o, int64_t i, BicgstabRow<W> &v)
{
    load_cols<W, VEC>(o.Ph + i * o.ldph, v.ph);
    if constexpr (!SR)
        load_cols<W, VEC>(o.Sh + i * o.ldsh, v.sh);
    load_cols<W, VEC>(o.T + i * o.ldt, v.t);
    load_cols<W, VEC>(o.R0 + i * o.ldr0, v.r0);
    load_cols<W, VEC>(o.X + i * o.ldx, v.x);
    load_cols<W, VEC>(o.R + i * o.ldr, v.r);
}

// x = fma(omega, sh, fma(alpha, ph, x)), r = fma(-omega, t, r), both stored,
// and the row's terms of r0 . r and r . r (new r) into one accumulator each
template <int W, bool VEC, bool SR>
__device__ __forceinline__ void bicgstab_row_update(const BicgstabOperands &o, int64_t i, BicgstabRow<W> &v,
                                                    const double (&alpha)[W], const double (&omega)[W],
                                                    double (&r0r)[W], double (&rr)[W])
{
#pragma unroll
    for (int q = 0; q < W; ++q) {
        const double sh = SR ? v.r[q] : v.sh[q];
        v.x[q] = fma(omega[q], sh, fma(alpha[q], v.ph[q], v.x[q]));
        v.r[q] = fma(-omega[q], v.t[q], v.r[q]);
        r0r[q] = fma(v.r0[q], v.r[q], r0r[q]);
        rr[q] = fma(v.r[q], v.r[q], rr[q]);
    }
    store_cols<W, VEC>(o.X + i * o.ldx, v.x);
    store_cols<W, VEC>(o.R + i * o.ldr, v.r);
}

// spmv_bicgstab_update_dot_multi for columns j0 + W*blockIdx.y + [0, W): the
// two updates of a BiCGSTAB iteration and the sums r0 . r, r . r over the new
// r in one pass.  The rows of a workgroup, the accumulator a row feeds and the
// fold are dot_multi_partial_kernel's (the shape of bjacobi_apply_kernel), so
// partial columns j and k + j give the bits of spmv_dot_multi(R0, R) and
// spmv_dot_multi(R, R) run afterwards.  SR: Sh is R; a thread takes its
// elements of R from the row it loaded, before it stores them.  Up to four
// columns a thread has both rows of a step in flight; with more it finishes
// one row before it loads the next (six operand rows of 8 doubles each),
// which keeps W = 8 clear of scratch.
template <int W, bool VEC, bool SR>
__global__ __launch_bounds__(kBlock) void bicgstab_update_dot_kernel(int64_t n, int32_t j0, int32_t k,
                                                                     const double *__restrict__ a_num,
                                                                     const double *__restrict__ a_den,
                                                                     const double *__restrict__ w_num,
                                                                     const double *__restrict__ w_den,
                                                                     BicgstabOperands o, double *__restrict__ partial)
{
    __shared__ double s_r0r[W][kBlock / kWave], s_rr[W][kBlock / kWave];
    const int32_t j = j0 + W * (int32_t)blockIdx.y;
    double alpha[W], omega[W];
#pragma unroll
    for (int q = 0; q < W; ++q) {
        alpha[q] = guarded_ratio(a_num[j + q], a_den[j + q]);
        omega[q] = guarded_ratio(w_num[j + q], w_den[j + q]);
    }
    o.Ph += j;
    o.Sh += j;
    o.T += j;
    o.R0 += j;
    o.X += j;
    o.R += j;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double r0r0[W], r0r1[W], rr0[W], rr1[W];
#pragma unroll
    for (int c = 0; c < W; ++c)
        r0r0[c] = r0r1[c] = rr0[c] = rr1[c] = 0.0;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + stride < n; i += 2 * stride) {
        if constexpr (W <= 4) {
            BicgstabRow<W> v0, v1;
            bicgstab_row_load<W, VEC, SR>(o, i, v0);
            bicgstab_row_load<W, VEC, SR>(o, i + stride, v1);
            bicgstab_row_update<W, VEC, SR>(o, i, v0, alpha, omega, r0r0, rr0);
            bicgstab_row_update<W, VEC, SR>(o, i + stride, v1, alpha, omega, r0r1, rr1);
        } else {
            BicgstabRow<W> v;
            bicgstab_row_load<W, VEC, SR>(o, i, v);
            bicgstab_row_update<W, VEC, SR>(o, i, v, alpha, omega, r0r0, rr0);
            bicgstab_row_load<W, VEC, SR>(o, i + stride, v);
            bicgstab_row_update<W, VEC, SR>(o, i + stride, v, alpha, omega, r0r1, rr1);
        }
    }
    if (i < n) {
        BicgstabRow<W> v;
        bicgstab_row_load<W, VEC, SR>(o, i, v);
        bicgstab_row_update<W, VEC, SR>(o, i, v, alpha, omega, r0r0, rr0);
    }
    dot_partial_store<W>(r0r0, r0r1, s_r0r, j, partial);
    dot_partial_store<W>(rr0, rr1, s_rr, (int64_t)k + j, partial);
}

// spmv_bicgstab_dir_multi: P = fma(beta_j, fma(-omega_j, V, P), R) with
// beta_j = ratio(rho_new, rv) * ratio(tt, ts), omega_j = ratio(ts, tt);
// update_multi_kernel's grid-stride shape with a third operand
template <int W, bool VEC>
__global__ __launch_bounds__(kBlock) void bicgstab_dir_kernel(int64_t n, int32_t j0,
                                                              const double *__restrict__ rho_new,
                                                              const double *__restrict__ rv,
                                                              const double *__restrict__ tt,
                                                              const double *__restrict__ ts,
                                                              const double *__restrict__ V, int64_t ldv,
                                                              const double *__restrict__ R, int64_t ldr,
                                                              double *__restrict__ P, int64_t ldp)
{
    constexpr int U = W >= 4 ? 2 : 4;
    const int32_t j = j0 + W * (int32_t)blockIdx.y;
    double beta[W], nomega[W];
#pragma unroll
    for (int q = 0; q < W; ++q) {
        beta[q] = guarded_ratio(rho_new[j + q], rv[j + q]) * guarded_ratio(tt[j + q], ts[j + q]);
        nomega[q] = -guarded_ratio(ts[j + q], tt[j + q]);
    }
    V += j;
    R += j;
    P += j;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + (U - 1) * stride < n; i += U * stride) {
        double v[U][W], r[U][W], p[U][W];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            load_cols<W, VEC>(V + (i + u * stride) * ldv, v[u]);
            load_cols<W, VEC>(R + (i + u * stride) * ldr, r[u]);
            load_cols<W, VEC>(P + (i + u * stride) * ldp, p[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int q = 0; q < W; ++q)
                p[u][q] = fma(beta[q], fma(nomega[q], v[u][q], p[u][q]), r[u][q]);
            store_cols<W, VEC>(P + (i + u * stride) * ldp, p[u]);
        }
    }
    for (; i < n; i += stride) {
        double v[W], r[W], p[W];
        load_cols<W, VEC>(V + i * ldv, v);
        load_cols<W, VEC>(R + i * ldr, r);
        load_cols<W, VEC>(P + i * ldp, p);
#pragma unroll
        for (int q = 0; q < W; ++q)
            p[q] = fma(beta[q], fma(nomega[q], v[q], p[q]), r[q]);
        store_cols<W, VEC>(P + i * ldp, p);
    }
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

extern "C" int spmv_dot2_multi(int64_t n, int32_t k, const double *A, int64_t lda, const double *B, int64_t ldb,
                               const double *C, int64_t ldc, double *out, void *ws, size_t ws_bytes, int device,
                               void *stream)
{
    if (n < 0 || k < 1 || !out || lda < k || ldb < k || ldc < k || (n > 0 && (!A || !B || !C)))
        return fail_msg(SPMV_OTHER_ERROR,
                        "spmv_dot2_multi: bad arguments (n >= 0, k >= 1, lda, ldb and ldc >= k)");
    const int g = dot_multi_blocks(n);
    if (!ws || ws_bytes < (size_t)g * 2 * (size_t)k * sizeof(double))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_dot2_multi: workspace too small (spmv_dot_multi_ws_bytes(n, 2k))");
    DeviceGuard guard(device);
    if (guard.rc() != SPMV_SUCCESS)
        return guard.rc();
    const hipStream_t st = (hipStream_t)stream;
    const bool same = C == A && ldc == lda;
    const auto ok = [&](int32_t j0, int w) {
        return vec_ok(A, lda, j0, w) && vec_ok(B, ldb, j0, w) && (same || vec_ok(C, ldc, j0, w));
    };
    for_column_blocks_if(k, ok, [&](auto Wc, auto V, int32_t j0, int32_t chunks) {
        constexpr int W = decltype(Wc)::value;
        constexpr bool VEC = decltype(V)::value && W % 2 == 0;
        with_bool(same, [&](auto S) {
            hipLaunchKernelGGL((dot2_multi_partial_kernel<W, VEC, decltype(S)::value>), dim3(g, (unsigned)chunks),
                               dim3(kBlock), 0, st, n, j0, k, A, lda, B, ldb, C, ldc, (double *)ws);
        });
    });
    hipLaunchKernelGGL(dot_multi_final_kernel, dim3(2 * (unsigned)k), dim3(1024), 0, st, g, (const double *)ws, out);
    SPMV_CHECK_LAUNCH("dot2_multi kernels");
    return SPMV_SUCCESS;
}

extern "C" int spmv_bicgstab_update_dot_multi(int64_t n, int32_t k, const double *a_num, const double *a_den,
                                              const double *w_num, const double *w_den, const double *Ph,
                                              int64_t ldph, const double *Sh, int64_t ldsh, const double *T,
                                              int64_t ldt, const double *R0, int64_t ldr0, double *X, int64_t ldx,
                                              double *R, int64_t ldr, double *out, void *ws, size_t ws_bytes,
                                              int device, void *stream)
{
    if (n < 0 || k < 1 || !a_num || !a_den || !w_num || !w_den || !out || ldph < k || ldsh < k || ldt < k ||
        ldr0 < k || ldx < k || ldr < k || (n > 0 && (!Ph || !Sh || !T || !R0 || !X || !R)) ||
        (Sh && Sh == R && ldsh != ldr))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_bicgstab_update_dot_multi: bad arguments (n >= 0, k >= 1, every ld >= k, "
                                          "Sh == R only with ldsh == ldr)");
    const int g = dot_multi_blocks(n);
    if (!ws || ws_bytes < (size_t)g * 2 * (size_t)k * sizeof(double))
        return fail_msg(SPMV_OTHER_ERROR,
                        "spmv_bicgstab_update_dot_multi: workspace too small (spmv_dot_multi_ws_bytes(n, 2k))");
    DeviceGuard guard(device);
    if (guard.rc() != SPMV_SUCCESS)
        return guard.rc();
    const hipStream_t st = (hipStream_t)stream;
    const bool sr = Sh == R;
    const BicgstabOperands o{Ph, ldph, Sh, ldsh, T, ldt, R0, ldr0, X, ldx, R, ldr};
    const auto ok = [&](int32_t j0, int w) {
        return vec_ok(Ph, ldph, j0, w) && (sr || vec_ok(Sh, ldsh, j0, w)) && vec_ok(T, ldt, j0, w) &&
               vec_ok(R0, ldr0, j0, w) && vec_ok(X, ldx, j0, w) && vec_ok(R, ldr, j0, w);
    };
    for_column_blocks_if(k, ok, [&](auto Wc, auto V, int32_t j0, int32_t chunks) {
        constexpr int W = decltype(Wc)::value;
        constexpr bool VEC = decltype(V)::value && W % 2 == 0;
        with_bool(sr, [&](auto S) {
            hipLaunchKernelGGL((bicgstab_update_dot_kernel<W, VEC, decltype(S)::value>), dim3(g, (unsigned)chunks),
                               dim3(kBlock), 0, st, n, j0, k, a_num, a_den, w_num, w_den, o, (double *)ws);
        });
    });
    hipLaunchKernelGGL(dot_multi_final_kernel, dim3(2 * (unsigned)k), dim3(1024), 0, st, g, (const double *)ws, out);
    SPMV_CHECK_LAUNCH("bicgstab_update_dot kernels");
    return SPMV_SUCCESS;
}

extern "C" int spmv_bicgstab_dir_multi(int64_t n, int32_t k, const double *rho_new, const double *rv,
                                       const double *tt, const double *ts, const double *V, int64_t ldv,
                                       const double *R, int64_t ldr, double *P, int64_t ldp, int device, void *stream)
{
    if (n < 0 || k < 1 || !rho_new || !rv || !tt || !ts || ldv < k || ldr < k || ldp < k ||
        (n > 0 && (!V || !R || !P)))
        return fail_msg(SPMV_OTHER_ERROR,
                        "spmv_bicgstab_dir_multi: bad arguments (n >= 0, k >= 1, ldv, ldr and ldp >= k)");
    if (n == 0)
        return SPMV_SUCCESS;
    DeviceGuard guard(device);
    if (guard.rc() != SPMV_SUCCESS)
        return guard.rc();
    const unsigned g = update_multi_grid(n);
    const auto ok = [&](int32_t j0, int w) {
        return vec_ok(V, ldv, j0, w) && vec_ok(R, ldr, j0, w) && vec_ok(P, ldp, j0, w);
    };
    for_column_blocks_if(k, ok, [&](auto Wc, auto Vc, int32_t j0, int32_t chunks) {
        constexpr int W = decltype(Wc)::value;
        constexpr bool VEC = decltype(Vc)::value && W % 2 == 0;
        hipLaunchKernelGGL((bicgstab_dir_kernel<W, VEC>), dim3(g, (unsigned)chunks), dim3(kBlock), 0,
                           (hipStream_t)stream, n, j0, rho_new, rv, tt, ts, V, ldv, R, ldr, P, ldp);
    });
    SPMV_CHECK_LAUNCH("bicgstab_dir_kernel");
    return SPMV_SUCCESS;
}
