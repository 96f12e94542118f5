// krylov.hip — the three fp64 kernels of restarted GMRES (iterate.gmres) on
// the Krylov basis, one row-major block V[i*ldv + j], j < c <= 32 <= ldv
// (vec_multi.hip's layout, 8-byte alignment): a Gram-Schmidt projection fused
// with the c + 1 inner products the next pass needs (spmv_krylov_project_dot),
// the basis times a small host vector (spmv_krylov_combine) and the scaling of
// a new basis column (spmv_krylov_normalize).  The reference has no counterpart
// (it runs one SpMV and stops, reference csr.c:198-236).
//
// Project.  A thread owns a ROW of V, all c columns of it: w' = w - V h is one
// fma chain along the row, and every one of the c inner products V[:, j] . w'
// needs the finished w', so the row stays in registers between the two.  The
// kernel is templated on NB = ceil(c / 8) blocks of 8 columns: a basis of 5
// columns carries 9 accumulator pairs, not 33.  Slot j < c of the accumulators
// is "column" j of spmv_dot_multi's tree with A = V + j, B = w'; slot c is
// w' . w'; the slots past c stay 0.  The rows of a workgroup, the accumulator a
// row feeds, dot_partial_store and dot_multi_final_kernel are vec_multi's, so
// out[j] has the bits of spmv_dot_multi(n, 1, V + j, ldv, w', ldo).
#include "spmv_ext.h"
#include "vec_multi.h"

namespace spmv {

constexpr int kKrylovMax = SPMV_KRYLOV_MAX_COLS;
static_assert(kKrylovMax == 4 * kVecW, "the kernels are instantiated for 1..4 blocks of kVecW columns");

// columns [0, c) of a row into v[0 .. 8 NB); the columns at and past c are not
// read and come back 0.0.  c > 8 (NB - 1): only the last block is cut.
template <int NB, bool VEC>
__device__ __forceinline__ void load_basis_row(const double *__restrict__ p, int32_t c, double (&v)[kVecW * NB])
{
#pragma unroll
    for (int b = 0; b < NB - 1; ++b) {
        double t[kVecW];
        load_cols<kVecW, VEC>(p + kVecW * b, t);
#pragma unroll
        for (int q = 0; q < kVecW; ++q)
            v[kVecW * b + q] = t[q];
    }
    constexpr int j0 = kVecW * (NB - 1);
#pragma unroll
    for (int q = 0; q < kVecW; q += 2) {
        if (VEC && j0 + q + 1 < c) {
            const double2 t = *reinterpret_cast<const double2 *>(p + j0 + q);
            v[j0 + q] = t.x;
            v[j0 + q + 1] = t.y;
        } else {
            v[j0 + q] = j0 + q < c ? p[j0 + q] : 0.0;
            v[j0 + q + 1] = j0 + q + 1 < c ? p[j0 + q + 1] : 0.0;
        }
    }
}

// one row of spmv_krylov_project_dot: the chain, the store and the row's terms
// of the c + 1 sums into acc (slot 8 NB exists for c == 8 NB)
template <int NB, bool VEC>
__device__ __forceinline__ void project_row(int64_t i, int32_t c, const double *__restrict__ V, int64_t ldv,
                                            bool chain, const double (&nh)[kVecW * NB], const double *w, int64_t ldw,
                                            double *w_out, int64_t ldo, double (&acc)[kVecW * NB + 1])
{
    constexpr int C8 = kVecW * NB;
    double v[C8];
    load_basis_row<NB, VEC>(V + i * ldv, c, v);
    double s = w[i * ldw];
    if (chain) {
#pragma unroll
        for (int j = 0; j < C8; ++j)
            if (j < kVecW * (NB - 1) || j < c)
                s = fma(nh[j], v[j], s);
    }
    if (w_out)
        w_out[i * ldo] = s;
#pragma unroll
    for (int j = 0; j < C8; ++j) {
        const double a = (j >= kVecW * (NB - 1) && j == c) ? s : v[j];
        acc[j] = fma(a, s, acc[j]);
    }
    acc[C8] = fma(c == C8 ? s : 0.0, s, acc[C8]);
}

// stage 1 of spmv_krylov_project_dot.  nh[j] = -h[j] is the same for every
// thread (scalar loads).  A thread finishes one row before it loads the next:
// a row of 32 columns and 33 accumulator pairs are the registers it has.
template <int NB, bool VEC>
__global__ __launch_bounds__(kBlock) void krylov_project_dot_kernel(int64_t n, int32_t c,
                                                                    const double *__restrict__ V, int64_t ldv,
                                                                    const double *__restrict__ h, const double *w,
                                                                    int64_t ldw, double *w_out, int64_t ldo,
                                                                    double *__restrict__ partial)
{
    constexpr int C8 = kVecW * NB;
    __shared__ double s_warp[NB][kVecW][kBlock / kWave], s_last[1][kBlock / kWave];
    double nh[C8];
#pragma unroll
    for (int j = 0; j < C8; ++j)
        nh[j] = (h != nullptr && j < c) ? -h[j] : 0.0;
    const bool chain = h != nullptr;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double s0[C8 + 1], s1[C8 + 1];
#pragma unroll
    for (int j = 0; j <= C8; ++j)
        s0[j] = s1[j] = 0.0;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + stride < n; i += 2 * stride) {
        project_row<NB, VEC>(i, c, V, ldv, chain, nh, w, ldw, w_out, ldo, s0);
        project_row<NB, VEC>(i + stride, c, V, ldv, chain, nh, w, ldw, w_out, ldo, s1);
    }
    if (i < n)
        project_row<NB, VEC>(i, c, V, ldv, chain, nh, w, ldw, w_out, ldo, s0);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        double t0[kVecW], t1[kVecW];
#pragma unroll
        for (int q = 0; q < kVecW; ++q) {
            t0[q] = s0[kVecW * b + q];
            t1[q] = s1[kVecW * b + q];
        }
        dot_partial_store<kVecW>(t0, t1, s_warp[b], kVecW * b, partial);
    }
    const double l0[1] = {s0[C8]}, l1[1] = {s1[C8]};
    dot_partial_store<1>(l0, l1, s_last, C8, partial);
}

// y of spmv_krylov_combine, by value
struct KrylovCoefficients {
    double y[kKrylovMax];
};

constexpr int kKrylovGridCap = 4096;  // workgroups; more rows: more steps per thread

// t[i] = the chain s = 0; s = fma(V[i][j], y[j], s), j = 0 .. c - 1
template <int NB, bool VEC>
__global__ __launch_bounds__(kBlock) void krylov_combine_kernel(int64_t n, int32_t c, const double *__restrict__ V,
                                                                int64_t ldv, KrylovCoefficients m,
                                                                double *__restrict__ t, int64_t ldt)
{
    constexpr int C8 = kVecW * NB;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        double v[C8];
        load_basis_row<NB, VEC>(V + i * ldv, c, v);
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < C8; ++j)
            if (j < kVecW * (NB - 1) || j < c)
                s = fma(v[j], m.y[j], s);
        t[i * ldt] = s;
    }
}

// v = w r, r = 1 / sqrt(*s) and 0 for *s <= 0; COPY: also into the contiguous copy
template <bool COPY>
__global__ __launch_bounds__(kBlock) void krylov_normalize_kernel(int64_t n, const double *__restrict__ s,
                                                                  const double *w, int64_t ldw, double *v, int64_t ldv,
                                                                  double *__restrict__ copy)
{
    const double s0 = *s;
    const double inv = 1.0 / sqrt(s0);
    const double r = s0 <= 0.0 ? 0.0 : inv;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double x = w[i * ldw] * r;
        v[i * ldv] = x;
        if constexpr (COPY)
            copy[i] = x;
    }
}

static unsigned krylov_grid(int64_t n)
{
    const int64_t g = (n + kBlock - 1) / kBlock;
    return (unsigned)(g < 1 ? 1 : (g > kKrylovGridCap ? kKrylovGridCap : g));
}

// the 16-byte loads of load_basis_row: a 16-byte base and an even ld
static bool basis_vec_ok(const double *p, int64_t ld)
{
    return ld % 2 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

}  // namespace spmv

using namespace spmv;

extern "C" int spmv_krylov_project_dot(int64_t n, int32_t c, const double *V, int64_t ldv, const double *h,
                                       const double *w, int64_t ldw, double *w_out, int64_t ldo, double *out,
                                       void *ws, size_t ws_bytes, int device, void *stream)
{
    if (n < 0 || c < 1 || c > kKrylovMax || ldv < c || ldw < 1 || (w_out && ldo < 1) || !out || (h && !w_out) ||
        (n > 0 && (!V || !w)))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_krylov_project_dot: bad arguments (n >= 0, c in 1..32, ldv >= c, ldw "
                                          "and ldo >= 1, w_out may be NULL only when h is)");
    const int g = dot_multi_blocks(n);
    const int nb = (c + kVecW - 1) / kVecW;
    if (!ws || ws_bytes < (size_t)g * (size_t)(kVecW * nb + 1) * sizeof(double))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_krylov_project_dot: workspace too small "
                                          "(spmv_dot_multi_ws_bytes(n, 8 * ceil(c / 8) + 1))");
    DeviceGuard guard(device);
    if (guard.rc() != SPMV_SUCCESS)
        return guard.rc();
    const hipStream_t st = (hipStream_t)stream;
    with_int<1, 2, 3, 4>(nb, [&](auto Nb) {
        with_bool(basis_vec_ok(V, ldv), [&](auto Vc) {
            hipLaunchKernelGGL((krylov_project_dot_kernel<decltype(Nb)::value, decltype(Vc)::value>), dim3(g),
                               dim3(kBlock), 0, st, n, c, V, ldv, h, w, ldw, w_out, ldo, (double *)ws);
        });
    });
    hipLaunchKernelGGL(dot_multi_final_kernel, dim3((unsigned)c + 1), dim3(1024), 0, st, g, (const double *)ws, out);
    SPMV_CHECK_LAUNCH("krylov_project_dot kernels");
    return SPMV_SUCCESS;
}

extern "C" int spmv_krylov_combine(int64_t n, int32_t c, const double *V, int64_t ldv, const double *y_host,
                                   double *t, int64_t ldt, int device, void *stream)
{
    if (n < 0 || c < 1 || c > kKrylovMax || ldv < c || ldt < 1 || !y_host || (n > 0 && (!V || !t)))
        return fail_msg(SPMV_OTHER_ERROR,
                        "spmv_krylov_combine: bad arguments (n >= 0, c in 1..32, ldv >= c, ldt >= 1)");
    if (n == 0)
        return SPMV_SUCCESS;
    DeviceGuard guard(device);
    if (guard.rc() != SPMV_SUCCESS)
        return guard.rc();
    KrylovCoefficients m;
    for (int32_t j = 0; j < kKrylovMax; ++j)
        m.y[j] = j < c ? y_host[j] : 0.0;
    with_int<1, 2, 3, 4>((c + kVecW - 1) / kVecW, [&](auto Nb) {
        with_bool(basis_vec_ok(V, ldv), [&](auto Vc) {
            hipLaunchKernelGGL((krylov_combine_kernel<decltype(Nb)::value, decltype(Vc)::value>),
                               dim3(krylov_grid(n)), dim3(kBlock), 0, (hipStream_t)stream, n, c, V, ldv, m, t, ldt);
        });
    });
    SPMV_CHECK_LAUNCH("krylov_combine_kernel");
    return SPMV_SUCCESS;
}

extern "C" int spmv_krylov_normalize(int64_t n, const double *s, const double *w, int64_t ldw, double *v, int64_t ldv,
                                     double *copy, int device, void *stream)
{
    if (n < 0 || !s || ldw < 1 || ldv < 1 || (n > 0 && (!w || !v)))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_krylov_normalize: bad arguments (n >= 0, ldw and ldv >= 1)");
    if (n == 0)
        return SPMV_SUCCESS;
    DeviceGuard guard(device);
    if (guard.rc() != SPMV_SUCCESS)
        return guard.rc();
    with_bool(copy != nullptr, [&](auto Cp) {
        hipLaunchKernelGGL((krylov_normalize_kernel<decltype(Cp)::value>), dim3(krylov_grid(n)), dim3(kBlock), 0,
                           (hipStream_t)stream, n, s, w, ldw, v, ldv, copy);
    });
    SPMV_CHECK_LAUNCH("krylov_normalize_kernel");
    return SPMV_SUCCESS;
}
