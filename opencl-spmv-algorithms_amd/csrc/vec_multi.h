// vec_multi.h — what the block vector kernels (vec_multi.hip) share with the
// fused preconditioner kernels (precond.hip): the lane shape (a thread owns a
// row and up to kVecW adjacent columns), the column loads, the 16-byte rule
// and the geometry of the fixed two-stage dot tree.  precond.hip's sums must
// have spmv_dot_multi's bits, so G(n) and the final kernel exist once, here.
#pragma once

#include "common.h"

namespace spmv {

constexpr int kVecW = 8;               // columns per thread and pass
constexpr int kDotMultiBlocks = 1024;  // stage-1 partials per column (fixed by n -> deterministic)

// W adjacent doubles of one row; VEC: p is 16-byte aligned and W is even
template <int W, bool VEC>
__device__ __forceinline__ void load_cols(const double *__restrict__ p, double (&v)[W])
{
    if constexpr (VEC) {
#pragma unroll
        for (int c = 0; c < W / 2; ++c) {
            const double2 t = reinterpret_cast<const double2 *>(p)[c];
            v[2 * c] = t.x;
            v[2 * c + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int c = 0; c < W; ++c)
            v[c] = p[c];
    }
}

template <int W, bool VEC>
__device__ __forceinline__ void store_cols(double *__restrict__ p, const double (&v)[W])
{
    if constexpr (VEC) {
#pragma unroll
        for (int c = 0; c < W / 2; ++c)
            reinterpret_cast<double2 *>(p)[c] = double2{v[2 * c], v[2 * c + 1]};
    } else {
#pragma unroll
        for (int c = 0; c < W; ++c)
            p[c] = v[c];
    }
}

// the end of a stage-1 workgroup: each of its W columns' accumulator pairs is
// summed over the wave (xor butterfly), the four wave sums pairwise, into
// partial[(col0 + c) * G + workgroup]
template <int W>
__device__ __forceinline__ void dot_partial_store(const double (&s0)[W], const double (&s1)[W],
                                                  double (&s_warp)[W][kBlock / kWave], int64_t col0,
                                                  double *__restrict__ partial)
{
#pragma unroll
    for (int c = 0; c < W; ++c) {
        const double t = group_sum<kWave>(s0[c] + s1[c]);
        if (threadIdx.x % kWave == 0)
            s_warp[c][threadIdx.x / kWave] = t;
    }
    __syncthreads();
    if ((int)threadIdx.x < W) {
        const double *s = s_warp[threadIdx.x];
        partial[(col0 + (int64_t)threadIdx.x) * gridDim.x + blockIdx.x] = (s[0] + s[1]) + (s[2] + s[3]);
    }
}

// stage 2 of the dot tree (vec_multi.hip): workgroup j folds column j's G
// partials in a fixed order
__global__ __launch_bounds__(1024) void dot_multi_final_kernel(int g, const double *__restrict__ partial, double *__restrict__ out);

// G: a function of n alone (the bit rule); every thread has two rows, one
// per accumulator, before another workgroup is added
inline int dot_multi_blocks(int64_t n)
{
    const int64_t per = (int64_t)kBlock * 2;
    const int64_t g = (n + per - 1) / per;
    return (int)(g < 1 ? 1 : (g > kDotMultiBlocks ? kDotMultiBlocks : g));
}

// the 16-byte path of a launch whose first column is j0: W even, the first
// element 16-byte aligned and an even ld, so that every row start is aligned
inline bool vec_ok(const double *p, int64_t ld, int32_t j0, int w)
{
    return w % 2 == 0 && ld % 2 == 0 && (reinterpret_cast<uintptr_t>(p + j0) & 15) == 0;
}

// f(W, VEC, j0, chunks) for the whole blocks of kVecW columns, then for the
// k % kVecW columns left: at most two launches.  ok(j0, w) says whether EVERY
// operand of the launch that starts at column j0 with w columns per thread
// passes vec_ok
template <typename OK, typename F>
inline void for_column_blocks_if(int32_t k, OK &&ok, F &&f)
{
    const int32_t whole = k / kVecW, rest = k % kVecW;
    if (whole > 0)
        with_bool(ok(0, kVecW), [&](auto V) { f(std::integral_constant<int, kVecW>{}, V, 0, whole); });
    if (rest > 0) {
        const int32_t j0 = whole * kVecW;
        with_bool(ok(j0, rest), [&](auto V) { with_int<1, 2, 3, 4, 5, 6, 7>(rest, [&](auto Wc) { f(Wc, V, j0, 1); }); });
    }
}

// the same for a kernel with two operands
template <typename F>
inline void for_column_blocks(int32_t k, const double *a, int64_t lda, const double *b, int64_t ldb, F &&f)
{
    for_column_blocks_if(k, [&](int32_t j0, int w) { return vec_ok(a, lda, j0, w) && vec_ok(b, ldb, j0, w); }, f);
}

}  // namespace spmv
