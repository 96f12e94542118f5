// precond.hip — the block-Jacobi preconditioner of iterate.cg / cg_multi
// (spmv_bjacobi_*, spmv_ext.h): M = blockdiag(D_0, D_1, ...) with bs x bs
// blocks of the matrix's diagonal, 1 <= bs <= 16.  The reference has no
// counterpart (it runs one SpMV and stops, reference csr.c:198-236).
//
// Build (spmv_bjacobi_create).  One kernel extracts and inverts every block,
// following host/precond.c step for step: a group of G = 2^ceil(log2 bs) lanes
// owns a block, lane r its row r of [D | I] in LDS (the elimination indexes the
// tile at run time; in LDS that costs no scratch), and the group walks the
// columns together, down and then up: pivot search (every lane reads the
// column and finds the same row), the swap by the lane of the pivot's place,
// elimination by the lanes below it; then scaling and elimination above.  A
// workgroup barrier separates the steps (BS is a template argument, so every
// group of the workgroup takes the same number of steps).
// No atomics: a block is written by its own lanes only, and the singular
// blocks are flagged per block and counted on the host.
//
// Apply (spmv_bjacobi_apply_multi, spmv_bjacobi_apply_dot_multi).  The lane
// shape of vec_multi.hip: a thread owns a row and up to 8 adjacent columns; it
// reads its row of the inverse (bs doubles: a wave's rows are one contiguous
// run of `inv`) and the rows of R of its block, and forms the fma chain of
// spmv_cpu_bjacobi_apply_multi.  The fused form also feeds the two dot
// products of a PCG iteration, sum r z and sum r r, through spmv_dot_multi's
// tree: same G(n), same row -> workgroup, thread and step rule, same two
// accumulators, same fold (dot_partial_store) and the same final kernel over
// the 2k columns, so its sums have spmv_dot_multi's bits.
//
// Chebyshev step (spmv_bjacobi_cheb_step_multi, spmv_bjacobi_cheb_step_dot_multi;
// iterate.Chebyshev).  The apply's lanes and chain over t_c = R_c - AZ_c, then
// d = a D + b s and Zout = Zin + d on the thread's own elements, as
// spmv_cpu_bjacobi_cheb_step_multi states it; a and b are kernel arguments.  The
// dot form sums r z (z = Zout) and r r exactly as the fused apply does.
#include <cstdio>
#include <cstdlib>

#include "vec_multi.h"

struct spmv_bjacobi {
    int32_t bs = 0, symmetric_half = 0;
    int64_t n = 0, n_blocks = 0, singular_blocks = 0, col_base = 0;
    int device = 0;
    double *inv = nullptr;  // owned: n_blocks * bs * bs
};

namespace spmv {

constexpr int kBjMax = 16;
constexpr int kBjThreads = 128;  // of the build kernel

constexpr int bj_group(int bs)
{
    return bs <= 1 ? 1 : bs <= 2 ? 2 : bs <= 4 ? 4 : bs <= 8 ? 8 : 16;
}

// blocks [blockIdx.x * PER, +PER), PER = 128 / G; tile rows are padded by one
// double so that the lanes of a group hit different LDS banks
template <int BS>
__global__ __launch_bounds__(kBjThreads) void bjacobi_build_kernel(int64_t n, int64_t n_blocks,
                                                                   const int64_t *__restrict__ row_ptr,
                                                                   const int32_t *__restrict__ col,
                                                                   const double *__restrict__ val, int64_t col_base,
                                                                   int symmetric_half, double *__restrict__ inv,
                                                                   uint8_t *__restrict__ bad_out)
{
    constexpr int G = bj_group(BS), PER = kBjThreads / G, LD = 2 * BS + 1;
    __shared__ double s_a[PER][BS][LD];
    __shared__ int s_bad[PER];
    const int slot = (int)threadIdx.x / G, r = (int)threadIdx.x % G;
    const int64_t q = (int64_t)blockIdx.x * PER + slot;
    const bool live = q < n_blocks && r < BS;  // a group past the last block reduces an identity and writes nothing
    const int64_t r0 = q * BS;
    const int nb = q < n_blocks ? (int)(n - r0 < BS ? n - r0 : BS) : 0;
    double(*a)[LD] = s_a[slot];
    if (r == 0)
        s_bad[slot] = 0;
    if (r < BS) {
        for (int j = 0; j < 2 * BS; ++j)
            a[r][j] = 0.0;
        a[r][BS + r] = 1.0;
        if (r >= nb)
            a[r][r] = 1.0;
    }
    __syncthreads();
    // extraction; a stored half also fills the mirrored places, row after row
    // in the host's order (one lane of the group at a time)
    const auto scan = [&](bool mirror) {
        for (int64_t e = row_ptr[r0 + r]; e < row_ptr[r0 + r + 1]; ++e) {
            const int64_t c = (int64_t)col[e] - col_base - r0;
            if (c < 0 || c >= nb)
                continue;
            a[r][c] += val[e];
            if (mirror && c != r)
                a[c][r] += val[e];
        }
    };
    if (!symmetric_half) {
        if (live && r < nb)
            scan(false);
    } else {
        for (int rr = 0; rr < BS; ++rr) {
            if (live && r == rr && r < nb)
                scan(true);
            __syncthreads();
        }
    }
    __syncthreads();
    bool sing = false;
#pragma unroll 1
    for (int p = 0; p < BS; ++p) {  // down: pivot, swap, clear the column below
        int pr = p;
        double best = fabs(a[p][p]);
        for (int r2 = p + 1; r2 < BS; ++r2) {
            const double v = fabs(a[r2][p]);
            if (v > best) {
                best = v;
                pr = r2;
            }
        }
        const double piv = a[pr][p];
        sing = sing || piv == 0.0 || !isfinite(piv);
        __syncthreads();  // every lane has its pivot before the rows move
        if (!sing && r == p && pr != p)
            for (int j = 0; j < 2 * BS; ++j) {
                const double t = a[pr][j];
                a[pr][j] = a[p][j];
                a[p][j] = t;
            }
        __syncthreads();
        if (!sing && r < BS && r > p) {
            const double f = -(a[r][p] / piv);
            for (int j = p + 1; j < 2 * BS; ++j)
                a[r][j] = fma(f, a[p][j], a[r][j]);
            a[r][p] = 0.0;
        }
        __syncthreads();
    }
#pragma unroll 1
    for (int p = BS - 1; p >= 0; --p) {  // up: scale the right half, clear the column above
        if (!sing && r == p) {
            const double piv = a[p][p];
            for (int j = BS; j < 2 * BS; ++j)
                a[p][j] = a[p][j] / piv;
        }
        __syncthreads();
        if (!sing && r < p) {
            const double f = -a[r][p];
            for (int j = BS; j < 2 * BS; ++j)
                a[r][j] = fma(f, a[p][j], a[r][j]);
        }
        __syncthreads();
    }
    if (r < BS) {
        bool bad = sing;
        for (int c = 0; c < BS; ++c)
            bad = bad || !isfinite(a[r][BS + c]);
        if (bad)
            s_bad[slot] = 1;  // every writer stores the same value
    }
    __syncthreads();
    if (live) {
        const bool bad = s_bad[slot] != 0;
        double *out = inv + (r0 + r) * BS;
        for (int c = 0; c < BS; ++c)
            out[c] = bad ? (r == c ? 1.0 : 0.0) : a[r][BS + c];
        if (r == 0)
            bad_out[q] = bad ? 1 : 0;
    }
}

// z = row i of M^-1 R for the W columns at R (already offset to the first
// column), `own` = row i of R itself.  The rows of the block are loaded four
// at a time (index clamped to the block's last row: never past row n - 1)
// before the first fma; the chain itself runs in column order, a product
// first, as spmv_cpu_bjacobi_apply_multi.
template <int W, bool VEC>
__device__ __forceinline__ void bjacobi_row(int64_t n, int32_t bs, int64_t i, const double *__restrict__ inv,
                                            const double *__restrict__ R, int64_t ldr, double (&z)[W],
                                            double (&own)[W])
{
    const int64_t q = i <= (int64_t)UINT32_MAX ? (int64_t)((uint32_t)i / (uint32_t)bs) : i / bs;
    const int64_t r0 = q * bs;
    const int32_t nb = n - r0 < bs ? (int32_t)(n - r0) : bs;
    const int32_t me = (int32_t)(i - r0);
    const double *a = inv + i * bs;
    const double *Rb = R + r0 * ldr;
#pragma unroll
    for (int w = 0; w < W; ++w)
        z[w] = own[w] = 0.0;
    for (int32_t c0 = 0; c0 < nb; c0 += 4) {
        double av[4], rv[4][W];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int32_t c = c0 + u < nb ? c0 + u : nb - 1;
            av[u] = a[c];
            load_cols<W, VEC>(Rb + (int64_t)c * ldr, rv[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int32_t c = c0 + u;
            if (c < nb) {
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    z[w] = c == 0 ? av[u] * rv[u][w] : fma(av[u], rv[u][w], z[w]);
                    own[w] = c == me ? rv[u][w] : own[w];
                }
            }
        }
    }
}

// Z = M^-1 R for columns j0 + W*blockIdx.y + [0, W).  DOT: workgroup b also
// sums r z and r r over its rows b*256 + t + s*G*256 (even steps s into the
// first accumulator, odd into the second: dot_multi_partial_kernel's rule)
// and writes partial[column * G + b], columns j (r z) and k + j (r r).
template <int W, bool VEC, bool DOT>
__global__ __launch_bounds__(kBlock) void bjacobi_apply_kernel(int64_t n, int32_t bs, int32_t j0, int32_t k,
                                                               const double *__restrict__ inv,
                                                               const double *__restrict__ R, int64_t ldr,
                                                               double *__restrict__ Z, int64_t ldz,
                                                               double *__restrict__ partial)
{
    const int32_t j = j0 + W * (int32_t)blockIdx.y;
    R += j;
    Z += j;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double rz0[W], rz1[W], rr0[W], rr1[W];
#pragma unroll
    for (int c = 0; c < W; ++c)
        rz0[c] = rz1[c] = rr0[c] = rr1[c] = 0.0;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + stride < n; i += 2 * stride) {
        double z0[W], o0[W], z1[W], o1[W];
        bjacobi_row<W, VEC>(n, bs, i, inv, R, ldr, z0, o0);
        bjacobi_row<W, VEC>(n, bs, i + stride, inv, R, ldr, z1, o1);
        store_cols<W, VEC>(Z + i * ldz, z0);
        store_cols<W, VEC>(Z + (i + stride) * ldz, z1);
        if constexpr (DOT) {
#pragma unroll
            for (int c = 0; c < W; ++c) {
                rz0[c] = fma(o0[c], z0[c], rz0[c]);
                rz1[c] = fma(o1[c], z1[c], rz1[c]);
                rr0[c] = fma(o0[c], o0[c], rr0[c]);
                rr1[c] = fma(o1[c], o1[c], rr1[c]);
            }
        }
    }
    if (i < n) {
        double z0[W], o0[W];
        bjacobi_row<W, VEC>(n, bs, i, inv, R, ldr, z0, o0);
        store_cols<W, VEC>(Z + i * ldz, z0);
        if constexpr (DOT) {
#pragma unroll
            for (int c = 0; c < W; ++c) {
                rz0[c] = fma(o0[c], z0[c], rz0[c]);
                rr0[c] = fma(o0[c], o0[c], rr0[c]);
            }
        }
    }
    if constexpr (DOT) {
        __shared__ double s_rz[W][kBlock / kWave], s_rr[W][kBlock / kWave];
        dot_partial_store<W>(rz0, rz1, s_rz, j, partial);
        dot_partial_store<W>(rr0, rr1, s_rr, (int64_t)k + j, partial);
    }
}

template <bool DOT>
static void launch_apply(const spmv_bjacobi *m, int32_t k, const double *R, int64_t ldr, double *Z, int64_t ldz,
                         double *partial, hipStream_t st)
{
    const int g = dot_multi_blocks(m->n);
    for_column_blocks(k, R, ldr, Z, ldz, [&](auto Wc, auto V, int32_t j0, int32_t chunks) {
        constexpr int W = decltype(Wc)::value;
        constexpr bool VEC = decltype(V)::value && W % 2 == 0;
        hipLaunchKernelGGL((bjacobi_apply_kernel<W, VEC, DOT>), dim3(g, (unsigned)chunks), dim3(kBlock), 0, st, m->n,
                           m->bs, j0, k, m->inv, R, ldr, Z, ldz, partial);
    });
}

// s = row i of M^-1 (R - AZ) (STEP0: of M^-1 R) for the W columns at R and AZ,
// `own` = row i of R itself: bjacobi_row with a second operand stream.  The
// difference is formed as the rows arrive, so a block row in flight costs 2 W
// doubles while it loads and W afterwards; with W > 4 two block rows are in
// flight instead of four, which keeps the W = 8 kernels clear of scratch.
template <int W, bool VEC, bool STEP0>
__device__ __forceinline__ void cheb_row(int64_t n, int32_t bs, int64_t i, const double *__restrict__ inv,
                                         const double *__restrict__ R, int64_t ldr, const double *__restrict__ AZ,
                                         int64_t ldaz, double (&s)[W], double (&own)[W])
{
    constexpr int U = W > 4 ? 2 : 4;
    const int64_t q = i <= (int64_t)UINT32_MAX ? (int64_t)((uint32_t)i / (uint32_t)bs) : i / bs;
    const int64_t r0 = q * bs;
    const int32_t nb = n - r0 < bs ? (int32_t)(n - r0) : bs;
    const int32_t me = (int32_t)(i - r0);
    const double *a = inv + i * bs;
    const double *Rb = R + r0 * ldr;
    const double *Ab = STEP0 ? nullptr : AZ + r0 * ldaz;
#pragma unroll
    for (int w = 0; w < W; ++w)
        s[w] = own[w] = 0.0;
    for (int32_t c0 = 0; c0 < nb; c0 += U) {
        double av[U], rv[U][W], tv[U][W];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int32_t c = c0 + u < nb ? c0 + u : nb - 1;
            av[u] = a[c];
            load_cols<W, VEC>(Rb + (int64_t)c * ldr, rv[u]);
            if constexpr (!STEP0)
                load_cols<W, VEC>(Ab + (int64_t)c * ldaz, tv[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int32_t c = c0 + u;
            if (c < nb) {
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const double t = STEP0 ? rv[u][w] : rv[u][w] - tv[u][w];
                    s[w] = c == 0 ? av[u] * t : fma(av[u], t, s[w]);
                    own[w] = c == me ? rv[u][w] : own[w];
                }
            }
        }
    }
}

// the thread's own elements: d = b s (STEP0) or fma(a, D, b s); D = d,
// Zout = d (STEP0) or Zin + d, which is also left in z
template <int W, bool VEC, bool STEP0>
__device__ __forceinline__ void cheb_update(double a, double b, const double (&s)[W], double *D, const double *Zin,
                                            double *Zout, double (&z)[W])
{
    double d[W];
    if constexpr (STEP0) {
#pragma unroll
        for (int w = 0; w < W; ++w)
            z[w] = d[w] = b * s[w];
    } else {
        double dv[W], zi[W];
        load_cols<W, VEC>(D, dv);
        load_cols<W, VEC>(Zin, zi);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            d[w] = fma(a, dv[w], b * s[w]);
            z[w] = zi[w] + d[w];
        }
    }
    store_cols<W, VEC>(D, d);
    store_cols<W, VEC>(Zout, z);
}

// One Chebyshev step (spmv_cpu_bjacobi_cheb_step_multi) for columns
// j0 + W*blockIdx.y + [0, W): bjacobi_apply_kernel's rows, lanes and, with DOT,
// its sums of r z and r r with z = Zout.  Zin and Zout may be one array: an
// element is read and written by its own thread only.
template <int W, bool VEC, bool DOT, bool STEP0>
__global__ __launch_bounds__(kBlock) void bjacobi_cheb_kernel(int64_t n, int32_t bs, int32_t j0, int32_t k, double a,
                                                              double b, const double *__restrict__ inv,
                                                              const double *__restrict__ R, int64_t ldr,
                                                              const double *__restrict__ AZ, int64_t ldaz,
                                                              double *__restrict__ D, int64_t ldd, const double *Zin,
                                                              int64_t ldzin, double *Zout, int64_t ldzout,
                                                              double *__restrict__ partial)
{
    const int32_t j = j0 + W * (int32_t)blockIdx.y;
    R += j;
    D += j;
    Zout += j;
    if constexpr (!STEP0) {
        AZ += j;
        Zin += j;
    }
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    double rz0[W], rz1[W], rr0[W], rr1[W];
#pragma unroll
    for (int c = 0; c < W; ++c)
        rz0[c] = rz1[c] = rr0[c] = rr1[c] = 0.0;
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (; i + stride < n; i += 2 * stride) {
        double s0[W], o0[W], z0[W], s1[W], o1[W], z1[W];
        cheb_row<W, VEC, STEP0>(n, bs, i, inv, R, ldr, AZ, ldaz, s0, o0);
        cheb_update<W, VEC, STEP0>(a, b, s0, D + i * ldd, Zin + i * ldzin, Zout + i * ldzout, z0);
        cheb_row<W, VEC, STEP0>(n, bs, i + stride, inv, R, ldr, AZ, ldaz, s1, o1);
        cheb_update<W, VEC, STEP0>(a, b, s1, D + (i + stride) * ldd, Zin + (i + stride) * ldzin,
                                   Zout + (i + stride) * ldzout, z1);
        if constexpr (DOT) {
#pragma unroll
            for (int c = 0; c < W; ++c) {
                rz0[c] = fma(o0[c], z0[c], rz0[c]);
                rz1[c] = fma(o1[c], z1[c], rz1[c]);
                rr0[c] = fma(o0[c], o0[c], rr0[c]);
                rr1[c] = fma(o1[c], o1[c], rr1[c]);
            }
        }
    }
    if (i < n) {
        double s0[W], o0[W], z0[W];
        cheb_row<W, VEC, STEP0>(n, bs, i, inv, R, ldr, AZ, ldaz, s0, o0);
        cheb_update<W, VEC, STEP0>(a, b, s0, D + i * ldd, Zin + i * ldzin, Zout + i * ldzout, z0);
        if constexpr (DOT) {
#pragma unroll
            for (int c = 0; c < W; ++c) {
                rz0[c] = fma(o0[c], z0[c], rz0[c]);
                rr0[c] = fma(o0[c], o0[c], rr0[c]);
            }
        }
    }
    if constexpr (DOT) {
        __shared__ double s_rz[W][kBlock / kWave], s_rr[W][kBlock / kWave];
        dot_partial_store<W>(rz0, rz1, s_rz, j, partial);
        dot_partial_store<W>(rr0, rr1, s_rr, (int64_t)k + j, partial);
    }
}

struct ChebOperands {
    double a, b;
    const double *R;
    int64_t ldr;
    const double *AZ;  // nullptr: step 0
    int64_t ldaz;
    double *D;
    int64_t ldd;
    const double *Zin;
    int64_t ldzin;
    double *Zout;
    int64_t ldzout;
};

// at most two launches, as for_column_blocks; the 16-byte path needs every
// array the step touches on it
template <bool DOT>
static void launch_cheb(const spmv_bjacobi *m, int32_t k, const ChebOperands &o, double *partial, hipStream_t st)
{
    const int g = dot_multi_blocks(m->n);
    const bool step0 = o.AZ == nullptr;
    const auto launch = [&](auto Wc, int32_t j0, int32_t chunks) {
        constexpr int W = decltype(Wc)::value;
        const bool vec = vec_ok(o.R, o.ldr, j0, W) && vec_ok(o.D, o.ldd, j0, W) && vec_ok(o.Zout, o.ldzout, j0, W) &&
                         (step0 || (vec_ok(o.AZ, o.ldaz, j0, W) && vec_ok(o.Zin, o.ldzin, j0, W)));
        with_bool(vec, [&](auto V) {
            with_bool(step0, [&](auto S0) {
                constexpr bool VEC = decltype(V)::value && W % 2 == 0;
                constexpr bool STEP0 = decltype(S0)::value;
                hipLaunchKernelGGL((bjacobi_cheb_kernel<W, VEC, DOT, STEP0>), dim3(g, (unsigned)chunks), dim3(kBlock),
                                   0, st, m->n, m->bs, j0, k, o.a, o.b, m->inv, o.R, o.ldr, o.AZ, o.ldaz, o.D, o.ldd,
                                   o.Zin, o.ldzin, o.Zout, o.ldzout, partial);
            });
        });
    };
    const int32_t whole = k / kVecW, rest = k % kVecW;
    if (whole > 0)
        launch(std::integral_constant<int, kVecW>{}, 0, whole);
    if (rest > 0)
        with_int<1, 2, 3, 4, 5, 6, 7>(rest, [&](auto Wc) { launch(Wc, whole * kVecW, 1); });
}

// the refusals of both step calls
static bool cheb_bad(const spmv_bjacobi *m, int32_t k, const ChebOperands &o)
{
    if (!m || k < 1 || o.ldr < k || o.ldd < k || o.ldzout < k)
        return true;
    if (o.AZ && (o.ldaz < k || o.ldzin < k))
        return true;
    if (m->n > 0 && (!o.R || !o.D || !o.Zout || (o.AZ && !o.Zin)))
        return true;
    return o.AZ && o.Zin && o.Zin == o.Zout && o.ldzin != o.ldzout;
}

}  // namespace spmv

using namespace spmv;

extern "C" int spmv_bjacobi_create(spmv_dims d, const int64_t *row_ptr, const int32_t *col, const double *val,
                                   int32_t bs, int64_t col_base, int32_t symmetric_half, spmv_bjacobi **out)
{
    if (out)
        *out = nullptr;
    const int64_t n = d.n_rows;
    if (!out || n < 0 || d.nnz < 0 || bs < 1 || bs > kBjMax || col_base < 0 || (n > 0 && !row_ptr) ||
        (n > 0 && d.nnz > 0 && (!col || !val)))
        return fail_msg(SPMV_OTHER_ERROR,
                        "spmv_bjacobi_create: bad arguments (n, nnz, col_base >= 0, 1 <= bs <= 16, no NULL array)");
    SPMV_GUARD(d);
    const hipStream_t st = (hipStream_t)d.stream;
    spmv_bjacobi *m = new spmv_bjacobi;
    m->bs = bs;
    m->symmetric_half = symmetric_half != 0;
    m->n = n;
    m->n_blocks = (n + bs - 1) / bs;
    m->col_base = col_base;
    m->device = d.device;
    if (m->n_blocks == 0) {
        *out = m;
        return SPMV_SUCCESS;
    }
    uint8_t *bad = nullptr, *bad_host = nullptr;
    const auto give_up = [&](const char *where, hipError_t e) {
        (void)hipFree(m->inv);
        (void)hipFree(bad);
        free(bad_host);
        delete m;
        return fail(SPMV_PROGRAM_ERROR, where, e);
    };
    hipError_t e = hipMalloc(&m->inv, (size_t)m->n_blocks * bs * bs * sizeof(double));
    if (e == hipSuccess)
        e = hipMalloc(&bad, (size_t)m->n_blocks);
    if (e != hipSuccess)
        return give_up("spmv_bjacobi_create: hipMalloc", e);
    bad_host = (uint8_t *)malloc((size_t)m->n_blocks);
    if (!bad_host)
        return give_up("spmv_bjacobi_create: out of host memory", hipErrorOutOfMemory);
    with_int<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>(bs, [&](auto B) {
        constexpr int BS = decltype(B)::value;
        constexpr int PER = kBjThreads / bj_group(BS);
        hipLaunchKernelGGL(bjacobi_build_kernel<BS>, dim3((unsigned)((m->n_blocks + PER - 1) / PER)),
                           dim3(kBjThreads), 0, st, n, m->n_blocks, row_ptr, col, val, col_base, m->symmetric_half,
                           m->inv, bad);
    });
    if ((e = hipGetLastError()) != hipSuccess ||
        (e = hipMemcpyAsync(bad_host, bad, (size_t)m->n_blocks, hipMemcpyDeviceToHost, st)) != hipSuccess ||
        (e = hipStreamSynchronize(st)) != hipSuccess)
        return give_up("spmv_bjacobi_create: build kernel", e);
    for (int64_t q = 0; q < m->n_blocks; ++q)
        m->singular_blocks += bad_host[q];
    (void)hipFree(bad);
    free(bad_host);
    *out = m;
    return SPMV_SUCCESS;
}

extern "C" int spmv_bjacobi_get_info(const spmv_bjacobi *m, spmv_bjacobi_info *info)
{
    if (!m || !info)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_bjacobi_get_info: NULL argument");
    *info = spmv_bjacobi_info{};
    info->bs = m->bs;
    info->symmetric_half = m->symmetric_half;
    info->n = m->n;
    info->n_blocks = m->n_blocks;
    info->singular_blocks = m->singular_blocks;
    info->col_base = m->col_base;
    info->owned_bytes = m->n_blocks * m->bs * m->bs * (int64_t)sizeof(double);
    snprintf(info->kernel, sizeof info->kernel, "bjacobi_apply_kernel");
    return SPMV_SUCCESS;
}

extern "C" int spmv_bjacobi_inverse(const spmv_bjacobi *m, const double **inv)
{
    if (!m || !inv)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_bjacobi_inverse: NULL argument");
    *inv = m->inv;
    return SPMV_SUCCESS;
}

extern "C" int spmv_bjacobi_apply_multi(const spmv_bjacobi *m, int32_t k, const double *R, int64_t ldr, double *Z,
                                        int64_t ldz, void *stream)
{
    if (!m || k < 1 || ldr < k || ldz < k || (m->n > 0 && (!R || !Z)))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_bjacobi_apply_multi: bad arguments (k >= 1, ldr and ldz >= k)");
    if (m->n == 0)
        return SPMV_SUCCESS;
    DeviceGuard guard(m->device);
    if (guard.rc() != SPMV_SUCCESS)
        return guard.rc();
    launch_apply<false>(m, k, R, ldr, Z, ldz, nullptr, (hipStream_t)stream);
    SPMV_CHECK_LAUNCH("bjacobi_apply_kernel");
    return SPMV_SUCCESS;
}

extern "C" size_t spmv_bjacobi_ws_bytes(int64_t n, int32_t k)
{
    return (size_t)dot_multi_blocks(n) * 2 * (size_t)(k < 1 ? 1 : k) * sizeof(double);
}

extern "C" int spmv_bjacobi_apply_dot_multi(const spmv_bjacobi *m, int32_t k, const double *R, int64_t ldr, double *Z,
                                            int64_t ldz, double *out, void *ws, size_t ws_bytes, void *stream)
{
    if (!m || k < 1 || ldr < k || ldz < k || !out || (m->n > 0 && (!R || !Z)))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_bjacobi_apply_dot_multi: bad arguments (k >= 1, ldr and ldz >= k)");
    if (!ws || ws_bytes < spmv_bjacobi_ws_bytes(m->n, k))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_bjacobi_apply_dot_multi: workspace too small");
    DeviceGuard guard(m->device);
    if (guard.rc() != SPMV_SUCCESS)
        return guard.rc();
    const hipStream_t st = (hipStream_t)stream;
    launch_apply<true>(m, k, R, ldr, Z, ldz, (double *)ws, st);
    hipLaunchKernelGGL(dot_multi_final_kernel, dim3(2 * (unsigned)k), dim3(1024), 0, st, dot_multi_blocks(m->n),
                       (const double *)ws, out);
    SPMV_CHECK_LAUNCH("bjacobi_apply_dot kernels");
    return SPMV_SUCCESS;
}

static ChebOperands cheb_operands(double a, double b, const double *R, int64_t ldr, const double *AZ, int64_t ldaz,
                                  double *D, int64_t ldd, const double *Zin, int64_t ldzin, double *Zout,
                                  int64_t ldzout)
{
    if (!AZ)  // step 0 reads neither: no stray operand reaches the kernel
        return ChebOperands{a, b, R, ldr, nullptr, 0, D, ldd, nullptr, 0, Zout, ldzout};
    return ChebOperands{a, b, R, ldr, AZ, ldaz, D, ldd, Zin, ldzin, Zout, ldzout};
}

extern "C" int spmv_bjacobi_cheb_step_multi(const spmv_bjacobi *m, int32_t k, double a, double b, const double *R,
                                            int64_t ldr, const double *AZ, int64_t ldaz, double *D, int64_t ldd,
                                            const double *Zin, int64_t ldzin, double *Zout, int64_t ldzout,
                                            void *stream)
{
    const ChebOperands o = cheb_operands(a, b, R, ldr, AZ, ldaz, D, ldd, Zin, ldzin, Zout, ldzout);
    if (cheb_bad(m, k, o))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_bjacobi_cheb_step_multi: bad arguments (k >= 1, every ld >= k, no "
                                          "NULL array, Zout == Zin with one ld)");
    if (m->n == 0)
        return SPMV_SUCCESS;
    DeviceGuard guard(m->device);
    if (guard.rc() != SPMV_SUCCESS)
        return guard.rc();
    launch_cheb<false>(m, k, o, nullptr, (hipStream_t)stream);
    SPMV_CHECK_LAUNCH("bjacobi_cheb_kernel");
    return SPMV_SUCCESS;
}

extern "C" int spmv_bjacobi_cheb_step_dot_multi(const spmv_bjacobi *m, int32_t k, double a, double b,
                                                const double *R, int64_t ldr, const double *AZ, int64_t ldaz,
                                                double *D, int64_t ldd, const double *Zin, int64_t ldzin,
                                                double *Zout, int64_t ldzout, double *out, void *ws, size_t ws_bytes,
                                                void *stream)
{
    const ChebOperands o = cheb_operands(a, b, R, ldr, AZ, ldaz, D, ldd, Zin, ldzin, Zout, ldzout);
    if (cheb_bad(m, k, o) || !out)
        return fail_msg(SPMV_OTHER_ERROR, "spmv_bjacobi_cheb_step_dot_multi: bad arguments (k >= 1, every ld >= k, "
                                          "no NULL array, Zout == Zin with one ld)");
    if (!ws || ws_bytes < spmv_bjacobi_ws_bytes(m->n, k))
        return fail_msg(SPMV_OTHER_ERROR, "spmv_bjacobi_cheb_step_dot_multi: workspace too small");
    DeviceGuard guard(m->device);
    if (guard.rc() != SPMV_SUCCESS)
        return guard.rc();
    const hipStream_t st = (hipStream_t)stream;
    launch_cheb<true>(m, k, o, (double *)ws, st);
    hipLaunchKernelGGL(dot_multi_final_kernel, dim3(2 * (unsigned)k), dim3(1024), 0, st, dot_multi_blocks(m->n),
                       (const double *)ws, out);
    SPMV_CHECK_LAUNCH("bjacobi_cheb_step_dot kernels");
    return SPMV_SUCCESS;
}

extern "C" int spmv_bjacobi_destroy(spmv_bjacobi *m)
{
    if (!m)
        return SPMV_SUCCESS;
    DeviceGuard guard(m->device);
    (void)hipFree(m->inv);
    delete m;
    return SPMV_SUCCESS;
}
