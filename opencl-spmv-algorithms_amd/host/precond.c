/*
 * precond.c — the host statement of the block-Jacobi preconditioner
 * (spmv_host.h): spmv_bjacobi_build extracts the bs x bs diagonal blocks of a
 * CSR matrix and inverts each, spmv_cpu_bjacobi_apply_multi is Z = M^-1 R on
 * row-major blocks of k vectors, spmv_cpu_bjacobi_cheb_step_multi one step of
 * the Chebyshev recurrence over M^-1.  The device object of csrc/precond.hip
 * follows all three step for step; never a device fallback.
 *
 * One block: D (bs x bs, a short last block completed with the identity) is
 * reduced next to an identity, [D | I] -> [I | D^-1], by row operations in the
 * two phases of Gauss-Jordan elimination:
 *   down, p = 0 .. bs-1: the pivot of column p is the entry of largest
 *      magnitude in rows p .. bs-1 (the first one on a tie), its row is swapped
 *      into place, and every row r below gets
 *      row[r][j] = fma(-(row[r][p] / pivot), row[p][j], row[r][j]);
 *      a zero or non-finite pivot ends the block: it becomes the identity and
 *      is counted as singular;
 *   up, p = bs-1 .. 0: the right half of row p is divided by its pivot, and
 *      every row r above gets row[r][j] = fma(-row[r][p], row[p][j], row[r][j])
 *      there.
 * Every column of the result is thereby a solve of D x = e_j by elimination
 * with partial pivoting and back substitution, whose residual I - D X is
 * small whatever the block's condition; clearing a column above and below
 * the pivot in ONE sweep computes the same matrix in exact arithmetic but its
 * residual grows with the condition of the triangular factor (measured on
 * 5 x 5 blocks of condition 1e4: 48 times LAPACK's against 1.1 times).
 * An inverse with a non-finite element (overflow) is replaced and counted like
 * a singular block.  The identity keeps the preconditioner positive definite.
 */
#include <math.h>
#include <string.h>

#include "spmv_host.h"

#define BJ_MAX 16

/* [D | I] of block q; the mirrored places of a stored half are filled in the
 * order of the rows, each entry right after its own place */
static void block_extract(int64_t n, const int64_t *row_ptr, const int32_t *col, const double *val, int32_t bs,
                          int64_t col_base, int32_t symmetric_half, int64_t q, double a[BJ_MAX][2 * BJ_MAX])
{
    const int64_t r0 = q * bs;
    const int32_t nb = (int32_t)(n - r0 < bs ? n - r0 : bs);
    for (int32_t r = 0; r < bs; ++r) {
        for (int32_t c = 0; c < 2 * bs; ++c)
            a[r][c] = 0.0;
        a[r][bs + r] = 1.0;
        if (r >= nb)
            a[r][r] = 1.0;
    }
    for (int32_t r = 0; r < nb; ++r)
        for (int64_t e = row_ptr[r0 + r]; e < row_ptr[r0 + r + 1]; ++e) {
            const int64_t c = (int64_t)col[e] - col_base - r0;
            if (c < 0 || c >= nb)
                continue;
            a[r][c] += val[e];
            if (symmetric_half && c != r)
                a[c][r] += val[e];
        }
}

/* returns 1 when the block is singular (a then holds garbage) */
static int block_invert(int32_t bs, double a[BJ_MAX][2 * BJ_MAX])
{
    for (int32_t p = 0; p < bs; ++p) {
        int32_t pr = p;
        double best = fabs(a[p][p]);
        for (int32_t r = p + 1; r < bs; ++r)
            if (fabs(a[r][p]) > best) {
                best = fabs(a[r][p]);
                pr = r;
            }
        const double piv = a[pr][p];
        if (piv == 0.0 || !isfinite(piv))
            return 1;
        for (int32_t j = 0; j < 2 * bs; ++j) {
            const double t = a[pr][j];
            a[pr][j] = a[p][j];
            a[p][j] = t;
        }
        for (int32_t r = p + 1; r < bs; ++r) {
            const double f = -(a[r][p] / piv);
            for (int32_t j = p + 1; j < 2 * bs; ++j)
                a[r][j] = fma(f, a[p][j], a[r][j]);
            a[r][p] = 0.0;
        }
    }
    for (int32_t p = bs - 1; p >= 0; --p) {
        const double piv = a[p][p];
        for (int32_t j = bs; j < 2 * bs; ++j)
            a[p][j] = a[p][j] / piv;
        for (int32_t r = 0; r < p; ++r) {
            const double f = -a[r][p];
            for (int32_t j = bs; j < 2 * bs; ++j)
                a[r][j] = fma(f, a[p][j], a[r][j]);
        }
    }
    for (int32_t r = 0; r < bs; ++r)
        for (int32_t c = 0; c < bs; ++c)
            if (!isfinite(a[r][bs + c]))
                return 1;
    return 0;
}

int spmv_bjacobi_build(int64_t n, const int64_t *row_ptr, const int32_t *col, const double *val, int32_t bs,
                       int64_t col_base, int32_t symmetric_half, double *inv, int64_t *singular_blocks)
{
    if (n < 0 || bs < 1 || bs > BJ_MAX || col_base < 0 || !row_ptr || !singular_blocks || (n > 0 && !inv))
        return SPMV_OTHER_ERROR;
    if (row_ptr[n] > row_ptr[0] && (!col || !val))
        return SPMV_OTHER_ERROR;
    const int64_t n_blocks = (n + bs - 1) / bs;
    int64_t singular = 0;
#pragma omp parallel for schedule(static) reduction(+ : singular)
    for (int64_t q = 0; q < n_blocks; ++q) {
        double a[BJ_MAX][2 * BJ_MAX];
        block_extract(n, row_ptr, col, val, bs, col_base, symmetric_half, q, a);
        const int bad = block_invert(bs, a);
        singular += bad;
        double *out = inv + q * bs * bs;
        for (int32_t r = 0; r < bs; ++r)
            for (int32_t c = 0; c < bs; ++c)
                out[r * bs + c] = bad ? (r == c ? 1.0 : 0.0) : a[r][bs + c];
    }
    *singular_blocks = singular;
    return SPMV_SUCCESS;
}

int spmv_cpu_bjacobi_apply_multi(int64_t n, int32_t bs, const double *inv, int32_t k, const double *R, int64_t ldr,
                                 double *Z, int64_t ldz)
{
    if (n < 0 || bs < 1 || bs > BJ_MAX || k < 1 || ldr < k || ldz < k || (n > 0 && (!inv || !R || !Z)))
        return SPMV_OTHER_ERROR;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r0 = i / bs * bs;
        const int32_t nb = (int32_t)(n - r0 < bs ? n - r0 : bs);
        const double *a = inv + i * bs;
        for (int32_t j = 0; j < k; ++j) {
            double s = a[0] * R[r0 * ldr + j];
            for (int32_t c = 1; c < nb; ++c)
                s = fma(a[c], R[(r0 + c) * ldr + j], s);
            Z[i * ldz + j] = s;
        }
    }
    return SPMV_SUCCESS;
}

/* One step of the Chebyshev recurrence over M^-1 (spmv_host.h).  A block's
 * rows of R and AZ are read before any of its rows of D and Zout is written,
 * and an element of D or Zin is read only by the row that rewrites it, so
 * Zout == Zin needs no copy. */
int spmv_cpu_bjacobi_cheb_step_multi(int64_t n, int32_t bs, const double *inv, int32_t k, double a, double b,
                                     const double *R, int64_t ldr, const double *AZ, int64_t ldaz, double *D,
                                     int64_t ldd, const double *Zin, int64_t ldzin, double *Zout, int64_t ldzout)
{
    if (n < 0 || bs < 1 || bs > BJ_MAX || k < 1 || ldr < k || ldd < k || ldzout < k ||
        (AZ && (ldaz < k || ldzin < k)) || (n > 0 && (!inv || !R || !D || !Zout || (AZ && !Zin))) ||
        (AZ && Zin == Zout && Zin && ldzin != ldzout))
        return SPMV_OTHER_ERROR;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r0 = i / bs * bs;
        const int32_t nb = (int32_t)(n - r0 < bs ? n - r0 : bs);
        const double *w = inv + i * bs;
        for (int32_t j = 0; j < k; ++j) {
            double t = AZ ? R[r0 * ldr + j] - AZ[r0 * ldaz + j] : R[r0 * ldr + j];
            double s = w[0] * t;
            for (int32_t c = 1; c < nb; ++c) {
                t = AZ ? R[(r0 + c) * ldr + j] - AZ[(r0 + c) * ldaz + j] : R[(r0 + c) * ldr + j];
                s = fma(w[c], t, s);
            }
            const double bsum = b * s;
            if (!AZ) {
                D[i * ldd + j] = bsum;
                Zout[i * ldzout + j] = bsum;
            } else {
                const double d = fma(a, D[i * ldd + j], bsum);
                D[i * ldd + j] = d;
                Zout[i * ldzout + j] = Zin[i * ldzin + j] + d;
            }
        }
    }
    return SPMV_SUCCESS;
}
