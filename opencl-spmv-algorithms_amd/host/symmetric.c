/*
 * symmetric.c — the host side of the symmetric product
 * y = (S + S^T - diag S) x from half-stored matrices (spmv_host.h):
 * spmv_coo_symmetrize, the Matrix Market expansion of a COO,
 * spmv_cpu_csr_sym, the plain loop on the half storage, and
 * spmv_cpu_csr_sym_multi, its k-vector form.
 *
 * Meaning of "symmetric" here: every stored off-diagonal entry (i, j, v) also
 * stands for (j, i, v); diagonal entries count once; duplicates and entries
 * stored on both sides each count as listed.  Skew-symmetric files (mirror
 * -v) and hermitian complex files (mirror conj v) are NOT covered: the
 * reader's `symmetric` flag does not tell the three banners apart.
 */
#include <string.h>

#include "spmv_host.h"

int spmv_coo_symmetrize(int64_t n, int64_t nnz, const int32_t *row, const int32_t *col, const double *val,
                        int64_t *nnz_out, int32_t *row_out, int32_t *col_out, double *val_out)
{
    if (n < 0 || nnz < 0 || !nnz_out || (nnz > 0 && (!row || !col)))
        return SPMV_OTHER_ERROR;
    int64_t off = 0;
    for (int64_t i = 0; i < nnz; ++i) {
        if (row[i] < 0 || row[i] >= n || col[i] < 0 || col[i] >= n)
            return SPMV_OTHER_ERROR;
        off += row[i] != col[i];
    }
    *nnz_out = nnz + off;
    if (!row_out)
        return SPMV_SUCCESS;
    if (nnz > 0 && (!col_out || !val_out || !val))
        return SPMV_OTHER_ERROR;
    int64_t k = nnz; /* the mirrored entries follow the nnz input entries */
    for (int64_t i = 0; i < nnz; ++i) {
        const int32_t r = row[i], c = col[i];
        const double v = val[i];
        row_out[i] = r;
        col_out[i] = c;
        val_out[i] = v;
        if (r != c) {
            row_out[k] = c;
            col_out[k] = r;
            val_out[k] = v;
            ++k;
        }
    }
    return SPMV_SUCCESS;
}

int spmv_cpu_csr_sym(int64_t n, const int64_t *row_ptr, const int32_t *col, const double *val, const double *x,
                     double *y)
{
    if (n < 0 || !row_ptr || (n > 0 && !y))
        return SPMV_OTHER_ERROR;
    if (row_ptr[n] > row_ptr[0] && (!col || !val || !x))
        return SPMV_OTHER_ERROR;
    if (n > 0)
        memset(y, 0, (size_t)n * sizeof(double));
    for (int64_t r = 0; r < n; ++r) {
        double s = 0.0;
        for (int64_t e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
            const int32_t c = col[e];
            if (c < 0 || c >= n)
                return SPMV_OTHER_ERROR;
            s += val[e] * x[c];
            if (c != r)
                y[c] += val[e] * x[r];
        }
        y[r] += s;
    }
    return SPMV_SUCCESS;
}

/* The k-vector form of spmv_cpu_csr_sym (the layout of spmv_plan_run_sym_multi,
 * spmv.h): the columns are taken in groups of 8, each by that loop with a row
 * sum per column, so column j has spmv_cpu_csr_sym's bits on column j.        */
int spmv_cpu_csr_sym_multi(int64_t n, const int64_t *row_ptr, const int32_t *col, const double *val, int32_t k,
                           const double *X, int64_t ldx, double *Y, int64_t ldy)
{
    if (n < 0 || k < 1 || ldx < k || ldy < k || !row_ptr || (n > 0 && !Y))
        return SPMV_OTHER_ERROR;
    if (row_ptr[n] > row_ptr[0] && (!col || !val || !X))
        return SPMV_OTHER_ERROR;
    for (int64_t e = row_ptr[0]; e < row_ptr[n]; ++e)
        if (col[e] < 0 || col[e] >= n)
            return SPMV_OTHER_ERROR;
    for (int64_t r = 0; r < n; ++r)
        memset(Y + r * ldy, 0, (size_t)k * sizeof(double));
    for (int32_t j0 = 0; j0 < k; j0 += 8) {
        const int32_t w = k - j0 < 8 ? k - j0 : 8;
        for (int64_t r = 0; r < n; ++r) {
            double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            double *yr = Y + r * ldy + j0;
            for (int64_t e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
                const int64_t c = col[e];
                const double v = val[e];
                const double *xc = X + c * ldx + j0, *xr = X + r * ldx + j0;
                for (int32_t j = 0; j < w; ++j)
                    s[j] += v * xc[j];
                if (c != r) {
                    double *yc = Y + c * ldy + j0;
                    for (int32_t j = 0; j < w; ++j)
                        yc[j] += v * xr[j];
                }
            }
            for (int32_t j = 0; j < w; ++j)
                yr[j] += s[j];
        }
    }
    return SPMV_SUCCESS;
}
