/*
 * bsr.c — the host side of block CSR (spmv_host.h): spmv_bsr_plan counts the
 * b x b blocks of a CSR matrix, spmv_bsr_fill writes brow_ptr / bcol / bval
 * (scipy's bsr_matrix.data[blk, r, c], rocSPARSE row-major) and spmv_cpu_bsr
 * is the plain loop, the host statement of the product.
 *
 * A block row's block columns are found with one marker per block column
 * (the block row that saw it last), so both passes are O(entries) plus a sort
 * of each block row's distinct block columns; the input's columns may come in
 * any order and duplicates add into their slot in CSR order.
 */
#include <stdlib.h>
#include <string.h>

#include "spmv_host.h"

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

/* the arguments both passes read: sizes, b, offsets and columns */
static int bsr_input_ok(int64_t n_rows, int64_t n_cols, const int64_t *row_ptr, const int32_t *col, int32_t b)
{
    if (b < 1 || b > SPMV_BSR_MAX_B || n_rows < 0 || n_cols < 0 || n_cols > (int64_t)INT32_MAX - 8)
        return 0;
    if (n_rows == 0)
        return 1;
    if (!row_ptr || row_ptr[0] < 0)
        return 0;
    for (int64_t r = 0; r < n_rows; ++r)
        if (row_ptr[r + 1] < row_ptr[r])
            return 0;
    const int64_t e0 = row_ptr[0], e1 = row_ptr[n_rows];
    if (e1 > e0 && !col)
        return 0;
    for (int64_t e = e0; e < e1; ++e)
        if (col[e] < 0 || col[e] >= n_cols)
            return 0;
    return 1;
}

static int cmp_i32(const void *a, const void *b)
{
    const int32_t x = *(const int32_t *)a, y = *(const int32_t *)b;
    return (x > y) - (x < y);
}

/* One walk over the block rows.  Counting (brow_ptr == NULL): *n_blocks only.
 * Filling: brow_ptr, bcol (ascending) and bval.  `seen[J]` = 1 + the block row
 * that met block column J last; `slot[J]` = J's block in the current block row. */
static int bsr_walk(int64_t n_rows, int64_t n_cols, const int64_t *row_ptr, const int32_t *col, const double *val,
                    int32_t b, int64_t *n_blocks, int64_t *brow_ptr, int32_t *bcol, double *bval)
{
    const int64_t n_brows = ceil_div(n_rows, b), n_bcols = ceil_div(n_cols, b);
    const int fill = brow_ptr != NULL;
    int64_t *seen = (int64_t *)calloc((size_t)(n_bcols > 0 ? n_bcols : 1), sizeof(int64_t));
    int64_t *slot = fill ? (int64_t *)malloc((size_t)(n_bcols > 0 ? n_bcols : 1) * sizeof(int64_t)) : NULL;
    if (!seen || (fill && !slot)) {
        free(seen);
        free(slot);
        return SPMV_OTHER_ERROR;
    }
    int64_t nb = 0;
    for (int64_t I = 0; I < n_brows; ++I) {
        const int64_t r0 = I * b, r1 = r0 + b < n_rows ? r0 + b : n_rows;
        const int64_t first = nb;
        if (fill)
            brow_ptr[I] = nb;
        for (int64_t e = row_ptr[r0]; e < row_ptr[r1]; ++e) {
            const int64_t J = col[e] / b;
            if (seen[J] != I + 1) {
                seen[J] = I + 1;
                if (fill)
                    bcol[nb] = (int32_t)J;
                ++nb;
            }
        }
        if (!fill)
            continue;
        qsort(bcol + first, (size_t)(nb - first), sizeof(int32_t), cmp_i32);
        for (int64_t k = first; k < nb; ++k)
            slot[bcol[k]] = k;
        for (int64_t r = r0; r < r1; ++r)
            for (int64_t e = row_ptr[r]; e < row_ptr[r + 1]; ++e) {
                const int32_t c = col[e];
                bval[(slot[c / b] * b + (r - r0)) * b + c % b] += val[e];
            }
    }
    if (fill)
        brow_ptr[n_brows] = nb;
    *n_blocks = nb;
    free(seen);
    free(slot);
    return SPMV_SUCCESS;
}

int spmv_bsr_plan(int64_t n_rows, int64_t n_cols, const int64_t *row_ptr, const int32_t *col, int32_t b,
                  int64_t *n_brows, int64_t *n_blocks)
{
    if (!n_brows || !n_blocks || !bsr_input_ok(n_rows, n_cols, row_ptr, col, b))
        return SPMV_OTHER_ERROR;
    int64_t nb = 0;
    const int rc = bsr_walk(n_rows, n_cols, row_ptr, col, NULL, b, &nb, NULL, NULL, NULL);
    if (rc != SPMV_SUCCESS)
        return rc;
    *n_brows = ceil_div(n_rows, b);
    *n_blocks = nb;
    return SPMV_SUCCESS;
}

int spmv_bsr_fill(int64_t n_rows, int64_t n_cols, const int64_t *row_ptr, const int32_t *col, const double *val,
                  int32_t b, int64_t *brow_ptr, int32_t *bcol, double *bval)
{
    if (!brow_ptr || !bsr_input_ok(n_rows, n_cols, row_ptr, col, b))
        return SPMV_OTHER_ERROR;
    int64_t nb = 0;
    if (n_rows > 0 && row_ptr[n_rows] > row_ptr[0]) {
        if (!val || !bcol || !bval)
            return SPMV_OTHER_ERROR;
        /* the count first: bval is zeroed (+0.0 in every slot) before entries add into it */
        const int rc = bsr_walk(n_rows, n_cols, row_ptr, col, NULL, b, &nb, NULL, NULL, NULL);
        if (rc != SPMV_SUCCESS)
            return rc;
        memset(bval, 0, (size_t)nb * (size_t)(b * b) * sizeof(double));
        return bsr_walk(n_rows, n_cols, row_ptr, col, val, b, &nb, brow_ptr, bcol, bval);
    }
    for (int64_t I = 0; I <= ceil_div(n_rows, b); ++I)
        brow_ptr[I] = 0;
    return SPMV_SUCCESS;
}

int spmv_cpu_bsr(int64_t n_rows, int64_t n_cols, int32_t b, int64_t n_brows, const int64_t *brow_ptr,
                 const int32_t *bcol, const double *bval, const double *x, double *y)
{
    if (b < 1 || b > SPMV_BSR_MAX_B || n_rows < 0 || n_cols < 0 || n_cols > (int64_t)INT32_MAX - 8 ||
        n_brows != ceil_div(n_rows, b) || !brow_ptr || (n_rows > 0 && !y))
        return SPMV_OTHER_ERROR;
    if (brow_ptr[0] < 0)
        return SPMV_OTHER_ERROR;
    for (int64_t I = 0; I < n_brows; ++I)
        if (brow_ptr[I + 1] < brow_ptr[I])
            return SPMV_OTHER_ERROR;
    const int64_t k0 = brow_ptr[0], k1 = brow_ptr[n_brows], n_bcols = ceil_div(n_cols, b);
    if (k1 > k0 && (!bcol || !bval || !x))
        return SPMV_OTHER_ERROR;
    for (int64_t k = k0; k < k1; ++k)
        if (bcol[k] < 0 || bcol[k] >= n_bcols)
            return SPMV_OTHER_ERROR;
    for (int64_t I = 0; I < n_brows; ++I) {
        double acc[SPMV_BSR_MAX_B] = {0.0};
        for (int64_t k = brow_ptr[I]; k < brow_ptr[I + 1]; ++k) {
            const int64_t c0 = (int64_t)bcol[k] * b;
            const int64_t cn = c0 + b <= n_cols ? b : n_cols - c0; /* a partial last block column */
            const double *blk = bval + k * (int64_t)(b * b);
            for (int64_t r = 0; r < b; ++r)
                for (int64_t c = 0; c < cn; ++c)
                    acc[r] += blk[r * b + c] * x[c0 + c];
        }
        for (int64_t r = 0; r < b && I * b + r < n_rows; ++r)
            y[I * b + r] = acc[r];
    }
    return SPMV_SUCCESS;
}
