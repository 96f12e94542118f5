/*
 * transpose_harness.c — the host side of the transposed product
 * (spmv_csr_transpose, spmv_cpu_csr_t; host/formats.c, host/cpu.c) compiled
 * into this binary with -fsanitize=address,undefined by
 * `make test-san-transpose`.
 *
 * usage: transpose_harness FILE.mtx...
 * For every file: CSR from the COO, A^T by spmv_csr_transpose (structure
 * checked entry by entry), y = A^T x by spmv_cpu_csr_t and by the forward CPU
 * loop over A^T, both checked against the file-order sum of the swapped COO
 * (spmv_check).  Every buffer has exactly the documented size, so a write or
 * read past one is a sanitizer report.  Then the refused inputs: columns out
 * of range, negative sizes, NULL arrays.  Any mismatch or report fails.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spmv_host.h"

static int g_fail = 0;

#define CHECK(cond, ...)                                                                 \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);                         \
            fprintf(stderr, __VA_ARGS__);                                                \
            fputc('\n', stderr);                                                         \
            g_fail = 1;                                                                  \
        }                                                                                \
    } while (0)

static void *xmalloc(size_t n)
{
    void *p = malloc(n ? n : 1);
    if (!p) {
        fprintf(stderr, "out of memory\n");
        exit(2);
    }
    return p;
}

static void check_yt(const char *what, int64_t n_cols, int64_t nnz, const int32_t *row, const int32_t *col,
                     const double *val, const double *x, const double *y)
{
    int64_t first = -1;
    double ref = 0.0;
    /* the swapped COO: rows of A^T are the columns of A */
    const int64_t bad = spmv_check(n_cols, nnz, col, row, val, x, y, 0.0, 1e-12, &first, &ref);
    CHECK(bad == 0, "%s: %lld bad rows, first %lld (got %g want %g)", what, (long long)bad, (long long)first,
          first >= 0 ? y[first] : 0.0, ref);
}

static void one_matrix(const char *name, int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *row,
                       const int32_t *col, const double *val)
{
    char what[600];
    int64_t *ptr = xmalloc((size_t)(n_rows + 1) * 8);
    int32_t *cc = xmalloc((size_t)nnz * 4);
    double *cv = xmalloc((size_t)nnz * 8);
    CHECK(spmv_csr_from_coo(n_rows, nnz, row, col, val, ptr, cc, cv) == SPMV_SUCCESS, "%s csr", name);

    int64_t *tp = xmalloc((size_t)(n_cols + 1) * 8);
    int32_t *tc = xmalloc((size_t)nnz * 4);
    double *tv = xmalloc((size_t)nnz * 8);
    CHECK(spmv_csr_transpose(n_rows, n_cols, ptr, cc, cv, tp, tc, tv) == SPMV_SUCCESS, "%s transpose", name);
    CHECK(tp[0] == 0 && tp[n_cols] == nnz, "%s: t_ptr ends %lld..%lld", name, (long long)tp[0], (long long)tp[n_cols]);
    for (int64_t c = 0; c < n_cols && !g_fail; ++c) {
        CHECK(tp[c] <= tp[c + 1], "%s: t_ptr decreases at %lld", name, (long long)c);
        for (int64_t e = tp[c]; e < tp[c + 1]; ++e) {
            CHECK(tc[e] >= 0 && tc[e] < n_rows, "%s: row id out of range at %lld", name, (long long)e);
            /* stable: increasing row of A inside a row of A^T */
            CHECK(e == tp[c] || tc[e - 1] <= tc[e], "%s: rows of A out of order at %lld", name, (long long)e);
        }
    }

    double *x = xmalloc((size_t)n_rows * 8);
    double *y = xmalloc((size_t)n_cols * 8);
    for (int64_t i = 0; i < n_rows; ++i)
        x[i] = 1.0 + (double)(i % 17) * 0.25;
    for (int64_t j = 0; j < n_cols; ++j)
        y[j] = -7.0;
    CHECK(spmv_cpu_csr_t(n_rows, n_cols, ptr, cc, cv, x, y) == SPMV_SUCCESS, "%s cpu csr_t", name);
    snprintf(what, sizeof what, "%s csr_t", name);
    check_yt(what, n_cols, nnz, row, col, val, x, y);
    /* the forward loop over the transposed arrays computes the same product */
    for (int64_t j = 0; j < n_cols; ++j)
        y[j] = -7.0;
    CHECK(spmv_cpu_csr(n_cols, tp, tc, tv, x, y, 2) == SPMV_SUCCESS, "%s cpu csr over A^T", name);
    snprintf(what, sizeof what, "%s csr over A^T", name);
    check_yt(what, n_cols, nnz, row, col, val, x, y);

    if (nnz > 0) { /* a column out of range is refused by both */
        const int32_t keep = cc[nnz - 1];
        cc[nnz - 1] = (int32_t)n_cols;
        CHECK(spmv_csr_transpose(n_rows, n_cols, ptr, cc, cv, tp, tc, tv) == SPMV_OTHER_ERROR, "%s: column n_cols accepted", name);
        CHECK(spmv_cpu_csr_t(n_rows, n_cols, ptr, cc, cv, x, y) == SPMV_OTHER_ERROR, "%s: cpu column n_cols accepted", name);
        cc[nnz - 1] = -1;
        CHECK(spmv_csr_transpose(n_rows, n_cols, ptr, cc, cv, tp, tc, tv) == SPMV_OTHER_ERROR, "%s: column -1 accepted", name);
        CHECK(spmv_cpu_csr_t(n_rows, n_cols, ptr, cc, cv, x, y) == SPMV_OTHER_ERROR, "%s: cpu column -1 accepted", name);
        cc[nnz - 1] = keep;
        CHECK(spmv_csr_transpose(n_rows, n_cols, ptr, NULL, cv, tp, tc, tv) == SPMV_OTHER_ERROR, "%s: NULL col", name);
        CHECK(spmv_csr_transpose(n_rows, n_cols, ptr, cc, cv, tp, NULL, tv) == SPMV_OTHER_ERROR, "%s: NULL t_col", name);
        CHECK(spmv_cpu_csr_t(n_rows, n_cols, ptr, cc, NULL, x, y) == SPMV_OTHER_ERROR, "%s: NULL val", name);
        CHECK(spmv_cpu_csr_t(n_rows, n_cols, ptr, cc, cv, NULL, y) == SPMV_OTHER_ERROR, "%s: NULL x", name);
    }
    if (n_cols > 0)
        CHECK(spmv_cpu_csr_t(n_rows, n_cols, ptr, cc, cv, x, NULL) == SPMV_OTHER_ERROR, "%s: NULL y", name);
    CHECK(spmv_csr_transpose(n_rows, n_cols, NULL, cc, cv, tp, tc, tv) == SPMV_OTHER_ERROR, "%s: NULL row_ptr", name);
    CHECK(spmv_csr_transpose(n_rows, n_cols, ptr, cc, cv, NULL, tc, tv) == SPMV_OTHER_ERROR, "%s: NULL t_ptr", name);
    CHECK(spmv_csr_transpose(-1, n_cols, ptr, cc, cv, tp, tc, tv) == SPMV_OTHER_ERROR, "%s: n_rows -1", name);
    CHECK(spmv_csr_transpose(n_rows, -1, ptr, cc, cv, tp, tc, tv) == SPMV_OTHER_ERROR, "%s: n_cols -1", name);
    CHECK(spmv_cpu_csr_t(-1, n_cols, ptr, cc, cv, x, y) == SPMV_OTHER_ERROR, "%s: cpu n_rows -1", name);
    CHECK(spmv_cpu_csr_t(n_rows, n_cols, NULL, cc, cv, x, y) == SPMV_OTHER_ERROR, "%s: cpu NULL row_ptr", name);

    free(ptr);
    free(cc);
    free(cv);
    free(tp);
    free(tc);
    free(tv);
    free(x);
    free(y);
}

int main(int argc, char **argv)
{
    int files = 0;
    for (int a = 1; a < argc; ++a) {
        spmv_mtx_info info;
        if (spmv_mtx_read_info(argv[a], &info) != SPMV_SUCCESS) {
            fprintf(stderr, "skip %s (not readable)\n", argv[a]);
            continue;
        }
        int32_t *row = xmalloc((size_t)info.nnz * 4), *col = xmalloc((size_t)info.nnz * 4);
        double *val = xmalloc((size_t)info.nnz * 8);
        CHECK(spmv_mtx_read(argv[a], &info, row, col, val) == SPMV_SUCCESS, "read %s", argv[a]);
        one_matrix(argv[a], info.n_rows, info.n_cols, info.nnz, row, col, val);
        free(row);
        free(col);
        free(val);
        ++files;
    }
    /* no rows and no columns at all */
    const int64_t zero = 0;
    int64_t tp0 = -1;
    CHECK(spmv_csr_transpose(0, 0, &zero, NULL, NULL, &tp0, NULL, NULL) == SPMV_SUCCESS && tp0 == 0, "0 x 0 transpose");
    CHECK(spmv_cpu_csr_t(0, 0, &zero, NULL, NULL, NULL, NULL) == SPMV_SUCCESS, "0 x 0 csr_t");
    if (g_fail)
        return 1;
    printf("transpose harness: %d files clean\n", files);
    return 0;
}
