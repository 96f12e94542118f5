/*
 * transpose_multi_harness.c — the host side of the multi-vector transposed
 * product (spmv_cpu_csr_t_multi; host/cpu.c) compiled into this binary with
 * -fsanitize=address,undefined by `make test-san-transpose-multi`.
 *
 * usage: transpose_multi_harness FILE.mtx...
 * For every file and k in {1, 3, 8, 9}: Y = A^T X by spmv_cpu_csr_t_multi with
 * exactly-sized allocations: X is n_rows * k doubles (ldx == k), Y has
 * ldy = k + 2 and ends with the k values of its last row, so a read past X's
 * last row, a write into Y's gaps beyond the last row or a write past row
 * n_cols is a sanitizer report.  Every column is compared bit for bit with
 * spmv_cpu_csr_t on that column and Y's gaps must keep their fill.  Then the
 * refused inputs.  Any mismatch or report fails.
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

static void one_k(const char *name, int64_t n_rows, int64_t n_cols, const int64_t *ptr, const int32_t *cc,
                  const double *cv, int32_t k)
{
    const int64_t ldx = k, ldy = k + 2;
    const double fill = 12345.0;
    /* Y: n_cols rows of ldy, the last one cut after its k live values */
    const size_t y_len = n_cols > 0 ? (size_t)((n_cols - 1) * ldy + k) : 0;
    double *X = xmalloc((size_t)(n_rows * ldx) * 8);
    double *Y = xmalloc(y_len * 8);
    double *x1 = xmalloc((size_t)n_rows * 8);
    double *y1 = xmalloc((size_t)n_cols * 8);
    for (int64_t i = 0; i < n_rows * ldx; ++i)
        X[i] = 1.0 + (double)((i * 7) % 23) * 0.125 - (double)(i % 3);
    for (size_t i = 0; i < y_len; ++i)
        Y[i] = fill;
    CHECK(spmv_cpu_csr_t_multi(n_rows, n_cols, ptr, cc, cv, k, X, ldx, Y, ldy) == SPMV_SUCCESS, "%s k=%d", name, k);
    for (int32_t j = 0; j < k && !g_fail; ++j) {
        for (int64_t r = 0; r < n_rows; ++r)
            x1[r] = X[r * ldx + j];
        CHECK(spmv_cpu_csr_t(n_rows, n_cols, ptr, cc, cv, x1, y1) == SPMV_SUCCESS, "%s csr_t", name);
        for (int64_t c = 0; c < n_cols; ++c)
            CHECK(memcmp(&Y[c * ldy + j], &y1[c], 8) == 0, "%s k=%d: Y[%lld][%d] = %a, csr_t gives %a", name, k,
                  (long long)c, j, Y[c * ldy + j], y1[c]);
    }
    for (int64_t c = 0; c + 1 < n_cols; ++c)
        for (int64_t j = k; j < ldy; ++j)
            CHECK(memcmp(&Y[c * ldy + j], &fill, 8) == 0, "%s k=%d: gap Y[%lld][%lld] written", name, k, (long long)c,
                  (long long)j);

    /* refusals: nothing may be written */
    for (size_t i = 0; i < y_len; ++i)
        Y[i] = fill;
    CHECK(spmv_cpu_csr_t_multi(-1, n_cols, ptr, cc, cv, k, X, ldx, Y, ldy) == SPMV_OTHER_ERROR, "%s: n_rows -1", name);
    CHECK(spmv_cpu_csr_t_multi(n_rows, -1, ptr, cc, cv, k, X, ldx, Y, ldy) == SPMV_OTHER_ERROR, "%s: n_cols -1", name);
    CHECK(spmv_cpu_csr_t_multi(n_rows, n_cols, ptr, cc, cv, 0, X, ldx, Y, ldy) == SPMV_OTHER_ERROR, "%s: k 0", name);
    CHECK(spmv_cpu_csr_t_multi(n_rows, n_cols, ptr, cc, cv, k, X, k - 1, Y, ldy) == SPMV_OTHER_ERROR, "%s: ldx", name);
    CHECK(spmv_cpu_csr_t_multi(n_rows, n_cols, ptr, cc, cv, k, X, ldx, Y, k - 1) == SPMV_OTHER_ERROR, "%s: ldy", name);
    CHECK(spmv_cpu_csr_t_multi(n_rows, n_cols, NULL, cc, cv, k, X, ldx, Y, ldy) == SPMV_OTHER_ERROR, "%s: NULL row_ptr",
          name);
    if (n_cols > 0)
        CHECK(spmv_cpu_csr_t_multi(n_rows, n_cols, ptr, cc, cv, k, X, ldx, NULL, ldy) == SPMV_OTHER_ERROR, "%s: NULL Y",
              name);
    if (ptr[n_rows] > 0) {
        CHECK(spmv_cpu_csr_t_multi(n_rows, n_cols, ptr, NULL, cv, k, X, ldx, Y, ldy) == SPMV_OTHER_ERROR, "%s: NULL col",
              name);
        CHECK(spmv_cpu_csr_t_multi(n_rows, n_cols, ptr, cc, NULL, k, X, ldx, Y, ldy) == SPMV_OTHER_ERROR, "%s: NULL val",
              name);
        CHECK(spmv_cpu_csr_t_multi(n_rows, n_cols, ptr, cc, cv, k, NULL, ldx, Y, ldy) == SPMV_OTHER_ERROR, "%s: NULL X",
              name);
    }
    for (size_t i = 0; i < y_len; ++i)
        CHECK(memcmp(&Y[i], &fill, 8) == 0, "%s k=%d: a refused call wrote Y[%zu]", name, k, i);
    free(X);
    free(Y);
    free(x1);
    free(y1);
}

static void one_matrix(const char *name, int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *row,
                       const int32_t *col, const double *val)
{
    static const int32_t ks[] = {1, 3, 8, 9};
    int64_t *ptr = xmalloc((size_t)(n_rows + 1) * 8);
    int32_t *cc = xmalloc((size_t)nnz * 4);
    double *cv = xmalloc((size_t)nnz * 8);
    CHECK(spmv_csr_from_coo(n_rows, nnz, row, col, val, ptr, cc, cv) == SPMV_SUCCESS, "%s csr", name);
    for (size_t i = 0; i < sizeof ks / sizeof ks[0]; ++i)
        one_k(name, n_rows, n_cols, ptr, cc, cv, ks[i]);
    if (nnz > 0) { /* a column out of range is refused */
        double *X = xmalloc((size_t)n_rows * 2 * 8), *Y = xmalloc((size_t)n_cols * 2 * 8);
        for (int64_t i = 0; i < n_rows * 2; ++i)
            X[i] = 1.0;
        const int32_t keep = cc[nnz - 1];
        cc[nnz - 1] = (int32_t)n_cols;
        CHECK(spmv_cpu_csr_t_multi(n_rows, n_cols, ptr, cc, cv, 2, X, 2, Y, 2) == SPMV_OTHER_ERROR, "%s: column n_cols",
              name);
        cc[nnz - 1] = -1;
        CHECK(spmv_cpu_csr_t_multi(n_rows, n_cols, ptr, cc, cv, 2, X, 2, Y, 2) == SPMV_OTHER_ERROR, "%s: column -1", name);
        cc[nnz - 1] = keep;
        free(X);
        free(Y);
    }
    free(ptr);
    free(cc);
    free(cv);
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
    CHECK(spmv_cpu_csr_t_multi(0, 0, &zero, NULL, NULL, 3, NULL, 3, NULL, 3) == SPMV_SUCCESS, "0 x 0 csr_t_multi");
    if (g_fail)
        return 1;
    printf("transpose multi harness: %d files clean\n", files);
    return 0;
}
