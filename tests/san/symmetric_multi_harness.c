/*
 * symmetric_multi_harness.c — the host side of the multi-vector symmetric
 * product (spmv_cpu_csr_sym_multi; host/symmetric.c) compiled into this binary
 * with -fsanitize=address,undefined by `make test-san-symmetric-multi`.
 *
 * usage: symmetric_multi_harness FILE.mtx...
 * For every square file, taken as the stored half S, k in {1, 3, 8} and both
 * ld == k and ld > k (ldx = k + 1, ldy = k + 2): Y = (S + S^T - diag S) X by
 * spmv_cpu_csr_sym_multi with exactly-sized allocations: X and Y end with the
 * k values of their last row, so a read of X's gaps past the last row, a write
 * into Y's gaps beyond the last row or a write past row n is a sanitizer
 * report.  Every column is compared bit for bit with spmv_cpu_csr_sym on that
 * column and Y's gaps must keep their fill.  Then the refused inputs, which
 * must leave Y as it was.  A file that is not square is skipped.  Any mismatch
 * or report fails.
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

static void one_k(const char *name, int64_t n, const int64_t *ptr, const int32_t *cc, const double *cv, int32_t k,
                  int64_t ldx, int64_t ldy)
{
    const double fill = 12345.0;
    /* n rows of ld, the last one cut after its k live values */
    const size_t x_len = n > 0 ? (size_t)((n - 1) * ldx + k) : 0;
    const size_t y_len = n > 0 ? (size_t)((n - 1) * ldy + k) : 0;
    double *X = xmalloc(x_len * 8), *Y = xmalloc(y_len * 8);
    double *x1 = xmalloc((size_t)n * 8), *y1 = xmalloc((size_t)n * 8);
    for (size_t i = 0; i < x_len; ++i)
        X[i] = 1.0 + (double)((i * 7) % 23) * 0.125 - (double)(i % 3);
    for (size_t i = 0; i < y_len; ++i)
        Y[i] = fill;
    CHECK(spmv_cpu_csr_sym_multi(n, ptr, cc, cv, k, X, ldx, Y, ldy) == SPMV_SUCCESS, "%s k=%d ldx=%lld", name, k,
          (long long)ldx);
    for (int32_t j = 0; j < k && !g_fail; ++j) {
        for (int64_t r = 0; r < n; ++r)
            x1[r] = X[r * ldx + j];
        CHECK(spmv_cpu_csr_sym(n, ptr, cc, cv, x1, y1) == SPMV_SUCCESS, "%s csr_sym", name);
        for (int64_t r = 0; r < n; ++r)
            CHECK(memcmp(&Y[r * ldy + j], &y1[r], 8) == 0, "%s k=%d: Y[%lld][%d] = %a, csr_sym gives %a", name, k,
                  (long long)r, j, Y[r * ldy + j], y1[r]);
    }
    for (int64_t r = 0; r + 1 < n; ++r)
        for (int64_t j = k; j < ldy; ++j)
            CHECK(memcmp(&Y[r * ldy + j], &fill, 8) == 0, "%s k=%d: gap Y[%lld][%lld] written", name, k, (long long)r,
                  (long long)j);

    /* refusals: nothing may be written */
    for (size_t i = 0; i < y_len; ++i)
        Y[i] = fill;
    CHECK(spmv_cpu_csr_sym_multi(-1, ptr, cc, cv, k, X, ldx, Y, ldy) == SPMV_OTHER_ERROR, "%s: n -1", name);
    CHECK(spmv_cpu_csr_sym_multi(n, ptr, cc, cv, 0, X, ldx, Y, ldy) == SPMV_OTHER_ERROR, "%s: k 0", name);
    CHECK(spmv_cpu_csr_sym_multi(n, ptr, cc, cv, k, X, k - 1, Y, ldy) == SPMV_OTHER_ERROR, "%s: ldx", name);
    CHECK(spmv_cpu_csr_sym_multi(n, ptr, cc, cv, k, X, ldx, Y, k - 1) == SPMV_OTHER_ERROR, "%s: ldy", name);
    CHECK(spmv_cpu_csr_sym_multi(n, NULL, cc, cv, k, X, ldx, Y, ldy) == SPMV_OTHER_ERROR, "%s: NULL row_ptr", name);
    if (n > 0)
        CHECK(spmv_cpu_csr_sym_multi(n, ptr, cc, cv, k, X, ldx, NULL, ldy) == SPMV_OTHER_ERROR, "%s: NULL Y", name);
    if (ptr[n] > 0) {
        CHECK(spmv_cpu_csr_sym_multi(n, ptr, NULL, cv, k, X, ldx, Y, ldy) == SPMV_OTHER_ERROR, "%s: NULL col", name);
        CHECK(spmv_cpu_csr_sym_multi(n, ptr, cc, NULL, k, X, ldx, Y, ldy) == SPMV_OTHER_ERROR, "%s: NULL val", name);
        CHECK(spmv_cpu_csr_sym_multi(n, ptr, cc, cv, k, NULL, ldx, Y, ldy) == SPMV_OTHER_ERROR, "%s: NULL X", name);
        int32_t *bad = xmalloc((size_t)ptr[n] * 4);
        const int32_t wrong[2] = {(int32_t)n, -1};
        for (int w = 0; w < 2; ++w) { /* a column out of range in the LAST entry: still nothing written */
            memcpy(bad, cc, (size_t)ptr[n] * 4);
            bad[ptr[n] - 1] = wrong[w];
            CHECK(spmv_cpu_csr_sym_multi(n, ptr, bad, cv, k, X, ldx, Y, ldy) == SPMV_OTHER_ERROR,
                  "%s: column %d accepted", name, wrong[w]);
        }
        free(bad);
    }
    for (size_t i = 0; i < y_len; ++i)
        CHECK(memcmp(&Y[i], &fill, 8) == 0, "%s k=%d: a refused call wrote Y[%zu]", name, k, i);
    free(X);
    free(Y);
    free(x1);
    free(y1);
}

static void one_matrix(const char *name, int64_t n, int64_t nnz, const int32_t *row, const int32_t *col,
                       const double *val)
{
    static const int32_t ks[] = {1, 3, 8};
    int64_t *ptr = xmalloc((size_t)(n + 1) * 8);
    int32_t *cc = xmalloc((size_t)nnz * 4);
    double *cv = xmalloc((size_t)nnz * 8);
    CHECK(spmv_csr_from_coo(n, nnz, row, col, val, ptr, cc, cv) == SPMV_SUCCESS, "%s csr", name);
    for (size_t i = 0; i < sizeof ks / sizeof ks[0]; ++i) {
        one_k(name, n, ptr, cc, cv, ks[i], ks[i], ks[i]);
        one_k(name, n, ptr, cc, cv, ks[i], ks[i] + 1, ks[i] + 2);
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
        if (info.n_rows != info.n_cols)
            continue;
        int32_t *row = xmalloc((size_t)info.nnz * 4), *col = xmalloc((size_t)info.nnz * 4);
        double *val = xmalloc((size_t)info.nnz * 8);
        CHECK(spmv_mtx_read(argv[a], &info, row, col, val) == SPMV_SUCCESS, "read %s", argv[a]);
        one_matrix(argv[a], info.n_rows, info.nnz, row, col, val);
        free(row);
        free(col);
        free(val);
        ++files;
    }
    /* no rows at all */
    const int64_t zero = 0;
    CHECK(spmv_cpu_csr_sym_multi(0, &zero, NULL, NULL, 3, NULL, 3, NULL, 3) == SPMV_SUCCESS, "0 x 0 csr_sym_multi");
    if (g_fail)
        return 1;
    printf("symmetric multi harness: %d files clean\n", files);
    return 0;
}
