/*
 * symmetric_harness.c — the host side of the symmetric product
 * (spmv_coo_symmetrize, spmv_cpu_csr_sym; host/symmetric.c) compiled into this
 * binary with -fsanitize=address,undefined by `make test-san-symmetric`.
 *
 * usage: symmetric_harness FILE.mtx...
 * For every square file, taken as the stored half S: the count-only call, the
 * expansion (order checked entry by entry), y = (S + S^T - diag S) x by
 * spmv_cpu_csr_sym on the half storage and by the forward CPU loop over the
 * CSR of the expansion, both checked against the file-order sum of the
 * expanded COO (spmv_check).  Every buffer has exactly the documented size,
 * so a write or read past one is a sanitizer report.  Then the refused
 * inputs: indices out of range, negative sizes, NULL arrays.  A file that is
 * not square is skipped.  Any mismatch or report fails.
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

static void check_y(const char *what, int64_t n, int64_t nnz, const int32_t *row, const int32_t *col,
                    const double *val, const double *x, const double *y)
{
    int64_t first = -1;
    double ref = 0.0;
    const int64_t bad = spmv_check(n, nnz, row, col, val, x, y, 0.0, 1e-12, &first, &ref);
    CHECK(bad == 0, "%s: %lld bad rows, first %lld (got %g want %g)", what, (long long)bad, (long long)first,
          first >= 0 ? y[first] : 0.0, ref);
}

static void one_matrix(const char *name, int64_t n, int64_t nnz, const int32_t *row, const int32_t *col,
                       const double *val)
{
    char what[600];
    int64_t za = -1;
    CHECK(spmv_coo_symmetrize(n, nnz, row, col, NULL, &za, NULL, NULL, NULL) == SPMV_SUCCESS, "%s count", name);
    int64_t off = 0;
    for (int64_t i = 0; i < nnz; ++i)
        off += row[i] != col[i];
    CHECK(za == nnz + off, "%s: count %lld, want %lld", name, (long long)za, (long long)(nnz + off));
    if (za < 0)
        return;
    int32_t *er = xmalloc((size_t)za * 4), *ec = xmalloc((size_t)za * 4);
    double *ev = xmalloc((size_t)za * 8);
    int64_t zb = -1;
    CHECK(spmv_coo_symmetrize(n, nnz, row, col, val, &zb, er, ec, ev) == SPMV_SUCCESS && zb == za, "%s expand", name);
    int64_t k = nnz;
    for (int64_t i = 0; i < nnz && !g_fail; ++i) {
        CHECK(er[i] == row[i] && ec[i] == col[i] && ev[i] == val[i], "%s: entry %lld changed", name, (long long)i);
        if (row[i] != col[i]) {
            CHECK(er[k] == col[i] && ec[k] == row[i] && ev[k] == val[i], "%s: mirror of %lld", name, (long long)i);
            ++k;
        }
    }
    CHECK(k == za, "%s: %lld mirrored entries placed, want %lld", name, (long long)(k - nnz), (long long)off);

    /* the half storage and the expansion as CSR */
    int64_t *hp = xmalloc((size_t)(n + 1) * 8), *ap = xmalloc((size_t)(n + 1) * 8);
    int32_t *hc = xmalloc((size_t)nnz * 4), *ac = xmalloc((size_t)za * 4);
    double *hv = xmalloc((size_t)nnz * 8), *av = xmalloc((size_t)za * 8);
    CHECK(spmv_csr_from_coo(n, nnz, row, col, val, hp, hc, hv) == SPMV_SUCCESS, "%s csr of the half", name);
    CHECK(spmv_csr_from_coo(n, za, er, ec, ev, ap, ac, av) == SPMV_SUCCESS, "%s csr of the expansion", name);

    double *x = xmalloc((size_t)n * 8), *y = xmalloc((size_t)n * 8);
    for (int64_t i = 0; i < n; ++i) {
        x[i] = 1.0 + (double)(i % 17) * 0.25;
        y[i] = -7.0;
    }
    CHECK(spmv_cpu_csr_sym(n, hp, hc, hv, x, y) == SPMV_SUCCESS, "%s cpu csr_sym", name);
    snprintf(what, sizeof what, "%s csr_sym", name);
    check_y(what, n, za, er, ec, ev, x, y);
    for (int64_t i = 0; i < n; ++i)
        y[i] = -7.0;
    CHECK(spmv_cpu_csr(n, ap, ac, av, x, y, 2) == SPMV_SUCCESS, "%s cpu csr over the expansion", name);
    snprintf(what, sizeof what, "%s csr over the expansion", name);
    check_y(what, n, za, er, ec, ev, x, y);

    if (nnz > 0) { /* an index out of range is refused by both, nothing past the buffers touched */
        int32_t *bad = xmalloc((size_t)nnz * 4);
        const int32_t wrong[2] = {(int32_t)n, -1};
        for (int w = 0; w < 2; ++w) {
            memcpy(bad, col, (size_t)nnz * 4);
            bad[nnz - 1] = wrong[w];
            CHECK(spmv_coo_symmetrize(n, nnz, row, bad, val, &zb, er, ec, ev) == SPMV_OTHER_ERROR, "%s: column %d accepted", name, wrong[w]);
            CHECK(spmv_coo_symmetrize(n, nnz, bad, col, val, &zb, NULL, NULL, NULL) == SPMV_OTHER_ERROR, "%s: row %d accepted", name, wrong[w]);
            memcpy(bad, hc, (size_t)nnz * 4);
            bad[nnz - 1] = wrong[w];
            CHECK(spmv_cpu_csr_sym(n, hp, bad, hv, x, y) == SPMV_OTHER_ERROR, "%s: cpu column %d accepted", name, wrong[w]);
        }
        free(bad);
        CHECK(spmv_coo_symmetrize(n, nnz, NULL, col, val, &zb, er, ec, ev) == SPMV_OTHER_ERROR, "%s: NULL row", name);
        CHECK(spmv_coo_symmetrize(n, nnz, row, col, NULL, &zb, er, ec, ev) == SPMV_OTHER_ERROR, "%s: NULL val", name);
        CHECK(spmv_coo_symmetrize(n, nnz, row, col, val, &zb, er, NULL, ev) == SPMV_OTHER_ERROR, "%s: NULL col_out", name);
        CHECK(spmv_cpu_csr_sym(n, hp, hc, NULL, x, y) == SPMV_OTHER_ERROR, "%s: cpu NULL val", name);
        CHECK(spmv_cpu_csr_sym(n, hp, hc, hv, NULL, y) == SPMV_OTHER_ERROR, "%s: cpu NULL x", name);
    }
    if (n > 0)
        CHECK(spmv_cpu_csr_sym(n, hp, hc, hv, x, NULL) == SPMV_OTHER_ERROR, "%s: cpu NULL y", name);
    CHECK(spmv_coo_symmetrize(n, nnz, row, col, val, NULL, er, ec, ev) == SPMV_OTHER_ERROR, "%s: NULL count", name);
    CHECK(spmv_coo_symmetrize(-1, nnz, row, col, val, &zb, er, ec, ev) == SPMV_OTHER_ERROR, "%s: n -1", name);
    CHECK(spmv_coo_symmetrize(n, -1, row, col, val, &zb, er, ec, ev) == SPMV_OTHER_ERROR, "%s: nnz -1", name);
    CHECK(spmv_cpu_csr_sym(-1, hp, hc, hv, x, y) == SPMV_OTHER_ERROR, "%s: cpu n -1", name);
    CHECK(spmv_cpu_csr_sym(n, NULL, hc, hv, x, y) == SPMV_OTHER_ERROR, "%s: cpu NULL row_ptr", name);

    free(er);
    free(ec);
    free(ev);
    free(hp);
    free(ap);
    free(hc);
    free(ac);
    free(hv);
    free(av);
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
    int64_t z0 = -1;
    CHECK(spmv_coo_symmetrize(0, 0, NULL, NULL, NULL, &z0, NULL, NULL, NULL) == SPMV_SUCCESS && z0 == 0, "0 x 0 expand");
    CHECK(spmv_cpu_csr_sym(0, &zero, NULL, NULL, NULL, NULL) == SPMV_SUCCESS, "0 x 0 csr_sym");
    if (g_fail)
        return 1;
    printf("symmetric harness: %d files clean\n", files);
    return 0;
}
