/*
 * bsr_harness.c — the host side of block CSR (spmv_bsr_plan, spmv_bsr_fill,
 * spmv_cpu_bsr; host/bsr.c) compiled into this binary with
 * -fsanitize=address,undefined by `make test-san-bsr`.
 *
 * usage: bsr_harness FILE.mtx...
 * For every file and every block size 1..SPMV_BSR_MAX_B: the CSR from the COO,
 * the block count, the three arrays (offsets monotone, block columns strictly
 * ascending and in range, the stored values summing to the entries'), and
 * y = A x by spmv_cpu_bsr checked against the file-order sum (spmv_check).
 * Every buffer has exactly the documented size, x and y included, so the
 * partial last block row and block column (sizes that are no multiple of b)
 * reading or writing past an end is a sanitizer report.  Then the refused
 * inputs: b out of range, negative sizes, columns out of range, too many
 * columns, NULL arrays.  Any mismatch or report fails.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spmv_host.h"

static int g_fail = 0;
static long g_calls = 0;

#define CHECK(cond, ...)                                                                 \
    do {                                                                                 \
        ++g_calls;                                                                       \
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

static void one_block_size(const char *name, int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *row,
                           const int32_t *col, const double *val, const int64_t *ptr, const int32_t *cc,
                           const double *cv, int32_t b)
{
    int64_t n_brows = -1, n_blocks = -1;
    CHECK(spmv_bsr_plan(n_rows, n_cols, ptr, cc, b, &n_brows, &n_blocks) == SPMV_SUCCESS, "%s b=%d plan", name, b);
    CHECK(n_brows == (n_rows + b - 1) / b && n_blocks >= 0 && n_blocks <= nnz, "%s b=%d: %lld block rows, %lld blocks",
          name, b, (long long)n_brows, (long long)n_blocks);
    if (g_fail)
        return;
    int64_t *bp = xmalloc((size_t)(n_brows + 1) * 8);
    int32_t *bc = xmalloc((size_t)n_blocks * 4);
    double *bv = xmalloc((size_t)n_blocks * (size_t)(b * b) * 8);
    CHECK(spmv_bsr_fill(n_rows, n_cols, ptr, cc, cv, b, bp, bc, bv) == SPMV_SUCCESS, "%s b=%d fill", name, b);
    CHECK(bp[0] == 0 && bp[n_brows] == n_blocks, "%s b=%d: brow_ptr ends %lld..%lld", name, b, (long long)bp[0],
          (long long)bp[n_brows]);
    const int64_t n_bcols = (n_cols + b - 1) / b;
    for (int64_t I = 0; I < n_brows && !g_fail; ++I) {
        CHECK(bp[I] <= bp[I + 1], "%s b=%d: brow_ptr decreases at %lld", name, b, (long long)I);
        for (int64_t k = bp[I]; k < bp[I + 1]; ++k) {
            CHECK(bc[k] >= 0 && bc[k] < n_bcols, "%s b=%d: block column out of range at %lld", name, b, (long long)k);
            CHECK(k == bp[I] || bc[k - 1] < bc[k], "%s b=%d: block columns not ascending at %lld", name, b, (long long)k);
        }
    }
    double sv = 0.0, se = 0.0; /* integer-valued or not, the same multiset sums to about the same */
    for (int64_t k = 0; k < n_blocks * b * b; ++k)
        sv += bv[k];
    for (int64_t e = 0; e < nnz; ++e)
        se += cv[e];
    CHECK(sv - se <= 1e-9 * (1.0 + (se < 0 ? -se : se)) && se - sv <= 1e-9 * (1.0 + (se < 0 ? -se : se)),
          "%s b=%d: stored values sum to %g, entries to %g", name, b, sv, se);

    double *x = xmalloc((size_t)n_cols * 8);
    double *y = xmalloc((size_t)n_rows * 8);
    for (int64_t j = 0; j < n_cols; ++j)
        x[j] = 1.0 + (double)(j % 17) * 0.25;
    for (int64_t i = 0; i < n_rows; ++i)
        y[i] = -7.0;
    CHECK(spmv_cpu_bsr(n_rows, n_cols, b, n_brows, bp, bc, bv, x, y) == SPMV_SUCCESS, "%s b=%d cpu bsr", name, b);
    int64_t first = -1;
    double ref = 0.0;
    const int64_t bad = spmv_check(n_rows, nnz, row, col, val, x, y, 0.0, 1e-12, &first, &ref);
    CHECK(bad == 0, "%s b=%d: %lld bad rows, first %lld (got %g want %g)", name, b, (long long)bad, (long long)first,
          first >= 0 ? y[first] : 0.0, ref);

    /* refused by the CPU loop, y untouched */
    CHECK(spmv_cpu_bsr(n_rows, n_cols, b, n_brows + 1, bp, bc, bv, x, y) == SPMV_OTHER_ERROR, "%s: n_brows + 1", name);
    CHECK(spmv_cpu_bsr(n_rows, n_cols, b, n_brows, NULL, bc, bv, x, y) == SPMV_OTHER_ERROR, "%s: NULL brow_ptr", name);
    if (n_rows > 0)
        CHECK(spmv_cpu_bsr(n_rows, n_cols, b, n_brows, bp, bc, bv, x, NULL) == SPMV_OTHER_ERROR, "%s: NULL y", name);
    if (n_blocks > 0) {
        CHECK(spmv_cpu_bsr(n_rows, n_cols, b, n_brows, bp, NULL, bv, x, y) == SPMV_OTHER_ERROR, "%s: NULL bcol", name);
        CHECK(spmv_cpu_bsr(n_rows, n_cols, b, n_brows, bp, bc, NULL, x, y) == SPMV_OTHER_ERROR, "%s: NULL bval", name);
        CHECK(spmv_cpu_bsr(n_rows, n_cols, b, n_brows, bp, bc, bv, NULL, y) == SPMV_OTHER_ERROR, "%s: NULL x", name);
        const int32_t keep = bc[n_blocks - 1];
        bc[n_blocks - 1] = (int32_t)n_bcols;
        CHECK(spmv_cpu_bsr(n_rows, n_cols, b, n_brows, bp, bc, bv, x, y) == SPMV_OTHER_ERROR, "%s: bcol = n_bcols", name);
        bc[n_blocks - 1] = -1;
        CHECK(spmv_cpu_bsr(n_rows, n_cols, b, n_brows, bp, bc, bv, x, y) == SPMV_OTHER_ERROR, "%s: bcol = -1", name);
        bc[n_blocks - 1] = keep;
        CHECK(spmv_bsr_fill(n_rows, n_cols, ptr, cc, NULL, b, bp, bc, bv) == SPMV_OTHER_ERROR, "%s: fill NULL val", name);
        CHECK(spmv_bsr_fill(n_rows, n_cols, ptr, cc, cv, b, bp, NULL, bv) == SPMV_OTHER_ERROR, "%s: fill NULL bcol", name);
        CHECK(spmv_bsr_fill(n_rows, n_cols, ptr, cc, cv, b, bp, bc, NULL) == SPMV_OTHER_ERROR, "%s: fill NULL bval", name);
        CHECK(spmv_bsr_plan(n_rows, n_cols, ptr, NULL, b, &n_brows, &n_blocks) == SPMV_OTHER_ERROR, "%s: plan NULL col", name);
    }
    CHECK(spmv_bsr_fill(n_rows, n_cols, ptr, cc, cv, b, NULL, bc, bv) == SPMV_OTHER_ERROR, "%s: fill NULL brow_ptr", name);
    free(bp);
    free(bc);
    free(bv);
    free(x);
    free(y);
}

static void one_matrix(const char *name, int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *row,
                       const int32_t *col, const double *val)
{
    int64_t *ptr = xmalloc((size_t)(n_rows + 1) * 8);
    int32_t *cc = xmalloc((size_t)nnz * 4);
    double *cv = xmalloc((size_t)nnz * 8);
    CHECK(spmv_csr_from_coo(n_rows, nnz, row, col, val, ptr, cc, cv) == SPMV_SUCCESS, "%s csr", name);
    for (int32_t b = 1; b <= SPMV_BSR_MAX_B && !g_fail; ++b)
        one_block_size(name, n_rows, n_cols, nnz, row, col, val, ptr, cc, cv, b);

    int64_t nbr = -5, nbl = -5;
    CHECK(spmv_bsr_plan(n_rows, n_cols, ptr, cc, 0, &nbr, &nbl) == SPMV_OTHER_ERROR, "%s: b = 0", name);
    CHECK(spmv_bsr_plan(n_rows, n_cols, ptr, cc, SPMV_BSR_MAX_B + 1, &nbr, &nbl) == SPMV_OTHER_ERROR, "%s: b = 9", name);
    CHECK(spmv_bsr_plan(-1, n_cols, ptr, cc, 3, &nbr, &nbl) == SPMV_OTHER_ERROR, "%s: n_rows -1", name);
    CHECK(spmv_bsr_plan(n_rows, -1, ptr, cc, 3, &nbr, &nbl) == SPMV_OTHER_ERROR, "%s: n_cols -1", name);
    CHECK(spmv_bsr_plan(n_rows, (int64_t)INT32_MAX - 7, ptr, cc, 3, &nbr, &nbl) == SPMV_OTHER_ERROR, "%s: n_cols too large",
          name);
    CHECK(spmv_bsr_plan(n_rows, n_cols, ptr, cc, 3, NULL, &nbl) == SPMV_OTHER_ERROR, "%s: NULL n_brows", name);
    CHECK(spmv_bsr_plan(n_rows, n_cols, ptr, cc, 3, &nbr, NULL) == SPMV_OTHER_ERROR, "%s: NULL n_blocks", name);
    if (n_rows > 0)
        CHECK(spmv_bsr_plan(n_rows, n_cols, NULL, cc, 3, &nbr, &nbl) == SPMV_OTHER_ERROR, "%s: NULL row_ptr", name);
    CHECK(nbr == -5 && nbl == -5, "%s: a refused plan wrote its counts", name);
    if (nnz > 0) { /* a column out of range is refused by both, nothing written */
        const int32_t keep = cc[nnz - 1];
        int64_t bp1 = -9;
        for (int pass = 0; pass < 2; ++pass) {
            cc[nnz - 1] = pass ? -1 : (int32_t)n_cols;
            CHECK(spmv_bsr_plan(n_rows, n_cols, ptr, cc, 3, &nbr, &nbl) == SPMV_OTHER_ERROR, "%s: bad column planned", name);
            CHECK(spmv_bsr_fill(n_rows, n_cols, ptr, cc, cv, 3, &bp1, NULL, NULL) == SPMV_OTHER_ERROR && bp1 == -9,
                  "%s: bad column filled", name);
        }
        cc[nnz - 1] = keep;
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
    /* 2 rows x 5 columns at every b: one partial block row, a partial last block column */
    {
        const int32_t r2[] = {0, 0, 1, 1, 1}, c2[] = {4, 0, 3, 4, 3};
        const double v2[] = {1.0, 2.0, 3.0, 4.0, 5.0};
        one_matrix("2x5 (hand)", 2, 5, 5, r2, c2, v2);
    }
    /* no rows and no columns at all */
    int64_t nbr = -1, nbl = -1, bp0 = -1;
    CHECK(spmv_bsr_plan(0, 0, NULL, NULL, 3, &nbr, &nbl) == SPMV_SUCCESS && nbr == 0 && nbl == 0, "0 x 0 plan");
    CHECK(spmv_bsr_fill(0, 0, NULL, NULL, NULL, 3, &bp0, NULL, NULL) == SPMV_SUCCESS && bp0 == 0, "0 x 0 fill");
    CHECK(spmv_cpu_bsr(0, 0, 3, 0, &bp0, NULL, NULL, NULL, NULL) == SPMV_SUCCESS, "0 x 0 cpu bsr");
    if (g_fail)
        return 1;
    printf("bsr harness: %d files, %ld calls clean\n", files, g_calls);
    return 0;
}
