/*
 * precond_harness.c — the host statement of the block-Jacobi preconditioner
 * (spmv_bjacobi_build, spmv_cpu_bjacobi_apply_multi; host/precond.c) compiled
 * into this binary with -fsanitize=address,undefined by `make test-san-precond`.
 *
 * usage: precond_harness FILE.mtx...
 * For every square file and every bs in 1..16, as the matrix itself and as a
 * stored half (symmetric_half), with col_base 0 and with the columns shifted by
 * 1000 (col_base = 1000): the build into an inv of exactly n_blocks*bs*bs
 * doubles, so a write past a short last block is a sanitizer report; every
 * element must be finite and the two col_base forms must agree bit for bit.
 * Then Z = M^-1 R for k in {1, 3, 8} with ld == k and ld > k into exactly-sized
 * R and Z (they end with the k values of their last row): a read of R's gaps
 * past the last row or of a row at or past n, or a write into Z's gaps, is a
 * report; every element is compared bit for bit with the fma chain written out
 * here and Z's gaps must keep their fill.  Then the refused inputs, which must
 * write nothing.  Any mismatch or report fails.
 */
#include <math.h>
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

static void one_apply(const char *name, int64_t n, int32_t bs, const double *inv, int32_t k, int64_t ldr, int64_t ldz)
{
    const double fill = 12345.0;
    const size_t r_len = n > 0 ? (size_t)((n - 1) * ldr + k) : 0;
    const size_t z_len = n > 0 ? (size_t)((n - 1) * ldz + k) : 0;
    double *R = xmalloc(r_len * 8), *Z = xmalloc(z_len * 8);
    for (size_t i = 0; i < r_len; ++i)
        R[i] = 1.0 + (double)((i * 7) % 23) * 0.125 - (double)(i % 3);
    for (size_t i = 0; i < z_len; ++i)
        Z[i] = fill;
    CHECK(spmv_cpu_bjacobi_apply_multi(n, bs, inv, k, R, ldr, Z, ldz) == SPMV_SUCCESS, "%s bs=%d k=%d", name, bs, k);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r0 = i / bs * bs;
        const int64_t nb = n - r0 < bs ? n - r0 : bs;
        for (int32_t j = 0; j < k; ++j) {
            double s = inv[i * bs] * R[r0 * ldr + j];
            for (int64_t c = 1; c < nb; ++c)
                s = fma(inv[i * bs + c], R[(r0 + c) * ldr + j], s);
            CHECK(memcmp(&s, &Z[i * ldz + j], 8) == 0, "%s bs=%d k=%d: Z[%lld][%d] = %a, the chain gives %a", name, bs,
                  k, (long long)i, j, Z[i * ldz + j], s);
        }
    }
    for (int64_t r = 0; r + 1 < n; ++r)
        for (int64_t j = k; j < ldz; ++j)
            CHECK(memcmp(&Z[r * ldz + j], &fill, 8) == 0, "%s bs=%d k=%d: gap Z[%lld][%lld] written", name, bs, k,
                  (long long)r, (long long)j);
    /* refusals: nothing may be written */
    for (size_t i = 0; i < z_len; ++i)
        Z[i] = fill;
    CHECK(spmv_cpu_bjacobi_apply_multi(-1, bs, inv, k, R, ldr, Z, ldz) == SPMV_OTHER_ERROR, "%s: n -1", name);
    CHECK(spmv_cpu_bjacobi_apply_multi(n, 0, inv, k, R, ldr, Z, ldz) == SPMV_OTHER_ERROR, "%s: bs 0", name);
    CHECK(spmv_cpu_bjacobi_apply_multi(n, 17, inv, k, R, ldr, Z, ldz) == SPMV_OTHER_ERROR, "%s: bs 17", name);
    CHECK(spmv_cpu_bjacobi_apply_multi(n, bs, inv, 0, R, ldr, Z, ldz) == SPMV_OTHER_ERROR, "%s: k 0", name);
    CHECK(spmv_cpu_bjacobi_apply_multi(n, bs, inv, k, R, k - 1, Z, ldz) == SPMV_OTHER_ERROR, "%s: ldr", name);
    CHECK(spmv_cpu_bjacobi_apply_multi(n, bs, inv, k, R, ldr, Z, k - 1) == SPMV_OTHER_ERROR, "%s: ldz", name);
    if (n > 0) {
        CHECK(spmv_cpu_bjacobi_apply_multi(n, bs, NULL, k, R, ldr, Z, ldz) == SPMV_OTHER_ERROR, "%s: NULL inv", name);
        CHECK(spmv_cpu_bjacobi_apply_multi(n, bs, inv, k, NULL, ldr, Z, ldz) == SPMV_OTHER_ERROR, "%s: NULL R", name);
        CHECK(spmv_cpu_bjacobi_apply_multi(n, bs, inv, k, R, ldr, NULL, ldz) == SPMV_OTHER_ERROR, "%s: NULL Z", name);
    }
    for (size_t i = 0; i < z_len; ++i)
        CHECK(memcmp(&Z[i], &fill, 8) == 0, "%s bs=%d k=%d: a refused call wrote Z[%zu]", name, bs, k, i);
    free(R);
    free(Z);
}

static void one_bs(const char *name, int64_t n, const int64_t *ptr, const int32_t *cc, const int32_t *cc_shift,
                   const double *cv, int32_t bs)
{
    static const int32_t ks[] = {1, 3, 8};
    const double fill = 12345.0;
    const int64_t nbk = (n + bs - 1) / bs;
    const size_t len = (size_t)(nbk * bs * bs);
    double *inv = xmalloc(len * 8), *inv2 = xmalloc(len * 8);
    for (int32_t half = 0; half < 2; ++half) {
        int64_t sing = -1, sing2 = -1;
        CHECK(spmv_bjacobi_build(n, ptr, cc, cv, bs, 0, half, inv, &sing) == SPMV_SUCCESS, "%s bs=%d", name, bs);
        CHECK(spmv_bjacobi_build(n, ptr, cc_shift, cv, bs, 1000, half, inv2, &sing2) == SPMV_SUCCESS, "%s bs=%d shifted",
              name, bs);
        CHECK(sing >= 0 && sing <= nbk && sing == sing2, "%s bs=%d: %lld / %lld singular of %lld", name, bs,
              (long long)sing, (long long)sing2, (long long)nbk);
        CHECK(len == 0 || memcmp(inv, inv2, len * 8) == 0, "%s bs=%d: col_base changes the inverse", name, bs);
        for (size_t i = 0; i < len; ++i)
            CHECK(isfinite(inv[i]), "%s bs=%d: inv[%zu] = %a", name, bs, i, inv[i]);
        for (size_t i = 0; i < sizeof ks / sizeof ks[0] && !g_fail; ++i) {
            one_apply(name, n, bs, inv, ks[i], ks[i], ks[i]);
            one_apply(name, n, bs, inv, ks[i], ks[i] + 1, ks[i] + 2);
        }
    }
    /* refusals: nothing may be written */
    int64_t sing = -7;
    for (size_t i = 0; i < len; ++i)
        inv[i] = fill;
    CHECK(spmv_bjacobi_build(-1, ptr, cc, cv, bs, 0, 0, inv, &sing) == SPMV_OTHER_ERROR, "%s: n -1", name);
    CHECK(spmv_bjacobi_build(n, ptr, cc, cv, 0, 0, 0, inv, &sing) == SPMV_OTHER_ERROR, "%s: bs 0", name);
    CHECK(spmv_bjacobi_build(n, ptr, cc, cv, 17, 0, 0, inv, &sing) == SPMV_OTHER_ERROR, "%s: bs 17", name);
    CHECK(spmv_bjacobi_build(n, ptr, cc, cv, bs, -1, 0, inv, &sing) == SPMV_OTHER_ERROR, "%s: col_base -1", name);
    CHECK(spmv_bjacobi_build(n, NULL, cc, cv, bs, 0, 0, inv, &sing) == SPMV_OTHER_ERROR, "%s: NULL row_ptr", name);
    CHECK(spmv_bjacobi_build(n, ptr, cc, cv, bs, 0, 0, inv, NULL) == SPMV_OTHER_ERROR, "%s: NULL count", name);
    if (n > 0)
        CHECK(spmv_bjacobi_build(n, ptr, cc, cv, bs, 0, 0, NULL, &sing) == SPMV_OTHER_ERROR, "%s: NULL inv", name);
    if (ptr[n] > 0) {
        CHECK(spmv_bjacobi_build(n, ptr, NULL, cv, bs, 0, 0, inv, &sing) == SPMV_OTHER_ERROR, "%s: NULL col", name);
        CHECK(spmv_bjacobi_build(n, ptr, cc, NULL, bs, 0, 0, inv, &sing) == SPMV_OTHER_ERROR, "%s: NULL val", name);
    }
    CHECK(sing == -7, "%s bs=%d: a refused build wrote the count", name, bs);
    for (size_t i = 0; i < len; ++i)
        CHECK(memcmp(&inv[i], &fill, 8) == 0, "%s bs=%d: a refused build wrote inv[%zu]", name, bs, i);
    free(inv);
    free(inv2);
}

static void one_matrix(const char *name, int64_t n, int64_t nnz, const int32_t *row, const int32_t *col,
                       const double *val)
{
    int64_t *ptr = xmalloc((size_t)(n + 1) * 8);
    int32_t *cc = xmalloc((size_t)nnz * 4), *cc_shift = xmalloc((size_t)nnz * 4);
    double *cv = xmalloc((size_t)nnz * 8);
    CHECK(spmv_csr_from_coo(n, nnz, row, col, val, ptr, cc, cv) == SPMV_SUCCESS, "%s csr", name);
    for (int64_t e = 0; e < nnz; ++e)
        cc_shift[e] = cc[e] + 1000;
    for (int32_t bs = 1; bs <= 16 && !g_fail; ++bs)
        one_bs(name, n, ptr, cc, cc_shift, cv, bs);
    free(ptr);
    free(cc);
    free(cc_shift);
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
    int64_t sing = -1;
    CHECK(spmv_bjacobi_build(0, &zero, NULL, NULL, 3, 0, 0, NULL, &sing) == SPMV_SUCCESS && sing == 0, "0 x 0 build");
    CHECK(spmv_cpu_bjacobi_apply_multi(0, 3, NULL, 3, NULL, 3, NULL, 3) == SPMV_SUCCESS, "0 x 0 apply");
    if (g_fail)
        return 1;
    printf("precond harness: %d files clean\n", files);
    return 0;
}
