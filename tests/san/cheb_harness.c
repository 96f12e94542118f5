/*
 * cheb_harness.c — the host statement of one Chebyshev step over block Jacobi
 * (spmv_cpu_bjacobi_cheb_step_multi; host/precond.c) compiled into this binary
 * with -fsanitize=address,undefined by `make test-san-cheb`.
 *
 * usage: cheb_harness
 * For every bs in 1..16 and n in {1, bs - 1, bs, 2 bs + 1 (a short last block),
 * 67}, k in {1, 3, 8} with ld == k and ld > k: step 0 and a general step, the
 * latter with Zout apart from Zin and with Zout == Zin, on R, AZ, D, Zin and
 * Zout of exactly (n - 1) ld + k doubles each and an inv of exactly
 * n_blocks bs bs doubles, so that a read of a gap past the last row, of a row
 * at or past n, or a write into a gap is a sanitizer report.  Every element of
 * D and Zout is compared bit for bit with the rule written out here; the gaps
 * of D and Zout must keep their fill, R, AZ and a separate Zin their values.
 * Then the refused inputs, which must write nothing.  Any mismatch or report
 * fails.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spmv_host.h"

static int g_fail = 0;
static long g_calls = 0;

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

static const double kFill = 12345.0;

/* exactly (n - 1) ld + k doubles: live elements from a formula, gaps = kFill */
static double *block_new(int64_t n, int32_t k, int64_t ld, int salt)
{
    const size_t len = n > 0 ? (size_t)((n - 1) * ld + k) : 0;
    double *p = xmalloc(len * 8);
    for (size_t i = 0; i < len; ++i)
        p[i] = (int64_t)(i % (size_t)ld) < k ? 0.25 + (double)((i * 7 + (size_t)salt * 3) % 23) * 0.125 - (double)(i % 3)
                                            : kFill;
    return p;
}

static double *block_copy(const double *src, int64_t n, int32_t k, int64_t ld)
{
    const size_t len = n > 0 ? (size_t)((n - 1) * ld + k) : 0;
    double *p = xmalloc(len * 8);
    if (len)
        memcpy(p, src, len * 8);
    return p;
}

static int block_same(const double *a, const double *b, int64_t n, int32_t k, int64_t ld)
{
    const size_t len = n > 0 ? (size_t)((n - 1) * ld + k) : 0;
    return len == 0 || memcmp(a, b, len * 8) == 0;
}

/* mode 0: step 0; 1: general, Zout apart from Zin; 2: general, Zout == Zin */
static void one_step(int64_t n, int32_t bs, const double *inv, int32_t k, int64_t ld, int mode)
{
    const double a = 0.375, b = 1.7;
    const int64_t ldr = ld, ldaz = ld + (ld > k), ldd = ld + 2 * (ld > k), ldz = ld;
    double *R = block_new(n, k, ldr, 1), *AZ = block_new(n, k, ldaz, 2), *D = block_new(n, k, ldd, 3);
    double *Zin = block_new(n, k, ldz, 4), *Zsep = block_new(n, k, ldz, 5);
    double *R0 = block_copy(R, n, k, ldr), *AZ0 = block_copy(AZ, n, k, ldaz), *D0 = block_copy(D, n, k, ldd);
    double *Zin0 = block_copy(Zin, n, k, ldz);
    double *Zout = mode == 2 ? Zin : Zsep;
    const int rc = spmv_cpu_bjacobi_cheb_step_multi(n, bs, inv, k, a, b, R, ldr, mode ? AZ : NULL, ldaz, D, ldd,
                                                    mode ? Zin : NULL, ldz, Zout, ldz);
    ++g_calls;
    CHECK(rc == SPMV_SUCCESS, "n=%lld bs=%d k=%d mode %d: rc %d", (long long)n, bs, k, mode, rc);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t r0 = i / bs * bs;
        const int64_t nb = n - r0 < bs ? n - r0 : bs;
        for (int32_t j = 0; j < k; ++j) {
            double s = 0.0;
            for (int64_t c = 0; c < nb; ++c) {
                const double t = mode ? R0[(r0 + c) * ldr + j] - AZ0[(r0 + c) * ldaz + j] : R0[(r0 + c) * ldr + j];
                s = c == 0 ? inv[i * bs] * t : fma(inv[i * bs + c], t, s);
            }
            const double p = b * s;
            const double d = mode ? fma(a, D0[i * ldd + j], p) : p;
            const double z = mode ? Zin0[i * ldz + j] + d : d;
            CHECK(memcmp(&d, &D[i * ldd + j], 8) == 0, "n=%lld bs=%d k=%d mode %d: D[%lld][%d] = %a, the rule gives %a",
                  (long long)n, bs, k, mode, (long long)i, j, D[i * ldd + j], d);
            CHECK(memcmp(&z, &Zout[i * ldz + j], 8) == 0,
                  "n=%lld bs=%d k=%d mode %d: Zout[%lld][%d] = %a, the rule gives %a", (long long)n, bs, k, mode,
                  (long long)i, j, Zout[i * ldz + j], z);
        }
    }
    for (int64_t r = 0; r + 1 < n; ++r) {
        for (int64_t j = k; j < ldd; ++j)
            CHECK(memcmp(&D[r * ldd + j], &kFill, 8) == 0, "n=%lld bs=%d k=%d: gap of D written", (long long)n, bs, k);
        for (int64_t j = k; j < ldz; ++j)
            CHECK(memcmp(&Zout[r * ldz + j], &kFill, 8) == 0, "n=%lld bs=%d k=%d: gap of Zout written", (long long)n,
                  bs, k);
    }
    CHECK(block_same(R, R0, n, k, ldr) && block_same(AZ, AZ0, n, k, ldaz), "n=%lld bs=%d k=%d: R or AZ written",
          (long long)n, bs, k);
    if (mode != 2)
        CHECK(block_same(Zin, Zin0, n, k, ldz), "n=%lld bs=%d k=%d mode %d: Zin written", (long long)n, bs, k, mode);
    free(R);
    free(AZ);
    free(D);
    free(Zin);
    free(Zsep);
    free(R0);
    free(AZ0);
    free(D0);
    free(Zin0);
}

static void refusals(int64_t n, int32_t bs, const double *inv, int32_t k)
{
    const int64_t ld = k + 1;
    double *R = block_new(n, k, ld, 1), *AZ = block_new(n, k, ld, 2), *D = block_new(n, k, ld, 3);
    double *Zin = block_new(n, k, ld, 4), *Zout = block_new(n, k, ld, 5);
    double *D0 = block_copy(D, n, k, ld), *Zin0 = block_copy(Zin, n, k, ld), *Zout0 = block_copy(Zout, n, k, ld);
#define STEP(...) CHECK(spmv_cpu_bjacobi_cheb_step_multi(__VA_ARGS__) == SPMV_OTHER_ERROR, "bs=%d: accepted " #__VA_ARGS__, bs)
    STEP(-1, bs, inv, k, .5, 2., R, ld, AZ, ld, D, ld, Zin, ld, Zout, ld);
    STEP(n, 0, inv, k, .5, 2., R, ld, AZ, ld, D, ld, Zin, ld, Zout, ld);
    STEP(n, 17, inv, k, .5, 2., R, ld, AZ, ld, D, ld, Zin, ld, Zout, ld);
    STEP(n, bs, inv, 0, .5, 2., R, ld, AZ, ld, D, ld, Zin, ld, Zout, ld);
    STEP(n, bs, inv, k, .5, 2., R, k - 1, AZ, ld, D, ld, Zin, ld, Zout, ld);
    STEP(n, bs, inv, k, .5, 2., R, ld, AZ, k - 1, D, ld, Zin, ld, Zout, ld);
    STEP(n, bs, inv, k, .5, 2., R, ld, AZ, ld, D, k - 1, Zin, ld, Zout, ld);
    STEP(n, bs, inv, k, .5, 2., R, ld, AZ, ld, D, ld, Zin, k - 1, Zout, ld);
    STEP(n, bs, inv, k, .5, 2., R, ld, AZ, ld, D, ld, Zin, ld, Zout, k - 1);
    STEP(n, bs, inv, k, .5, 2., R, ld, AZ, ld, D, ld, Zin, ld, Zin, ld + 1); /* Zout == Zin, two lds */
    STEP(n, bs, NULL, k, .5, 2., R, ld, AZ, ld, D, ld, Zin, ld, Zout, ld);
    STEP(n, bs, inv, k, .5, 2., NULL, ld, AZ, ld, D, ld, Zin, ld, Zout, ld);
    STEP(n, bs, inv, k, .5, 2., R, ld, AZ, ld, NULL, ld, Zin, ld, Zout, ld);
    STEP(n, bs, inv, k, .5, 2., R, ld, AZ, ld, D, ld, NULL, ld, Zout, ld);
    STEP(n, bs, inv, k, .5, 2., R, ld, AZ, ld, D, ld, Zin, ld, NULL, ld);
    STEP(n, bs, inv, k, .5, 2., R, ld, NULL, ld, D, k - 1, NULL, ld, Zout, ld); /* step 0 */
    STEP(n, bs, inv, k, .5, 2., R, ld, NULL, ld, NULL, ld, NULL, ld, Zout, ld);
    STEP(n, bs, inv, k, .5, 2., R, ld, NULL, ld, D, ld, NULL, ld, NULL, ld);
#undef STEP
    g_calls += 18;
    CHECK(block_same(D, D0, n, k, ld) && block_same(Zin, Zin0, n, k, ld) && block_same(Zout, Zout0, n, k, ld),
          "bs=%d: a refused step wrote", bs);
    free(R);
    free(AZ);
    free(D);
    free(Zin);
    free(Zout);
    free(D0);
    free(Zin0);
    free(Zout0);
}

int main(void)
{
    static const int32_t ks[] = {1, 3, 8};
    for (int32_t bs = 1; bs <= 16 && !g_fail; ++bs) {
        const int64_t ns[] = {1, bs - 1, bs, 2 * bs + 1, 67};
        for (size_t a = 0; a < sizeof ns / sizeof ns[0]; ++a) {
            const int64_t n = ns[a];
            if (n < 1)
                continue;
            const int64_t nbk = (n + bs - 1) / bs;
            const size_t len = (size_t)(nbk * bs * bs);
            double *inv = xmalloc(len * 8);
            for (size_t i = 0; i < len; ++i)
                inv[i] = 0.5 - (double)((i * 11) % 17) * 0.0625;
            for (size_t i = 0; i < sizeof ks / sizeof ks[0]; ++i)
                for (int mode = 0; mode < 3; ++mode) {
                    one_step(n, bs, inv, ks[i], ks[i], mode);
                    one_step(n, bs, inv, ks[i], ks[i] + 1, mode);
                }
            if (n == 67)
                refusals(n, bs, inv, 3);
            free(inv);
        }
    }
    /* no rows at all */
    CHECK(spmv_cpu_bjacobi_cheb_step_multi(0, 3, NULL, 3, .5, 2., NULL, 3, NULL, 3, NULL, 3, NULL, 3, NULL, 3) ==
              SPMV_SUCCESS,
          "0 rows, step 0");
    if (g_fail)
        return 1;
    printf("cheb harness: %ld calls clean\n", g_calls);
    return 0;
}
