/*
 * bicgstab_harness.c — the host statements of BiCGSTAB's two fused vector
 * updates (spmv_cpu_bicgstab_update_multi, spmv_cpu_bicgstab_dir_multi;
 * host/bicgstab.c) compiled into this binary with -fsanitize=address,undefined
 * by `make test-san-bicgstab`.
 *
 * usage: bicgstab_harness
 * For n in {0, 1, 2, 67, 1025} and k in {1, 3, 8, 9} with ld == k and ld > k:
 * the update with Sh apart from R and with Sh == R, and the direction update,
 * each with plain scalars and with zero denominators, on blocks of exactly
 * (n - 1) ld + k doubles and scalar arrays of exactly k doubles, so that a read
 * of a gap past the last row, of a row at or past n, or a write into a gap is a
 * sanitizer report.  Every element written is compared bit for bit with the
 * rule written out here; the gaps of the outputs must keep their fill and the
 * inputs their values.  Then the refused inputs, which must write nothing.
 * Any mismatch or report fails.
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

static size_t block_len(int64_t n, int32_t k, int64_t ld)
{
    return n > 0 ? (size_t)((n - 1) * ld + k) : 0;
}

/* exactly (n - 1) ld + k doubles: live elements from a formula, gaps = kFill */
static double *block_new(int64_t n, int32_t k, int64_t ld, int salt)
{
    const size_t len = block_len(n, k, ld);
    double *p = xmalloc(len * 8);
    for (size_t i = 0; i < len; ++i)
        p[i] = (int64_t)(i % (size_t)ld) < k ? 0.25 + (double)((i * 7 + (size_t)salt * 3) % 23) * 0.125 - (double)(i % 3)
                                            : kFill;
    return p;
}

static double *block_copy(const double *src, int64_t n, int32_t k, int64_t ld)
{
    const size_t len = block_len(n, k, ld);
    double *p = xmalloc(len * 8);
    if (len)
        memcpy(p, src, len * 8);
    return p;
}

static int block_same(const double *a, const double *b, int64_t n, int32_t k, int64_t ld)
{
    const size_t len = block_len(n, k, ld);
    return len == 0 || memcmp(a, b, len * 8) == 0;
}

/* exactly k doubles, none zero; zero_at >= 0: that one is 0 */
static double *scalars_new(int32_t k, int salt, int zero_at)
{
    double *p = xmalloc((size_t)k * 8);
    for (int32_t j = 0; j < k; ++j)
        p[j] = ((j + salt) % 2 ? -1.0 : 1.0) * (0.5 + 0.375 * (double)((j * 5 + salt) % 7));
    if (zero_at >= 0)
        p[zero_at % k] = 0.0;
    return p;
}

static double ratio(double a, double b)
{
    return b == 0.0 ? 0.0 : a / b;
}

static int same_bits(double a, double b)
{
    return memcmp(&a, &b, 8) == 0;
}

static void run_update(int64_t n, int32_t k, int64_t pad, int alias, int zeros)
{
    const int64_t ldph = k + pad, ldsh = k + (alias ? 3 * pad : 2 * pad), ldt = k + pad, ldx = k + 2 * pad,
                  ldr = k + 3 * pad;
    double *an = scalars_new(k, 1, -1), *ad = scalars_new(k, 2, zeros ? 0 : -1);
    double *wn = scalars_new(k, 3, -1), *wd = scalars_new(k, 4, zeros ? k - 1 : -1);
    double *Ph = block_new(n, k, ldph, 1), *T = block_new(n, k, ldt, 2), *X = block_new(n, k, ldx, 3);
    double *R = block_new(n, k, ldr, 4), *Sh = alias ? R : block_new(n, k, ldsh, 5);
    double *Ph0 = block_copy(Ph, n, k, ldph), *T0 = block_copy(T, n, k, ldt), *X0 = block_copy(X, n, k, ldx);
    double *R0 = block_copy(R, n, k, ldr), *Sh0 = alias ? R0 : block_copy(Sh, n, k, ldsh);
    const int rc = spmv_cpu_bicgstab_update_multi(n, k, an, ad, wn, wd, Ph, ldph, Sh, ldsh, T, ldt, X, ldx, R, ldr);
    ++g_calls;
    CHECK(rc == SPMV_SUCCESS, "update n=%lld k=%d pad=%lld alias=%d: rc %d", (long long)n, k, (long long)pad, alias, rc);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < ldx && (i < n - 1 || j < k); ++j) {
            const double got = X[i * ldx + j];
            if (j >= k) {
                CHECK(same_bits(got, kFill), "update: X gap (%lld, %lld) written", (long long)i, (long long)j);
                continue;
            }
            const double al = ratio(an[j], ad[j]), om = ratio(wn[j], wd[j]);
            const double want = fma(om, Sh0[i * ldsh + j], fma(al, Ph0[i * ldph + j], X0[i * ldx + j]));
            CHECK(same_bits(got, want), "update: X(%lld, %lld) = %a, want %a", (long long)i, (long long)j, got, want);
        }
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < ldr && (i < n - 1 || j < k); ++j) {
            const double got = R[i * ldr + j];
            if (j >= k) {
                CHECK(same_bits(got, kFill), "update: R gap (%lld, %lld) written", (long long)i, (long long)j);
                continue;
            }
            const double want = fma(-ratio(wn[j], wd[j]), T0[i * ldt + j], R0[i * ldr + j]);
            CHECK(same_bits(got, want), "update: R(%lld, %lld) = %a, want %a", (long long)i, (long long)j, got, want);
            if (zeros && j == k - 1)
                CHECK(same_bits(got, R0[i * ldr + j]), "update: omega = 0 moved R(%lld, %lld)", (long long)i, (long long)j);
        }
    CHECK(block_same(Ph, Ph0, n, k, ldph) && block_same(T, T0, n, k, ldt), "update: an input changed");
    if (!alias)
        CHECK(block_same(Sh, Sh0, n, k, ldsh), "update: Sh changed");
    free(an), free(ad), free(wn), free(wd), free(Ph), free(T), free(X), free(R), free(Ph0), free(T0), free(X0), free(R0);
    if (!alias)
        free(Sh), free(Sh0);
}

static void run_dir(int64_t n, int32_t k, int64_t pad, int zeros)
{
    const int64_t ldv = k + pad, ldr = k + 2 * pad, ldp = k + 3 * pad;
    /* zeros 1: rv = 0 (beta = 0); 2: ts = 0 (beta = 0, omega = 0); 3: tt = 0 (omega = 0) */
    double *rho = scalars_new(k, 5, -1), *rv = scalars_new(k, 6, zeros == 1 ? 0 : -1);
    double *tt = scalars_new(k, 7, zeros == 3 ? 0 : -1), *ts = scalars_new(k, 8, zeros == 2 ? 0 : -1);
    double *V = block_new(n, k, ldv, 6), *R = block_new(n, k, ldr, 7), *P = block_new(n, k, ldp, 8);
    double *V0 = block_copy(V, n, k, ldv), *R0 = block_copy(R, n, k, ldr), *P0 = block_copy(P, n, k, ldp);
    const int rc = spmv_cpu_bicgstab_dir_multi(n, k, rho, rv, tt, ts, V, ldv, R, ldr, P, ldp);
    ++g_calls;
    CHECK(rc == SPMV_SUCCESS, "dir n=%lld k=%d pad=%lld: rc %d", (long long)n, k, (long long)pad, rc);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t j = 0; j < ldp && (i < n - 1 || j < k); ++j) {
            const double got = P[i * ldp + j];
            if (j >= k) {
                CHECK(same_bits(got, kFill), "dir: P gap (%lld, %lld) written", (long long)i, (long long)j);
                continue;
            }
            const double beta = ratio(rho[j], rv[j]) * ratio(tt[j], ts[j]), om = ratio(ts[j], tt[j]);
            const double want = fma(beta, fma(-om, V0[i * ldv + j], P0[i * ldp + j]), R0[i * ldr + j]);
            CHECK(same_bits(got, want) && isfinite(got), "dir: P(%lld, %lld) = %a, want %a", (long long)i,
                  (long long)j, got, want);
            if ((zeros == 1 || zeros == 2) && j == 0)
                CHECK(same_bits(got, R0[i * ldr + j]), "dir: beta = 0 but P(%lld, 0) != R", (long long)i);
        }
    CHECK(block_same(V, V0, n, k, ldv) && block_same(R, R0, n, k, ldr), "dir: an input changed");
    free(rho), free(rv), free(tt), free(ts), free(V), free(R), free(P), free(V0), free(R0), free(P0);
}

static void refusals(void)
{
    const int64_t n = 3;
    const int32_t k = 2;
    double s[2] = {1.0, 2.0};
    double *A = block_new(n, k, k, 1), *B = block_new(n, k, k, 2), *C = block_new(n, k, k, 3);
    double *X = block_new(n, k, k, 4), *R = block_new(n, k, k + 1, 5);
    double *X0 = block_copy(X, n, k, k), *R0 = block_copy(R, n, k, k + 1);
#define UPD(...) CHECK(spmv_cpu_bicgstab_update_multi(__VA_ARGS__) == SPMV_OTHER_ERROR, "accepted update(" #__VA_ARGS__ ")")
    UPD(-1, k, s, s, s, s, A, k, B, k, C, k, X, k, R, k + 1);
    UPD(n, 0, s, s, s, s, A, k, B, k, C, k, X, k, R, k + 1);
    UPD(n, k, NULL, s, s, s, A, k, B, k, C, k, X, k, R, k + 1);
    UPD(n, k, s, NULL, s, s, A, k, B, k, C, k, X, k, R, k + 1);
    UPD(n, k, s, s, NULL, s, A, k, B, k, C, k, X, k, R, k + 1);
    UPD(n, k, s, s, s, NULL, A, k, B, k, C, k, X, k, R, k + 1);
    UPD(n, k, s, s, s, s, NULL, k, B, k, C, k, X, k, R, k + 1);
    UPD(n, k, s, s, s, s, A, k, NULL, k, C, k, X, k, R, k + 1);
    UPD(n, k, s, s, s, s, A, k, B, k, NULL, k, X, k, R, k + 1);
    UPD(n, k, s, s, s, s, A, k, B, k, C, k, NULL, k, R, k + 1);
    UPD(n, k, s, s, s, s, A, k, B, k, C, k, X, k, NULL, k + 1);
    UPD(n, k, s, s, s, s, A, k - 1, B, k, C, k, X, k, R, k + 1);
    UPD(n, k, s, s, s, s, A, k, B, k - 1, C, k, X, k, R, k + 1);
    UPD(n, k, s, s, s, s, A, k, B, k, C, k - 1, X, k, R, k + 1);
    UPD(n, k, s, s, s, s, A, k, B, k, C, k, X, k - 1, R, k + 1);
    UPD(n, k, s, s, s, s, A, k, B, k, C, k, X, k, R, k - 1);
    UPD(n, k, s, s, s, s, A, k, R, k, C, k, X, k, R, k + 1); /* Sh == R, two leading dimensions */
#undef UPD
#define DIR(...) CHECK(spmv_cpu_bicgstab_dir_multi(__VA_ARGS__) == SPMV_OTHER_ERROR, "accepted dir(" #__VA_ARGS__ ")")
    DIR(-1, k, s, s, s, s, A, k, B, k, X, k);
    DIR(n, 0, s, s, s, s, A, k, B, k, X, k);
    DIR(n, k, NULL, s, s, s, A, k, B, k, X, k);
    DIR(n, k, s, NULL, s, s, A, k, B, k, X, k);
    DIR(n, k, s, s, NULL, s, A, k, B, k, X, k);
    DIR(n, k, s, s, s, NULL, A, k, B, k, X, k);
    DIR(n, k, s, s, s, s, NULL, k, B, k, X, k);
    DIR(n, k, s, s, s, s, A, k, NULL, k, X, k);
    DIR(n, k, s, s, s, s, A, k, B, k, NULL, k);
    DIR(n, k, s, s, s, s, A, k - 1, B, k, X, k);
    DIR(n, k, s, s, s, s, A, k, B, k - 1, X, k);
    DIR(n, k, s, s, s, s, A, k, B, k, X, k - 1);
#undef DIR
    CHECK(block_same(X, X0, n, k, k) && block_same(R, R0, n, k, k + 1), "a refused call wrote");
    /* n == 0: no array is needed, nothing is touched */
    CHECK(spmv_cpu_bicgstab_update_multi(0, k, s, s, s, s, NULL, k, NULL, k, NULL, k, NULL, k, NULL, k) == SPMV_SUCCESS,
          "update refused n == 0");
    CHECK(spmv_cpu_bicgstab_dir_multi(0, k, s, s, s, s, NULL, k, NULL, k, NULL, k) == SPMV_SUCCESS, "dir refused n == 0");
    g_calls += 31;
    free(A), free(B), free(C), free(X), free(R), free(X0), free(R0);
}

int main(void)
{
    static const int64_t ns[] = {0, 1, 2, 67, 1025};
    static const int32_t ks[] = {1, 3, 8, 9};
    for (size_t a = 0; a < sizeof ns / sizeof *ns; ++a)
        for (size_t b = 0; b < sizeof ks / sizeof *ks; ++b)
            for (int64_t pad = 0; pad < 2; ++pad) {
                for (int alias = 0; alias < 2; ++alias)
                    for (int zeros = 0; zeros < 2; ++zeros)
                        run_update(ns[a], ks[b], pad, alias, zeros);
                for (int zeros = 0; zeros < 4; ++zeros)
                    run_dir(ns[a], ks[b], pad, zeros);
            }
    refusals();
    if (g_fail) {
        fprintf(stderr, "bicgstab harness: FAILED\n");
        return 1;
    }
    printf("bicgstab harness: %ld calls clean\n", g_calls);
    return 0;
}
