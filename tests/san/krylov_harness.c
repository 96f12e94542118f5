/*
 * krylov_harness.c — the host statements of GMRES's three basis kernels
 * (spmv_cpu_krylov_project, spmv_cpu_krylov_combine, spmv_cpu_krylov_normalize;
 * host/krylov.c) compiled into this binary with -fsanitize=address,undefined by
 * `make test-san-krylov`.
 *
 * usage: krylov_harness
 * For n in {0, 1, 2, 67, 1025}, c in {1, 8, 9, 32} and ld == c, ld == c + 1 (the
 * vectors: ld 1 and 2): a basis of exactly (n - 1) ldv + c doubles, vectors of
 * exactly (n - 1) ld + 1, h and y of exactly c, so that a read of a gap past
 * the last row, of a row at or past n, or a write into a gap is a sanitizer
 * report.  project also runs with w_out == w and with w_out = column c of the
 * basis' own allocation; normalize with v == w, with and without a copy and
 * with s = 0.  Every element written is compared bit for bit with the chain
 * written out here; gaps must keep their fill and inputs their values.  Then
 * the refused inputs, which must write nothing.  Any mismatch or report fails.
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

static double *block_copy(const double *src, size_t len)
{
    double *p = xmalloc(len * 8);
    if (len)
        memcpy(p, src, len * 8);
    return p;
}

static int same_bits(double a, double b)
{
    return memcmp(&a, &b, 8) == 0;
}

static double *coefficients(int32_t c)
{
    double *h = xmalloc((size_t)c * 8);
    for (int32_t j = 0; j < c; ++j)
        h[j] = (j % 2 ? -1.0 : 1.0) * (0.5 + 0.375 * (double)((j * 5) % 7)) * (j % 5 == 3 ? 0.0 : 1.0);
    return h;
}

/* a vector's gaps (ld > 1) must hold kFill */
static void check_gaps(const double *p, int64_t n, int64_t ld, const char *what)
{
    for (int64_t i = 0; i + 1 < n; ++i)
        for (int64_t q = 1; q < ld; ++q)
            CHECK(same_bits(p[i * ld + q], kFill), "%s gap (%lld, %lld) written", what, (long long)i, (long long)q);
}

/* mode 0: w_out apart; 1: w_out == w; 2: w_out = column c of the basis' allocation (ldv > c) */
static void run_project(int64_t n, int32_t c, int64_t pad, int mode)
{
    const int64_t ldv = c + pad, ldw = 1 + pad;
    const int32_t cols = mode == 2 ? c + 1 : c; /* the allocation also holds column c */
    double *V = block_new(n, cols, ldv, 1), *V0 = block_copy(V, block_len(n, cols, ldv));
    double *w = block_new(n, 1, ldw, 2), *w0 = block_copy(w, block_len(n, 1, ldw));
    double *h = coefficients(c);
    double *sep = mode == 0 ? block_new(n, 1, ldw + 1, 3) : NULL;
    double *out = mode == 0 ? sep : (mode == 1 ? w : V + c);
    const int64_t ldo = mode == 0 ? ldw + 1 : (mode == 1 ? ldw : ldv);
    const int rc = spmv_cpu_krylov_project(n, c, V, ldv, h, w, ldw, out, ldo);
    ++g_calls;
    CHECK(rc == SPMV_SUCCESS, "project n=%lld c=%d pad=%lld mode=%d: rc %d", (long long)n, c, (long long)pad, mode, rc);
    for (int64_t i = 0; i < n; ++i) {
        double s = w0[i * ldw];
        for (int32_t j = 0; j < c; ++j)
            s = fma(-h[j], V0[i * ldv + j], s);
        CHECK(same_bits(out[i * ldo], s), "project w_out(%lld) = %a, want %a", (long long)i, out[i * ldo], s);
        for (int64_t j = 0; j < ldv && (i < n - 1 || j < cols); ++j)
            if (!(mode == 2 && j == c))
                CHECK(same_bits(V[i * ldv + j], V0[i * ldv + j]), "project changed V(%lld, %lld)", (long long)i,
                      (long long)j);
    }
    if (mode != 1)
        CHECK(block_len(n, 1, ldw) == 0 || memcmp(w, w0, block_len(n, 1, ldw) * 8) == 0, "project changed w");
    else
        check_gaps(w, n, ldw, "w");
    if (mode == 0)
        check_gaps(sep, n, ldo, "w_out");
    free(V), free(V0), free(w), free(w0), free(h), free(sep);
}

static void run_combine(int64_t n, int32_t c, int64_t pad)
{
    const int64_t ldv = c + pad, ldt = 1 + 2 * pad;
    double *V = block_new(n, c, ldv, 4), *V0 = block_copy(V, block_len(n, c, ldv));
    double *y = coefficients(c);
    double *t = xmalloc(block_len(n, 1, ldt) * 8);
    for (size_t i = 0; i < block_len(n, 1, ldt); ++i)
        t[i] = kFill;
    const int rc = spmv_cpu_krylov_combine(n, c, V, ldv, y, t, ldt);
    ++g_calls;
    CHECK(rc == SPMV_SUCCESS, "combine n=%lld c=%d pad=%lld: rc %d", (long long)n, c, (long long)pad, rc);
    for (int64_t i = 0; i < n; ++i) {
        double s = 0.0;
        for (int32_t j = 0; j < c; ++j)
            s = fma(V0[i * ldv + j], y[j], s);
        CHECK(same_bits(t[i * ldt], s), "combine t(%lld) = %a, want %a", (long long)i, t[i * ldt], s);
    }
    check_gaps(t, n, ldt, "t");
    CHECK(block_len(n, c, ldv) == 0 || memcmp(V, V0, block_len(n, c, ldv) * 8) == 0, "combine changed V");
    free(V), free(V0), free(y), free(t);
}

/* alias: v == w; with_copy: a contiguous copy of exactly n doubles */
static void run_normalize(int64_t n, int64_t pad, double s, int alias, int with_copy)
{
    const int64_t ldw = 1 + pad, ldv = alias ? ldw : 1 + 2 * pad;
    double *w = block_new(n, 1, ldw, 5), *w0 = block_copy(w, block_len(n, 1, ldw));
    double *v = alias ? w : xmalloc(block_len(n, 1, ldv) * 8);
    double *copy = with_copy ? xmalloc((size_t)n * 8) : NULL;
    if (!alias)
        for (size_t i = 0; i < block_len(n, 1, ldv); ++i)
            v[i] = kFill;
    const int rc = spmv_cpu_krylov_normalize(n, &s, w, ldw, v, ldv, copy);
    ++g_calls;
    CHECK(rc == SPMV_SUCCESS, "normalize n=%lld pad=%lld: rc %d", (long long)n, (long long)pad, rc);
    const double r = s <= 0.0 ? 0.0 : 1.0 / sqrt(s);
    for (int64_t i = 0; i < n; ++i) {
        const double want = w0[i * ldw] * r;
        CHECK(same_bits(v[i * ldv], want), "normalize v(%lld) = %a, want %a", (long long)i, v[i * ldv], want);
        CHECK(!copy || same_bits(copy[i], want), "normalize copy(%lld)", (long long)i);
        CHECK(s > 0.0 || v[i * ldv] == 0.0, "normalize: s = 0 left %a", v[i * ldv]);
    }
    check_gaps(v, n, ldv, "v");
    if (!alias) {
        CHECK(block_len(n, 1, ldw) == 0 || memcmp(w, w0, block_len(n, 1, ldw) * 8) == 0, "normalize changed w");
        free(v);
    }
    free(w), free(w0), free(copy);
}

static void refusals(void)
{
    const int64_t n = 3;
    const int32_t c = 2;
    double *V = block_new(n, c, c, 1), *w = block_new(n, 1, 1, 2), *o = block_new(n, 1, 1, 3);
    double *o0 = block_copy(o, (size_t)n);
    double h[2] = {0.5, -1.5}, s = 4.0;
    double *wide = block_new(n, 33, 33, 4);
#define REF(f, ...)                                                                      \
    do {                                                                                 \
        CHECK(f(__VA_ARGS__) == SPMV_OTHER_ERROR, "accepted " #f "(" #__VA_ARGS__ ")"); \
        ++g_calls;                                                                       \
    } while (0)
    REF(spmv_cpu_krylov_project, -1, c, V, c, h, w, 1, o, 1);
    REF(spmv_cpu_krylov_project, n, 0, V, c, h, w, 1, o, 1);
    REF(spmv_cpu_krylov_project, n, 33, wide, 33, h, w, 1, o, 1);
    REF(spmv_cpu_krylov_project, n, c, NULL, c, h, w, 1, o, 1);
    REF(spmv_cpu_krylov_project, n, c, V, c - 1, h, w, 1, o, 1);
    REF(spmv_cpu_krylov_project, n, c, V, c, NULL, w, 1, o, 1);
    REF(spmv_cpu_krylov_project, n, c, V, c, h, NULL, 1, o, 1);
    REF(spmv_cpu_krylov_project, n, c, V, c, h, w, 0, o, 1);
    REF(spmv_cpu_krylov_project, n, c, V, c, h, w, 1, NULL, 1);
    REF(spmv_cpu_krylov_project, n, c, V, c, h, w, 1, o, 0);
    REF(spmv_cpu_krylov_combine, -1, c, V, c, h, o, 1);
    REF(spmv_cpu_krylov_combine, n, 0, V, c, h, o, 1);
    REF(spmv_cpu_krylov_combine, n, 33, wide, 33, h, o, 1);
    REF(spmv_cpu_krylov_combine, n, c, NULL, c, h, o, 1);
    REF(spmv_cpu_krylov_combine, n, c, V, c - 1, h, o, 1);
    REF(spmv_cpu_krylov_combine, n, c, V, c, NULL, o, 1);
    REF(spmv_cpu_krylov_combine, n, c, V, c, h, NULL, 1);
    REF(spmv_cpu_krylov_combine, n, c, V, c, h, o, 0);
    REF(spmv_cpu_krylov_normalize, -1, &s, w, 1, o, 1, NULL);
    REF(spmv_cpu_krylov_normalize, n, NULL, w, 1, o, 1, NULL);
    REF(spmv_cpu_krylov_normalize, n, &s, NULL, 1, o, 1, NULL);
    REF(spmv_cpu_krylov_normalize, n, &s, w, 0, o, 1, NULL);
    REF(spmv_cpu_krylov_normalize, n, &s, w, 1, NULL, 1, NULL);
    REF(spmv_cpu_krylov_normalize, n, &s, w, 1, o, 0, NULL);
#undef REF
    CHECK(memcmp(o, o0, (size_t)n * 8) == 0, "a refused call wrote");
    /* n == 0: only the scalars are needed, nothing is touched */
    CHECK(spmv_cpu_krylov_project(0, c, NULL, c, h, NULL, 1, NULL, 1) == SPMV_SUCCESS, "project refused n == 0");
    CHECK(spmv_cpu_krylov_combine(0, c, NULL, c, h, NULL, 1) == SPMV_SUCCESS, "combine refused n == 0");
    CHECK(spmv_cpu_krylov_normalize(0, &s, NULL, 1, NULL, 1, NULL) == SPMV_SUCCESS, "normalize refused n == 0");
    g_calls += 3;
    free(V), free(w), free(o), free(o0), free(wide);
}

int main(void)
{
    static const int64_t ns[] = {0, 1, 2, 67, 1025};
    static const int32_t cs[] = {1, 8, 9, 32};
    for (size_t a = 0; a < sizeof ns / sizeof *ns; ++a) {
        for (size_t b = 0; b < sizeof cs / sizeof *cs; ++b)
            for (int64_t pad = 0; pad < 2; ++pad) {
                run_project(ns[a], cs[b], pad, 0);
                run_project(ns[a], cs[b], pad, 1);
                if (pad > 0)
                    run_project(ns[a], cs[b], pad, 2);
                run_combine(ns[a], cs[b], pad);
            }
        for (int64_t pad = 0; pad < 2; ++pad)
            for (int alias = 0; alias < 2; ++alias)
                for (int with_copy = 0; with_copy < 2; ++with_copy) {
                    run_normalize(ns[a], pad, 2.75, alias, with_copy);
                    run_normalize(ns[a], pad, 0.0, alias, with_copy);
                }
    }
    refusals();
    if (g_fail) {
        fprintf(stderr, "krylov harness: FAILED\n");
        return 1;
    }
    printf("krylov harness: %ld calls clean\n", g_calls);
    return 0;
}
