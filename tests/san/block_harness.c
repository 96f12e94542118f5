/*
 * block_harness.c — the host statement of the block combine
 * (spmv_cpu_block_combine_multi; host/block.c) compiled into this binary with
 * -fsanitize=address,undefined by `make test-san-block`.
 *
 * usage: block_harness
 * For n in {0, 1, 2, 67, 1025}, kc in {1, 5, 8}, every operand count (1, 2 and
 * 3, widths out of {1, 3, 8}) with ld == width and ld > width: operands of
 * exactly (n - 1) ld + width doubles, C of exactly (sum of the widths) * kc and
 * Y of exactly (n - 1) ldy + kc, so that a read of a gap past the last row, of
 * a row at or past n, or a write into a gap is a sanitizer report.  Every
 * element written is compared bit for bit with the fma chain written out here;
 * the gaps of Y must keep their fill and the operands their values.  Then the
 * refused inputs, which must write nothing.  Any mismatch or report fails.
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

/* nops operands of the widths w[0 .. nops), absent ones with a NULL pointer */
static void run(int64_t n, int32_t kc, int nops, const int32_t *w, int64_t pad)
{
    int32_t ka[3] = {0, 0, 0}, total = 0;
    int64_t ld[3] = {0, 0, 0};
    double *A[3] = {NULL, NULL, NULL}, *A0[3] = {NULL, NULL, NULL};
    for (int q = 0; q < nops; ++q) {
        ka[q] = w[q];
        ld[q] = w[q] + pad * (q + 1);
        A[q] = block_new(n, ka[q], ld[q], q + 1);
        A0[q] = block_copy(A[q], block_len(n, ka[q], ld[q]));
        total += ka[q];
    }
    const int64_t ldy = kc + 2 * pad;
    double *C = xmalloc((size_t)(total * kc) * 8);
    for (int32_t e = 0; e < total * kc; ++e)
        C[e] = (e % 2 ? -1.0 : 1.0) * (0.5 + 0.375 * (double)((e * 5) % 7)) * (e % 11 == 3 ? 0.0 : 1.0);
    const size_t ylen = block_len(n, kc, ldy);
    double *Y = xmalloc(ylen * 8);
    for (size_t i = 0; i < ylen; ++i)
        Y[i] = kFill;
    const int rc = spmv_cpu_block_combine_multi(n, kc, C, ka[0], A[0], ld[0], ka[1], A[1], ld[1], ka[2], A[2], ld[2], Y,
                                                ldy);
    ++g_calls;
    CHECK(rc == SPMV_SUCCESS, "n=%lld kc=%d nops=%d pad=%lld: rc %d", (long long)n, kc, nops, (long long)pad, rc);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t c = 0; c < ldy && (i < n - 1 || c < kc); ++c) {
            const double got = Y[i * ldy + c];
            if (c >= kc) {
                CHECK(same_bits(got, kFill), "Y gap (%lld, %lld) written", (long long)i, (long long)c);
                continue;
            }
            double s = 0.0;
            int32_t r0 = 0;
            for (int q = 0; q < nops; ++q) {
                for (int32_t r = 0; r < ka[q]; ++r)
                    s = fma(A0[q][i * ld[q] + r], C[(r0 + r) * kc + c], s);
                r0 += ka[q];
            }
            CHECK(same_bits(got, s), "Y(%lld, %lld) = %a, want %a", (long long)i, (long long)c, got, s);
        }
    for (int q = 0; q < nops; ++q) {
        const size_t len = block_len(n, ka[q], ld[q]);
        CHECK(len == 0 || memcmp(A[q], A0[q], len * 8) == 0, "operand %d changed", q);
        free(A[q]), free(A0[q]);
    }
    free(C), free(Y);
}

static void refusals(void)
{
    const int64_t n = 3;
    const int32_t k = 2;
    double *A = block_new(n, k, k, 1), *B = block_new(n, k, k + 1, 2), *Y = block_new(n, k, k, 3);
    double *Y0 = block_copy(Y, block_len(n, k, k));
    double C[3 * 2 * 2];
    for (int e = 0; e < 12; ++e)
        C[e] = 1.0 + e;
#define REF(...) CHECK(spmv_cpu_block_combine_multi(__VA_ARGS__) == SPMV_OTHER_ERROR, "accepted combine(" #__VA_ARGS__ ")")
    REF(-1, k, C, k, A, k, 0, NULL, 0, 0, NULL, 0, Y, k);
    REF(n, 0, C, k, A, k, 0, NULL, 0, 0, NULL, 0, Y, k);
    REF(n, 9, C, k, A, k, 0, NULL, 0, 0, NULL, 0, Y, 9);
    REF(n, k, NULL, k, A, k, 0, NULL, 0, 0, NULL, 0, Y, k);
    REF(n, k, C, 0, A, k, 0, B, k + 1, 0, NULL, 0, Y, k); /* no operand present */
    REF(n, k, C, -1, A, k, 0, NULL, 0, 0, NULL, 0, Y, k);
    REF(n, k, C, 9, A, 9, 0, NULL, 0, 0, NULL, 0, Y, k);
    REF(n, k, C, k, NULL, k, 0, NULL, 0, 0, NULL, 0, Y, k);
    REF(n, k, C, k, A, k - 1, 0, NULL, 0, 0, NULL, 0, Y, k);
    REF(n, k, C, k, A, k, k, NULL, k + 1, 0, NULL, 0, Y, k);
    REF(n, k, C, k, A, k, k, B, k - 1, 0, NULL, 0, Y, k);
    REF(n, k, C, k, A, k, k, B, k + 1, k, NULL, k, Y, k);
    REF(n, k, C, k, A, k, k, B, k + 1, 9, A, 9, Y, k);
    REF(n, k, C, k, A, k, 0, NULL, 0, 0, NULL, 0, NULL, k);
    REF(n, k, C, k, A, k, 0, NULL, 0, 0, NULL, 0, Y, k - 1);
#undef REF
    CHECK(memcmp(Y, Y0, block_len(n, k, k) * 8) == 0, "a refused call wrote");
    /* n == 0: no array but C is needed, nothing is touched */
    CHECK(spmv_cpu_block_combine_multi(0, k, C, k, NULL, k, k, NULL, k, 0, NULL, 0, NULL, k) == SPMV_SUCCESS,
          "refused n == 0");
    /* an absent operand's pointer and leading dimension are ignored; operands may overlap */
    CHECK(spmv_cpu_block_combine_multi(n, k, C, k, A, k, 0, (const double *)8, -5, k, A, k, Y, k) == SPMV_SUCCESS,
          "refused an absent middle operand");
    g_calls += 17;
    free(A), free(B), free(Y), free(Y0);
}

int main(void)
{
    static const int64_t ns[] = {0, 1, 2, 67, 1025};
    static const int32_t kcs[] = {1, 5, 8};
    static const int32_t ws[][3] = {{1, 0, 0}, {3, 0, 0}, {8, 0, 0}, {1, 8, 0}, {8, 3, 0}, {3, 1, 8}, {8, 8, 8}};
    static const int nops[] = {1, 1, 1, 2, 2, 3, 3};
    for (size_t a = 0; a < sizeof ns / sizeof *ns; ++a)
        for (size_t b = 0; b < sizeof kcs / sizeof *kcs; ++b)
            for (size_t c = 0; c < sizeof nops / sizeof *nops; ++c)
                for (int64_t pad = 0; pad < 2; ++pad)
                    run(ns[a], kcs[b], nops[c], ws[c], pad);
    refusals();
    if (g_fail) {
        fprintf(stderr, "block harness: FAILED\n");
        return 1;
    }
    printf("block harness: %ld calls clean\n", g_calls);
    return 0;
}
