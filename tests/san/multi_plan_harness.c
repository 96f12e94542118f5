/*
 * multi_plan_harness.c — the host planner of the balanced multi-vector CSR run
 * (spmv_csr_multi_plan; host/formats.c) compiled into this binary with
 * -fsanitize=address,undefined by `make test-san-multi-plan`.
 *
 * usage: multi_plan_harness FILE.mtx...
 * For every file at (long_len, seg_len) in {(4, 8), (0, 3), (0, 1)}, for a
 * hand-made offset array with rows at every edge of both thresholds, for one
 * row of 20,001 entries and for the 100,000-row R-MAT at (128, 1024): the
 * counts by the NULL call, then the tables into heap arrays of exactly the
 * counted sizes, so a write past a table is a sanitizer report.  The tables
 * are checked entry by entry against the definition in spmv_host.h.  Then the
 * refused inputs, which must leave sentinel-filled outputs untouched.
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

static void verify(const char *name, int64_t n_rows, const int64_t *ptr, int32_t long_len, int32_t seg_len)
{
    int64_t nl = -1, ns = -1, nsl = -1, nl2 = -1, ns2 = -1, nsl2 = -1;
    CHECK(spmv_csr_multi_plan(n_rows, ptr, long_len, seg_len, &nl, &ns, &nsl, NULL, NULL, NULL, NULL, NULL) ==
              SPMV_SUCCESS, "%s (%d, %d): counts", name, long_len, seg_len);
    if (nl < 0 || ns < 0 || nsl < 0) {
        CHECK(0, "%s: negative counts", name);
        return;
    }
    int64_t *sb = xmalloc((size_t)ns * 8);
    int32_t *sc = xmalloc((size_t)ns * 4), *sd = xmalloc((size_t)ns * 4);
    int32_t *lr = xmalloc((size_t)(nl + 1) * 4), *lf = xmalloc((size_t)(nl + 1) * 4);
    CHECK(spmv_csr_multi_plan(n_rows, ptr, long_len, seg_len, &nl2, &ns2, &nsl2, sb, sc, sd, lr, lf) == SPMV_SUCCESS,
          "%s (%d, %d): fill", name, long_len, seg_len);
    CHECK(nl == nl2 && ns == ns2 && nsl == nsl2, "%s: the two calls count differently", name);
    int64_t i = 0, s = 0, slot = 0;
    for (int64_t r = 0; r < n_rows && !g_fail; ++r) {
        const int64_t len = ptr[r + 1] - ptr[r];
        if (len <= long_len)
            continue;
        CHECK(i < nl && lr[i] == r && lf[i] == slot, "%s: long row %lld listed as (%d, %d), slot %lld", name,
              (long long)r, i < nl ? lr[i] : -2, i < nl ? lf[i] : -2, (long long)slot);
        ++i;
        const int split = len > seg_len;
        for (int64_t b = ptr[r]; b < ptr[r + 1] && !g_fail; b += seg_len, ++s) {
            const int64_t want = ptr[r + 1] - b < seg_len ? ptr[r + 1] - b : seg_len;
            CHECK(s < ns && sb[s] == b && sc[s] == want, "%s: row %lld segment %lld", name, (long long)r, (long long)s);
            CHECK(s < ns && sd[s] == (split ? (int32_t)~slot : (int32_t)r), "%s: row %lld segment %lld dest %d", name,
                  (long long)r, (long long)s, s < ns ? sd[s] : 0);
            slot += split;
        }
    }
    CHECK(i == nl && s == ns && slot == nsl, "%s: counts %lld %lld %lld, walked %lld %lld %lld", name, (long long)nl,
          (long long)ns, (long long)nsl, (long long)i, (long long)s, (long long)slot);
    CHECK(lr[nl] == -1 && lf[nl] == nsl, "%s: closing entry (%d, %d)", name, lr[nl], lf[nl]);
    free(sb);
    free(sc);
    free(sd);
    free(lr);
    free(lf);
}

/* every refusal, on sentinel-filled outputs that must stay as they are */
static void refusals(const char *name, int64_t n_rows, const int64_t *ptr)
{
    enum { N = 64 };
    if (n_rows < 2 || ptr[n_rows] > N)
        return;
    int64_t cnt[3], sb[N], cnt0[3], sb0[N];
    int32_t i32[4][N + 1], i320[4][N + 1];
    memset(cnt, 0x5a, sizeof cnt);
    memset(sb, 0x5a, sizeof sb);
    memset(i32, 0x5a, sizeof i32);
    memcpy(cnt0, cnt, sizeof cnt);
    memcpy(sb0, sb, sizeof sb);
    memcpy(i320, i32, sizeof i32);
    int64_t *bad = xmalloc((size_t)(n_rows + 1) * 8);
    memcpy(bad, ptr, (size_t)(n_rows + 1) * 8);
    bad[n_rows / 2] = bad[n_rows] + 1; /* decreasing after it */
#define CALL(nr, p, ll, sl, c0, c1, c2, a0, a1, a2, a3, a4) \
    CHECK(spmv_csr_multi_plan(nr, p, ll, sl, c0, c1, c2, a0, a1, a2, a3, a4) == SPMV_OTHER_ERROR, "%s: accepted " #nr \
          " " #p " " #ll " " #sl, name)
    CALL(-1, ptr, 0, 3, &cnt[0], &cnt[1], &cnt[2], sb, i32[0], i32[1], i32[2], i32[3]);
    CALL(n_rows, NULL, 0, 3, &cnt[0], &cnt[1], &cnt[2], sb, i32[0], i32[1], i32[2], i32[3]);
    CALL(n_rows, bad, 0, 3, &cnt[0], &cnt[1], &cnt[2], sb, i32[0], i32[1], i32[2], i32[3]);
    CALL(n_rows, ptr, -1, 3, &cnt[0], &cnt[1], &cnt[2], sb, i32[0], i32[1], i32[2], i32[3]);
    CALL(n_rows, ptr, 0, 0, &cnt[0], &cnt[1], &cnt[2], sb, i32[0], i32[1], i32[2], i32[3]);
    CALL(n_rows, ptr, 0, -5, &cnt[0], &cnt[1], &cnt[2], sb, i32[0], i32[1], i32[2], i32[3]);
    CALL(n_rows, ptr, 0, 3, NULL, &cnt[1], &cnt[2], sb, i32[0], i32[1], i32[2], i32[3]);
    CALL(n_rows, ptr, 0, 3, &cnt[0], &cnt[1], &cnt[2], sb, NULL, i32[1], i32[2], i32[3]);
#undef CALL
    CHECK(!memcmp(cnt, cnt0, sizeof cnt) && !memcmp(sb, sb0, sizeof sb) && !memcmp(i32, i320, sizeof i32),
          "%s: a refused call wrote an output", name);
    free(bad);
}

static void cases(const char *name, int64_t n_rows, const int64_t *ptr)
{
    static const int32_t opts[][2] = {{4, 8}, {0, 3}, {0, 1}};
    for (size_t i = 0; i < sizeof opts / sizeof opts[0]; ++i)
        verify(name, n_rows, ptr, opts[i][0], opts[i][1]);
    refusals(name, n_rows, ptr);
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
        int64_t *ptr = xmalloc((size_t)(info.n_rows + 1) * 8);
        int32_t *cc = xmalloc((size_t)info.nnz * 4);
        double *cv = xmalloc((size_t)info.nnz * 8);
        CHECK(spmv_csr_from_coo(info.n_rows, info.nnz, row, col, val, ptr, cc, cv) == SPMV_SUCCESS, "%s csr", argv[a]);
        cases(argv[a], info.n_rows, ptr);
        verify(argv[a], info.n_rows, ptr, 128, 1024);
        free(row);
        free(col);
        free(val);
        free(ptr);
        free(cc);
        free(cv);
        ++files;
    }
    /* rows of exactly long_len, long_len + 1, seg_len, seg_len + 1, 2 seg_len,
     * 2 seg_len + 1 entries for (4, 8), empty rows between them, a long last row */
    {
        static const int64_t lens[] = {4, 0, 5, 0, 0, 8, 9, 0, 16, 17, 0, 1, 40};
        enum { NR = sizeof lens / sizeof lens[0] };
        int64_t ptr[NR + 1];
        ptr[0] = 0;
        for (int r = 0; r < NR; ++r)
            ptr[r + 1] = ptr[r] + lens[r];
        cases("hand-made edges", NR, ptr);
        verify("hand-made edges", NR, ptr, 8, 8);
        verify("hand-made edges", NR, ptr, 100, 8);
        refusals("hand-made edges", 4, ptr);
    }
    { /* 3 rows, one of 20,001 entries */
        const int64_t ptr[4] = {0, 0, 20001, 20001};
        cases("one row", 3, ptr);
        verify("one row", 3, ptr, 128, 1024);
    }
    { /* rows without entries; no rows at all */
        const int64_t ptr[6] = {0, 0, 0, 0, 0, 0};
        cases("all empty", 5, ptr);
        cases("no rows", 0, ptr);
    }
    { /* the 100,000-row power-law R-MAT */
        const int64_t n = 100000, nnz = 1000000;
        int32_t *row = xmalloc((size_t)nnz * 4), *col = xmalloc((size_t)nnz * 4);
        double *val = xmalloc((size_t)nnz * 8);
        int64_t *ptr = xmalloc((size_t)(n + 1) * 8);
        int32_t *cc = xmalloc((size_t)nnz * 4);
        double *cv = xmalloc((size_t)nnz * 8);
        CHECK(spmv_gen_rmat(n, nnz, 17, 1, row, col, val) == SPMV_SUCCESS, "gen_rmat");
        CHECK(spmv_csr_from_coo(n, nnz, row, col, val, ptr, cc, cv) == SPMV_SUCCESS, "rmat csr");
        verify("rmat", n, ptr, 128, 1024);
        verify("rmat", n, ptr, 0, 3);
        free(row);
        free(col);
        free(val);
        free(ptr);
        free(cc);
        free(cv);
    }
    if (g_fail)
        return 1;
    printf("multi plan harness: %d files clean\n", files);
    return 0;
}
