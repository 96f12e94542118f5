/* block.c — the CPU statement of the block combine Y = [A0 A1 A2] C
 * (spmv_host.h): it fixes the bits of every element that
 * spmv_block_combine_multi (csrc/block.hip) writes.  The reference has no
 * counterpart (it runs one SpMV and stops). */
#include <math.h>
#include <stddef.h>

#include "spmv_host.h"
#include "spmv_rc.h"

int spmv_cpu_block_combine_multi(int64_t n, int32_t kc, const double *C, int32_t ka0, const double *A0, int64_t lda0,
                                 int32_t ka1, const double *A1, int64_t lda1, int32_t ka2, const double *A2,
                                 int64_t lda2, double *Y, int64_t ldy)
{
    const int32_t ka[3] = {ka0, ka1, ka2};
    const double *const p[3] = {A0, A1, A2};
    const int64_t ld[3] = {lda0, lda1, lda2};
    int32_t total = 0;
    if (n < 0 || kc < 1 || kc > 8 || !C || ldy < kc || (n > 0 && !Y))
        return SPMV_OTHER_ERROR;
    for (int q = 0; q < 3; ++q) {
        if (ka[q] < 0 || ka[q] > 8 || (ka[q] > 0 && (ld[q] < ka[q] || (n > 0 && !p[q]))))
            return SPMV_OTHER_ERROR;
        total += ka[q];
    }
    if (total < 1)
        return SPMV_OTHER_ERROR;
    for (int64_t i = 0; i < n; ++i) {
        double s[8];
        for (int32_t c = 0; c < kc; ++c)
            s[c] = 0.0;
        int32_t r0 = 0;
        for (int q = 0; q < 3; ++q) {
            for (int32_t r = 0; r < ka[q]; ++r) {
                const double a = p[q][i * ld[q] + r];
                for (int32_t c = 0; c < kc; ++c)
                    s[c] = fma(a, C[(r0 + r) * kc + c], s[c]);
            }
            r0 += ka[q];
        }
        for (int32_t c = 0; c < kc; ++c) /* after the whole row is read */
            Y[i * ldy + c] = s[c];
    }
    return SPMV_SUCCESS;
}
