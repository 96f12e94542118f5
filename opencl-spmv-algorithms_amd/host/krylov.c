/* krylov.c — the CPU statements of GMRES's three basis kernels
 * (spmv_host.h): they fix the bits of every element that
 * spmv_krylov_project_dot, spmv_krylov_combine and spmv_krylov_normalize
 * (csrc/krylov.hip) write; the sums of the first are fixed by spmv_dot_multi.
 * The reference has no counterpart (it runs one SpMV and stops). */
#include <math.h>
#include <stddef.h>

#include "spmv_host.h"
#include "spmv_rc.h"

#define KRYLOV_MAX_COLS 32

int spmv_cpu_krylov_project(int64_t n, int32_t c, const double *V, int64_t ldv, const double *h, const double *w,
                            int64_t ldw, double *w_out, int64_t ldo)
{
    if (n < 0 || c < 1 || c > KRYLOV_MAX_COLS || ldv < c || ldw < 1 || ldo < 1 || !h ||
        (n > 0 && (!V || !w || !w_out)))
        return SPMV_OTHER_ERROR;
    for (int64_t i = 0; i < n; ++i) {
        double s = w[i * ldw]; /* before w_out[i] is written: w_out may be w */
        for (int32_t j = 0; j < c; ++j)
            s = fma(-h[j], V[i * ldv + j], s);
        w_out[i * ldo] = s;
    }
    return SPMV_SUCCESS;
}

int spmv_cpu_krylov_combine(int64_t n, int32_t c, const double *V, int64_t ldv, const double *y, double *t,
                            int64_t ldt)
{
    if (n < 0 || c < 1 || c > KRYLOV_MAX_COLS || ldv < c || ldt < 1 || !y || (n > 0 && (!V || !t)))
        return SPMV_OTHER_ERROR;
    for (int64_t i = 0; i < n; ++i) {
        double s = 0.0;
        for (int32_t j = 0; j < c; ++j)
            s = fma(V[i * ldv + j], y[j], s);
        t[i * ldt] = s;
    }
    return SPMV_SUCCESS;
}

int spmv_cpu_krylov_normalize(int64_t n, const double *s, const double *w, int64_t ldw, double *v, int64_t ldv,
                              double *copy)
{
    if (n < 0 || !s || ldw < 1 || ldv < 1 || (n > 0 && (!w || !v)))
        return SPMV_OTHER_ERROR;
    const double r = s[0] <= 0.0 ? 0.0 : 1.0 / sqrt(s[0]);
    for (int64_t i = 0; i < n; ++i) {
        const double x = w[i * ldw] * r; /* v may be w */
        v[i * ldv] = x;
        if (copy)
            copy[i] = x;
    }
    return SPMV_SUCCESS;
}
