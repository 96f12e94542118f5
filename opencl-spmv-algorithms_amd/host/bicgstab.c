/* bicgstab.c — the CPU statements of BiCGSTAB's two fused vector updates
 * (spmv_host.h): they fix the bits of every element that
 * spmv_bicgstab_update_dot_multi and spmv_bicgstab_dir_multi (csrc/vec_multi.hip)
 * write.  The reference has no counterpart (it runs one SpMV and stops). */
#include <math.h>
#include <stddef.h>

#include "spmv_host.h"
#include "spmv_rc.h"

/* a / b, and 0 when b == 0: the rule of the block ratio kernels */
static double ratio(double a, double b)
{
    return b == 0.0 ? 0.0 : a / b;
}

int spmv_cpu_bicgstab_update_multi(int64_t n, int32_t k, const double *a_num, const double *a_den,
                                   const double *w_num, const double *w_den, const double *Ph, int64_t ldph,
                                   const double *Sh, int64_t ldsh, const double *T, int64_t ldt, double *X,
                                   int64_t ldx, double *R, int64_t ldr)
{
    if (n < 0 || k < 1 || !a_num || !a_den || !w_num || !w_den || ldph < k || ldsh < k || ldt < k || ldx < k ||
        ldr < k || (n > 0 && (!Ph || !Sh || !T || !X || !R)) || (Sh && Sh == R && ldsh != ldr))
        return SPMV_OTHER_ERROR;
    for (int64_t i = 0; i < n; ++i)
        for (int32_t j = 0; j < k; ++j) {
            const double alpha = ratio(a_num[j], a_den[j]), omega = ratio(w_num[j], w_den[j]);
            const double sh = Sh[i * ldsh + j]; /* before R[i][j] is written: Sh may be R */
            X[i * ldx + j] = fma(omega, sh, fma(alpha, Ph[i * ldph + j], X[i * ldx + j]));
            R[i * ldr + j] = fma(-omega, T[i * ldt + j], R[i * ldr + j]);
        }
    return SPMV_SUCCESS;
}

int spmv_cpu_bicgstab_dir_multi(int64_t n, int32_t k, const double *rho_new, const double *rv, const double *tt,
                                const double *ts, const double *V, int64_t ldv, const double *R, int64_t ldr,
                                double *P, int64_t ldp)
{
    if (n < 0 || k < 1 || !rho_new || !rv || !tt || !ts || ldv < k || ldr < k || ldp < k ||
        (n > 0 && (!V || !R || !P)))
        return SPMV_OTHER_ERROR;
    for (int64_t i = 0; i < n; ++i)
        for (int32_t j = 0; j < k; ++j) {
            const double beta = ratio(rho_new[j], rv[j]) * ratio(tt[j], ts[j]), omega = ratio(ts[j], tt[j]);
            P[i * ldp + j] = fma(beta, fma(-omega, V[i * ldv + j], P[i * ldp + j]), R[i * ldr + j]);
        }
    return SPMV_SUCCESS;
}
