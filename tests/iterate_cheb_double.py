"""Numpy stand-in for the Chebyshev step methods of iterate.HipKernels, and
numpy references of the recurrence: TEST INFRASTRUCTURE ONLY (as
tests/iterate_precond_double.py, which it extends).

The step itself is the host statement (sa.cpu_bjacobi_cheb_step_multi) on the
double's HostBlockJacobi; the references below use dense / scipy numpy only.
"""
from __future__ import annotations

import numpy as np
import torch

import iterate as it
import spmv_amd as sa
from iterate_precond_double import NumpyPrecondKernels, np_precond_operator
from precond_cases import block_jacobi_apply, numpy_pcg, scipy_csr


def _np(t):
    """A writable 2-D numpy view of a CPU tensor block (None stays None)."""
    return None if t is None else t.numpy()


class NumpyChebKernels(NumpyPrecondKernels):
    def cheb_step(self, M, n, a, b, R, AZ, D, Zin, Zout):
        assert n == M.n
        sa.cpu_bjacobi_cheb_step_multi(n, M.bs, M.inv, a, b, _np(R), _np(AZ), _np(D), _np(Zin), _np(Zout))

    def cheb_step_dot(self, M, n, a, b, R, AZ, D, Zin, Zout, out, ws):
        self.cheb_step(M, n, a, b, R, AZ, D, Zin, Zout)
        k = R.shape[1]
        r, z = R[:n].numpy(), Zout[:n].numpy()
        out[:k] = torch.from_numpy((r * z).sum(axis=0))
        out[k:2 * k] = torch.from_numpy((r * r).sum(axis=0))


def np_cheb_operator(m: sa.Coo, rank: int, world: int, bs: int, degree: int | None, bounds=None):
    """np_precond_operator with the Chebyshev-capable kernels; degree given:
    its preconditioner wrapped into iterate.Chebyshev with `bounds`."""
    op = np_precond_operator(m, rank, world, bs)
    op.kernels = NumpyChebKernels(it.local_shard(m, op.layout, rank))
    if degree is not None:
        op.precond = it.Chebyshev(op.precond, degree, *bounds)
    return op


# ------------------------------------------------------- numpy references
def cheb_apply(A, minv, degree: int, lmin: float, lmax: float):
    """r -> z: the recurrence of iterate.Chebyshev in plain numpy (its own
    coefficients, not iterate.chebyshev_coefficients)."""
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma = theta / delta

    def apply(r):
        d = minv(r) / theta
        z = d.copy()
        rho = 1 / sigma
        for _ in range(1, degree):
            rho_new = 1 / (2 * sigma - rho)
            d = rho_new * rho * d + (2 * rho_new / delta) * minv(r - A @ z)
            z = z + d
            rho = rho_new
        return z

    return apply


def lambda_max(m: sa.Coo, bs: int, bounds=None) -> float:
    """The largest eigenvalue of M^-1 A from dense numpy (blocks cut per row
    range of `bounds`, as the ranks cut them)."""
    import scipy.linalg as sl

    A = scipy_csr(m).toarray()
    Minv = block_jacobi_apply(m, bs, bounds)(np.eye(m.n_rows))
    # A and M are symmetric positive definite: the symmetric-definite pencil
    # A v = lambda M v has M^-1 A's eigenvalues
    M = np.linalg.inv(Minv)
    n = m.n_rows
    return float(sl.eigh((A + A.T) / 2, (M + M.T) / 2, eigvals_only=True, subset_by_index=[n - 1, n - 1])[0])


def numpy_cheb_pcg_count(m: sa.Coo, B: np.ndarray, bs: int, degree: int, lmin: float, lmax: float, bounds=None,
                         tol: float = 1e-10) -> int:
    """The largest iteration count of the textbook PCG over B's non-zero
    columns with the numpy recurrence as the preconditioner."""
    A = scipy_csr(m)
    apply = cheb_apply(A, block_jacobi_apply(m, bs, bounds), degree, lmin, lmax)
    return max(numpy_pcg(A, B[:, j].copy(), apply, tol)[1] for j in range(B.shape[1]) if B[:, j].any())
