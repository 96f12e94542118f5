"""Numpy stand-in for the GMRES methods of iterate.HipKernels, the extra test
matrices and scipy's iteration counts: TEST INFRASTRUCTURE ONLY (as
tests/iterate_bicgstab_double.py, which it extends; the existing doubles stay
as they are).

The three basis kernels are the host statements (sa.cpu_krylov_project,
sa.cpu_krylov_combine, sa.cpu_krylov_normalize); the sums of the projection are
math.fsum column sums, correctly rounded, so that a count does not rest on
numpy's summation order.
"""
from __future__ import annotations

import inspect
import math

import numpy as np
import scipy.sparse.linalg as spl
import torch

import spmv_amd as sa
from iterate_bicgstab_double import CASES, NumpyBicgstabKernels, np_bicgstab_operator, rhs, scipy_csr, upwind

TOL = 1e-10
MAXIT = 600
RESTARTS = (5, 20)
BLOCK_SIZES = (None, 3)


class NumpyGmresKernels(NumpyBicgstabKernels):
    def krylov_project_dot(self, n, V, h, w, w_out, out, ws):
        c = V.shape[1]
        Vn = V.numpy()
        if h is not None:
            sa.cpu_krylov_project(n, Vn, np.ascontiguousarray(h.numpy()), w.numpy(), w_out.numpy(), c=c)
            w = w_out
        elif w_out is not None:
            w_out[:n] = w[:n]
        r = w.numpy()[:n, 0]
        for j in range(c):
            out[j] = math.fsum((Vn[:n, j] * r).tolist())
        out[c] = math.fsum((r * r).tolist())

    def krylov_project_ws(self, n):
        return torch.empty(8, dtype=torch.uint8)

    def krylov_combine(self, n, V, y, t):
        sa.cpu_krylov_combine(n, V.numpy(), np.ascontiguousarray(y, np.float64), t.numpy())

    def krylov_normalize(self, n, s, w, v, copy=None):
        sa.cpu_krylov_normalize(n, s.numpy(), w.numpy(), v.numpy(), None if copy is None else copy.numpy())


def np_gmres_operator(m: sa.Coo, rank: int = 0, world: int = 1, bs: int | None = None, split: bool = False):
    """iterate.build_operator on the numpy double (bs: its block Jacobi)."""
    return np_bicgstab_operator(m, rank, world, bs, split, kernels=NumpyGmresKernels)


def coo_of(a) -> sa.Coo:
    """The non-zeros of a small dense matrix, by rows."""
    a = np.asarray(a, dtype=np.float64)
    r, c = np.nonzero(a)
    return sa.Coo(a.shape[0], a.shape[1], r.astype(np.int32), c.astype(np.int32), a[r, c], False, "dense")


def rotations(blocks: int = 32) -> sa.Coo:
    """kron(I_blocks, [[0, 1], [-1, 0]]): skew-symmetric, so b . A b = 0 for
    every b and BiCGSTAB's first alpha is 0 / 0; A^2 = -I, so GMRES ends in two
    steps."""
    return coo_of(np.kron(np.eye(blocks), np.array([[0.0, 1.0], [-1.0, 0.0]])))


def case_rhs(case) -> np.ndarray:
    nx, ny = case[0], case[1]
    return rhs(nx * ny, 1)[:, 0].copy()


_scipy_counts = {}


def scipy_inner_count(case, restart: int) -> int:
    """Inner iterations of scipy.sparse.linalg.gmres (no preconditioner, x0 = 0,
    callback_type="pr_norm": one call per inner iteration) on upwind(*case) to
    TOL, computed once per (case, restart)."""
    key = (tuple(case), restart)
    if key not in _scipy_counts:
        A, b = scipy_csr(upwind(*case)), case_rhs(case)
        calls = []
        tol_kw = "rtol" if "rtol" in inspect.signature(spl.gmres).parameters else "tol"
        _, info = spl.gmres(A, b, restart=restart, maxiter=MAXIT, atol=0.0, callback=calls.append,
                            callback_type="pr_norm", **{tol_kw: TOL})
        assert info == 0
        _scipy_counts[key] = len(calls)
    return _scipy_counts[key]


_double_counts = {}


def double_count(case, restart: int, bs) -> int:
    """Arnoldi steps of iterate.gmres on the numpy double for upwind(*case),
    computed once per setting: what the device solver's count is compared
    with."""
    import iterate as it

    key = (tuple(case), restart, bs)
    if key not in _double_counts:
        op = np_gmres_operator(upwind(*case), bs=bs)
        _, its, _ = it.gmres(op, torch.from_numpy(case_rhs(case)), tol=TOL, maxit=MAXIT, restart=restart)
        _double_counts[key] = its
    return _double_counts[key]


__all__ = ["NumpyGmresKernels", "np_gmres_operator", "coo_of", "rotations", "case_rhs", "scipy_inner_count",
           "double_count", "CASES", "TOL", "MAXIT", "RESTARTS", "BLOCK_SIZES"]
