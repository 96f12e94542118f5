"""Numpy stand-in for the BiCGSTAB methods of iterate.HipKernels, the upwind
convection-diffusion test matrix and the bound of the convergence tests: TEST
INFRASTRUCTURE ONLY (as tests/iterate_precond_double.py, which it extends, and
through it tests/iterate_multi_double.py's NumpyMultiKernels).

The two updates are the host statements (sa.cpu_bicgstab_update_multi,
sa.cpu_bicgstab_dir_multi); the preconditioner is the host block Jacobi of
iterate_precond_double.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp
import torch

import spmv_amd as sa
from iterate_precond_double import NumpyPrecondKernels, np_precond_operator

TOL = 1e-10
# A numpy prototype of the recurrence of iterate._bicgstab reached true
# residuals <= 8e-11 on the CASES below at tol = 1e-10, check_every = 10, in 30
# to 90 iterations.  The solver may end with 10 x the larger of tol and that
# figure: the factor covers another summation order and BiCGSTAB's uneven
# convergence between two stop tests.
REL_BOUND = 10 * max(TOL, 8e-11)
# (nx, ny, px, py)
CASES = ((48, 48, 1.5, 0.5), (48, 48, 8.0, 3.0), (31, 17, 20.0, 0.0))


def _a(t):
    return t.numpy()


def _colsums(n, A, B):
    """Column sums of A B over the first n rows, each correctly rounded
    (math.fsum): column j's bits depend on column j alone, as on the device."""
    prod = (A[:n] * B[:n]).numpy()
    return torch.tensor([math.fsum(prod[:, j].tolist()) for j in range(prod.shape[1])], dtype=torch.float64)


class NumpyBicgstabKernels(NumpyPrecondKernels):
    def dot_multi(self, n, A, B, out, ws):
        out[:] = _colsums(n, A, B)

    def dot2_multi(self, n, A, B, C, out, ws):
        k = A.shape[1]
        out[:k] = _colsums(n, A, B)
        out[k:2 * k] = _colsums(n, A, C)

    def bicgstab_update_dot(self, n, a_num, a_den, w_num, w_den, Ph, Sh, T, R0, X, R, out, ws):
        k = X.shape[1]
        same = Sh.data_ptr() == R.data_ptr()
        r = _a(R)
        sa.cpu_bicgstab_update_multi(n, _a(a_num), _a(a_den), _a(w_num), _a(w_den), _a(Ph), r if same else _a(Sh),
                                     _a(T), _a(X), r, k=k)
        out[:k] = _colsums(n, R0, R)
        out[k:2 * k] = _colsums(n, R, R)

    def bicgstab_dir(self, n, rho_new, rv, tt, ts, V, R, P):
        sa.cpu_bicgstab_dir_multi(n, _a(rho_new), _a(rv), _a(tt), _a(ts), _a(V), _a(R), _a(P), k=P.shape[1])

    def precond_apply(self, M, n, R, Z):
        assert n == M.n
        r = np.ascontiguousarray(R[:n].numpy())
        z = np.empty_like(r)
        sa.cpu_bjacobi_apply_multi(n, M.bs, M.inv, r, z)
        Z[:n] = torch.from_numpy(z)


def np_bicgstab_operator(m: sa.Coo, rank: int = 0, world: int = 1, bs: int | None = None, split: bool = False,
                         kernels=NumpyBicgstabKernels):
    """np_precond_operator with the BiCGSTAB-capable kernels."""
    import iterate as it

    op = np_precond_operator(m, rank, world, bs, split=split)
    loc = it.local_shard(m, op.layout, rank)
    if split:
        local, remote = it.split_local_remote(loc, op.layout, rank)
        op.kernels, op.remote = kernels(local), kernels(remote)
    else:
        op.kernels = kernels(loc)
    return op


def upwind(nx: int, ny: int, px: float, py: float) -> sa.Coo:
    """5-point diffusion plus first-order upwind convection on an nx x ny grid
    (x runs fastest): diagonal 4 + px + py, west -1 - px, south -1 - py, east
    and north -1.  Non-symmetric for px or py != 0, an M-matrix."""
    n = nx * ny
    idx = np.arange(n).reshape(ny, nx)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(n, 4.0 + px + py)]
    for me, nb, v in ((idx[:, 1:], idx[:, :-1], -1.0 - px), (idx[1:, :], idx[:-1, :], -1.0 - py),
                      (idx[:, :-1], idx[:, 1:], -1.0), (idx[:-1, :], idx[1:, :], -1.0)):
        rows.append(me.ravel())
        cols.append(nb.ravel())
        vals.append(np.full(me.size, v))
    r = np.concatenate(rows).astype(np.int32)
    c = np.concatenate(cols).astype(np.int32)
    v = np.concatenate(vals)
    o = np.lexsort((c, r))
    return sa.Coo(n, n, r[o], c[o], v[o], False, f"upwind {nx}x{ny} p=({px},{py})")


def scipy_csr(m: sa.Coo):
    return sp.csr_matrix((m.val, (m.row, m.col)), shape=(m.n_rows, m.n_cols))


def rhs(n: int, k: int, zero_col: int | None = None) -> np.ndarray:
    """(n, k): uniform(-0.5, 0.5) columns from a fixed seed per column (so
    column j does not depend on k); zero_col: that one 0.
    No constant column on purpose.  With r^ = b = 1 on the strongly convective
    cases the residual of plain textbook BiCGSTAB (numpy, no code of this
    project) first GROWS by 4e6 to 8e6 before it falls, and the recurrence then
    parts from the true residual by about 2^-53 times that peak, 2e-9 to 5e-9:
    the method's attainable accuracy there, above any bound near tol.  The
    random columns peak below 10 on all three cases."""
    B = np.empty((n, k))
    for j in range(k):
        B[:, j] = np.random.default_rng(40 + j).random(n) - 0.5
    if zero_col is not None:
        B[:, zero_col] = 0.0
    return B


def true_rel(A, B: np.ndarray, X: np.ndarray) -> np.ndarray:
    """||b_j - A x_j|| / ||b_j|| per column, 0 for a zero column."""
    num = np.linalg.norm(B - A @ X, axis=0)
    den = np.linalg.norm(B, axis=0)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)
