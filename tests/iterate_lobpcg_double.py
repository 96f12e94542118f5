"""Numpy stand-in for the LOBPCG methods of iterate.HipKernels, the test
matrices and the shared assertions of the eigensolver tests: TEST
INFRASTRUCTURE ONLY (as tests/iterate_bicgstab_double.py, which it extends, and
through it tests/iterate_multi_double.py's NumpyMultiKernels; the existing
doubles stay as they are).

The combine is the host statement (sa.cpu_block_combine_multi); the Gram
matrix is numpy's A^T B.
"""
from __future__ import annotations

import numpy as np
import torch

import iterate as it
import spmv_amd as sa
from iterate_bicgstab_double import NumpyBicgstabKernels, np_bicgstab_operator

TOL = 1e-8
U = 2.0 ** -53
# the 20 x 23-node 5-point Laplacian: n = 460, no repeated eigenvalue among the
# extreme ones (a square grid has pairs)
GRID = (20, 23)


class NumpyLobpcgKernels(NumpyBicgstabKernels):
    def gram(self, n, A, B, out, ws):
        ka, kb = A.shape[1], B.shape[1]
        out[:ka * kb] = torch.from_numpy((A[:n].numpy().T @ B[:n].numpy()).reshape(-1))

    def gram_ws(self, n, ka, kb):
        return torch.empty(8, dtype=torch.uint8)

    def block_combine(self, n, C, blocks, Y):
        sa.cpu_block_combine_multi(n, C, [t.numpy() for t in blocks], Y.numpy())


def np_lobpcg_operator(m: sa.Coo, rank: int = 0, world: int = 1, bs: int | None = None, split: bool = False):
    """iterate.build_operator on the numpy double (bs: its block Jacobi)."""
    return np_bicgstab_operator(m, rank, world, bs, split, kernels=NumpyLobpcgKernels)


def laplacian_rect(nx: int, ny: int) -> sa.Coo:
    """5-point Laplacian on an nx x ny grid (x runs fastest), sorted by row,
    then column."""
    n = nx * ny
    idx = np.arange(n).reshape(ny, nx)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(n, 4.0)]
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        rows += [a.ravel(), b.ravel()]
        cols += [b.ravel(), a.ravel()]
        vals += [np.full(a.size, -1.0), np.full(a.size, -1.0)]
    r = np.concatenate(rows).astype(np.int32)
    c = np.concatenate(cols).astype(np.int32)
    v = np.concatenate(vals)
    o = np.lexsort((c, r))
    return sa.Coo(n, n, r[o], c[o], v[o], False, f"laplacian {nx}x{ny}")


def dense(m: sa.Coo) -> np.ndarray:
    A = np.zeros((m.n_rows, m.n_cols))
    np.add.at(A, (m.row, m.col), m.val)
    return A


_spectra = {}


def spectrum(m: sa.Coo):
    """(dense A, numpy.linalg.eigvalsh(A) ascending, ||A||_1), computed once
    per matrix label and never changed."""
    if m.label not in _spectra:
        A = dense(m)
        w = np.linalg.eigvalsh(A)
        for a in (A, w):
            a.setflags(write=False)
        _spectra[m.label] = (A, w, float(np.abs(A).sum(axis=0).max()))
    return _spectra[m.label]


def check_eigenpairs(m: sa.Coo, lam, X, its, res, k: int, largest: bool, tol: float = TOL, maxit: int = 500,
                     what: str = ""):
    """The assertions every converged lobpcg run must meet.  X: the whole
    (n, k) block as a numpy array.  Prints the figures before it asserts."""
    A, w, norm1 = spectrum(m)
    want = w[::-1][:k] if largest else w[:k]
    lam, res = np.asarray(lam), np.asarray(res)
    err = np.abs(lam - want)
    bound = np.maximum(res, 64 * U * norm1)
    res_np = np.linalg.norm(A @ X - X * lam, axis=0)
    orth = float(np.abs(X.T @ X - np.eye(k)).max())
    print(f"{what}: its={its} max|lam-w|/bound={float((err / bound).max()):.3g} "
          f"max res/(tol|lam|)={float((res / (tol * np.abs(lam))).max()):.3g} "
          f"|res-res_np|={float(np.abs(res - res_np).max()):.3g} orth={orth:.3g}")
    assert lam.shape == (k,) and res.shape == (k,) and X.shape == (m.n_rows, k)
    assert its < maxit, (what, its)
    assert (np.diff(lam) <= 0).all() if largest else (np.diff(lam) >= 0).all(), (what, lam)
    # an eigenvalue of a symmetric matrix lies within the residual norm of every
    # Ritz value; matching the j-th to the j-th checks that none was skipped
    assert (err <= bound).all(), (what, lam, want, res)
    assert (np.abs(res - res_np) <= 1e-12 * norm1).all(), (what, res, res_np)
    assert orth <= 1e-12, (what, orth)
    assert (res <= tol * np.abs(lam)).all(), (what, res, lam)


def gathered_block(parts):
    """The whole (n, k) block from the ranks' (lo, X) pairs."""
    return np.concatenate([x for _, x in sorted(parts, key=lambda t: t[0])])


__all__ = ["NumpyLobpcgKernels", "np_lobpcg_operator", "laplacian_rect", "dense", "spectrum", "check_eigenpairs",
           "gathered_block", "TOL", "GRID", "it"]
