"""Matrices and numpy references of the block-Jacobi tests: TEST
INFRASTRUCTURE ONLY (tests/test_precond.py, tests/test_precond_gpu.py).

block_congruence(g, b, seed): A = L_g (x) I_b, the 5-point Laplacian on a
g x g grid with b unknowns per node, then A' = W A W^T (symmetrised) with
W = blockdiag(W_q), W_q = U_q diag(10^u) V_q^T, u uniform in [0, 2], U_q and
V_q orthogonal (QR of normal samples).  A' is SPD with the badly scaled,
coupled b x b node blocks of an FE matrix with several unknowns per node.
Block Jacobi at bs = b is invariant under W (M'^-1 A' = W^-T (M^-1 A) W^T is
similar to the plain Laplacian's), point Jacobi and plain CG are not: at
g = 20, b = 3, tol 1e-10 they take 1,649 and 2,960 iterations against 77.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

import spmv_amd as sa
from iterate_double import laplacian_2d

_cache = {}


def block_congruence(g: int, b: int, seed: int = 0) -> sa.Coo:
    """Sorted by row, then column; made once per (g, b, seed), never changed."""
    key = (g, b, seed)
    if key not in _cache:
        lap = laplacian_2d(g)
        L = sp.csr_matrix((lap.val, (lap.row, lap.col)), shape=(lap.n_rows, lap.n_rows))
        rng = np.random.default_rng(seed)
        blocks = []
        for _ in range(lap.n_rows):
            U = np.linalg.qr(rng.standard_normal((b, b)))[0]
            V = np.linalg.qr(rng.standard_normal((b, b)))[0]
            blocks.append(U @ np.diag(10.0 ** rng.uniform(0.0, 2.0, b)) @ V.T)
        W = sp.block_diag(blocks, format="csr")
        A = W @ sp.kron(L, sp.identity(b), format="csr") @ W.T
        A = ((A + A.T) * 0.5).tocoo()
        o = np.lexsort((A.col, A.row))
        m = sa.Coo(A.shape[0], A.shape[0], A.row[o].astype(np.int32), A.col[o].astype(np.int32),
                   A.data[o].astype(np.float64), False, f"block congruence g={g} b={b} seed={seed}")
        for a in (m.row, m.col, m.val):
            a.setflags(write=False)
        _cache[key] = m
    return _cache[key]


def lower_half(m: sa.Coo) -> sa.Coo:
    keep = m.row >= m.col
    return sa.Coo(m.n_rows, m.n_cols, m.row[keep].copy(), m.col[keep].copy(), m.val[keep].copy(), True,
                  m.label + " (lower)")


def scipy_csr(m: sa.Coo):
    return sp.csr_matrix((m.val, (m.row, m.col)), shape=(m.n_rows, m.n_cols))


def rhs(n: int, k: int = 3) -> np.ndarray:
    """(n, k): all ones, uniform(-0.5, 0.5), e_0, then zero columns."""
    B = np.zeros((n, k))
    B[:, 0] = 1.0
    if k > 1:
        B[:, 1] = np.random.default_rng(7).random(n) - 0.5
    if k > 2:
        B[0, 2] = 1.0
    return B


def dense_blocks(m: sa.Coo, bs: int, row_lo: int = 0, row_hi: int | None = None, symmetric_half: bool = False):
    """The diagonal blocks D_q of rows [row_lo, row_hi) of m (columns in m's
    own numbering: block q covers rows AND columns row_lo + q*bs + [0, bs)),
    by a dense numpy extraction: (n_blocks, bs, bs), a short last block
    completed with the identity; duplicates add in storage order
    (np.add.at)."""
    row_hi = m.n_rows if row_hi is None else row_hi
    n = row_hi - row_lo
    nbk = (n + bs - 1) // bs
    D = np.zeros((nbk, bs, bs))
    r = m.row.astype(np.int64) - row_lo
    c = m.col.astype(np.int64) - row_lo
    ok = (r >= 0) & (r < n) & (c >= 0) & (c < n)
    ok &= np.where(ok, r // bs == c // bs, False)
    r, c, v = r[ok], c[ok], m.val[ok]
    np.add.at(D, (r // bs, r % bs, c % bs), v)
    if symmetric_half:
        off = r != c
        np.add.at(D, (r[off] // bs, c[off] % bs, r[off] % bs), v[off])
    for i in range(n, nbk * bs):
        D[i // bs, i % bs, i % bs] = 1.0
    return D


def block_jacobi_apply(m: sa.Coo, bs: int, bounds=None):
    """z = M^-1 r as a function, M the block-Jacobi preconditioner whose
    blocks are cut from each row range [bounds[i], bounds[i+1]) separately
    (one range: the whole matrix), inverted by np.linalg.inv."""
    bounds = [0, m.n_rows] if bounds is None else [int(b) for b in bounds]
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        D = dense_blocks(m, bs, lo, hi)
        inv = np.linalg.inv(D)
        parts.append(sp.block_diag(list(inv), format="csr")[:hi - lo, :hi - lo] if hi > lo else None)
    Minv = sp.block_diag([p for p in parts if p is not None], format="csr")
    return lambda r: Minv @ r


def numpy_pcg(A, b, apply_minv=None, tol: float = 1e-10, maxit: int = 20000):
    """Textbook (P)CG in numpy, x0 = 0, residual test ||r|| <= tol ||b|| after
    every iteration.  Returns (x, iterations)."""
    x = np.zeros_like(b)
    r = b.copy()
    z = apply_minv(r) if apply_minv else r
    p = z.copy()
    rz = r @ z
    stop = tol * np.linalg.norm(b)
    for it in range(1, maxit + 1):
        Ap = A @ p
        alpha = rz / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        if np.linalg.norm(r) <= stop:
            return x, it
        z = apply_minv(r) if apply_minv else r
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, maxit


def numpy_pcg_count(m: sa.Coo, B: np.ndarray, bs: int | None, bounds=None, tol: float = 1e-10) -> int:
    """The largest iteration count over the non-zero columns of B (bs = None:
    plain CG)."""
    A = scipy_csr(m)
    minv = block_jacobi_apply(m, bs, bounds) if bs else None
    return max(numpy_pcg(A, B[:, j].copy(), minv, tol)[1] for j in range(B.shape[1]) if B[:, j].any())
