"""LOBPCG (iterate.lobpcg) on the MI355X through libspmv_hip: the same solver
and the same assertions as tests/test_lobpcg.py runs on the numpy double
(tests/iterate_lobpcg_double.py has the matrices and check_eigenpairs with its
bounds and their reasons).

Iteration counts.  maxit = 500 is a condition, not a measurement: scipy's
LOBPCG needs 139 (k = 4) and 138 (k = 8) iterations on the 20 x 23 Laplacian at
tol = 1e-8, the numpy double of this implementation 118 to 180.  On
block_congruence(16, 3) the double needs 267 iterations with bjacobi = 3 and
has not converged after 3,000 without.
"""
from __future__ import annotations

import numpy as np
import pytest

import iterate as it
import spmv_amd as sa
from iterate_lobpcg_double import GRID, TOL, check_eigenpairs, laplacian_rect
from precond_cases import block_congruence, lower_half

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lap():
    return laplacian_rect(*GRID)


_ops = {}


def _operator(m, dev, kind, **kw):
    """One operator per (matrix, kind, keywords) for the module."""
    key = (m.label, kind, tuple(sorted(kw.items())))
    if key not in _ops:
        if kind in ("fused", "expand"):
            _ops[key] = it.build_operator(lower_half(m), 0, 1, "csr", dev, align=64, symmetric=kind, **kw)
        else:
            _ops[key] = it.build_operator(m, 0, 1, kind, dev, align=64, **kw)
    return _ops[key]


def _run(op, k, largest, **kw):
    lam, X, its, res = it.lobpcg(op, k=k, largest=largest, tol=TOL, **kw)
    return lam, X.cpu().numpy(), its, res


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("fmt", ["csr", "ell", "sell"])
def test_lobpcg_laplacian(lap, dev, fmt, k, largest):
    lam, X, its, res = _run(_operator(lap, dev, fmt), k, largest)
    check_eigenpairs(lap, lam, X, its, res, k, largest, what=f"{fmt} k={k} largest={largest}")


@pytest.mark.parametrize("k", [1, 3])
def test_lobpcg_narrow_blocks(lap, dev, k):
    for largest in (False, True):
        lam, X, its, res = _run(_operator(lap, dev, "csr"), k, largest)
        check_eigenpairs(lap, lam, X, its, res, k, largest, what=f"csr k={k} largest={largest}")


@pytest.mark.parametrize("kind", ["expand", "fused"])
def test_lobpcg_on_the_stored_half(lap, dev, kind):
    op = _operator(lap, dev, kind)
    lam, X, its, res = _run(op, 4, False)
    check_eigenpairs(lap, lam, X, its, res, 4, False, what=f"symmetric={kind}")
    if kind == "expand":  # reproducible: fixed trees, fma chains, a deterministic host step
        lam2, X2, its2, res2 = _run(op, 4, False)
        assert its2 == its and np.array_equal(lam, lam2) and np.array_equal(X, X2) and np.array_equal(res, res2)


def test_lobpcg_is_reproducible(lap, dev):
    op = _operator(lap, dev, "csr")
    a = _run(op, 8, False)
    b = _run(op, 8, False)
    assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])


def test_lobpcg_block_jacobi_on_the_congruence_matrix(dev):
    m = block_congruence(16, 3)
    op = _operator(m, dev, "csr", bjacobi=3)
    lam, X, its, res = _run(op, 4, False)
    check_eigenpairs(m, lam, X, its, res, 4, False, what="congruence bjacobi=3")
    lam_p, _, its_plain, res_plain = _run(op, 4, False, precond=False)
    print(f"congruence: {its} iterations with block Jacobi, {its_plain} without (cap 500)")
    assert its < its_plain


def test_lobpcg_default_start_is_the_seeded_x0(lap, dev):
    """The default start is default_rng(seed) by global row: passing it as X0
    gives the same bits."""
    import torch

    op = _operator(lap, dev, "csr")
    a = _run(op, 4, False)
    X0 = torch.from_numpy(np.random.default_rng(0).standard_normal((lap.n_rows, 4))).to(dev)
    b = _run(op, None, False, X0=X0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_refusals(lap, dev):
    import torch

    n = lap.n_rows
    op = _operator(lap, dev, "csr")
    for k in (0, 9, -1):
        with pytest.raises(sa.SpmvError):
            it.lobpcg(op, k=k)
    with pytest.raises(sa.SpmvError):  # 3k > n
        it.lobpcg(_operator(laplacian_rect(2, 4), dev, "csr"), k=3)
    for bad in (torch.ones(n, dtype=torch.float64, device=dev), torch.ones(n, 2, dtype=torch.float32, device=dev),
                torch.ones(n + 1, 2, dtype=torch.float64, device=dev), torch.ones(n, 9, dtype=torch.float64, device=dev),
                torch.ones(n, 2, dtype=torch.float64), np.ones((n, 2))):
        with pytest.raises(sa.SpmvError):
            it.lobpcg(op, X0=bad)
    with pytest.raises(sa.SpmvError, match="rank-deficient"):
        it.lobpcg(op, X0=torch.ones(n, 2, dtype=torch.float64, device=dev))
    for fmt in ("coo", "cmrs"):  # formats without a multi-vector run
        with pytest.raises(sa.SpmvError, match="multi-vector"):
            it.lobpcg(_operator(lap, dev, fmt), k=2)
    with pytest.raises(sa.SpmvError):  # a split operator
        it.lobpcg(it.build_operator(lap, 0, 1, "csr", dev, align=64, split=True), k=2)
    with pytest.raises(sa.SpmvError, match="Chebyshev"):
        it.lobpcg(_operator(lap, dev, "csr", chebyshev=2, cheb_bounds=(0.1, 2.0)), k=2)
    # a shard that is not this layout's: 460 rows, but 459 columns
    wide = it.build_operator(lap, 0, 1, "csr", dev, align=64)
    keep = lap.col < n - 1
    wide.kernels = it.HipKernels(sa.to_device(sa.Coo(n, n - 1, lap.row[keep], lap.col[keep], lap.val[keep]), "csr", dev))
    with pytest.raises(sa.SpmvError, match="not square"):
        it.lobpcg(wide, k=2)
