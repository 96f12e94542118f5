"""LOBPCG (iterate.lobpcg) — the parts that need no GPU: the host statement of
the block combine (spmv_cpu_block_combine_multi), the eigensolver loop on the
numpy double (tests/iterate_lobpcg_double.py) on one rank and on two gloo
ranks, the refusals, and the text of the C-ABI.  tests/test_block_gpu.py and
tests/test_lobpcg_gpu.py run the device kernels and the same solver through
libspmv_hip.

Combine bound.  Y[i][c] is a chain of R fmas from 0: R products, each rounded
into the running sum once, so by the textbook bound of a recursive sum
|Y - exact| <= R u sum_r |S[i][r] C[r][c]| to first order (u = 2^-53); the test
allows (R + 2) u times the sum, as tests/exact.py does, for the second-order
terms and the rounding of the longdouble reference.

Iteration counts.  scipy.sparse.linalg.lobpcg needs 139 (k = 4) and 138 (k = 8)
iterations on the 20 x 23 Laplacian at tol = 1e-8; this implementation's numpy
double needs 118 to 180 over k in {1, 3, 4, 8}, smallest and largest.  maxit
stays at 500.  On block_congruence(16, 3) it needs 267 with bjacobi = 3 and has
not converged after 3,000 without.
"""
from __future__ import annotations

import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch

import iterate as it
import precond_cases as pc
import spmv_amd as sa
from conftest import PKG, REPO
from exact import wide_range
from iterate_double import NumpyKernels
from iterate_lobpcg_double import (GRID, TOL, check_eigenpairs, laplacian_rect, np_lobpcg_operator, spectrum)
from iterate_precond_double import HostBlockJacobi

U = 2.0 ** -53
FILL = 12345.0


# ------------------------------------------------------------- host statement
def _operands(rng, n, widths, pad, integer):
    out = []
    for w in widths:
        a = np.full((n + 2, w + pad), FILL)
        a[:, :w] = rng.integers(-99, 100, (n + 2, w)).astype(np.float64) if integer else wide_range(rng, (n + 2, w))
        out.append(a)
    return out


@pytest.mark.parametrize("widths", [(1,), (3,), (8,), (1, 8), (8, 3), (3, 1, 8), (8, 8, 8)])
@pytest.mark.parametrize("kc", [1, 5, 8])
def test_host_combine_exact_on_integers(widths, kc):
    """Small integers: every product and partial sum is exact, the result must
    EQUAL the int64 one; padding columns and rows at or past n keep their fill."""
    rng = np.random.default_rng(sum(widths) * 10 + kc)
    n = 37
    for pad in (0, 1):
        ops = _operands(rng, n, widths, pad, True)
        C = rng.integers(-99, 100, (sum(widths), kc)).astype(np.float64)
        Y = np.full((n + 2, kc + pad), FILL)
        sa.cpu_block_combine_multi(n, C, [a[:, :w] for a, w in zip(ops, widths)], Y[:, :kc])
        S = np.hstack([a[:n, :w] for a, w in zip(ops, widths)]).astype(np.int64)
        assert np.array_equal(Y[:n, :kc], (S @ C.astype(np.int64)).astype(np.float64))
        assert (Y[n:] == FILL).all() and (Y[:, kc:] == FILL).all()


@pytest.mark.parametrize("widths", [(8,), (3, 5), (8, 8, 8)])
def test_host_combine_within_the_fp64_bound(widths):
    rng = np.random.default_rng(5 + len(widths))
    n, kc = 201, 7
    ops = _operands(rng, n, widths, 1, False)
    C = wide_range(rng, (sum(widths), kc))
    Y = np.full((n, kc), FILL)
    sa.cpu_block_combine_multi(n, C, [a[:, :w] for a, w in zip(ops, widths)], Y)
    S = np.hstack([a[:n, :w] for a, w in zip(ops, widths)])
    ref = S.astype(np.longdouble) @ C.astype(np.longdouble)
    bound = (sum(widths) + 2) * U * (np.abs(S) @ np.abs(C))
    assert (np.abs(Y.astype(np.longdouble) - ref).astype(np.float64) <= bound).all()


def test_host_combine_special_values_and_refusals():
    """A zero in C does not skip a term: Inf and NaN in S[i][r] reach every
    column of row i and no other row; -0.0 + 0.0 chains give +0.0."""
    n = 4
    A = np.ones((n, 2))
    A[1, 0] = np.inf
    A[2, 1] = np.nan
    A[3] = -0.0
    C = np.array([[0.0, 1.0], [1.0, 0.0]])
    Y = np.full((n, 2), FILL)
    sa.cpu_block_combine_multi(n, C, [A], Y)
    assert np.array_equal(Y[0], [1.0, 1.0])
    assert np.isnan(Y[1, 0]) and Y[1, 1] == np.inf  # inf * 0 = NaN in column 0
    assert np.isnan(Y[2]).all()
    assert np.array_equal(Y[3], [0.0, 0.0]) and not np.signbit(Y[3]).any()  # fma(-0, 1, +0) = +0
    lib = sa.host_lib()
    a = np.ones((3, 2))
    y = np.full((3, 2), FILL)
    c = np.ones((6, 2))
    p = sa._ptr

    def call(n=3, kc=2, C=c, ka0=2, A0=a, ld0=2, ka1=0, A1=None, ld1=0, ka2=0, A2=None, ld2=0, Y=y, ldy=2):
        return lib.spmv_cpu_block_combine_multi(n, kc, p(C), ka0, p(A0), ld0, ka1, p(A1), ld1, ka2, p(A2), ld2, p(Y), ldy)

    assert call() == sa.SUCCESS
    y[:] = FILL
    for kw in (dict(n=-1), dict(kc=0), dict(kc=9), dict(C=None), dict(ka0=-1), dict(ka0=9), dict(ka0=0),
               dict(A0=None), dict(ld0=1), dict(ka1=2, A1=None, ld1=2), dict(ka1=2, A1=a, ld1=1),
               dict(ka2=9, A2=a, ld2=9), dict(Y=None), dict(ldy=1)):
        assert call(**kw) == sa.OTHER_ERROR, kw
    assert (y == FILL).all()
    assert call(n=0, A0=None, Y=None) == sa.SUCCESS  # nothing is needed, nothing is touched
    for bad in (dict(blocks=[]), dict(blocks=[a] * 4), dict(C=np.ones((3, 2))), dict(C=np.ones((2, 9))),
                dict(blocks=[np.ones((3, 9))], C=np.ones((9, 2))), dict(blocks=[np.ones((3, 2), np.float32)]),
                dict(blocks=[np.ones((2, 2))]), dict(Y=np.ones((3, 1)))):
        kw = dict(dict(C=np.ones((2, 2)), blocks=[a], Y=y), **bad)
        with pytest.raises(sa.SpmvError):
            sa.cpu_block_combine_multi(3, kw["C"], kw["blocks"], kw["Y"])


# ----------------------------------------------------------------- the C-ABI
def test_header_symbols_and_signatures():
    ext = (REPO / "include" / "spmv_ext.h").read_text()
    host = (REPO / "include" / "spmv_host.h").read_text()
    flat = re.sub(r"\s+", " ", ext)
    assert "size_t spmv_gram_multi_ws_bytes(int64_t n, int32_t ka, int32_t kb);" in flat
    assert ("int spmv_gram_multi(int64_t n, int32_t ka, const double *A, int64_t lda, int32_t kb, const double *B, "
            "int64_t ldb, double *out, void *ws, size_t ws_bytes, int device, void *stream);") in flat
    assert ("int spmv_block_combine_multi(int64_t n, int32_t kc, const double *C, int32_t ka0, const double *A0, "
            "int64_t lda0, int32_t ka1, const double *A1, int64_t lda1, int32_t ka2, const double *A2, int64_t lda2, "
            "double *Y, int64_t ldy, int device, void *stream);") in flat
    assert "spmv_cpu_block_combine_multi(" in host
    # the contract's own words: the launch bound, the host matrix, the bit rules
    for words in ("At most FOUR stage-1 launches", "C is a HOST array", "bit for bit what spmv_dot_multi(n, 1, A + a",
                  "spmv_cpu_block_combine_multi"):
        assert words in flat, words
    i64, i32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    assert sa.HIP_SYMBOLS["spmv_gram_multi_ws_bytes"] == (ctypes.c_size_t, [i64, i32, i32])
    assert sa.HIP_SYMBOLS["spmv_gram_multi"] == (ctypes.c_int, [i64, i32, vp, i64, i32, vp, i64, vp, vp, ctypes.c_size_t,
                                                                ctypes.c_int, vp])
    assert sa.HIP_SYMBOLS["spmv_block_combine_multi"] == (ctypes.c_int, [i64, i32, vp, i32, vp, i64, i32, vp, i64, i32, vp,
                                                                         i64, vp, i64, ctypes.c_int, vp])
    assert sa.HOST_SYMBOLS["spmv_cpu_block_combine_multi"] == (ctypes.c_int, [i64, i32, vp, i32, vp, i64, i32, vp, i64,
                                                                              i32, vp, i64, vp, i64])
    lib = sa.hip_lib()
    for name in ("spmv_gram_multi_ws_bytes", "spmv_gram_multi", "spmv_block_combine_multi"):
        assert hasattr(lib, name)
    # the workspace is spmv_dot_multi's per pair: G(n) = min(ceil(n / 512), 1024) partials of 8 bytes
    for n, g in ((0, 1), (512, 1), (513, 2), (524288, 1024), (10 ** 7, 1024)):
        assert lib.spmv_gram_multi_ws_bytes(n, 3, 5) == g * 15 * 8 == lib.spmv_dot_multi_ws_bytes(n, 15)


# ------------------------------------------------------------------ the solver
@pytest.fixture(scope="module")
def lap():
    return laplacian_rect(*GRID)


def _solve(m, k, largest, rank=0, world=1, comm=None, bs=None, **kw):
    op = np_lobpcg_operator(m, rank, world, bs)
    lam, X, its, res = it.lobpcg(op, k=k, largest=largest, tol=TOL, comm=comm, **kw)
    return lam, X.numpy().copy(), its, res, op.lo


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("k", [1, 3, 4, 8])
def test_lobpcg_laplacian(lap, k, largest):
    lam, X, its, res, _ = _solve(lap, k, largest)
    check_eigenpairs(lap, lam, X, its, res, k, largest, what=f"double k={k} largest={largest}")
    # the cap is a condition: the numpy double must stay well below it
    assert its <= 250


def test_lobpcg_is_reproducible_and_takes_x0(lap):
    a = _solve(lap, 4, False)
    b = _solve(lap, 4, False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    X0 = torch.from_numpy(np.random.default_rng(0).standard_normal((lap.n_rows, 4)))
    c = _solve(lap, None, False, X0=X0)  # the default start is seed 0 by global row
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
    d = _solve(lap, 4, False, seed=1)
    assert not np.array_equal(a[1], d[1])
    check_eigenpairs(lap, d[0], d[1], d[2], d[3], 4, False, what="seed 1")


def test_lobpcg_block_jacobi_on_the_congruence_matrix():
    m = pc.block_congruence(16, 3)
    lam, X, its, res, _ = _solve(m, 4, False, bs=3)
    check_eigenpairs(m, lam, X, its, res, 4, False, what="congruence bjacobi=3")
    _, _, its_plain, res_plain, _ = _solve(m, 4, False, bs=3, precond=False)
    print(f"congruence: {its} iterations with block Jacobi, {its_plain} without (cap 500)")
    assert its < its_plain == 500 and not (res_plain <= TOL * np.abs(lam)).all()


def test_lobpcg_maxit_and_atol(lap):
    lam, X, its, res, _ = _solve(lap, 2, False, maxit=7)
    assert its == 7 and np.isfinite(res).all() and (res > TOL * np.abs(lam)).any()
    A, w, norm1 = spectrum(lap)
    assert np.allclose(res, np.linalg.norm(A @ X - X * lam, axis=0), rtol=0, atol=1e-12 * norm1)
    lam2, _, its2, res2, _ = _solve(lap, 2, False, atol=1e-3)
    assert its2 < 100 and (res2 <= TOL * np.abs(lam2) + 1e-3).all()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path[:0] = [str(PKG), str(REPO), str(REPO / "tests")]
    import torch.distributed as dist

    import iterate as it2

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank,) + _solve(laplacian_rect(*GRID), 4, False, rank, world, it2.Comm(dist)))
    finally:
        dist.destroy_process_group()


def test_lobpcg_two_ranks(lap):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out = sorted((q.get(timeout=240) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, lam0, x0, its0, res0, lo0), (_, lam1, x1, its1, res1, lo1) = out
    # every rank sees the all-reduced small matrices: the same host step
    assert its0 == its1 and np.array_equal(lam0, lam1) and np.array_equal(res0, res1)
    assert lo0 == 0 and lo1 == x0.shape[0]
    check_eigenpairs(lap, lam0, np.concatenate([x0, x1]), its0, res0, 4, False, what="two ranks")
    lam, _, _, res, _ = _solve(lap, 4, False)
    _, _, norm1 = spectrum(lap)
    # both lie within their residual of the same eigenvalue
    assert (np.abs(lam0 - lam) <= np.maximum(res0, 64 * U * norm1) + np.maximum(res, 64 * U * norm1)).all()


def test_refusals(lap):
    n = lap.n_rows
    op = np_lobpcg_operator(lap)
    for k in (0, 9, -1, 2.0, True):
        with pytest.raises(sa.SpmvError):
            it.lobpcg(op, k=k)
    small = np_lobpcg_operator(laplacian_rect(2, 4))
    with pytest.raises(sa.SpmvError):  # 3k > n
        it.lobpcg(small, k=3)
    for bad in (torch.ones(n, dtype=torch.float64),  # 1-D
                torch.ones(n, 2, dtype=torch.float32),  # dtype
                torch.ones(n + 1, 2, dtype=torch.float64),  # rows
                torch.ones(n, 9, dtype=torch.float64),  # k = 9
                np.ones((n, 2))):  # not a tensor
        with pytest.raises(sa.SpmvError):
            it.lobpcg(op, X0=bad)
    with pytest.raises(sa.SpmvError):  # X0's width against k
        it.lobpcg(op, k=3, X0=torch.ones(n, 2, dtype=torch.float64))
    with pytest.raises(sa.SpmvError):  # a split operator
        it.lobpcg(np_lobpcg_operator(lap, split=True), k=2)
    plain = np_lobpcg_operator(lap)
    plain.kernels = NumpyKernels(it.local_shard(lap, plain.layout, 0))
    with pytest.raises(sa.SpmvError):  # kernels without a multi-vector run
        it.lobpcg(plain, k=2)
    wide = np_lobpcg_operator(lap)
    wide.kernels.A = wide.kernels.A[:, :-1]
    with pytest.raises(sa.SpmvError):  # not square
        it.lobpcg(wide, k=2)
    X0 = torch.ones(n, 2, dtype=torch.float64)  # two equal columns
    with pytest.raises(sa.SpmvError, match="rank-deficient"):
        it.lobpcg(op, X0=X0)

    class NoDeviceWork:  # every refusal above and the Chebyshev one come before any kernel runs
        multi_supported = True
        stream = None
        dm = None
        A = None

        def __getattr__(self, name):
            raise AssertionError(f"kernels.{name} was reached")

    loc = it.local_shard(lap, op.layout, 0)
    quiet = it.DistOperator(op.layout, 0, n, NoDeviceWork(), "cpu")
    for kw in (dict(k=0), dict(k=9), dict(X0=torch.ones(n, 2, dtype=torch.float32)),
               dict(k=2, precond=it.Chebyshev(HostBlockJacobi(loc, 2), 3, 0.1, 2.0))):
        with pytest.raises(sa.SpmvError):
            it.lobpcg(quiet, **kw)
    quiet.n = 5
    with pytest.raises(sa.SpmvError):
        it.lobpcg(quiet, k=2)
