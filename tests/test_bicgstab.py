"""BiCGSTAB (iterate.bicgstab, iterate.bicgstab_multi) — the parts that need no
GPU: the two host statements (spmv_cpu_bicgstab_update_multi,
spmv_cpu_bicgstab_dir_multi), the solver loop on the numpy double
(tests/iterate_bicgstab_double.py) on one rank and on two gloo ranks, the two
breakdown cases and the refusals.  tests/test_bicgstab_gpu.py runs the device
kernels and the same solvers through libspmv_hip.

Statement bounds.  With u = 2^-53 and alpha, omega, beta the exact ratios:
    x' = fma(fl(omega), sh, fma(fl(alpha), ph, x))   each of the three terms
         carries at most three roundings (its ratio, the inner fma, the outer):
         |x' - exact| <= 3u (|omega sh| + |alpha ph| + |x|) to first order;
    r' = fma(-fl(omega), t, r)                       two: 2u (|omega t| + |r|);
    p' = fma(fl(beta), fma(-fl(omega), v, p), r)     beta is two divisions and
         a product (three roundings), omega one, the two fmas one each: at most
         six on a term: 6u (|beta| (|omega v| + |p|) + |r|).
The tests allow one more u times the same sums (4u, 3u, 7u) for the
second-order terms and the rounding of the longdouble reference itself.

Solves.  iterate_bicgstab_double has the matrices (upwind), the cases and the
bound REL_BOUND with its reasons.  The solution is also compared with
scipy's spsolve: ||x - x_ref|| <= ||A^-1||_2 (||b - A x|| + ||b - A x_ref||) with
||A^-1||_2 <= sqrt(||A^-1||_1 ||A^-1||_inf), and for an M-matrix (A^-1 >= 0)
those two norms are max(A^-T 1) and max(A^-1 1), two more sparse solves.
"""
from __future__ import annotations

import os
import socket
import sys

import numpy as np
import pytest
import scipy.sparse.linalg as spl
import torch

import iterate as it
import spmv_amd as sa
from conftest import PKG, REPO
from iterate_bicgstab_double import (CASES, REL_BOUND, TOL, np_bicgstab_operator, rhs, scipy_csr, true_rel,
                                     upwind)
from iterate_double import NumpyKernels
from iterate_precond_double import HostBlockJacobi

U = 2.0 ** -53
L = np.longdouble
FILL = 12345.0
K = 5
ZERO_COL = 2
MAXIT = 400


# ------------------------------------------------------------ host statements
def _ratio_l(a, b):
    out = np.zeros(len(a), L)
    nz = b != 0.0
    out[nz] = a[nz].astype(L) / b[nz].astype(L)
    return out


def _guarded(rng, n, k, ld, fill=None):
    """(n + 2, ld) buffer, random or `fill` everywhere: two rows past n and
    ld - k padding columns."""
    return rng.uniform(-1, 1, (n + 2, ld)) if fill is None else np.full((n + 2, ld), fill)


def _scalars(rng, k, zero_den):
    """Four k-vectors (num, den, num, den); zero_den: column 0 gets a zero
    first denominator, the last column a zero second one (both for k = 1)."""
    s = [rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k) for _ in range(4)]
    if zero_den:
        s[1][0] = 0.0
        s[3][-1] = 0.0
    return s


@pytest.mark.parametrize("zero_den", [False, True])
@pytest.mark.parametrize("alias", [False, True])
def test_host_update_against_longdouble(alias, zero_den):
    rng = np.random.default_rng(11 + 2 * alias + zero_den)
    worst = 0.0
    for n in (1, 67, 4097):
        for k, ld in ((1, 1), (3, 3), (5, 8)):
            an, ad, wn, wd = _scalars(rng, k, zero_den)
            Phb, Tb = _guarded(rng, n, k, ld), _guarded(rng, n, k, ld + 1)
            Xb, Rb = _guarded(rng, n, k, ld + 2), _guarded(rng, n, k, ld + 3)
            Shb = Rb if alias else _guarded(rng, n, k, ld)
            for buf in (Phb, Tb) + (() if alias else (Shb,)):  # padding and rows past n must not be read
                buf[:, k:] = np.nan
                buf[n:] = np.nan
            X0, R0, Sh0 = Xb.copy(), Rb.copy(), Shb.copy()
            sa.cpu_bicgstab_update_multi(n, an, ad, wn, wd, Phb[:, :k], Shb[:, :k], Tb[:, :k], Xb[:, :k], Rb[:, :k],
                                         k=k)
            al, om = _ratio_l(an, ad), _ratio_l(wn, wd)
            ph, sh, t, x, r = (b[:n, :k].astype(L) for b in (Phb, Sh0, Tb, X0, R0))
            x_ref, r_ref = x + al * ph + om * sh, r - om * t
            x_bound = 4 * U * (np.abs(om * sh) + np.abs(al * ph) + np.abs(x))
            r_bound = 3 * U * (np.abs(om * t) + np.abs(r))
            for name, got, ref, bound in (("X", Xb, x_ref, x_bound), ("R", Rb, r_ref, r_bound)):
                err = np.abs(got[:n, :k].astype(L) - ref)
                assert (err <= bound).all(), (name, n, k, ld, float((err / bound).max()))
                worst = max(worst, float((err / bound).max()))
            for got, before in ((Xb, X0), (Rb, R0)):
                assert np.array_equal(got[n:], before[n:]) and np.array_equal(got[:, k:], before[:, k:])
            if not alias:
                assert np.array_equal(Shb, Sh0, equal_nan=True)
            if zero_den:  # alpha_0 = 0: x_0 moves by omega sh alone; omega_last = 0: r_last stands still
                assert np.array_equal(Rb[:n, k - 1], R0[:n, k - 1])
                if k == 1:
                    assert np.array_equal(Xb[:n, 0], X0[:n, 0])
    print(f"update: max error / bound {worst:.3g}")


def test_host_update_alias_equals_copy():
    """Sh == R gives the bits of the call with a copy of R as Sh."""
    rng = np.random.default_rng(3)
    n, k = 67, 3
    an, ad, wn, wd = _scalars(rng, k, False)
    Ph, T, X, R = (rng.uniform(-1, 1, (n, k)) for _ in range(4))
    X1, R1, X2, R2 = X.copy(), R.copy(), X.copy(), R.copy()
    sa.cpu_bicgstab_update_multi(n, an, ad, wn, wd, Ph, R1, T, X1, R1)
    sa.cpu_bicgstab_update_multi(n, an, ad, wn, wd, Ph, R.copy(), T, X2, R2)
    assert np.array_equal(X1, X2) and np.array_equal(R1, R2)


@pytest.mark.parametrize("zero", [None, "rv", "ts", "tt"])
def test_host_dir_against_longdouble(zero):
    rng = np.random.default_rng(21)
    worst = 0.0
    for n in (1, 67, 4097):
        for k, ld in ((1, 1), (3, 3), (5, 8)):
            rho, rv, tt, ts = _scalars(rng, k, False)
            if zero is not None:
                dict(rv=rv, ts=ts, tt=tt)[zero][0] = 0.0
            Vb, Rb, Pb = _guarded(rng, n, k, ld), _guarded(rng, n, k, ld + 1), _guarded(rng, n, k, ld + 2)
            for buf in (Vb, Rb):
                buf[:, k:] = np.nan
                buf[n:] = np.nan
            P0 = Pb.copy()
            sa.cpu_bicgstab_dir_multi(n, rho, rv, tt, ts, Vb[:, :k], Rb[:, :k], Pb[:, :k], k=k)
            beta, om = _ratio_l(rho, rv) * _ratio_l(tt, ts), _ratio_l(ts, tt)
            v, r, p = (b[:n, :k].astype(L) for b in (Vb, Rb, P0))
            ref = r + beta * (p - om * v)
            bound = 7 * U * (np.abs(beta) * (np.abs(om * v) + np.abs(p)) + np.abs(r))
            err = np.abs(Pb[:n, :k].astype(L) - ref)
            assert (err <= bound).all(), (n, k, ld, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
            assert np.array_equal(Pb[n:], P0[n:]) and np.array_equal(Pb[:, k:], P0[:, k:])
            if zero in ("rv", "ts"):  # beta_0 = 0: p_0 = r_0 exactly
                assert np.array_equal(Pb[:n, 0], Rb[:n, 0])
            assert np.isfinite(Pb[:n, :k]).all()
    print(f"dir: max error / bound {worst:.3g}")


def test_host_statement_refusals_and_empty():
    one = np.ones(2)
    blk = np.ones((3, 2))
    h = sa.host_lib()
    p = sa._ptr
    ok = (3, 2, p(one), p(one), p(one), p(one), p(blk), 2, p(blk), 2, p(blk), 2, p(blk), 2, p(blk), 2)
    for pos, bad in ((0, -1), (1, 0), (2, None), (5, None), (6, None), (7, 1), (8, None), (9, 1), (11, 1), (12, None),
                     (13, 1), (15, 1)):
        args = list(ok)
        args[pos] = bad
        assert h.spmv_cpu_bicgstab_update_multi(*args) == sa.OTHER_ERROR, pos
    args = list(ok)
    args[8], args[9], args[14], args[15] = p(blk), 2, p(blk), 3  # Sh == R with two leading dimensions
    assert h.spmv_cpu_bicgstab_update_multi(*args) == sa.OTHER_ERROR
    assert h.spmv_cpu_bicgstab_update_multi(0, 2, p(one), p(one), p(one), p(one), None, 2, None, 2, None, 2, None, 2,
                                            None, 2) == sa.SUCCESS
    okd = (3, 2, p(one), p(one), p(one), p(one), p(blk), 2, p(blk), 2, p(blk), 2)
    for pos, bad in ((0, -1), (1, 0), (2, None), (3, None), (4, None), (5, None), (6, None), (7, 1), (8, None), (9, 1),
                     (10, None), (11, 1)):
        args = list(okd)
        args[pos] = bad
        assert h.spmv_cpu_bicgstab_dir_multi(*args) == sa.OTHER_ERROR, pos
    assert h.spmv_cpu_bicgstab_dir_multi(0, 2, p(one), p(one), p(one), p(one), None, 2, None, 2, None, 2) == sa.SUCCESS
    with pytest.raises(sa.SpmvError):  # a float32 block
        sa.cpu_bicgstab_dir_multi(3, one, one, one, one, blk.astype(np.float32), blk, blk.copy())
    with pytest.raises(sa.SpmvError):  # too few scalars
        sa.cpu_bicgstab_dir_multi(3, np.ones(1), one, one, one, blk, blk, blk.copy())


# -------------------------------------------------------------------- solves
def _inverse_norm_bound(A):
    """sqrt(||A^-1||_1 ||A^-1||_inf) >= ||A^-1||_2 for an M-matrix (docstring)."""
    ones = np.ones(A.shape[0])
    rows, cols = spl.spsolve(A.tocsc(), ones), spl.spsolve(A.T.tocsc(), ones)
    assert (rows > 0).all() and (cols > 0).all()
    return float(np.sqrt(rows.max() * cols.max()))


def _solve_case(case, bs, rank=0, world=1, comm=None, k=K, zero_col=ZERO_COL):
    m = upwind(*case)
    op = np_bicgstab_operator(m, rank, world, bs)
    B = torch.from_numpy(rhs(m.n_rows, k, zero_col)[op.lo:op.lo + op.rows].copy())
    X, its, rel = it.bicgstab_multi(op, B, comm, tol=TOL, maxit=MAXIT, check_every=10)
    return its, rel, op.lo, X.numpy().copy()


def _check_solution(case, X, its, rel):
    m = upwind(*case)
    A = scipy_csr(m)
    B = rhs(m.n_rows, K, ZERO_COL)
    print(f"{m.label}: its {its}, rel {rel}")
    assert its < MAXIT and rel.shape == (K,)
    assert (rel <= REL_BOUND).all()
    mine = true_rel(A, B, X)
    assert (mine <= REL_BOUND).all()
    assert np.allclose(rel, mine, rtol=1e-3, atol=1e-14)  # the solver's own figure is the true residual
    assert (X[:, ZERO_COL] == 0.0).all() and rel[ZERO_COL] == 0.0
    X_ref = spl.spsolve(A.tocsc(), B)
    ainv = _inverse_norm_bound(A)
    for j in range(K):
        res = np.linalg.norm(B[:, j] - A @ X[:, j]) + np.linalg.norm(B[:, j] - A @ X_ref[:, j])
        assert np.linalg.norm(X[:, j] - X_ref[:, j]) <= ainv * res * (1 + 1e-6) + 1e-300


@pytest.mark.parametrize("bs", [None, 2])
@pytest.mark.parametrize("case", CASES)
def test_bicgstab_multi_converges(case, bs):
    its, rel, lo, X = _solve_case(case, bs)
    assert lo == 0
    _check_solution(case, X, its, rel)


@pytest.mark.parametrize("bs", [None, 2])
def test_column_independence_and_single(bs):
    """Column j of the block solve has the bits of the solve of column j
    alone; bicgstab (the single-vector form) solves the same system."""
    case = CASES[2]
    m = upwind(*case)
    B = rhs(m.n_rows, 3, 1)
    op = np_bicgstab_operator(m, bs=bs)
    X, its, rel = it.bicgstab_multi(op, torch.from_numpy(B.copy()), tol=TOL, maxit=MAXIT, check_every=10)
    for j in range(3):
        Xj, itsj, relj = it.bicgstab_multi(op, torch.from_numpy(B[:, j:j + 1].copy()), tol=TOL, maxit=its,
                                           check_every=its)
        # one column stops when IT has converged: run it for the block's count
        assert itsj in (its, 0)
        assert np.array_equal(Xj.numpy()[:, 0], X.numpy()[:, j]) and relj[0] == rel[j]
    x, its1, rel1 = it.bicgstab(op, torch.from_numpy(B[:, 0].copy()), tol=TOL, maxit=MAXIT, check_every=10)
    assert its1 < MAXIT and rel1 <= REL_BOUND and x.shape == (m.n_rows,)
    assert true_rel(scipy_csr(m), B[:, :1], x.numpy()[:, None])[0] <= REL_BOUND


def test_zero_block_returns_at_once():
    m = upwind(*CASES[2])
    op = np_bicgstab_operator(m)
    X, its, rel = it.bicgstab_multi(op, torch.zeros(m.n_rows, 2, dtype=torch.float64))
    assert its == 0 and (rel == 0.0).all() and (X == 0.0).all()
    x, its, rel = it.bicgstab(op, torch.zeros(m.n_rows, dtype=torch.float64))
    assert its == 0 and rel == 0.0 and (x == 0.0).all()


def test_bicgstab_on_a_split_operator():
    case = CASES[2]
    m = upwind(*case)
    b = torch.from_numpy(rhs(m.n_rows, 1)[:, 0].copy())
    x, its, rel = it.bicgstab(np_bicgstab_operator(m, split=True), b, tol=TOL, maxit=MAXIT)
    x1, _, _ = it.bicgstab(np_bicgstab_operator(m), b, tol=TOL, maxit=MAXIT)
    assert its < MAXIT and rel <= REL_BOUND
    assert np.linalg.norm(x.numpy() - x1.numpy()) <= 1e-6 * np.linalg.norm(x1.numpy())


def _tiny(rows):
    a = np.array(rows, dtype=np.float64)
    r, c = np.nonzero(a)
    return sa.Coo(a.shape[0], a.shape[1], r.astype(np.int32), c.astype(np.int32), a[r, c], False, "tiny")


def test_breakdown_rv_zero_stands_still():
    """A = [[0, 1], [-1, 0]], b = e_0: v = A b is orthogonal to r^ = b, so
    alpha = 0, then omega = 0 and beta = 0: x stays 0, nothing becomes NaN."""
    op = np_bicgstab_operator(_tiny([[0, 1], [-1, 0]]))
    x, its, rel = it.bicgstab(op, torch.tensor([1.0, 0.0], dtype=torch.float64), maxit=25, check_every=10)
    assert its == 25 and rel == 1.0
    assert (x == 0.0).all()


def test_breakdown_ts_zero_stagnates():
    """A = [[1, 2], [0, 1]], b = (1, 1): the first half step reaches
    x = (0.5, 0.5) with t.s = 0, so omega = 0, rho' = 0 and the column stays
    there: rel = 0.5 exactly.  Next to it b = (0, 1) stays finite."""
    op = np_bicgstab_operator(_tiny([[1, 2], [0, 1]]))
    B = torch.tensor([[1.0, 0.0], [1.0, 1.0]], dtype=torch.float64)
    X, its, rel = it.bicgstab_multi(op, B, maxit=25, check_every=10)
    assert its == 25
    assert np.array_equal(X.numpy()[:, 0], [0.5, 0.5]) and rel[0] == 0.5
    assert torch.isfinite(X).all() and np.isfinite(rel).all()


# ------------------------------------------------------------------ two ranks
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
        for bs in (None, 2):
            q.put((rank, bs) + _solve_case(CASES[0], bs, rank, world, it2.Comm(dist)))
    finally:
        dist.destroy_process_group()


def test_bicgstab_multi_two_ranks():
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(4)), key=lambda t: (t[1] is not None, t[0]))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for bs, pair in ((None, res[:2]), (2, res[2:])):
        (_, _, its0, rel0, lo0, x0), (_, _, its1, rel1, lo1, x1) = pair
        assert its0 == its1 and np.array_equal(rel0, rel1)  # every rank sees the all-reduced scalars
        assert lo0 == 0 and lo1 == x0.shape[0]
        _check_solution(CASES[0], np.concatenate([x0, x1]), its0, rel0)


# ------------------------------------------------------------------- refusals
def test_refusals():
    m = upwind(*CASES[2])
    n = m.n_rows
    op = np_bicgstab_operator(m)
    good = torch.ones(n, 2, dtype=torch.float64)
    for bad in (torch.ones(n, dtype=torch.float64),  # 1-D
                torch.ones(n, 2, dtype=torch.float32),  # dtype
                torch.ones(n + 1, 2, dtype=torch.float64),  # rows
                torch.ones(n, 0, dtype=torch.float64),  # k = 0
                torch.ones(2, n, dtype=torch.float64).t(),  # not contiguous
                np.ones((n, 2))):  # not a tensor
        with pytest.raises(sa.SpmvError):
            it.bicgstab_multi(op, bad)
    with pytest.raises(sa.SpmvError):  # a split operator
        it.bicgstab_multi(np_bicgstab_operator(m, split=True), good)
    with pytest.raises(sa.SpmvError):  # kernels without a multi-vector run
        it.bicgstab_multi(np_bicgstab_operator(m, kernels=NumpyKernels), good)

    class NoDeviceWork:  # a Chebyshev preconditioner is refused before any kernel runs
        multi_supported = True
        stream = None

        def __getattr__(self, name):
            raise AssertionError(f"kernels.{name} was reached")

    loc = it.local_shard(m, op.layout, 0)
    cheb = it.Chebyshev(HostBlockJacobi(loc, 2), 3, 0.1, 2.0)
    quiet = it.DistOperator(op.layout, 0, n, NoDeviceWork(), "cpu", precond=cheb)
    with pytest.raises(sa.SpmvError):
        it.bicgstab_multi(quiet, good)
    with pytest.raises(sa.SpmvError):
        it.bicgstab(quiet, good[:, 0].contiguous())
    with pytest.raises(sa.SpmvError):
        it.bicgstab(op, good[:, 0].contiguous(), precond=cheb)
