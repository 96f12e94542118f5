"""Restarted GMRES (iterate.gmres) — the parts that need no GPU: the three host
statements (spmv_cpu_krylov_project, spmv_cpu_krylov_combine,
spmv_cpu_krylov_normalize), the solver loop on the numpy double
(tests/iterate_gmres_double.py) on one rank and on two gloo ranks, its end
cases and the refusals.  tests/test_gmres_gpu.py runs the device kernels and
the same solver through libspmv_hip.

Statement bounds.  With u = 2^-53:
    project    s_0 = w, s_(j+1) = fma(-h_j, V_j, s_j): negating h_j is exact and
               each of the c fmas rounds once, an error of at most u |s_(j+1)|,
               and every partial sum is at most S = |w| + sum_j |h_j V_j| to
               first order: |w_out - exact| <= c u S;
    combine    s_0 = 0, s_(j+1) = fma(V_j, y_j, s_j): the same with
               S = sum_j |V_j y_j|: c u S;
    normalize  r = fl(1 / fl(sqrt(s))) carries two roundings and the product
               one: 3 u |w| / sqrt(s).
The tests allow one more u times the same sums (c + 1, c + 1, 4) for the
second-order terms and the rounding of the longdouble reference itself.

Solves.  iterate_gmres_double has the matrices, the settings and scipy's
inner-iteration counts.  GMRES minimises the residual over the Krylov space, so
two correct implementations cross tol at the same step up to rounding; a cycle
(`restart` steps) is the allowed difference, a wrong recurrence is off by
factors.  The returned rel is the true residual, so rel <= tol is asserted as
it stands whenever the solver stopped before maxit.
"""
from __future__ import annotations

import os
import socket
import sys

import numpy as np
import pytest
import torch

import iterate as it
import spmv_amd as sa
from conftest import PKG, REPO
from iterate_bicgstab_double import scipy_csr, true_rel, upwind
from iterate_gmres_double import (BLOCK_SIZES, CASES, MAXIT, RESTARTS, TOL, case_rhs, coo_of, np_gmres_operator,
                                  rotations, scipy_inner_count)
from iterate_precond_double import HostBlockJacobi

U = 2.0 ** -53
L = np.longdouble
FILL = 12345.0
WIDTHS = (1, 8, 9, 32)
SIZES = (0, 1, 67, 1030)


# ------------------------------------------------------------ host statements
def _block(rng, n, c, ld, ints=False):
    """(n + 2, ld) buffer: data in [:n, :c], NaN in the padding columns and the
    two rows past n (they must not be read)."""
    buf = np.full((n + 2, ld), np.nan)
    buf[:n, :c] = rng.integers(-3, 4, (n, c)) if ints else rng.uniform(-1, 1, (n, c))
    return buf


def _column(rng, n, ld, ints=False):
    """(n + 2, ld) buffer whose column 0 is a vector with leading dimension ld;
    FILL everywhere else."""
    buf = np.full((n + 2, ld), FILL)
    buf[:n, 0] = rng.integers(-3, 4, n) if ints else rng.uniform(-1, 1, n)
    return buf


def _coefficients(rng, c, ints=False):
    h = rng.integers(-3, 4, c).astype(np.float64) if ints else rng.uniform(-2, 2, c)
    if c > 1:
        h[c // 2] = 0.0  # a zero does not skip a term
    return h


def _only_column_written(buf, before, n):
    after = buf.copy()
    after[:n, 0] = before[:n, 0]
    return np.array_equal(after, before)


@pytest.mark.parametrize("alias", [False, True])
def test_host_project_against_longdouble(alias):
    rng = np.random.default_rng(5 + alias)
    worst = 0.0
    for n in SIZES:
        for c in WIDTHS:
            for ldv in (c, c + 3):
                Vb, h = _block(rng, n, c, ldv), _coefficients(rng, c)
                wb = _column(rng, n, 2)
                ob = wb if alias else _column(rng, n, 3)
                w0, o0 = wb.copy(), ob.copy()
                sa.cpu_krylov_project(n, Vb[:, :c], h, wb[:, :1], ob[:, :1], c=c)
                V, w = Vb[:n, :c].astype(L), w0[:n, 0].astype(L)
                ref = w - V @ h.astype(L)
                bound = (c + 1) * U * (np.abs(w) + np.abs(V) @ np.abs(h).astype(L))
                err = np.abs(ob[:n, 0].astype(L) - ref)
                assert (err <= bound).all(), (n, c, ldv, float((err / bound).max()))
                if n:
                    worst = max(worst, float((err / bound).max()))
                assert _only_column_written(ob, o0, n)
                if not alias:
                    assert np.array_equal(wb, w0)
    print(f"project: max error / bound {worst:.3g}")


def test_host_combine_against_longdouble():
    rng = np.random.default_rng(7)
    worst = 0.0
    for n in SIZES:
        for c in WIDTHS:
            for ldv in (c, c + 1):
                Vb, y = _block(rng, n, c, ldv), _coefficients(rng, c)
                tb = _column(rng, n, 2)
                t0 = tb.copy()
                sa.cpu_krylov_combine(n, Vb[:, :c], y, tb[:, :1], c=c)
                V = Vb[:n, :c].astype(L)
                ref = V @ y.astype(L)
                bound = (c + 1) * U * (np.abs(V) @ np.abs(y).astype(L))
                err = np.abs(tb[:n, 0].astype(L) - ref)
                assert (err <= bound).all(), (n, c, ldv)
                if n and (bound > 0).all():
                    worst = max(worst, float((err / bound).max()))
                assert _only_column_written(tb, t0, n)
    print(f"combine: max error / bound {worst:.3g}")


@pytest.mark.parametrize("alias", [False, True])
def test_host_normalize_against_longdouble(alias):
    rng = np.random.default_rng(9)
    for n in SIZES:
        for s in (2.75, 1e-300, 0.0, -1.0):
            for with_copy in (False, True):
                wb = _column(rng, n, 2)
                vb = wb if alias else _column(rng, n, 3)
                w0, v0 = wb.copy(), vb.copy()
                copy = np.full(n + 2, FILL) if with_copy else None
                sa.cpu_krylov_normalize(n, np.array([s]), wb[:, :1], vb[:, :1], None if copy is None else copy[:n])
                got = vb[:n, 0]
                if s <= 0.0:  # the zero-denominator rule: exactly zero, never NaN
                    assert (got == 0.0).all()
                else:
                    w = w0[:n, 0].astype(L)
                    ref = w / np.sqrt(L(s))
                    assert (np.abs(got.astype(L) - ref) <= 4 * U * np.abs(ref)).all(), (n, s)
                assert _only_column_written(vb, v0, n)
                if not alias:
                    assert np.array_equal(wb, w0)
                if with_copy:
                    assert np.array_equal(copy[:n], got) and (copy[n:] == FILL).all()


def test_host_statements_exact_on_integers():
    """Entries in -3..3: every product and partial sum is an integer far below
    2^53, so any order is exact and the result is the int64 one."""
    rng = np.random.default_rng(13)
    for n in (1, 67, 513):
        for c in WIDTHS:
            Vb, h = _block(rng, n, c, c + 1, ints=True), _coefficients(rng, c, ints=True)
            wb, ob = _column(rng, n, 1, ints=True), _column(rng, n, 2)
            sa.cpu_krylov_project(n, Vb[:, :c], h, wb[:, :1], ob[:, :1], c=c)
            Vi, hi = Vb[:n, :c].astype(np.int64), h.astype(np.int64)
            assert np.array_equal(ob[:n, 0], (wb[:n, 0].astype(np.int64) - Vi @ hi).astype(np.float64))
            sa.cpu_krylov_combine(n, Vb[:, :c], h, ob[:, :1], c=c)
            assert np.array_equal(ob[:n, 0], (Vi @ hi).astype(np.float64))
    w = np.array([[3.0], [-2.0], [0.0]])
    v = np.empty_like(w)
    sa.cpu_krylov_normalize(3, np.array([4.0]), w, v)
    assert np.array_equal(v[:, 0], [1.5, -1.0, 0.0])


def test_host_statement_refusals_and_empty():
    V, col, h, s = np.ones((3, 2)), np.ones((3, 1)), np.ones(2), np.ones(1)
    lib = sa.host_lib()
    p = sa._ptr
    okp = (3, 2, p(V), 2, p(h), p(col), 1, p(col), 1)
    for pos, bad in ((0, -1), (1, 0), (1, 33), (2, None), (3, 1), (4, None), (5, None), (6, 0), (7, None), (8, 0)):
        args = list(okp)
        args[pos] = bad
        assert lib.spmv_cpu_krylov_project(*args) == sa.OTHER_ERROR, pos
    okc = (3, 2, p(V), 2, p(h), p(col), 1)
    for pos, bad in ((0, -1), (1, 0), (1, 33), (2, None), (3, 1), (4, None), (5, None), (6, 0)):
        args = list(okc)
        args[pos] = bad
        assert lib.spmv_cpu_krylov_combine(*args) == sa.OTHER_ERROR, pos
    okn = (3, p(s), p(col), 1, p(col), 1, None)
    for pos, bad in ((0, -1), (1, None), (2, None), (3, 0), (4, None), (5, 0)):
        args = list(okn)
        args[pos] = bad
        assert lib.spmv_cpu_krylov_normalize(*args) == sa.OTHER_ERROR, pos
    assert lib.spmv_cpu_krylov_project(0, 2, None, 2, p(h), None, 1, None, 1) == sa.SUCCESS
    assert lib.spmv_cpu_krylov_combine(0, 2, None, 2, p(h), None, 1) == sa.SUCCESS
    assert lib.spmv_cpu_krylov_normalize(0, p(s), None, 1, None, 1, None) == sa.SUCCESS
    # the wrappers: each refuses before the library is called
    out = np.full((3, 1), FILL)
    wide = np.ones((3, 33))
    for call in (lambda: sa.cpu_krylov_project(3, V.astype(np.float32), h, col, out),  # dtype of the basis
                 lambda: sa.cpu_krylov_project(3, V, h, col[:, 0], out),  # a 1-D vector
                 lambda: sa.cpu_krylov_project(3, V, h[:1], col, out),  # too few scalars
                 lambda: sa.cpu_krylov_project(4, V, h, col, out),  # too few rows
                 lambda: sa.cpu_krylov_project(3, V, h, col, out, c=3),  # more columns than the basis has
                 lambda: sa.cpu_krylov_project(3, V, h, col, out, c=0),
                 lambda: sa.cpu_krylov_project(3, wide, np.ones(33), col, out),  # a basis of 33 columns
                 lambda: sa.cpu_krylov_project(3, V, h.astype(np.float32), col, out),
                 lambda: sa.cpu_krylov_project(3, V[:, ::-1], h, col, out),  # an inner stride
                 lambda: sa.cpu_krylov_combine(3, V, h[:1], out),
                 lambda: sa.cpu_krylov_combine(3, V, h, out[:2]),
                 lambda: sa.cpu_krylov_combine(3, wide, np.ones(33), out),
                 lambda: sa.cpu_krylov_combine(3, [[1.0, 2.0]] * 3, h, out),  # not an array
                 lambda: sa.cpu_krylov_normalize(3, s, col, out[:2]),
                 lambda: sa.cpu_krylov_normalize(3, np.ones(0), col, out),
                 lambda: sa.cpu_krylov_normalize(3, s, col.astype(np.float32), out),
                 lambda: sa.cpu_krylov_normalize(3, s, col, out, np.ones(2)),  # a short copy
                 lambda: sa.cpu_krylov_normalize(3, s, col, out, np.ones((3, 1)))):  # a 2-D copy
        with pytest.raises(sa.SpmvError):
            call()
    assert (out == FILL).all()


# -------------------------------------------------------------------- solves
def _solve_case(case, restart, bs, rank=0, world=1, comm=None):
    m = upwind(*case)
    op = np_gmres_operator(m, rank, world, bs)
    b = torch.from_numpy(case_rhs(case)[op.lo:op.lo + op.rows].copy())
    x, its, rel = it.gmres(op, b, comm, tol=TOL, maxit=MAXIT, restart=restart)
    return its, rel, op.lo, x.numpy().copy()


def _check_solution(case, x, its, rel, what):
    A, b = scipy_csr(upwind(*case)), case_rhs(case)
    mine = float(true_rel(A, b[:, None], x[:, None])[0])
    print(f"{what}: its {its}, rel {rel:.3g}, fresh true_rel {mine:.3g}")
    assert its < MAXIT
    assert rel <= TOL and mine <= TOL
    assert np.isfinite(x).all()


@pytest.mark.parametrize("bs", BLOCK_SIZES)
@pytest.mark.parametrize("restart", RESTARTS)
@pytest.mark.parametrize("case", CASES)
def test_gmres_converges(case, restart, bs):
    its, rel, lo, x = _solve_case(case, restart, bs)
    assert lo == 0
    _check_solution(case, x, its, rel, f"{case} restart {restart} bs {bs}")
    if bs is None:
        ref = scipy_inner_count(case, restart)
        print(f"iterations {its}, scipy {ref}, difference {its - ref}")
        assert abs(its - ref) <= restart


def test_restart_beyond_the_dimension():
    """restart >= n: the Krylov space fills the whole space within n steps."""
    rng = np.random.default_rng(2)
    a = rng.uniform(-1, 1, (12, 12)) + 4.0 * np.eye(12)
    b = rng.uniform(-1, 1, 12)
    x, its, rel = it.gmres(np_gmres_operator(coo_of(a)), torch.from_numpy(b), tol=TOL, maxit=100, restart=31)
    print(f"12 rows, restart 31: its {its}, rel {rel:.3g}")
    assert its <= 12 and rel <= TOL
    assert np.linalg.norm(b - a @ x.numpy()) <= TOL * np.linalg.norm(b)


def test_rotations_where_bicgstab_stands_still():
    """A = kron(I, [[0, 1], [-1, 0]]): b . A b = 0 exactly, BiCGSTAB's first
    alpha is 0 / 0 and it never moves; A^2 = -I, so GMRES ends in two steps."""
    op = np_gmres_operator(rotations())
    b = torch.from_numpy(np.random.default_rng(1).uniform(-0.5, 0.5, 64))
    x, its, rel = it.gmres(op, b, tol=TOL, maxit=50, restart=20)
    _, _, rel_b = it.bicgstab(op, b, tol=TOL, maxit=50)
    print(f"rotations: gmres its {its} rel {rel:.3g}, bicgstab rel {rel_b:.3g}")
    assert its <= 2 and rel <= TOL
    assert rel_b > 0.5


def test_invariant_subspace_after_one_step():
    """b an eigenvector of a diagonal matrix: w = A v_0 = 4 v_0, both passes
    leave exactly 0, H[1, 0] = 0 ends the cycle after one step; the zero norm
    makes no NaN."""
    op = np_gmres_operator(coo_of(np.diag(np.arange(1.0, 9.0))))
    b = np.zeros(8)
    b[3] = 2.0
    x, its, rel = it.gmres(op, torch.from_numpy(b), tol=TOL, maxit=50, restart=5)
    assert its == 1 and rel == 0.0
    assert np.array_equal(x.numpy(), b / 4.0)


def test_zero_right_hand_side():
    op = np_gmres_operator(upwind(*CASES[2]))
    x, its, rel = it.gmres(op, torch.zeros(op.rows, dtype=torch.float64))
    assert its == 0 and rel == 0.0 and (x == 0.0).all()


def test_maxit_is_respected_and_rel_is_the_true_residual():
    case = CASES[0]
    A, b = scipy_csr(upwind(*case)), case_rhs(case)
    x, its, rel = it.gmres(np_gmres_operator(upwind(*case)), torch.from_numpy(b), tol=TOL, maxit=13, restart=5)
    assert its == 13 and TOL < rel < 1.0
    assert abs(rel - true_rel(A, b[:, None], x.numpy()[:, None])[0]) <= 1e-12


def test_gmres_on_a_split_operator():
    case = CASES[2]
    m = upwind(*case)
    b = torch.from_numpy(case_rhs(case))
    for bs in BLOCK_SIZES:
        x, its, rel = it.gmres(np_gmres_operator(m, bs=bs, split=True), b, tol=TOL, maxit=MAXIT, restart=20)
        x1, its1, _ = it.gmres(np_gmres_operator(m, bs=bs), b, tol=TOL, maxit=MAXIT, restart=20)
        assert its < MAXIT and rel <= TOL and abs(its - its1) <= 20
        assert np.linalg.norm(x.numpy() - x1.numpy()) <= 1e-6 * np.linalg.norm(x1.numpy())


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
        for bs in BLOCK_SIZES:
            q.put((rank, bs) + _solve_case(CASES[0], 20, bs, rank, world, it2.Comm(dist)))
    finally:
        dist.destroy_process_group()


def test_gmres_two_ranks():
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
    for bs, pair in ((None, res[:2]), (3, res[2:])):
        (_, _, its0, rel0, lo0, x0), (_, _, its1, rel1, lo1, x1) = pair
        assert its0 == its1 and rel0 == rel1  # every rank sees the all-reduced scalars
        assert lo0 == 0 and lo1 == x0.shape[0]
        x = np.concatenate([x0, x1])
        _check_solution(CASES[0], x, its0, rel0, f"two ranks, bs {bs}")
        _, _, _, x_one = _solve_case(CASES[0], 20, bs)
        # the blocks of a two-rank block Jacobi are cut per rank: another
        # preconditioner, the same solution
        assert np.linalg.norm(x - x_one) <= 1e-9 * np.linalg.norm(x_one)


# ------------------------------------------------------------------- refusals
def test_refusals():
    m = upwind(*CASES[2])
    n = m.n_rows

    class NoDeviceWork:  # every refusal comes before any kernel runs
        stream = None

        def __getattr__(self, name):
            raise AssertionError(f"kernels.{name} was reached")

    real = np_gmres_operator(m)
    op = it.DistOperator(real.layout, 0, n, NoDeviceWork(), "cpu")
    good = torch.ones(n, dtype=torch.float64)
    for restart in (0, 32, -1, 2.0, "5", None, True):
        with pytest.raises(sa.SpmvError, match="restart"):
            it.gmres(op, good, restart=restart)
    for bad in (torch.ones(n, 1, dtype=torch.float64),  # 2-D
                torch.ones(n, dtype=torch.float32),  # dtype
                torch.ones(n + 1, dtype=torch.float64),  # rows
                torch.ones(2 * n, dtype=torch.float64)[::2],  # not contiguous
                np.ones(n)):  # not a tensor
        with pytest.raises(sa.SpmvError):
            it.gmres(op, bad)
    loc = it.local_shard(m, real.layout, 0)
    cheb = it.Chebyshev(HostBlockJacobi(loc, 2), 3, 0.1, 2.0)
    with pytest.raises(sa.SpmvError, match="Chebyshev"):
        it.gmres(op, good, precond=cheb)
    quiet = it.DistOperator(real.layout, 0, n, NoDeviceWork(), "cpu", precond=cheb)
    with pytest.raises(sa.SpmvError, match="Chebyshev"):
        it.gmres(quiet, good)
