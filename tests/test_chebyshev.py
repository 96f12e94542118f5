"""The Chebyshev polynomial preconditioner over block Jacobi — the parts that
need no GPU: the host statement of one step
(spmv_cpu_bjacobi_cheb_step_multi), iterate.Chebyshev and estimate_lmax on the
numpy double (one rank and two gloo ranks) and the refusals.
tests/test_chebyshev_gpu.py runs the device kernels and the same solvers
through libspmv_hip.

Step bound.  With u = 2^-53, one element of the statement is computed as
    t_c = fl(R_c - AZ_c)                     one rounding per difference,
    s   = the fma chain over nb <= bs terms  a product and nb - 1 fmas: the
                                             classic (nb)-term bound, gamma_nb,
                                             on top of the differences: nb + 1,
    p   = fl(b s)                            one more,
    d   = fma(a, D, p)                       one more,
    z   = fl(Zin + d)                        one more,
so |z - z_exact| <= gamma_(bs + 4) (|b| sum_c |inv_c| (|R_c| + |AZ_c|) + |a D|
+ |Zin|) to first order, each input magnitude carrying at most bs + 4
roundings; the test allows (bs + 5) u times that sum, which covers the
second-order terms (bs <= 16: (bs + 4)^2 u^2 is far below u) and the rounding
of the longdouble reference itself.  D alone obeys the same bound without its
last term.

Solves.  N_ref is the iteration count of the textbook numpy PCG
(precond_cases.numpy_pcg) preconditioned with a plain numpy evaluation of the
recurrence, blocks cut per rank range; the solver checks rr every check_every
iterations and rounds differently, hence at most N_ref + check_every +
N_ref // 10 iterations (tests/test_precond.py's rule).  On
block_congruence(20, 3), bs = 3, degree 4, bounds (1.1 lambda / 30,
1.1 lambda): N_ref = 25 against 78 for block Jacobi alone.
"""
from __future__ import annotations

import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch

import iterate as it
import spmv_amd as sa
from conftest import PKG, REPO
from iterate_cheb_double import cheb_apply, lambda_max, np_cheb_operator, numpy_cheb_pcg_count
from precond_cases import block_congruence, block_jacobi_apply, lower_half, numpy_pcg_count, rhs, scipy_csr

BSS = (1, 2, 3, 4, 5, 8, 16)
U = 2.0 ** -53
TOL = 1e-10
CHECK_EVERY = 5
GRID, B_NODE, DEGREE = 20, 3, 4
FILL = 12345.0


# ------------------------------------------------------------ host statement
def _longdouble_step(n, bs, inv, a, b, R, AZ, D, Zin):
    """(d, z, bound) of every element in np.longdouble; AZ None: step 0."""
    L = np.longdouble
    k = R.shape[1]
    nbk = (n + bs - 1) // bs

    def blocks(x):  # (nbk, bs, k), rows >= n as zeros
        out = np.zeros((nbk * bs, k), L)
        out[:n] = x
        return out.reshape(nbk, bs, k)

    W = inv[:nbk * bs].astype(L).reshape(nbk, bs, bs)
    T = blocks(R if AZ is None else R.astype(L) - AZ.astype(L))
    Tmag = blocks(np.abs(R) if AZ is None else np.abs(R).astype(L) + np.abs(AZ).astype(L))
    s = np.matmul(W, T).reshape(nbk * bs, k)[:n]
    smag = np.matmul(np.abs(W), Tmag).reshape(nbk * bs, k)[:n]
    if AZ is None:
        d = L(b) * s
        return d, d, (bs + 5) * U * abs(L(b)) * smag
    d = L(a) * D.astype(L) + L(b) * s
    z = Zin.astype(L) + d
    return d, z, (bs + 5) * U * (abs(L(b)) * smag + np.abs(L(a) * D.astype(L)) + np.abs(Zin).astype(L))


def _guarded(rng, n, k, ld, fill=None):
    """(n + 2, ld) buffer, random or `fill` everywhere: two rows past n and
    ld - k padding columns."""
    return rng.uniform(-1, 1, (n + 2, ld)) if fill is None else np.full((n + 2, ld), fill)


@pytest.mark.parametrize("bs", BSS)
def test_host_step_against_longdouble(bs):
    """Docstring of the module: every element of D and Zout within
    (bs + 5) 2^-53 (|b| sum_c |inv_c| (|R_c| + |AZ_c|) + |a D| + |Zin|) of the
    longdouble evaluation; padding columns and rows >= n keep their values."""
    rng = np.random.default_rng(100 + bs)
    a, b = 0.37, 1.9
    worst = 0.0
    for n in sorted({1, bs - 1, 67, 4097} - {0}):
        nbk = (n + bs - 1) // bs
        inv = rng.uniform(-1, 1, (nbk * bs, bs))
        for k, ld in ((1, 1), (3, 3), (5, 8)):
            Rb, AZb = _guarded(rng, n, k, ld), _guarded(rng, n, k, ld + 1)
            Rb[:, k:] = np.nan  # padding and the rows past n must not be read
            AZb[:, k:] = np.nan
            Rb[n:] = np.nan
            AZb[n:] = np.nan
            R, AZ = Rb[:n, :k], AZb[:n, :k]
            for step0 in (True, False):
                for in_place in (False, True):
                    if step0 and in_place:
                        continue
                    Db = _guarded(rng, n, k, ld + 2)
                    Zinb = _guarded(rng, n, k, ld)
                    Zoutb = Zinb if in_place else _guarded(rng, n, k, ld + 3, FILL)
                    D0, Zin0, Zout0 = Db.copy(), Zinb.copy(), Zoutb.copy()
                    sa.cpu_bjacobi_cheb_step_multi(n, bs, inv, a, b, Rb[:, :k], None if step0 else AZb[:, :k],
                                                   Db[:, :k], None if step0 else Zinb[:, :k], Zoutb[:, :k], k=k)
                    d, z, bound = _longdouble_step(n, bs, inv, a, b, R, None if step0 else AZ, D0[:n, :k],
                                                   Zin0[:n, :k])
                    for name, got, ref in (("D", Db, d), ("Zout", Zoutb, z)):
                        err = np.abs(got[:n, :k].astype(np.longdouble) - ref)
                        assert (err <= bound).all(), (name, bs, n, k, step0, in_place, float((err / bound).max()))
                        live = bound > 0
                        worst = max(worst, float((err[live] / bound[live]).max())) if live.any() else worst
                    for got, before in ((Db, D0), (Zoutb, Zout0)):
                        assert np.array_equal(got[n:], before[n:]) and np.array_equal(got[:, k:], before[:, k:])
                    if not in_place:
                        assert np.array_equal(Zinb, Zin0)
                    if step0:  # D and Zout are one value; a, the old D and Zin play no part
                        assert np.array_equal(Db[:n, :k], Zoutb[:n, :k])
    print(f"bs={bs}: max error / bound {worst:.3g}")


def test_host_step_in_place_equals_out_of_place():
    rng = np.random.default_rng(5)
    n, bs, k = 67, 5, 3
    inv = rng.uniform(-1, 1, ((n + bs - 1) // bs * bs, bs))
    R, AZ, D, Z = (rng.uniform(-1, 1, (n, k)) for _ in range(4))
    D1, D2, Z1, Z2 = D.copy(), D.copy(), Z.copy(), np.empty_like(Z)
    sa.cpu_bjacobi_cheb_step_multi(n, bs, inv, 0.3, 1.7, R, AZ, D1, Z1, Z1)
    sa.cpu_bjacobi_cheb_step_multi(n, bs, inv, 0.3, 1.7, R, AZ, D2, Z, Z2)
    assert np.array_equal(D1, D2) and np.array_equal(Z1, Z2)
    # step 0 is b times the apply statement's chain
    ref = np.empty_like(R)
    sa.cpu_bjacobi_apply_multi(n, bs, inv, R, ref)
    sa.cpu_bjacobi_cheb_step_multi(n, bs, inv, 99.0, 1.7, R, None, D1, None, Z1)
    assert np.array_equal(D1, 1.7 * ref) and np.array_equal(Z1, D1)


def test_host_step_refusals_write_nothing():
    lib = sa.host_lib()
    P = sa._ptr
    n, bs, k = 4, 2, 3
    inv = np.ones((4, 2))
    R, AZ, Zin = np.ones((n, k)), np.ones((n, k)), np.ones((n, k))
    D, Zout = np.full((n, k), 7.0), np.full((n, k), 7.0)
    ok = [n, bs, P(inv), k, 0.5, 2.0, P(R), k, P(AZ), k, P(D), k, P(Zin), k, P(Zout), k]

    def call(**kw):
        args = list(ok)
        for i, v in kw.items():
            args[int(i[1:])] = v
        return lib.spmv_cpu_bjacobi_cheb_step_multi(*args)

    bad = [dict(a0=-1), dict(a1=0), dict(a1=17), dict(a3=0), dict(a7=2), dict(a9=2), dict(a11=2), dict(a13=2),
           dict(a15=2), dict(a2=None), dict(a6=None), dict(a10=None), dict(a12=None), dict(a14=None),
           dict(a12=P(Zout), a13=k + 1)]  # Zout == Zin with two leading dimensions
    for kw in bad:
        assert call(**kw) == sa.OTHER_ERROR, kw
    for kw in (dict(a0=-1), dict(a1=17), dict(a3=0), dict(a7=2), dict(a11=2), dict(a15=2), dict(a6=None),
               dict(a10=None), dict(a14=None)):  # the same at step 0
        assert call(a8=None, a12=None, **kw) == sa.OTHER_ERROR, kw
    assert (D == 7.0).all() and (Zout == 7.0).all()
    assert call() == sa.SUCCESS and not (D == 7.0).any()
    assert call(a8=None, a9=0, a12=None, a13=0) == sa.SUCCESS  # step 0: AZ's and Zin's ld are not looked at
    assert call(a0=0, a2=None, a6=None, a8=None, a10=None, a12=None, a14=None) == sa.SUCCESS  # no rows
    with pytest.raises(sa.SpmvError):
        sa.cpu_bjacobi_cheb_step_multi(n, bs, inv, 0.5, 2.0, R, AZ, D, None, Zout)  # a general step needs Zin
    with pytest.raises(sa.SpmvError):
        sa.cpu_bjacobi_cheb_step_multi(n, bs, inv, 0.5, 2.0, R, AZ, D[:, :2], Zin, Zout)
    with pytest.raises(sa.SpmvError):
        sa.cpu_bjacobi_cheb_step_multi(n, bs, inv[:3], 0.5, 2.0, R, AZ, D, Zin, Zout)
    with pytest.raises(sa.SpmvError):
        sa.cpu_bjacobi_cheb_step_multi(n, bs, inv, 0.5, 2.0, R[:2], AZ, D, Zin, Zout)


def test_device_entry_points_refuse_before_touching_a_device():
    lib = sa.hip_lib()
    buf = (ctypes.c_int64 * 3)(0, 1, 2)
    a = ctypes.addressof(buf)  # never dereferenced: every call below is refused
    assert lib.spmv_bjacobi_cheb_step_multi(None, 1, 0.5, 2.0, a, 1, a, 1, a, 1, a, 1, a, 1, None) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_cheb_step_dot_multi(None, 1, 0.5, 2.0, a, 1, a, 1, a, 1, a, 1, a, 1, a, a, 1 << 20,
                                                None) == sa.OTHER_ERROR


# --------------------------------------------------------------- recurrence
@pytest.fixture(scope="module")
def case():
    m = block_congruence(GRID, B_NODE)
    lam = lambda_max(m, B_NODE)
    B = rhs(m.n_rows, 4)
    B.setflags(write=False)
    return m, scipy_csr(m), B, lam, (1.1 * lam / 30.0, 1.1 * lam)


def test_coefficients():
    lmin, lmax = 0.07, 2.1
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    coef = it.chebyshev_coefficients(3, lmin, lmax)
    rho0 = delta / theta
    rho1 = 1 / (2 * theta / delta - rho0)
    rho2 = 1 / (2 * theta / delta - rho1)
    assert np.allclose(coef, [(0.0, 1 / theta), (rho1 * rho0, 2 * rho1 / delta), (rho2 * rho1, 2 * rho2 / delta)],
                       rtol=1e-15, atol=0)
    c = it.Chebyshev(object(), 16, lmin, lmax)
    assert len(c.coef) == 16 and c.M is not None and (c.lmin, c.lmax, c.degree) == (lmin, lmax, 16)
    for deg, lo, hi in ((0, lmin, lmax), (17, lmin, lmax), (2.0, lmin, lmax), (True, lmin, lmax), (4, 0.0, lmax),
                        (4, -1.0, lmax), (4, lmax, lmax), (4, lmax, lmin), (4, lmin, float("inf")),
                        (4, float("nan"), lmax)):
        with pytest.raises(sa.SpmvError):
            it.Chebyshev(object(), deg, lo, hi)


@pytest.mark.parametrize("degree", [DEGREE, 1])
def test_recurrence_against_dense_numpy(case, degree):
    """iterate.Chebyshev on the numpy double against a plain numpy evaluation
    of the recurrence: 1e-12 relative, per column; the sums are r.z and r.r."""
    m, A, B, lam, (lmin, lmax) = case
    assert 1.98 < lam < 2.0  # the spectrum of M^-1 A at bs = 3 is [0.011169, 1.988831]
    n = m.n_rows
    op = np_cheb_operator(m, 0, 1, B_NODE, degree, (lmin, lmax))
    minv = block_jacobi_apply(m, B_NODE)
    ref = cheb_apply(A, minv, degree, lmin, lmax)
    comm = it.Comm()
    for cols, multi in (([0, 1, 2, 3], True), ([1], False)):
        R = torch.from_numpy(np.ascontiguousarray(B[:, cols]))
        R0 = R.clone()
        Z = torch.full((n, len(cols)), float("nan"), dtype=torch.float64)
        out = torch.full((2 * len(cols),), float("nan"), dtype=torch.float64)
        for _ in range(2):  # the second apply reuses the buffers of the first
            op.precond.apply_dot(op, comm, R, Z, out, None, multi)
        assert torch.equal(R, R0)
        for j, c in enumerate(cols):
            want = ref(B[:, c])
            if degree == 1:
                assert np.allclose(want, minv(B[:, c]) / ((lmin + lmax) / 2), rtol=1e-15, atol=0)
            err = np.linalg.norm(Z[:, j].numpy() - want)
            print(f"degree {degree}, column {c}: relative difference {err / max(np.linalg.norm(want), 1e-300):.3g}")
            assert err <= 1e-12 * np.linalg.norm(want), (degree, c, err)
            assert abs(out[j] - B[:, c] @ want) <= 1e-12 * abs(B[:, c] @ want)
            assert abs(out[len(cols) + j] - B[:, c] @ B[:, c]) <= 1e-12 * (B[:, c] @ B[:, c])
        if multi:
            assert (Z[:, 3] == 0).all()  # the zero column
    made = dict(op.precond._state[1])
    assert set(made) == {(4, True), (1, False)}
    op.precond.apply_dot(op, comm, R, Z, out, None, False)
    assert all(op.precond._state[1][key] is val for key, val in made.items())  # a further apply allocates nothing


# ------------------------------------------------------------------- solves
def _solve(rank, world, lam, comm=None):
    m = block_congruence(GRID, B_NODE)
    B = rhs(m.n_rows, 4)
    bounds = (1.1 * lam / 30.0, 1.1 * lam)
    op = np_cheb_operator(m, rank, world, B_NODE, DEGREE, bounds)
    rb = op.layout.bounds
    Bl = torch.from_numpy(B[op.lo:op.lo + op.rows].copy())
    out = {}
    N = numpy_cheb_pcg_count(m, B, B_NODE, DEGREE, *bounds, bounds=rb)
    X, its, rel = it.cg_multi(op, Bl, comm, tol=TOL, maxit=10 * N, check_every=CHECK_EVERY)
    out["multi"] = (N, numpy_pcg_count(m, B, B_NODE, rb), its, rel, X.numpy().copy())
    N1 = numpy_cheb_pcg_count(m, B[:, 1:2], B_NODE, DEGREE, *bounds, bounds=rb)
    x, its, rel = it.cg(op, Bl[:, 1].contiguous(), comm, tol=TOL, maxit=10 * N, check_every=CHECK_EVERY)
    out["cg"] = (N1, numpy_pcg_count(m, B[:, 1:2], B_NODE, rb), its, np.array([rel]), x.numpy().copy()[:, None])
    return op.lo, out


def _check_case(key, N, N_bj, its, rel, X):
    m = block_congruence(GRID, B_NODE)
    A, B = scipy_csr(m), rhs(m.n_rows, 4)
    cols = [1] if key == "cg" else [0, 1, 2, 3]
    print(f"{key}: N_ref = {N} (block Jacobi alone: {N_bj}), {its} iterations, rel {rel}")
    assert 2 * N < N_bj, (key, N, N_bj)
    assert its <= N + CHECK_EVERY + N // 10, (key, its, N)
    assert (rel <= TOL).all()
    for j, c in enumerate(cols):
        nb = np.linalg.norm(B[:, c])
        res = np.linalg.norm(B[:, c] - A @ X[:, j])
        print(f"   column {c}: true residual {res:.3g} against {2e-10 * nb:.3g}")
        assert res <= 2e-10 * nb, (key, c, res)
        if nb == 0.0:
            assert (X[:, j] == 0.0).all() and not np.signbit(X[:, j]).any() and rel[j] == 0.0


@pytest.fixture(scope="module")
def one_rank(case):
    return _solve(0, 1, case[3])


def test_solves_single_rank(one_rank):
    lo, out = one_rank
    assert lo == 0 and out["multi"][0] == 25 and out["multi"][1] == 78
    for key, res in out.items():
        _check_case(key, *res)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, lam, q):
    sys.path[:0] = [str(PKG), str(REPO), str(REPO / "tests")]
    import torch.distributed as dist

    import iterate as it2

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        comm = it2.Comm(dist)
        lo, out = _solve(rank, world, lam, comm)
        # the estimator's all-reduces, on the same two ranks
        m = block_congruence(GRID, B_NODE)
        op = np_cheb_operator(m, rank, world, B_NODE, None)
        q.put((rank, lo, out, it2.estimate_lmax(op, op.precond, comm, iters=10)))
    finally:
        dist.destroy_process_group()


def test_solves_two_ranks(case, one_rank):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, case[3], q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, lo0, out0, est0), (_, lo1, out1, est1) = res
    assert lo0 == 0 and lo1 == out0["multi"][4].shape[0]
    assert est0 == est1 and case[3] <= 1.1 * est0 <= 1.1 * case[3]
    for key in out0:
        N, N_bj, its, rel, x0 = out0[key]
        assert (N, N_bj, its) == out1[key][:3] and np.array_equal(rel, out1[key][3])  # the all-reduced scalars
        X = np.concatenate([x0, out1[key][4]])
        _check_case(key, N, N_bj, its, rel, X)
        X1 = one_rank[1][key][4]
        for j in range(X.shape[1]):
            if np.linalg.norm(X1[:, j]) > 0:
                d = np.linalg.norm(X[:, j] - X1[:, j]) / np.linalg.norm(X1[:, j])
                print(f"   column {j}: two ranks against one {d:.3g}")
                assert d <= 1e-9, (key, j, d)


def test_chebyshev_by_keyword_and_precond_false(case):
    """A bare operator takes the Chebyshev object by keyword and gives the same
    iterates; precond=False on a Chebyshev operator is plain CG."""
    m, _, B, lam, bounds = case
    Bt = torch.from_numpy(B.copy())
    op = np_cheb_operator(m, 0, 1, B_NODE, DEGREE, bounds)
    bare = np_cheb_operator(m, 0, 1, B_NODE, None)
    bare.precond = None
    X1, its1, _ = it.cg_multi(op, Bt, tol=0.0, maxit=10)
    X2, its2, _ = it.cg_multi(bare, Bt, tol=0.0, maxit=10, precond=op.precond)
    assert its1 == its2 == 10 and torch.equal(X1, X2)
    X3 = it.cg_multi(op, Bt, tol=0.0, maxit=10, precond=False)[0]
    X4 = it.cg_multi(bare, Bt, tol=0.0, maxit=10)[0]
    assert torch.equal(X3, X4) and not torch.equal(X3, X1)
    x3 = it.cg(op, Bt[:, 1].contiguous(), tol=0.0, maxit=10, precond=False)[0]
    x4 = it.cg(bare, Bt[:, 1].contiguous(), tol=0.0, maxit=10)[0]
    assert torch.equal(x3, x4)


# ---------------------------------------------------------------- estimator
def test_estimate_lmax(case):
    """1.1 x the estimate after 10 steps covers lambda and is no more than
    1.1 lambda (the power method approaches from below)."""
    m, _, _, lam, _ = case
    op = np_cheb_operator(m, 0, 1, B_NODE, None)
    est = {i: it.estimate_lmax(op, op.precond, iters=i) for i in (5, 10, 20)}
    print(f"lambda {lam:.6f}: estimate / lambda after 5, 10, 20 steps: "
          f"{est[5] / lam:.4f} {est[10] / lam:.4f} {est[20] / lam:.4f}")
    assert lam <= 1.1 * est[10] <= 1.1 * lam
    assert est[5] <= est[10] <= est[20] <= lam
    assert it.estimate_lmax(op, op.precond) == est[10]  # the default
    with pytest.raises(sa.SpmvError):
        it.estimate_lmax(op, op.precond, iters=0)


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw", [dict(chebyshev=0), dict(chebyshev=17), dict(chebyshev=-1), dict(chebyshev=2.5),
                                dict(chebyshev=True), dict(chebyshev=4, cheb_bounds=(0.0, 2.0)),
                                dict(chebyshev=4, cheb_bounds=(2.0, 2.0)), dict(chebyshev=4, cheb_bounds=(2.0, 1.0)),
                                dict(chebyshev=4, cheb_bounds=(-1.0, 2.0)), dict(chebyshev=4, cheb_bounds=(1.0,)),
                                dict(chebyshev=4, cheb_bounds=(0.1, float("nan"))), dict(chebyshev=4, cheb_bounds=3.0),
                                dict(chebyshev=4, split=True), dict(chebyshev=4, overlap=True),
                                dict(chebyshev=4, cheb_ratio=1.0), dict(chebyshev=4, cheb_boost=0.0),
                                dict(chebyshev=4, bjacobi=17), dict(cheb_bounds=(0.1, 2.0))])
def test_build_operator_refusals_before_any_upload(kw, monkeypatch):
    def no_upload(*a, **k):
        raise AssertionError("uploaded before refusing")

    monkeypatch.setattr(sa, "to_device", no_upload)
    monkeypatch.setattr(sa, "_dev_tensor", no_upload)
    m = block_congruence(6, 3)
    with pytest.raises(sa.SpmvError):
        it.build_operator(m, **kw)
    if "split" not in kw and "overlap" not in kw:
        with pytest.raises(sa.SpmvError):
            it.build_operator(lower_half(m), symmetric="expand", **kw)


def test_split_operator_is_refused_before_any_kernel(case):
    """A Chebyshev object handed to a split operator by keyword: SpmvError
    before any product or step."""
    from iterate_precond_double import np_precond_operator

    m, _, B, lam, bounds = case
    sp_op = np_precond_operator(m, 0, 1, B_NODE, split=True)
    calls = []
    sp_op.kernels.spmv = lambda *a: calls.append("spmv")
    sp_op.kernels.precond_apply_dot = lambda *a: calls.append("apply")
    cheb = it.Chebyshev(sp_op.precond, DEGREE, *bounds)
    with pytest.raises(sa.SpmvError):
        it.cg(sp_op, torch.from_numpy(B[:, 0].copy()), precond=cheb)
    with pytest.raises(sa.SpmvError):
        it.estimate_lmax(sp_op, sp_op.precond)
    assert not calls
