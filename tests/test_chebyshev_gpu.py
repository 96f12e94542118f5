"""The Chebyshev polynomial preconditioner over block Jacobi on the MI355X
through libspmv_hip: the step kernels (csrc/precond.hip, bjacobi_cheb_kernel)
and iterate.cg / cg_multi with build_operator(bjacobi=3, chebyshev=4).

Bits.  D and Zout must equal spmv_cpu_bjacobi_cheb_step_multi on the
downloaded inverse bit for bit in every layout; the 2k sums of the dot form
must equal spmv_dot_multi(R, Zout) and spmv_dot_multi(R, R) bit for bit.  The
solves follow the iteration and residual rules of tests/test_chebyshev.py:
N_ref from the textbook numpy PCG with a numpy evaluation of the recurrence
(25 on block_congruence(20, 3) at bs = 3, degree 4), at most
N_ref + check_every + N_ref // 10 iterations.
"""
from __future__ import annotations

import numpy as np
import pytest

import iterate as it
import spmv_amd as sa
from iterate_cheb_double import lambda_max, numpy_cheb_pcg_count
from precond_cases import block_congruence, lower_half, numpy_pcg_count, rhs, scipy_csr
from test_iterate_multi_gpu import EVEN, GUARD, KS, LAYOUTS, _dot, _host_block, _place, _stream
from test_precond_gpu import BSS, dominant, precond_for

pytestmark = pytest.mark.gpu

TOL = 1e-10
CHECK_EVERY = 5
A_COEF, B_COEF = 0.37, 1.9
MODES = ("step0", "apart", "in place")  # step 0; a general step with Zout apart from Zin, and with Zout == Zin


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch, torch.device("cuda:0")


# --------------------------------------------------------------------- bits
def run_step(torch, dev, M, inv, n, bs, k, layouts, mode, fused):
    """One step (fused: the dot form) on guarded buffers, R, AZ, D, Zin, Zout
    in `layouts` (one name for all five, or five names); checks D's and Zout's
    bits against the host statement and that nothing else changed.  Returns
    (R's and Zout's (tensor, address, ld), out)."""
    lib = sa.hip_lib()
    lay = (layouts,) * 5 if isinstance(layouts, str) else layouts
    step0, in_place = mode == "step0", mode == "in place"
    host = [_host_block(n, s) for s in (5, 7, 6, 8, 9)]
    tr, pr, ldr, _ = _place(torch, dev, host[0], n, k, lay[0], 15)
    taz, paz, ldaz, _ = _place(torch, dev, host[1], n, k, lay[1], 17)
    td, pd, ldd, live_d = _place(torch, dev, host[2], n, k, lay[2], 16)
    tzi, pzi, ldzi, live_zi = _place(torch, dev, host[3], n, k, lay[3], 18)
    tzo, pzo, ldzo, live_zo = (tzi, pzi, ldzi, live_zi) if in_place else _place(torch, dev, host[4], n, k, lay[4], 19)
    before = [t.cpu().numpy() for t in (tr, taz, td, tzi, tzo)]
    args = (M.handle, k, A_COEF, B_COEF, pr, ldr, None if step0 else paz, ldaz, pd, ldd, None if step0 else pzi, ldzi,
            pzo, ldzo)
    dout = None
    if fused:
        ws = M.ws(n, k)
        dout = torch.full((2 * k + 4,), float("nan"), dtype=torch.float64, device=dev)
        dout[:2] = GUARD
        dout[-2:] = GUARD
        rc = lib.spmv_bjacobi_cheb_step_dot_multi(*args, dout.data_ptr() + 16, sa._ptr(ws), ws.numel(),
                                                  _stream(torch, dev))
    else:
        rc = lib.spmv_bjacobi_cheb_step_multi(*args, _stream(torch, dev))
    assert rc == 0, lib.spmv_last_error().decode()
    after = [t.cpu().numpy() for t in (tr, taz, td, tzi, tzo)]
    tag = (n, bs, k, layouts, mode, fused)
    for i in (0, 1) + (() if in_place else (3,)):  # R, AZ and a separate Zin: untouched
        assert np.array_equal(after[i].view(np.int64), before[i].view(np.int64)), (tag, i)
    for i, live in ((2, live_d), (4, live_zo)):  # padding, rows >= n, guards
        assert np.array_equal(after[i].view(np.int64)[~live], before[i].view(np.int64)[~live]), (tag, i)
    R, AZ, D, Zin = (np.array(h[:n, :k]) for h in host[:4])  # copies: the statement rewrites D
    Zref = np.full((n, k), np.nan)
    sa.cpu_bjacobi_cheb_step_multi(n, bs, inv, A_COEF, B_COEF, R, None if step0 else AZ, D, None if step0 else Zin,
                                   Zref)
    assert np.array_equal(after[2][live_d].reshape(n, k).view(np.int64), D.view(np.int64)), (tag, "D")
    assert np.array_equal(after[4][live_zo].reshape(n, k).view(np.int64), Zref.view(np.int64)), (tag, "Zout")
    out = None
    if fused:
        h = dout.cpu().numpy()
        assert (h[:2] == GUARD).all() and (h[-2:] == GUARD).all()
        out = h[2:-2].copy()
    return (tr, pr, ldr), (tzo, pzo, ldzo), out  # the tensors keep the addresses alive


def check_sums(torch, dev, n, k, rd, zd, out):
    (_, pr, ldr), (_, pz, ldz) = rd, zd
    rz = _dot(torch, dev, n, k, pr, ldr, pz, ldz)
    rr = _dot(torch, dev, n, k, pr, ldr, pr, ldr)
    assert np.isfinite(out).all()
    assert np.array_equal(out[:k].view(np.int64), rz.view(np.int64)), (n, k, "r.z")
    assert np.array_equal(out[k:].view(np.int64), rr.view(np.int64)), (n, k, "r.r")


@pytest.mark.parametrize("n", [67, 4097])
@pytest.mark.parametrize("bs", BSS)
def test_step_bits(torch_dev, bs, n):
    torch, dev = torch_dev
    M, inv = precond_for(dev, n, bs)
    for k in KS:
        for layout in LAYOUTS + (EVEN,):
            for mode in MODES:
                run_step(torch, dev, M, inv, n, bs, k, layout, mode, False)
                rd, zd, out = run_step(torch, dev, M, inv, n, bs, k, layout, mode, True)
                check_sums(torch, dev, n, k, rd, zd, out)


def test_step_bits_mixed_alignment(torch_dev):
    """The 16-byte path only when every array of the step is on it: one
    8-byte-aligned or odd-ld array among aligned ones gives the same bits."""
    torch, dev = torch_dev
    n, bs = 4097, 3
    M, inv = precond_for(dev, n, bs)
    for k in (2, 8, 10):
        for odd in range(5):
            lay = tuple("padded" if i == odd else ("tight", EVEN)[i % 2] for i in range(5))
            for mode in ("step0", "apart"):
                rd, zd, out = run_step(torch, dev, M, inv, n, bs, k, lay, mode, True)
                check_sums(torch, dev, n, k, rd, zd, out)


def test_step_dot_past_the_block_cap(torch_dev):
    """n = 600,011 rows: more than 1,024 workgroups of two steps, so every
    thread takes several rows into each accumulator; bs = 3 blocks straddle
    every workgroup."""
    torch, dev = torch_dev
    n, bs, k = 600_011, 3, 2
    i = np.arange(n, dtype=np.int64)
    row = np.repeat(i, bs)
    col = (i // bs * bs)[:, None] + np.arange(bs)[None, :]
    val = np.random.default_rng(9).uniform(-1, 1, (n, bs))
    val[col == i[:, None]] += 4.0
    keep = (col < n).ravel()
    m = sa.Coo(n, n, row[keep].astype(np.int32), col.ravel()[keep].astype(np.int32), val.ravel()[keep], False, "blocks")
    M = sa.BlockJacobi.from_coo(m, bs, dev)
    assert M.info()["singular_blocks"] == 0
    inv = M.inverse().cpu().numpy()
    for layout, mode in (("tight", "in place"), ("padded", "apart")):
        rd, zd, out = run_step(torch, dev, M, inv, n, bs, k, layout, mode, True)
        check_sums(torch, dev, n, k, rd, zd, out)


def test_empty_refusals_and_python_wrappers(torch_dev):
    torch, dev = torch_dev
    lib = sa.hip_lib()
    P = sa._ptr
    M0 = sa.BlockJacobi.from_coo(dominant(0), 3, dev)
    out = torch.full((4,), float("nan"), dtype=torch.float64, device=dev)
    e = torch.zeros(0, 2, dtype=torch.float64, device=dev)
    M0.cheb_step(0.5, 2.0, e, None, e.clone(), None, e.clone())
    M0.cheb_step_dot(0.5, 2.0, e, e.clone(), e.clone(), e.clone(), e.clone(), out, M0.ws(0, 2))
    h = out.cpu().numpy()
    assert (h == 0.0).all() and not np.signbit(h).any()  # n == 0 writes 2k positive zeros
    # refused calls leave D, Z and out untouched
    n, bs, k = 4097, 3, 3
    M, inv = precond_for(dev, n, bs)
    R = torch.ones(n, k, dtype=torch.float64, device=dev)
    AZ = torch.ones(n, k, dtype=torch.float64, device=dev)
    D, Zin, Zout = (torch.full((n, k), 7.0, dtype=torch.float64, device=dev) for _ in range(3))
    out = torch.full((2 * k,), 7.0, dtype=torch.float64, device=dev)
    need = lib.spmv_bjacobi_ws_bytes(n, k)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s = _stream(torch, dev)
    ok = [M.handle, k, 0.5, 2.0, P(R), k, P(AZ), k, P(D), k, P(Zin), k, P(Zout), k]

    def args(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return a

    bad = [dict(a0=None), dict(a1=0), dict(a5=k - 1), dict(a7=k - 1), dict(a9=k - 1), dict(a11=k - 1),
           dict(a13=k - 1), dict(a4=None), dict(a8=None), dict(a10=None), dict(a12=None),
           dict(a12=P(Zin), a13=k + 1), dict(a6=None, a9=k - 1), dict(a6=None, a8=None), dict(a6=None, a12=None)]
    for kw in bad:
        assert lib.spmv_bjacobi_cheb_step_multi(*args(**kw), s) == sa.OTHER_ERROR, kw
        assert lib.spmv_bjacobi_cheb_step_dot_multi(*args(**kw), P(out), P(ws), need, s) == sa.OTHER_ERROR, kw
    assert lib.spmv_bjacobi_cheb_step_dot_multi(*ok, None, P(ws), need, s) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_cheb_step_dot_multi(*ok, P(out), None, need, s) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_cheb_step_dot_multi(*ok, P(out), P(ws), need - 8, s) == sa.OTHER_ERROR
    torch.cuda.synchronize()
    assert (D == 7.0).all() and (Zin == 7.0).all() and (Zout == 7.0).all() and (out == 7.0).all()
    with pytest.raises(sa.SpmvError):
        M.cheb_step(0.5, 2.0, R, AZ, D, None, Zout)  # a general step needs Zin
    with pytest.raises(sa.SpmvError):
        M.cheb_step(0.5, 2.0, R, AZ, D[:, :2], Zin, Zout)
    with pytest.raises(sa.SpmvError):
        M.cheb_step(0.5, 2.0, R, AZ.float(), D, Zin, Zout)
    with pytest.raises(sa.SpmvError):
        M.cheb_step(0.5, 2.0, R[:100], AZ, D, Zin, Zout)
    with pytest.raises(sa.SpmvError):
        M.cheb_step_dot(0.5, 2.0, R, AZ, D, Zin, Zout, out[:3], ws)
    assert (D == 7.0).all() and (Zout == 7.0).all()
    # the wrappers against the host statement, 2-D blocks and 1-D vectors (k = 1, ld = 1)
    Rh, AZh, Dh, Zh = (np.array(_host_block(n, s)[:n, :k]) for s in (5, 7, 6, 8))
    Rd, AZd, Dd, Zd = (torch.from_numpy(a.copy()).to(dev) for a in (Rh, AZh, Dh, Zh))
    Dref, Zref = Dh.copy(), Zh.copy()
    sa.cpu_bjacobi_cheb_step_multi(n, bs, inv, 0.5, 2.0, Rh, AZh, Dref, Zref, Zref)
    M.cheb_step_dot(0.5, 2.0, Rd, AZd, Dd, Zd, Zd, out, ws)
    assert np.array_equal(Dd.cpu().numpy().view(np.int64), Dref.view(np.int64))
    assert np.array_equal(Zd.cpu().numpy().view(np.int64), Zref.view(np.int64))
    r1, d1, z1 = Rd[:, 0].contiguous(), torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(
        n, dtype=torch.float64, device=dev)
    M.cheb_step(0.5, 2.0, r1, None, d1, None, z1)
    D1, Z1 = np.empty((n, 1)), np.empty((n, 1))
    sa.cpu_bjacobi_cheb_step_multi(n, bs, inv, 0.5, 2.0, np.ascontiguousarray(Rh[:, :1]), None, D1, None, Z1)
    assert np.array_equal(z1.cpu().numpy().view(np.int64), Z1[:, 0].view(np.int64))
    assert np.array_equal(d1.cpu().numpy().view(np.int64), D1[:, 0].view(np.int64))


# -------------------------------------------------------------------- solves
GRID, B_NODE, DEGREE = 20, 3, 4


@pytest.fixture(scope="module")
def case():
    m = block_congruence(GRID, B_NODE)
    B = rhs(m.n_rows, 4)  # ones, uniform - 0.5, e_0, zeros
    B.setflags(write=False)
    lam = lambda_max(m, B_NODE)
    bounds = (1.1 * lam / 30.0, 1.1 * lam)
    return dict(m=m, half=lower_half(m), A=scipy_csr(m), B=B, lam=lam, bounds=bounds,
                N=numpy_cheb_pcg_count(m, B, B_NODE, DEGREE, *bounds),
                N1=numpy_cheb_pcg_count(m, B[:, 1:2], B_NODE, DEGREE, *bounds))


def _operator(case, dev, kind, **kw):
    kw.setdefault("bjacobi", B_NODE)
    if kind in ("fused", "expand"):
        return it.build_operator(case["half"], 0, 1, "csr", dev, align=64, symmetric=kind, **kw)
    return it.build_operator(case["m"], 0, 1, kind, dev, align=64, **kw)


def _cheb_operator(case, dev, kind):
    return _operator(case, dev, kind, chebyshev=DEGREE, cheb_bounds=case["bounds"])


def _check_true_residual(A, B, X):
    assert np.isfinite(X).all()
    for j in range(B.shape[1]):
        nb = np.linalg.norm(B[:, j])
        res = np.linalg.norm(B[:, j] - A @ X[:, j])
        print(f"column {j}: true residual {res:.3g} against {2e-10 * nb:.3g}")
        assert res <= 2e-10 * nb, (j, res, nb)


@pytest.mark.parametrize("kind", ["csr", "sell", "ell", "expand", "fused"])
def test_chebyshev_pcg_solves(torch_dev, case, kind):
    torch, dev = torch_dev
    A, B, N, N1 = case["A"], case["B"], case["N"], case["N1"]
    assert 2 * N < numpy_pcg_count(case["m"], B, B_NODE)
    op = _cheb_operator(case, dev, kind)
    assert isinstance(op.precond, it.Chebyshev) and isinstance(op.precond.M, sa.BlockJacobi)
    assert (op.precond.degree, op.precond.lmin, op.precond.lmax) == (DEGREE,) + case["bounds"]
    assert op.precond.M.info()["bs"] == B_NODE and op.precond.M.info()["singular_blocks"] == 0
    Bd = torch.from_numpy(B.copy()).to(dev)
    X, its, rel = it.cg_multi(op, Bd, tol=TOL, maxit=10 * N, check_every=CHECK_EVERY)
    X = X.cpu().numpy()
    print(f"{kind}: cg_multi {its} iterations (N_ref = {N}), rel {rel}")
    assert its <= N + CHECK_EVERY + N // 10
    assert rel.shape == (4,) and (rel <= TOL).all() and rel[3] == 0.0
    assert (X[:, 3] == 0.0).all() and not np.signbit(X[:, 3]).any()  # the zero column: exactly 0
    _check_true_residual(A, B, X)
    x, its, rel1 = it.cg(op, Bd[:, 1].contiguous(), tol=TOL, maxit=10 * N, check_every=CHECK_EVERY)
    print(f"{kind}: cg {its} iterations (N_ref = {N1}), rel {rel1}")
    assert its <= N1 + CHECK_EVERY + N1 // 10 and rel1 <= TOL
    _check_true_residual(A, B[:, 1:2], x.cpu().numpy()[:, None])


def test_estimated_bounds(torch_dev, case):
    """build_operator's own bounds: 1.1 x the power method's estimate covers
    lambda, lmin = lmax / 30, bjacobi=None means point Jacobi."""
    torch, dev = torch_dev
    lam = case["lam"]
    op = _operator(case, dev, "csr", chebyshev=DEGREE)
    c = op.precond
    print(f"lambda {lam:.6f}: lmax {c.lmax:.6f} = {c.lmax / lam:.4f} lambda")
    assert lam <= c.lmax <= 1.1 * lam and c.lmin == c.lmax / 30.0
    assert c.lmax == 1.1 * it.estimate_lmax(op, c.M)
    N = numpy_cheb_pcg_count(case["m"], case["B"], B_NODE, DEGREE, c.lmin, c.lmax)
    Bd = torch.from_numpy(case["B"].copy()).to(dev)
    X, its, rel = it.cg_multi(op, Bd, tol=TOL, maxit=10 * N, check_every=CHECK_EVERY)
    assert its <= N + CHECK_EVERY + N // 10 and (rel <= TOL).all()
    _check_true_residual(case["A"], case["B"], X.cpu().numpy())
    point = _operator(case, dev, "csr", bjacobi=None, chebyshev=2, cheb_ratio=10.0, cheb_boost=1.2)
    assert point.precond.M.info()["bs"] == 1 and point.precond.lmin == point.precond.lmax / 10.0
    assert point.precond.lmax == 1.2 * it.estimate_lmax(point, point.precond.M)


@pytest.mark.parametrize("kind", ["csr", "expand"])
def test_chebyshev_column_bits(torch_dev, case, kind):
    """A column's iterates do not depend on the columns solved with it."""
    torch, dev = torch_dev
    n = case["m"].n_rows
    op = _cheb_operator(case, dev, kind)
    B = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (n, 5))).to(dev)
    X = it.cg_multi(op, B, tol=0.0, maxit=10)[0].clone()
    X2 = it.cg_multi(op, B, tol=0.0, maxit=10)[0].clone()
    assert torch.equal(X.view(torch.int64), X2.view(torch.int64))
    assert torch.isfinite(X).all() and (X != 0.0).any()
    for j in range(5):
        xj = it.cg_multi(op, B[:, j:j + 1].contiguous(), tol=0.0, maxit=10)[0]
        assert torch.equal(xj[:, 0].view(torch.int64), X[:, j].contiguous().view(torch.int64)), j


def test_chebyshev_side_stream_same_bits(torch_dev, case):
    torch, dev = torch_dev
    n = case["m"].n_rows
    B = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (n, 3))).to(dev)
    X1 = it.cg_multi(_cheb_operator(case, dev, "csr"), B, tol=0.0, maxit=10)[0].clone()
    x1 = it.cg(_cheb_operator(case, dev, "csr"), B[:, 0].contiguous(), tol=0.0, maxit=10)[0].clone()
    op = _cheb_operator(case, dev, "csr")
    op.kernels.stream = torch.cuda.Stream(dev)
    X2, its, rel = it.cg_multi(op, B, tol=0.0, maxit=10)
    x2 = it.cg(op, B[:, 0].contiguous(), tol=0.0, maxit=10)[0]
    torch.cuda.synchronize()
    assert its == 10 and np.isfinite(rel).all()
    assert torch.equal(X1.view(torch.int64), X2.view(torch.int64))
    assert torch.equal(x1.view(torch.int64), x2.view(torch.int64))


def _old_way(case, dev, bjacobi):
    """The operator as build_operator assembled it before it knew `chebyshev`:
    layout, shard, device matrix and the sa.BlockJacobi of the shard, put
    together here piece by piece."""
    m = case["m"]
    counts = np.bincount(m.row, minlength=m.n_rows).astype(np.int64)
    layout = it.layout_for(m.n_rows, counts, 1, 64)
    loc = it.local_shard(m, layout, 0)
    M = None if bjacobi is None else sa.BlockJacobi.from_coo(loc, bjacobi, dev, 0, False)
    return it.DistOperator(layout, 0, m.n_rows, it.HipKernels(sa.to_device(loc, "csr", dev)), dev, precond=M)


def _old_pcg_multi(torch, op, B, maxit):
    """_pcg's loop as it stood before Chebyshev, call for call (tol = 0)."""
    k, M, rows, nv, dev = op.kernels, op.precond, op.rows, B.shape[1], B.device

    def z(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=dev)

    send = z(op.pad, nv)
    P, X, R, Z, AP = send[:rows], z(rows, nv), B.clone(), z(rows, nv), z(rows, nv)
    ws, pws, pAp = k.dot_multi_ws(rows, nv), k.precond_ws(M, rows, nv), z(nv)
    s, s_new = z(2 * nv), z(2 * nv)
    k.precond_apply_dot(M, rows, R, Z, s, pws)
    P.copy_(Z)
    for _ in range(maxit):
        k.spmm(send, AP)
        k.dot_multi(rows, P, AP, pAp, ws)
        k.axpy_ratio_multi(rows, s[:nv], pAp, 1.0, P, X)
        k.axpy_ratio_multi(rows, s[:nv], pAp, -1.0, AP, R)
        k.precond_apply_dot(M, rows, R, Z, s_new, pws)
        k.xpay_ratio_multi(rows, s_new[:nv], s[:nv], Z, P)
        s, s_new = s_new, s
    return X


def test_operators_without_chebyshev_keep_their_bits(torch_dev, case):
    """Built without `chebyshev`, cg_multi and cg run what they ran before,
    with and without bjacobi: the operator assembled the old way and the old
    loop written out give the same bits."""
    torch, dev = torch_dev
    n = case["m"].n_rows
    B = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (n, 3))).to(dev)
    for bjacobi in (None, B_NODE):
        new, old = _operator(case, dev, "csr", bjacobi=bjacobi), _old_way(case, dev, bjacobi)
        assert (new.precond is None) == (bjacobi is None) and not isinstance(new.precond, it.Chebyshev)
        X0 = it.cg_multi(old, B, tol=0.0, maxit=25)[0].clone()
        X1 = it.cg_multi(new, B, tol=0.0, maxit=25)[0].clone()
        assert torch.equal(X0.view(torch.int64), X1.view(torch.int64)) and (X1 != 0).any()
        x0 = it.cg(old, B[:, 0].contiguous(), tol=0.0, maxit=25)[0].clone()
        x1 = it.cg(new, B[:, 0].contiguous(), tol=0.0, maxit=25)[0].clone()
        assert torch.equal(x0.view(torch.int64), x1.view(torch.int64))
        if bjacobi is not None:
            X2 = _old_pcg_multi(torch, old, B, 25)
            torch.cuda.synchronize()
            assert torch.equal(X2.view(torch.int64), X1.view(torch.int64))


def test_precond_false_on_a_chebyshev_operator(torch_dev, case):
    torch, dev = torch_dev
    n = case["m"].n_rows
    B = torch.from_numpy(np.random.default_rng(6).uniform(-1, 1, (n, 3))).to(dev)
    bare = _operator(case, dev, "csr", bjacobi=None)
    op = _cheb_operator(case, dev, "csr")
    X0 = it.cg_multi(bare, B, tol=0.0, maxit=25)[0].clone()
    X1 = it.cg_multi(op, B, tol=0.0, maxit=25, precond=False)[0].clone()
    assert torch.equal(X0.view(torch.int64), X1.view(torch.int64))
    x0 = it.cg(bare, B[:, 0].contiguous(), tol=0.0, maxit=25)[0].clone()
    x1 = it.cg(op, B[:, 0].contiguous(), tol=0.0, maxit=25, precond=False)[0].clone()
    assert torch.equal(x0.view(torch.int64), x1.view(torch.int64))
    # and the Chebyshev object given by keyword is the operator's own
    X2 = it.cg_multi(bare, B, tol=0.0, maxit=10, precond=op.precond)[0].clone()
    X3 = it.cg_multi(op, B, tol=0.0, maxit=10)[0].clone()
    assert torch.equal(X2.view(torch.int64), X3.view(torch.int64))
    # precond.M alone is block-Jacobi PCG
    X4 = it.cg_multi(bare, B, tol=0.0, maxit=10, precond=op.precond.M)[0].clone()
    X5 = it.cg_multi(_operator(case, dev, "csr"), B, tol=0.0, maxit=10)[0].clone()
    assert torch.equal(X4.view(torch.int64), X5.view(torch.int64)) and not torch.equal(X4, X3)


def test_split_and_bad_degrees_are_refused(torch_dev, case):
    torch, dev = torch_dev
    for kw in (dict(chebyshev=0), dict(chebyshev=17), dict(chebyshev=4, split=True), dict(chebyshev=4, overlap=True),
               dict(chebyshev=4, cheb_bounds=(2.0, 1.0))):
        with pytest.raises(sa.SpmvError):
            it.build_operator(case["m"], 0, 1, "csr", dev, align=64, **kw)
    sp_op = it.build_operator(case["m"], 0, 1, "csr", dev, align=64, split=True, bjacobi=B_NODE)
    cheb = it.Chebyshev(sp_op.precond, DEGREE, *case["bounds"])
    with pytest.raises(sa.SpmvError):
        it.cg(sp_op, torch.ones(case["m"].n_rows, dtype=torch.float64, device=dev), precond=cheb)
