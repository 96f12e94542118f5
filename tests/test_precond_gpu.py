"""Block-Jacobi preconditioned CG on the MI355X through libspmv_hip: the device
build (spmv_bjacobi_create), the two apply kernels (csrc/precond.hip) and
iterate.cg / cg_multi with build_operator(bjacobi=3).

Bounds.  The device inverse is held to the inverse rule of
tests/test_precond.py with the HOST statement's residual as the reference:
e_dev <= 8 max_q e_host + bs 2^-52, e(X) = max |I - D_q X| in np.longdouble
against a dense numpy extraction.  Z must equal spmv_cpu_bjacobi_apply_multi
on the downloaded inverse bit for bit; the 2k sums of the fused kernel must
equal spmv_dot_multi(R, Z) and spmv_dot_multi(R, R) bit for bit and meet that
test's (n + 2) 2^-53 sum |a b| bound.  The solves follow the iteration and
residual rules of the CPU test (N = 78 on block_congruence(20, 3) at bs = 3).
"""
from __future__ import annotations

import numpy as np
import pytest

import iterate as it
import spmv_amd as sa
from precond_cases import block_congruence, dense_blocks, lower_half, numpy_pcg_count, rhs, scipy_csr
from test_iterate_multi_gpu import EVEN, GUARD, KS, LAYOUTS, U, _dot, _host_block, _place, _stream

pytestmark = pytest.mark.gpu

BSS = (1, 2, 3, 4, 5, 8, 16)
U52 = 2.0 ** -52
TOL = 1e-10
CHECK_EVERY = 5


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch, torch.device("cuda:0")


# ------------------------------------------------------------------ matrices
_mats = {}


def dominant(n, holes=False):
    """sa.gen_random(n, n, 1, 8) plus five random neighbours per row (so the
    blocks are full) and a diagonal that dominates its row; made once.
    holes: the rows i % 97 == 5 lose every entry (singular blocks) and row 11
    gets a NaN on its diagonal."""
    key = (n, holes)
    if key not in _mats:
        if n == 0:
            m = sa.Coo(0, 0, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), False, "empty")
        else:
            g = sa.gen_random(n, n, 1, 8, seed=n)
            mag = np.bincount(g.row, weights=np.abs(g.val), minlength=n)
            d = np.arange(n, dtype=np.int32)
            rng = np.random.default_rng(n)
            near = [(d[(d + o >= 0) & (d + o < n)], o) for o in (-5, -2, -1, 1, 2)]  # neighbours: full blocks
            n_row = np.concatenate([r for r, _ in near])
            n_col = np.concatenate([r + o for r, o in near]).astype(np.int32)
            n_val = rng.uniform(-1.0, 1.0, n_row.size)
            mag = mag + np.bincount(n_row, weights=np.abs(n_val), minlength=n)
            row = np.concatenate([g.row, n_row, d])
            col = np.concatenate([g.col, n_col, d])
            val = np.concatenate([g.val, n_val, mag + 1.0])
            if holes:
                keep = row % 97 != 5
                row, col, val = row[keep], col[keep], val[keep]
                val = val.copy()
                val[(row == 11) & (col == 11)] = np.nan
            o = np.argsort(row, kind="stable")
            m = sa.Coo(n, n, row[o], col[o], val[o], False, f"dominant {n}")
        _mats[key] = m
    return _mats[key]


def residuals(D, inv, bs):
    X = inv.reshape(-1, bs, bs).astype(np.longdouble)
    eye = np.eye(bs, dtype=np.longdouble)
    return np.abs(eye - np.matmul(D.astype(np.longdouble), X)).reshape(D.shape[0], -1).max(axis=1)


def host_inverse(m, bs, half=False):
    ptr, col, val = sa.csr_from_coo(m)
    return sa.bjacobi_build_host(m.n_rows, ptr, col, val, bs, 0, half)


# -------------------------------------------------------------------- create
@pytest.mark.parametrize("half", [False, True], ids=["full", "half"])
@pytest.mark.parametrize("bs", BSS)
def test_create(torch_dev, bs, half):
    torch, dev = torch_dev
    for n in sorted({0, 1, bs - 1, 67, 4097}):
        full = dominant(n)
        m = lower_half(full) if half else full
        M = sa.BlockJacobi.from_coo(m, bs, dev, symmetric_half=half)
        M2 = sa.BlockJacobi.from_coo(m, bs, dev, symmetric_half=half)
        info = M.info()
        nbk = (n + bs - 1) // bs
        assert (info["bs"], info["n"], info["n_blocks"], info["col_base"]) == (bs, n, nbk, 0)
        assert info["symmetric_half"] == half and info["owned_bytes"] == 8 * nbk * bs * bs
        assert info["kernel"] == "bjacobi_apply_kernel"
        inv = M.inverse()
        assert tuple(inv.shape) == (nbk * bs, bs)
        assert torch.equal(inv.view(torch.int64), M2.inverse().view(torch.int64))  # two builds: the same bits
        inv = inv.cpu().numpy()
        h_inv, h_sing = host_inverse(m, bs, half)
        assert info["singular_blocks"] == h_sing == 0
        if n == 0:
            continue
        D = dense_blocks(m, bs, symmetric_half=half)
        e_host, e_dev = residuals(D, h_inv, bs), residuals(D, inv, bs)
        bound = 8 * e_host.max() + bs * U52
        same = np.array_equal(inv.view(np.int64), h_inv.view(np.int64))
        print(f"bs={bs} n={n} half={half}: max e_dev/bound {float(e_dev.max() / bound):.3g}, host bits: {same}")
        assert np.isfinite(inv).all() and (e_dev <= bound).all(), (bs, n, float(e_dev.max()), float(bound))


@pytest.mark.parametrize("bs", [1, 3, 16])
def test_create_counts_singular_blocks(torch_dev, bs):
    torch, dev = torch_dev
    n = 4097
    m = dominant(n, holes=True)
    M = sa.BlockJacobi.from_coo(m, bs, dev)
    h_inv, h_sing = host_inverse(m, bs)
    assert M.info()["singular_blocks"] == h_sing and h_sing >= n // 97 // 2
    inv = M.inverse().cpu().numpy().reshape(-1, bs, bs)
    eye = np.eye(bs)
    dev_eye = np.array([np.array_equal(b, eye) for b in inv])
    host_eye = np.array([np.array_equal(b, eye) for b in h_inv.reshape(-1, bs, bs)])
    assert np.isfinite(inv).all() and np.array_equal(dev_eye, host_eye) and dev_eye.sum() >= h_sing


def test_create_with_col_base(torch_dev):
    """Rank 1 of 2 in the gathered layout against the global matrix's blocks."""
    torch, dev = torch_dev
    m = block_congruence(6, 3)
    counts = np.bincount(m.row, minlength=m.n_rows).astype(np.int64)
    layout = it.layout_for(m.n_rows, counts, 2, 8)
    lo, hi = int(layout.bounds[1]), int(layout.bounds[2])
    loc = it.local_shard(m, layout, 1)
    for bs in (3, 4):
        M = sa.BlockJacobi.from_coo(loc, bs, dev, col_base=layout.pad)
        assert M.info()["col_base"] == layout.pad and M.info()["singular_blocks"] == 0
        ptr, col, val = sa.csr_from_coo(loc)
        h_inv, _ = sa.bjacobi_build_host(loc.n_rows, ptr, col, val, bs, layout.pad)
        D = dense_blocks(m, bs, lo, hi)
        e_dev = residuals(D, M.inverse().cpu().numpy(), bs)
        assert (e_dev <= 8 * residuals(D, h_inv, bs).max() + bs * U52).all()


# --------------------------------------------------------------------- apply
_precs = {}


def precond_for(dev, n, bs):
    if (n, bs) not in _precs:
        _precs[n, bs] = sa.BlockJacobi.from_coo(dominant(n), bs, dev)
    M = _precs[n, bs]
    return M, M.inverse().cpu().numpy()


def run_apply(torch, dev, M, inv, n, bs, k, layout, fused):
    """One apply (fused: apply_dot) on guarded buffers; checks Z's bits against
    the host statement and that nothing else changed.  Returns (R, Z, out)."""
    lib = sa.hip_lib()
    r, z0 = _host_block(n, 5), _host_block(n, 6)
    tr, pr, ldr, _ = _place(torch, dev, r, n, k, layout, 15)
    tz, pz, ldz, live = _place(torch, dev, z0, n, k, layout, 16)
    r_before, z_before = tr.cpu().numpy(), tz.cpu().numpy()
    out = None
    if fused:
        ws = M.ws(n, k)
        dout = torch.full((2 * k + 4,), float("nan"), dtype=torch.float64, device=dev)
        dout[:2] = GUARD
        dout[-2:] = GUARD
        rc = lib.spmv_bjacobi_apply_dot_multi(M.handle, k, pr, ldr, pz, ldz, dout.data_ptr() + 16, sa._ptr(ws),
                                              ws.numel(), _stream(torch, dev))
    else:
        rc = lib.spmv_bjacobi_apply_multi(M.handle, k, pr, ldr, pz, ldz, _stream(torch, dev))
    assert rc == 0, lib.spmv_last_error().decode()
    z_after = tz.cpu().numpy()
    assert np.array_equal(tr.cpu().numpy().view(np.int64), r_before.view(np.int64))  # R untouched
    assert np.array_equal(z_after.view(np.int64)[~live], z_before.view(np.int64)[~live])  # padding, rows >= n, guards
    R = np.ascontiguousarray(r[:n, :k])
    ref = np.full((n, k), np.nan)
    sa.cpu_bjacobi_apply_multi(n, bs, inv, R, ref)
    Z = z_after[live].reshape(n, k)
    assert np.array_equal(Z.view(np.int64), ref.view(np.int64)), (n, bs, k, layout, fused)
    if fused:
        h = dout.cpu().numpy()
        assert (h[:2] == GUARD).all() and (h[-2:] == GUARD).all()
        out = h[2:-2].copy()
    return (tr, pr, ldr), (tz, pz, ldz), R, Z, out


def check_sums(torch, dev, n, k, rd, zd, R, Z, out):
    """out against spmv_dot_multi(R, Z) and (R, R), bit for bit, and against
    the longdouble sums within the dot product's bound."""
    (_, pr, ldr), (_, pz, ldz) = rd, zd
    rz = _dot(torch, dev, n, k, pr, ldr, pz, ldz)
    rr = _dot(torch, dev, n, k, pr, ldr, pr, ldr)
    assert np.array_equal(out[:k].view(np.int64), rz.view(np.int64)), (n, k, "r.z")
    assert np.array_equal(out[k:].view(np.int64), rr.view(np.int64)), (n, k, "r.r")
    Rl, Zl = R.astype(np.longdouble), Z.astype(np.longdouble)
    for got, prod in ((out[:k], Rl * Zl), (out[k:], Rl * Rl)):
        err = np.abs(got.astype(np.longdouble) - prod.sum(axis=0))
        assert np.isfinite(got).all() and (err <= (n + 2) * U * np.abs(prod).sum(axis=0)).all(), (n, k)


@pytest.mark.parametrize("n", [67, 4097])
@pytest.mark.parametrize("bs", BSS)
def test_apply_and_apply_dot(torch_dev, bs, n):
    torch, dev = torch_dev
    M, inv = precond_for(dev, n, bs)
    for k in KS:
        for layout in LAYOUTS + (EVEN,):
            run_apply(torch, dev, M, inv, n, bs, k, layout, False)
            rd, zd, R, Z, out = run_apply(torch, dev, M, inv, n, bs, k, layout, True)
            check_sums(torch, dev, n, k, rd, zd, R, Z, out)


def test_apply_dot_past_the_block_cap(torch_dev):
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
    for layout in ("tight", "padded"):
        rd, zd, R, Z, out = run_apply(torch, dev, M, inv, n, bs, k, layout, True)
        check_sums(torch, dev, n, k, rd, zd, R, Z, out)


def test_apply_empty_and_python_wrappers(torch_dev):
    torch, dev = torch_dev
    M0 = sa.BlockJacobi.from_coo(dominant(0), 3, dev)
    out = torch.full((4,), float("nan"), dtype=torch.float64, device=dev)
    e = torch.zeros(0, 2, dtype=torch.float64, device=dev)
    M0.apply(e, e.clone())
    M0.apply_dot(e, e.clone(), out, M0.ws(0, 2))
    assert (out.cpu().numpy() == 0.0).all() and not np.signbit(out.cpu().numpy()).any()  # n == 0 writes 2k zeros
    n, bs = 67, 4
    M, inv = precond_for(dev, n, bs)
    Rh = np.ascontiguousarray(_host_block(n, 5)[:n, :3])
    ref = np.empty_like(Rh)
    sa.cpu_bjacobi_apply_multi(n, bs, inv, Rh, ref)
    R = torch.from_numpy(Rh).to(dev)
    Z = torch.zeros_like(R)
    M.apply(R, Z)
    assert np.array_equal(Z.cpu().numpy().view(np.int64), ref.view(np.int64))
    r1, z1 = R[:, 0].contiguous(), torch.zeros(n, dtype=torch.float64, device=dev)  # 1-D: k = 1, ld = 1
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    M.apply_dot(r1, z1, out, M.ws(n, 1))
    assert np.array_equal(z1.cpu().numpy().view(np.int64), np.ascontiguousarray(ref[:, 0]).view(np.int64))


def test_refusals(torch_dev):
    torch, dev = torch_dev
    lib = sa.hip_lib()
    n, bs, k = 4097, 3, 3
    M, _ = precond_for(dev, n, bs)
    R = torch.ones(n, k, dtype=torch.float64, device=dev)
    Z = torch.full((n, k), 7.0, dtype=torch.float64, device=dev)
    out = torch.full((2 * k,), 7.0, dtype=torch.float64, device=dev)
    need = lib.spmv_bjacobi_ws_bytes(n, k)
    assert need == 2 * lib.spmv_dot_multi_ws_bytes(n, k)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s = _stream(torch, dev)
    P = sa._ptr
    h = M.handle
    assert lib.spmv_bjacobi_apply_dot_multi(h, k, P(R), k, P(Z), k, P(out), P(ws), need - 8, s) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_apply_dot_multi(h, k, P(R), k, P(Z), k, P(out), None, need, s) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_apply_dot_multi(h, 0, P(R), k, P(Z), k, P(out), P(ws), need, s) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_apply_dot_multi(h, k, P(R), k - 1, P(Z), k, P(out), P(ws), need, s) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_apply_dot_multi(h, k, P(R), k, P(Z), k - 1, P(out), P(ws), need, s) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_apply_dot_multi(h, k, P(R), k, P(Z), k, None, P(ws), need, s) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_apply_dot_multi(h, k, None, k, P(Z), k, P(out), P(ws), need, s) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_apply_multi(h, 0, P(R), k, P(Z), k, s) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_apply_multi(h, k, P(R), k - 1, P(Z), k, s) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_apply_multi(h, k, P(R), k, None, k, s) == sa.OTHER_ERROR
    torch.cuda.synchronize()
    assert (Z == 7.0).all() and (out == 7.0).all()  # the refused calls wrote nothing
    with pytest.raises(sa.SpmvError):
        M.apply(R, Z[:, :2])
    with pytest.raises(sa.SpmvError):
        M.apply(R.float(), Z)
    with pytest.raises(sa.SpmvError):
        M.apply(R[:100], Z)
    with pytest.raises(sa.SpmvError):
        M.apply_dot(R, Z, out[:3], ws)
    for bad in (0, 17):
        with pytest.raises(sa.SpmvError):
            sa.BlockJacobi.from_coo(dominant(67), bad, dev)
        with pytest.raises(sa.SpmvError):
            it.build_operator(dominant(67), 0, 1, "csr", dev, bjacobi=bad)


# -------------------------------------------------------------------- solves
GRID, B_NODE = 20, 3


@pytest.fixture(scope="module")
def case():
    m = block_congruence(GRID, B_NODE)
    B = rhs(m.n_rows, 4)  # ones, uniform - 0.5, e_0, zeros
    B.setflags(write=False)
    return m, lower_half(m), scipy_csr(m), B, numpy_pcg_count(m, B, B_NODE)


def _operator(case, dev, kind, bjacobi=B_NODE):
    m, half = case[0], case[1]
    if kind in ("fused", "expand"):
        return it.build_operator(half, 0, 1, "csr", dev, align=64, symmetric=kind, bjacobi=bjacobi)
    return it.build_operator(m, 0, 1, kind, dev, align=64, bjacobi=bjacobi)


def _check_true_residual(A, B, X):
    assert np.isfinite(X).all()
    for j in range(B.shape[1]):
        nb = np.linalg.norm(B[:, j])
        res = np.linalg.norm(B[:, j] - A @ X[:, j])
        print(f"column {j}: true residual {res:.3g} against {2e-10 * nb:.3g}")
        assert res <= 2e-10 * nb, (j, res, nb)


@pytest.mark.parametrize("kind", ["csr", "sell", "ell", "expand", "fused"])
def test_pcg_solves(torch_dev, case, kind):
    torch, dev = torch_dev
    _, _, A, B, N = case
    assert N == 78
    op = _operator(case, dev, kind)
    assert op.precond.info()["singular_blocks"] == 0 and op.precond.info()["symmetric_half"] == (kind in ("fused", "expand"))
    Bd = torch.from_numpy(B.copy()).to(dev)
    X, its, rel = it.cg_multi(op, Bd, tol=TOL, maxit=10 * N, check_every=CHECK_EVERY)
    X = X.cpu().numpy()
    print(f"{kind}: cg_multi {its} iterations (N = {N}), rel {rel}")
    assert its <= N + CHECK_EVERY + N // 10
    assert rel.shape == (4,) and (rel <= TOL).all() and rel[3] == 0.0
    assert (X[:, 3] == 0.0).all() and not np.signbit(X[:, 3]).any()  # the zero column: exactly 0
    _check_true_residual(A, B, X)
    N1 = numpy_pcg_count(case[0], B[:, 1:2], B_NODE)
    x, its, rel1 = it.cg(op, Bd[:, 1].contiguous(), tol=TOL, maxit=10 * N, check_every=CHECK_EVERY)
    print(f"{kind}: cg {its} iterations (N = {N1}), rel {rel1}")
    assert its <= N1 + CHECK_EVERY + N1 // 10 and rel1 <= TOL
    _check_true_residual(A, B[:, 1:2], x.cpu().numpy()[:, None])
    # no preconditioner: 4 N iterations are far from enough
    _, its, rel = it.cg_multi(op, Bd, tol=TOL, maxit=4 * N, check_every=CHECK_EVERY, precond=False)
    assert its == 4 * N and not (rel <= TOL).all()
    _, its, rel1 = it.cg(op, Bd[:, 1].contiguous(), tol=TOL, maxit=4 * N, check_every=CHECK_EVERY, precond=False)
    assert its == 4 * N and rel1 > TOL


@pytest.mark.parametrize("kind", ["csr", "expand"])
def test_pcg_column_bits(torch_dev, case, kind):
    """A column's iterates do not depend on the columns solved with it."""
    torch, dev = torch_dev
    n = case[0].n_rows
    op = _operator(case, dev, kind)
    B = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (n, 5))).to(dev)
    X = it.cg_multi(op, B, tol=0.0, maxit=25)[0].clone()
    X2 = it.cg_multi(op, B, tol=0.0, maxit=25)[0].clone()
    assert torch.equal(X.view(torch.int64), X2.view(torch.int64))
    assert torch.isfinite(X).all() and (X != 0.0).any()
    for j in range(5):
        xj = it.cg_multi(op, B[:, j:j + 1].contiguous(), tol=0.0, maxit=25)[0]
        assert torch.equal(xj[:, 0].view(torch.int64), X[:, j].contiguous().view(torch.int64)), j


def test_pcg_side_stream_same_bits(torch_dev, case):
    torch, dev = torch_dev
    n = case[0].n_rows
    B = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (n, 3))).to(dev)
    X1 = it.cg_multi(_operator(case, dev, "csr"), B, tol=0.0, maxit=25)[0].clone()
    x1 = it.cg(_operator(case, dev, "csr"), B[:, 0].contiguous(), tol=0.0, maxit=25)[0].clone()
    op = _operator(case, dev, "csr")
    op.kernels.stream = torch.cuda.Stream(dev)
    X2, its, rel = it.cg_multi(op, B, tol=0.0, maxit=25)
    x2 = it.cg(op, B[:, 0].contiguous(), tol=0.0, maxit=25)[0]
    torch.cuda.synchronize()
    assert its == 25 and np.isfinite(rel).all()
    assert torch.equal(X1.view(torch.int64), X2.view(torch.int64))
    assert torch.equal(x1.view(torch.int64), x2.view(torch.int64))


def test_unpreconditioned_solvers_keep_their_bits(torch_dev, case):
    """precond=False on an operator with a preconditioner is the solver of an
    operator without one, bit for bit."""
    torch, dev = torch_dev
    n = case[0].n_rows
    B = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (n, 3))).to(dev)
    bare = _operator(case, dev, "csr", bjacobi=None)
    assert bare.precond is None
    op = _operator(case, dev, "csr")
    X0 = it.cg_multi(bare, B, tol=0.0, maxit=25)[0].clone()
    X1 = it.cg_multi(op, B, tol=0.0, maxit=25, precond=False)[0].clone()
    assert torch.equal(X0.view(torch.int64), X1.view(torch.int64))
    x0 = it.cg(bare, B[:, 0].contiguous(), tol=0.0, maxit=25)[0].clone()
    x1 = it.cg(op, B[:, 0].contiguous(), tol=0.0, maxit=25, precond=False)[0].clone()
    assert torch.equal(x0.view(torch.int64), x1.view(torch.int64))
    # and a preconditioner given by keyword is the operator's own
    X2 = it.cg_multi(bare, B, tol=0.0, maxit=25, precond=op.precond)[0].clone()
    X3 = it.cg_multi(op, B, tol=0.0, maxit=25)[0].clone()
    assert torch.equal(X2.view(torch.int64), X3.view(torch.int64)) and not torch.equal(X2, X0)
