"""Multi-right-hand-side CG on the MI355X through libspmv_hip: the block
vector kernels (csrc/vec_multi.hip) and iterate.cg_multi.

Bounds.  dot_multi: n rounded products summed in any order,
|out - ref| <= (n + 2) 2^-53 sum |a b| against an np.longdouble column sum
(the project's textbook bound, no measured constant).  The ratio updates:
one rounding each for the quotient, the product and the sum, plus one ulp of
slack for the device quotient: 4 2^-53 (|y| + |c x|).  CG: the true residual
against scipy within twice the recurrence tolerance, as
test_cg_laplacian_residual.
"""
from __future__ import annotations

import numpy as np
import pytest
import scipy.sparse as sp

import iterate as it
import spmv_amd as sa
from iterate_double import laplacian_2d

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 5, 8, 9, 17)
LAYOUTS = ("tight", "padded")  # ld = k at the tensor base; ld = k + 3, one element into a larger buffer
EVEN = "even"  # ld = k + 2 at the tensor base: the 16-byte path with ld > k when k is even
U = 2.0 ** -53
GUARD = -7.25e300  # sentinel around every buffer the kernels write


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch, torch.device("cuda:0")


_blocks = {}


def _host_block(n, seed):
    """(max(n, 1), 17) uniform(-1, 1) without zeros; made once, never changed."""
    key = (n, seed)
    if key not in _blocks:
        a = np.random.default_rng(1000 * seed + n % 997).uniform(-1.0, 1.0, (max(n, 1), max(KS)))
        a[a == 0.0] = 0.5
        a.setflags(write=False)
        _blocks[key] = a
    return _blocks[key]


def _place(torch, dev, host, n, k, layout, fill_seed):
    """The first k columns of `host` on the device in `layout`.  Returns
    (whole buffer, address of element [0, 0], ld, live mask over the buffer):
    the buffer starts and ends with GUARD and holds two rows past n; padding
    columns and extra rows hold random values."""
    ld = {"tight": k, "padded": k + 3, EVEN: k + 2}[layout]
    off = 1 if layout == "padded" else 0
    rows = n + 2
    buf = np.random.default_rng(fill_seed).uniform(-1.0, 1.0, off + rows * ld + 2)
    body = buf[off:off + rows * ld].reshape(rows, ld)
    body[:n, :k] = host[:n, :k]
    mask = np.zeros(buf.shape, bool)
    mask[off:off + rows * ld].reshape(rows, ld)[:n, :k] = True
    if off:
        buf[0] = GUARD
    buf[-2:] = GUARD
    t = torch.from_numpy(buf).to(dev)
    return t, t.data_ptr() + 8 * off, ld, mask


def _stream(torch, dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _dot(torch, dev, n, k, pa, lda, pb, ldb):
    """One spmv_dot_multi into a NaN-filled, guarded out; returns out (k,)."""
    lib = sa.hip_lib()
    ws = torch.empty(lib.spmv_dot_multi_ws_bytes(n, k), dtype=torch.uint8, device=dev)
    out = torch.full((k + 4,), float("nan"), dtype=torch.float64, device=dev)
    out[:2] = GUARD
    out[-2:] = GUARD
    rc = lib.spmv_dot_multi(n, k, pa, lda, pb, ldb, out.data_ptr() + 16, sa._ptr(ws), ws.numel(), 0,
                            _stream(torch, dev))
    assert rc == 0, lib.spmv_last_error().decode()
    h = out.cpu().numpy()
    assert (h[:2] == GUARD).all() and (h[-2:] == GUARD).all()
    return h[2:-2].copy()


# ------------------------------------------------------------------ dot_multi
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [0, 1, 255, 4097, 300_001])
def test_dot_multi_values(torch_dev, n, layout):
    torch, dev = torch_dev
    a, b = _host_block(n, 1), _host_block(n, 2)
    for k in KS:
        ta, pa, lda, _ = _place(torch, dev, a, n, k, layout, 11)
        tb, pb, ldb, _ = _place(torch, dev, b, n, k, layout, 12)
        before = (ta.clone(), tb.clone())
        out = _dot(torch, dev, n, k, pa, lda, pb, ldb)
        prod = a[:n, :k].astype(np.longdouble) * b[:n, :k].astype(np.longdouble)
        ref, mag = prod.sum(axis=0), np.abs(prod).sum(axis=0)
        err = np.abs(out.astype(np.longdouble) - ref)
        bound = (n + 2) * U * mag
        print(f"n={n} k={k} {layout}: max err/bound {float(np.max(err / np.maximum(bound, 1e-300))):.3g}")
        assert np.isfinite(out).all() and (err <= bound).all(), (n, k, layout, err, bound)
        if n == 0:
            assert (out == 0.0).all() and not np.signbit(out).any()
        assert torch.equal(ta, before[0]) and torch.equal(tb, before[1])  # inputs untouched


@pytest.mark.parametrize("k,layout", [(17, "padded"), (8, "tight"), (6, "padded"), (2, "tight"), (6, EVEN), (16, EVEN)])
@pytest.mark.parametrize("n", [4097, 300_001])
def test_dot_multi_bits(torch_dev, n, k, layout):
    """Column j of a k-wide call (k = 17, ld = 20, one element off the base:
    the 8-byte path; k = 8 and 2 at the base, k = 6 and 16 with ld = k + 2:
    the 16-byte path) equals the k = 1 call on a contiguous copy of that
    column bit for bit, and a second identical call gives the same bits."""
    torch, dev = torch_dev
    a, b = _host_block(n, 1), _host_block(n, 2)
    ta, pa, lda, _ = _place(torch, dev, a, n, k, layout, 11)
    tb, pb, ldb, _ = _place(torch, dev, b, n, k, layout, 12)
    wide = _dot(torch, dev, n, k, pa, lda, pb, ldb)
    again = _dot(torch, dev, n, k, pa, lda, pb, ldb)
    assert np.array_equal(wide.view(np.int64), again.view(np.int64))
    for j in range(k):
        ca = torch.from_numpy(np.ascontiguousarray(a[:n, j])).to(dev)
        cb = torch.from_numpy(np.ascontiguousarray(b[:n, j])).to(dev)
        one = _dot(torch, dev, n, 1, ca.data_ptr(), 1, cb.data_ptr(), 1)
        assert one.view(np.int64)[0] == wide.view(np.int64)[j], (n, k, j)


def test_dot_multi_refusals(torch_dev):
    torch, dev = torch_dev
    lib = sa.hip_lib()
    n, k = 5000, 3
    a = torch.ones(n, k, dtype=torch.float64, device=dev)
    out = torch.zeros(k, dtype=torch.float64, device=dev)
    need = lib.spmv_dot_multi_ws_bytes(n, k)
    assert need >= 8 * k and lib.spmv_dot_multi_ws_bytes(n, 1) * k == need
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s = _stream(torch, dev)
    args = lambda k_, ld, nbytes: (n, k_, sa._ptr(a), ld, sa._ptr(a), k, sa._ptr(out), sa._ptr(ws), nbytes, 0, s)  # noqa: E731
    assert lib.spmv_dot_multi(*args(k, k, need)) == 0
    assert lib.spmv_dot_multi(*args(k, k, need - 8)) == sa.OTHER_ERROR  # workspace one double short
    assert lib.spmv_dot_multi(*args(0, k, need)) == sa.OTHER_ERROR  # k = 0
    assert lib.spmv_dot_multi(*args(k, k - 1, need)) == sa.OTHER_ERROR  # lda < k
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == n).all()  # the refused calls wrote nothing


# ---------------------------------------------------------------- the updates
def _update(torch, dev, what, n, k, layout, num, den, sign=1.0):
    """Runs one update; returns (x, y0, y1) live parts as numpy (n, k) after
    checking that nothing outside Y's live part changed, X included."""
    lib = sa.hip_lib()
    x, y = _host_block(n, 3), _host_block(n, 4)
    tx, px, ldx, _ = _place(torch, dev, x, n, k, layout, 13)
    ty, py, ldy, live = _place(torch, dev, y, n, k, layout, 14)
    x_before, y_before = tx.cpu().numpy(), ty.cpu().numpy()
    dn = torch.from_numpy(np.asarray(num, np.float64)).to(dev)
    dd = torch.from_numpy(np.asarray(den, np.float64)).to(dev)
    if what == "axpy":
        rc = lib.spmv_axpy_ratio_multi(n, k, sa._ptr(dn), sa._ptr(dd), sign, px, ldx, py, ldy, 0, _stream(torch, dev))
    else:
        rc = lib.spmv_xpay_ratio_multi(n, k, sa._ptr(dn), sa._ptr(dd), px, ldx, py, ldy, 0, _stream(torch, dev))
    assert rc == 0, lib.spmv_last_error().decode()
    y_after = ty.cpu().numpy()
    assert np.array_equal(tx.cpu().numpy().view(np.int64), x_before.view(np.int64))
    assert np.array_equal(y_after.view(np.int64)[~live], y_before.view(np.int64)[~live])  # padding, rows >= n, guards
    return x[:n, :k], y[:n, :k], y_after[live].reshape(n, k)


@pytest.mark.parametrize("n,layout", [(4097, "tight"), (4097, "padded"), (4097, EVEN), (300_001, "tight"),
                                      (300_001, "padded")])
def test_ratio_updates(torch_dev, n, layout):
    torch, dev = torch_dev
    rng = np.random.default_rng(5)
    for k in KS:
        num = rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)
        den = rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)
        x, y0, y1 = _update(torch, dev, "axpy", n, k, layout, num, den, -1.0)
        c = -1.0 * (num / den)
        assert (np.abs(y1 - (y0 + c * x)) <= 4 * U * (np.abs(y0) + np.abs(c * x))).all(), ("axpy", n, k, layout)
        x, y0, y1 = _update(torch, dev, "xpay", n, k, layout, num, den)
        c = num / den
        assert (np.abs(y1 - (x + c * y0)) <= 4 * U * (np.abs(x) + np.abs(c * y0))).all(), ("xpay", n, k, layout)


def test_ratio_updates_same_bits_in_every_layout(torch_dev):
    """An element's result depends on its inputs and c_j only: the contiguous
    block, the padded 8-byte path and the padded 16-byte path agree bit for
    bit (n * k odd for odd k: the contiguous block's last element included)."""
    torch, dev = torch_dev
    n = 4097
    rng = np.random.default_rng(6)
    for k in KS:
        num, den = rng.uniform(0.5, 2.0, k), rng.uniform(-2.0, -0.5, k)
        for what in ("axpy", "xpay"):
            got = [_update(torch, dev, what, n, k, layout, num, den, -1.0)[2] for layout in LAYOUTS + (EVEN,)]
            assert np.array_equal(got[0].view(np.int64), got[1].view(np.int64)), (what, k)
            assert np.array_equal(got[0].view(np.int64), got[2].view(np.int64)), (what, k)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_ratio_updates_zero_denominator(torch_dev, layout):
    """den[j] == 0 gives the ratio 0: axpy leaves column j as it was, xpay
    makes it X's column; no NaN, and the other columns get their update."""
    torch, dev = torch_dev
    n = 4097
    for k in KS:
        j = k - 1
        num = np.full(k, 3.0)
        den = np.full(k, 7.0)
        den[j] = 0.0
        if k > 2:
            num[0], den[0] = 0.0, -0.0  # 0 / -0 as well
        zero = den == 0.0
        x, y0, y1 = _update(torch, dev, "axpy", n, k, layout, num, den, 1.0)
        assert np.isfinite(y1).all() and np.array_equal(y1[:, zero], y0[:, zero])
        c = 3.0 / 7.0
        assert (np.abs(y1 - (y0 + c * x)) <= 4 * U * (np.abs(y0) + np.abs(c * x)))[:, ~zero].all()
        x, y0, y1 = _update(torch, dev, "xpay", n, k, layout, num, den)
        assert np.isfinite(y1).all() and np.array_equal(y1[:, zero], x[:, zero])
        assert (np.abs(y1 - (x + c * y0)) <= 4 * U * (np.abs(x) + np.abs(c * y0)))[:, ~zero].all()


def test_update_refusals(torch_dev):
    torch, dev = torch_dev
    lib = sa.hip_lib()
    n, k = 100, 3
    x = torch.ones(n, k, dtype=torch.float64, device=dev)
    y = torch.ones(n, k, dtype=torch.float64, device=dev)
    c = torch.ones(k, dtype=torch.float64, device=dev)
    s = _stream(torch, dev)
    P = sa._ptr
    assert lib.spmv_axpy_ratio_multi(n, 0, P(c), P(c), 1.0, P(x), k, P(y), k, 0, s) == sa.OTHER_ERROR
    assert lib.spmv_axpy_ratio_multi(n, k, P(c), P(c), 1.0, P(x), k - 1, P(y), k, 0, s) == sa.OTHER_ERROR
    assert lib.spmv_xpay_ratio_multi(n, k, P(c), P(c), P(x), k, P(y), k - 1, 0, s) == sa.OTHER_ERROR
    assert lib.spmv_xpay_ratio_multi(n, k, None, P(c), P(x), k, P(y), k, 0, s) == sa.OTHER_ERROR
    torch.cuda.synchronize()
    assert (y == 1.0).all()


# ------------------------------------------------------------------- cg_multi
GRID = 60


@pytest.fixture(scope="module")
def lap():
    """laplacian_2d(60): the matrix, its lower triangle, scipy's copy and the
    four right-hand sides (ones, uniform - 0.5, e_0, zeros)."""
    m = laplacian_2d(GRID)
    n = m.n_rows
    low = m.row >= m.col
    half = sa.Coo(n, n, m.row[low], m.col[low], m.val[low], True, "laplacian lower")
    A = sp.csr_matrix((m.val, (m.row, m.col)), shape=(n, n))
    B = np.zeros((n, 4))
    B[:, 0] = 1.0
    B[:, 1] = np.random.default_rng(7).random(n) - 0.5
    B[0, 2] = 1.0
    B.setflags(write=False)
    return m, half, A, B


def _operator(lap, dev, kind):
    m, half = lap[0], lap[1]
    if kind in ("fused", "expand"):
        return it.build_operator(half, 0, 1, "csr", dev, align=64, symmetric=kind)
    return it.build_operator(m, 0, 1, kind, dev, align=64)


def _check_true_residual(A, B, X):
    assert np.isfinite(X).all()
    for j in range(B.shape[1]):
        nb = np.linalg.norm(B[:, j])
        res = np.linalg.norm(B[:, j] - A @ X[:, j])
        print(f"column {j}: true residual {res:.3g} against {2e-10 * nb:.3g}")
        assert res <= 2e-10 * nb, (j, res, nb)


@pytest.mark.parametrize("kind", ["csr", "sell", "ell", "expand", "fused"])
def test_cg_multi_solves(torch_dev, lap, kind):
    torch, dev = torch_dev
    _, _, A, B = lap
    op = _operator(lap, dev, kind)
    X, its, rel = it.cg_multi(op, torch.from_numpy(B.copy()).to(dev), tol=1e-10, maxit=2000)
    X = X.cpu().numpy()
    print(f"{kind}: {its} iterations, rel {rel}")
    assert its < 2000
    assert rel.shape == (4,) and (rel <= 1e-10).all() and rel[3] == 0.0
    assert (X[:, 3] == 0.0).all() and not np.signbit(X[:, 3]).any()  # the zero column: exactly 0
    _check_true_residual(A, B, X)


def test_cg_multi_past_underflow(torch_dev, lap):
    """tol = 0 for 3000 iterations: residuals underflow to exactly 0 and the
    den == 0 rule keeps every column finite (0/0 otherwise)."""
    torch, dev = torch_dev
    _, _, A, B = lap
    op = _operator(lap, dev, "csr")
    X, its, rel = it.cg_multi(op, torch.from_numpy(B.copy()).to(dev), tol=0.0, maxit=3000)
    print(f"{its} iterations, rel {rel}")
    assert np.isfinite(rel).all()
    _check_true_residual(A, B, X.cpu().numpy())


@pytest.mark.parametrize("kind", ["csr", "expand"])
def test_cg_multi_column_bits(torch_dev, lap, kind):
    """A column's iterates do not depend on the columns solved with it."""
    torch, dev = torch_dev
    n = lap[0].n_rows
    op = _operator(lap, dev, kind)
    B = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (n, 5))).to(dev)
    X = it.cg_multi(op, B, tol=0.0, maxit=25)[0].clone()
    X2 = it.cg_multi(op, B, tol=0.0, maxit=25)[0].clone()
    assert torch.equal(X.view(torch.int64), X2.view(torch.int64))
    assert torch.isfinite(X).all() and (X != 0.0).any()
    for j in range(5):
        xj = it.cg_multi(op, B[:, j:j + 1].contiguous(), tol=0.0, maxit=25)[0]
        assert torch.equal(xj[:, 0].view(torch.int64), X[:, j].contiguous().view(torch.int64)), j


def test_cg_on_symmetric_operator(torch_dev, lap):
    """The existing single-vector CG on an operator built on the stored half
    (test_cg_laplacian_residual's two bounds)."""
    torch, dev = torch_dev
    _, _, A, _ = lap
    n = A.shape[0]
    op = _operator(lap, dev, "expand")
    x, its, rel = it.cg(op, torch.ones(n, dtype=torch.float64, device=dev), tol=1e-10, maxit=2000, check_every=10)
    assert rel <= 1e-10 and its < 2000
    assert np.linalg.norm(1.0 - A @ x.cpu().numpy()) <= 2e-10 * np.sqrt(n)


def test_cg_multi_side_stream_same_bits(torch_dev, lap):
    torch, dev = torch_dev
    n = lap[0].n_rows
    B = torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (n, 3))).to(dev)
    X1 = it.cg_multi(_operator(lap, dev, "csr"), B, tol=0.0, maxit=25)[0].clone()
    op = _operator(lap, dev, "csr")
    op.kernels.stream = torch.cuda.Stream(dev)
    X2, its, rel = it.cg_multi(op, B, tol=0.0, maxit=25)
    torch.cuda.synchronize()
    assert its == 25 and np.isfinite(rel).all()
    assert torch.equal(X1.view(torch.int64), X2.view(torch.int64))


def test_cg_multi_refusals(torch_dev, lap):
    torch, dev = torch_dev
    m, half = lap[0], lap[1]
    n = m.n_rows
    good = torch.ones(n, 2, dtype=torch.float64, device=dev)
    with pytest.raises(sa.SpmvError):  # COO has no multi-vector run
        it.cg_multi(it.build_operator(m, 0, 1, "coo", dev, align=64), good)
    with pytest.raises(sa.SpmvError):
        it.cg_multi(it.build_operator(m, 0, 1, "csr", dev, align=64, split=True), good)
    op = _operator(lap, dev, "csr")
    for bad in (torch.ones(n, dtype=torch.float64, device=dev), torch.ones(n, 2, dtype=torch.float32, device=dev),
                torch.ones(n, 2, dtype=torch.float64)):  # 1-D, float32, on the host
        with pytest.raises(sa.SpmvError):
            it.cg_multi(op, bad)
    with pytest.raises(sa.SpmvError):
        it.build_operator(half, 0, 1, "sell", dev, symmetric="fused")
    with pytest.raises(sa.SpmvError):
        it.build_operator(half, 0, 1, "csr", dev, symmetric="expand", expand_symmetric=True)
