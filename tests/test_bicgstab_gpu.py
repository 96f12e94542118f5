"""BiCGSTAB on the MI355X through libspmv_hip: the three fused block vector
kernels (spmv_dot2_multi, spmv_bicgstab_update_dot_multi,
spmv_bicgstab_dir_multi; csrc/vec_multi.hip) and iterate.bicgstab /
iterate.bicgstab_multi.

Rules.  Every element the two updates write has the bits of the host statements
(spmv_cpu_bicgstab_update_multi, spmv_cpu_bicgstab_dir_multi); nothing else in
a buffer changes (guards, padding columns, rows past n).  The sums of the dot
forms have the bits of spmv_dot_multi on the same operands and meet its bound
against np.longdouble, (n + 2) 2^-53 sum |a b| (tests/test_thresholds_gpu.py).
Solves: tests/iterate_bicgstab_double.py has the matrices, the right-hand
sides and the bound REL_BOUND with its reasons.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import iterate as it
import spmv_amd as sa
from iterate_bicgstab_double import CASES, REL_BOUND, TOL, rhs, scipy_csr, true_rel, upwind

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
GUARD = -7.25e300
NS = (1, 255, 256, 257, 1023, 1024, 1025, 2049, 5000)
KS = (1, 2, 3, 4, 5, 8, 9, 17)
# name -> (ld - k, elements between the 16-byte aligned base and element [0, 0])
LAYOUTS = {"tight": (0, 0), "tight+8": (0, 1), "padded": (3, 0), "padded+8": (3, 1), "even": (2, 0)}
MAXIT = 400


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch, torch.device("cuda:0")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _stream(torch, dev):
    return torch.cuda.current_stream(dev).cuda_stream


@functools.lru_cache(maxsize=None)
def host_block(rows, seed, cols=max(KS)):
    """(rows, cols) uniform(-1, 1) without zeros; made once, never changed."""
    a = np.random.default_rng(7000 + seed).uniform(-1.0, 1.0, (rows, cols))
    a[a == 0.0] = 0.5
    a.setflags(write=False)
    return a


class Placed:
    """The first k columns of `host` on the device in a layout: a buffer that
    begins (when off > 0) and ends with GUARD and holds two rows past n;
    padding columns and the extra rows hold random values."""

    def __init__(self, torch, dev, host, n, k, layout, fill_seed):
        extra, off = LAYOUTS[layout] if isinstance(layout, str) else layout
        self.n, self.k, self.ld = n, k, k + extra
        rows = n + 2
        buf = np.random.default_rng(fill_seed).uniform(-1.0, 1.0, off + rows * self.ld + 2)
        self.span = slice(off, off + rows * self.ld)
        buf[self.span].reshape(rows, self.ld)[:n, :k] = host[:n, :k]
        buf[:off] = GUARD
        buf[-2:] = GUARD
        self.before = buf
        self.t = torch.from_numpy(buf).to(dev)
        self.ptr = self.t.data_ptr() + 8 * off
        assert self.t.data_ptr() % 16 == 0

    def live(self, h):
        return h[self.span].reshape(self.n + 2, self.ld)[: self.n, : self.k]

    def after(self, expect=None):
        """The live part now, after checking that everything else (and, with
        expect None, the live part too) kept its bits."""
        h = self.t.cpu().numpy()
        want = self.before.copy()
        if expect is not None:
            self.live(want)[...] = expect
        assert same_bits(h, want), "an element outside the rule changed, or a live one has other bits"
        return self.live(h).copy()


def _dev(torch, dev, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _out(torch, dev, count):
    out = torch.full((count + 4,), float("nan"), dtype=torch.float64, device=dev)
    out[:2] = GUARD
    out[-2:] = GUARD
    return out


def _out_live(out):
    h = out.cpu().numpy()
    assert (h[:2] == GUARD).all() and (h[-2:] == GUARD).all()
    return h[2:-2].copy()


def _ws(torch, dev, n, k):
    return torch.empty(sa.hip_lib().spmv_dot_multi_ws_bytes(n, 2 * k), dtype=torch.uint8, device=dev)


def _dot(torch, dev, n, k, a, b):
    """spmv_dot_multi of two Placed blocks -> (k,) host."""
    lib = sa.hip_lib()
    ws = _ws(torch, dev, n, k)
    out = _out(torch, dev, k)
    rc = lib.spmv_dot_multi(n, k, a.ptr, a.ld, b.ptr, b.ld, out.data_ptr() + 16, sa._ptr(ws), ws.numel(), 0,
                            _stream(torch, dev))
    assert rc == 0, lib.spmv_last_error().decode()
    return _out_live(out)


def _dot_bound_ok(got, a, b):
    """(n + 2) 2^-53 sum |a b| against the longdouble column sums, in slices."""
    n, k = a.shape
    ref, mag = np.zeros(k, LD), np.zeros(k, LD)
    for lo in range(0, n, 1 << 20):
        prod = a[lo:lo + (1 << 20)].astype(LD) * b[lo:lo + (1 << 20)].astype(LD)
        ref += prod.sum(axis=0)
        mag += np.abs(prod).sum(axis=0)
    err = np.abs(got.astype(LD) - ref)
    assert np.isfinite(got).all() and (err <= (n + 2) * U * mag).all(), (n, k, err, (n + 2) * U * mag)


def _scalars(seed, k, zero_first=False, zero_last=False):
    """Four (k,) arrays: num, den, num, den, none zero unless asked."""
    rng = np.random.default_rng(seed)
    s = [rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k) for _ in range(4)]
    if zero_first:
        s[1][0] = 0.0
    if zero_last:
        s[3][-1] = 0.0
    return s


# ---------------------------------------------------------------- the kernels
def run_update(torch, dev, n, k, layouts, alias, scal, blocks=None, check_bound=True):
    """One spmv_bicgstab_update_dot_multi against the host statement and
    spmv_dot_multi.  layouts: one name, or six (Ph, Sh, T, R0, X, R)."""
    lib = sa.hip_lib()
    if isinstance(layouts, str):
        layouts = (layouts,) * 6
    hosts = blocks or [host_block(max(NS), s) for s in range(1, 7)]
    Ph, Sh, T, R0, X, R = (Placed(torch, dev, h, n, k, lay, 20 + i)
                           for i, (h, lay) in enumerate(zip(hosts, layouts)))
    if alias:
        Sh = R
    ds = [_dev(torch, dev, s) for s in scal]
    ws = _ws(torch, dev, n, k)
    out = _out(torch, dev, 2 * k)
    rc = lib.spmv_bicgstab_update_dot_multi(n, k, *(sa._ptr(d) for d in ds), Ph.ptr, Ph.ld, Sh.ptr, Sh.ld, T.ptr, T.ld,
                                            R0.ptr, R0.ld, X.ptr, X.ld, R.ptr, R.ld, out.data_ptr() + 16, sa._ptr(ws),
                                            ws.numel(), 0, _stream(torch, dev))
    assert rc == 0, lib.spmv_last_error().decode()
    torch.cuda.synchronize()
    hx, hr = (np.ascontiguousarray(h[:n, :k]).copy() for h in (hosts[4], hosts[5]))
    hsh = hr if alias else np.ascontiguousarray(hosts[1][:n, :k])
    if n > 0:
        sa.cpu_bicgstab_update_multi(n, *scal, np.ascontiguousarray(hosts[0][:n, :k]), hsh,
                                     np.ascontiguousarray(hosts[2][:n, :k]), hx, hr, k=k)
    for blk in (Ph, T, R0) + (() if alias else (Sh,)):
        blk.after()
    X.after(hx)
    R.after(hr)
    sums = _out_live(out)
    assert same_bits(sums[:k], _dot(torch, dev, n, k, R0, R)) and same_bits(sums[k:], _dot(torch, dev, n, k, R, R))
    if check_bound:
        _dot_bound_ok(sums[:k], hosts[3][:n, :k], hr)
        _dot_bound_ok(sums[k:], hr, hr)
    for d, s in zip(ds, scal):
        assert same_bits(d.cpu().numpy(), s)
    return hx, hr, sums


def run_dir(torch, dev, n, k, layouts, scal, blocks=None):
    lib = sa.hip_lib()
    if isinstance(layouts, str):
        layouts = (layouts,) * 3
    hosts = blocks or [host_block(max(NS), s) for s in (7, 8, 9)]
    V, R, P = (Placed(torch, dev, h, n, k, lay, 30 + i) for i, (h, lay) in enumerate(zip(hosts, layouts)))
    ds = [_dev(torch, dev, s) for s in scal]
    rc = lib.spmv_bicgstab_dir_multi(n, k, *(sa._ptr(d) for d in ds), V.ptr, V.ld, R.ptr, R.ld, P.ptr, P.ld, 0,
                                     _stream(torch, dev))
    assert rc == 0, lib.spmv_last_error().decode()
    torch.cuda.synchronize()
    hp = np.ascontiguousarray(hosts[2][:n, :k]).copy()
    if n > 0:
        sa.cpu_bicgstab_dir_multi(n, *scal, np.ascontiguousarray(hosts[0][:n, :k]),
                                  np.ascontiguousarray(hosts[1][:n, :k]), hp, k=k)
    V.after()
    R.after()
    P.after(hp)
    return hp


def run_dot2(torch, dev, n, k, layouts, same, blocks=None, check_bound=True):
    lib = sa.hip_lib()
    if isinstance(layouts, str):
        layouts = (layouts,) * 3
    hosts = blocks or [host_block(max(NS), s) for s in (10, 11, 12)]
    A, B, C = (Placed(torch, dev, h, n, k, lay, 40 + i) for i, (h, lay) in enumerate(zip(hosts, layouts)))
    if same:
        C = A
    ws = _ws(torch, dev, n, k)
    out = _out(torch, dev, 2 * k)
    rc = lib.spmv_dot2_multi(n, k, A.ptr, A.ld, B.ptr, B.ld, C.ptr, C.ld, out.data_ptr() + 16, sa._ptr(ws), ws.numel(),
                             0, _stream(torch, dev))
    assert rc == 0, lib.spmv_last_error().decode()
    sums = _out_live(out)
    for blk in (A, B, C):
        blk.after()
    assert same_bits(sums[:k], _dot(torch, dev, n, k, A, B)) and same_bits(sums[k:], _dot(torch, dev, n, k, A, C))
    if check_bound:
        hc = hosts[0] if same else hosts[2]
        _dot_bound_ok(sums[:k], hosts[0][:n, :k], hosts[1][:n, :k])
        _dot_bound_ok(sums[k:], hosts[0][:n, :k], hc[:n, :k])
    return sums


@pytest.mark.parametrize("n", NS)
def test_update_dot_bits(torch_dev, n):
    torch, dev = torch_dev
    for k in KS:
        scal = _scalars(100 + k, k)
        for layout in LAYOUTS:
            for alias in (False, True):
                run_update(torch, dev, n, k, layout, alias, scal)
        # operands in different layouts: the 16-byte path needs every one of them
        run_update(torch, dev, n, k, ("tight", "even", "tight", "tight+8", "tight", "even"), False, scal)
        run_update(torch, dev, n, k, ("even", "even", "tight", "tight", "padded+8", "even"), True, scal)


@pytest.mark.parametrize("n", NS)
def test_dir_bits(torch_dev, n):
    torch, dev = torch_dev
    for k in KS:
        scal = _scalars(200 + k, k)
        for layout in LAYOUTS:
            run_dir(torch, dev, n, k, layout, scal)
        run_dir(torch, dev, n, k, ("tight", "even", "padded+8"), scal)


@pytest.mark.parametrize("n", NS)
def test_dot2_bits(torch_dev, n):
    torch, dev = torch_dev
    for k in KS:
        for layout in LAYOUTS:
            for same in (False, True):
                run_dot2(torch, dev, n, k, layout, same)
        run_dot2(torch, dev, n, k, ("tight", "tight+8", "even"), False)


def test_column_rule(torch_dev):
    """Column j of a wide update has the bits of the k = 1 call on that
    column, its two sums included."""
    torch, dev = torch_dev
    n, k = 2049, 17
    scal = _scalars(5, k)
    hosts = [host_block(max(NS), s) for s in range(1, 7)]
    X, R, sums = run_update(torch, dev, n, k, "padded+8", False, scal)
    for j in (0, 7, 8, 16):
        one = [np.ascontiguousarray(h[:, j:j + 1]) for h in hosts]
        x1, r1, s1 = run_update(torch, dev, n, 1, "tight", False, [s[j:j + 1].copy() for s in scal], blocks=one)
        assert same_bits(x1[:, 0], X[:, j]) and same_bits(r1[:, 0], R[:, j])
        assert same_bits(s1, sums[[j, k + j]])


@pytest.mark.parametrize("k", [1, 3, 8, 9])
def test_zero_denominators(torch_dev, k):
    """A zero denominator gives the ratio 0: nothing becomes NaN or Inf, the
    column stands still where the rule says so."""
    torch, dev = torch_dev
    n = 1025
    hosts = [host_block(max(NS), s) for s in range(1, 10)]
    for alias in (False, True):
        X, R, sums = run_update(torch, dev, n, k, "tight", alias, _scalars(9, k, True, True))
        assert np.isfinite(X).all() and np.isfinite(R).all() and np.isfinite(sums).all()
        assert same_bits(R[:, k - 1], hosts[5][:n, k - 1])  # omega = 0
        if k == 1:
            assert same_bits(X[:, 0], hosts[4][:n, 0])  # alpha = omega = 0
    rho, rv, tt, ts = _scalars(10, k)
    for zero in ("rv", "ts", "tt"):
        s = [a.copy() for a in (rho, rv, tt, ts)]
        s[{"rv": 1, "tt": 2, "ts": 3}[zero]][0] = 0.0
        P = run_dir(torch, dev, n, k, "tight", s)
        assert np.isfinite(P).all()
        assert same_bits(P[:, 0], hosts[7][:n, 0])  # beta = 0 in all three: p = r


def test_empty(torch_dev):
    """n == 0: the dot forms write 2k zeros, the plain update nothing; no
    vector is needed."""
    torch, dev = torch_dev
    lib = sa.hip_lib()
    k = 3
    s = _dev(torch, dev, np.ones(k))
    ws = _ws(torch, dev, 0, k)
    st = _stream(torch, dev)
    out = _out(torch, dev, 2 * k)
    assert lib.spmv_dot2_multi(0, k, None, k, None, k, None, k, out.data_ptr() + 16, sa._ptr(ws), ws.numel(), 0, st) == 0
    h = _out_live(out)
    assert (h == 0.0).all() and not np.signbit(h).any()
    out = _out(torch, dev, 2 * k)
    assert lib.spmv_bicgstab_update_dot_multi(0, k, sa._ptr(s), sa._ptr(s), sa._ptr(s), sa._ptr(s), None, k, None, k,
                                              None, k, None, k, None, k, None, k, out.data_ptr() + 16, sa._ptr(ws),
                                              ws.numel(), 0, st) == 0
    h = _out_live(out)
    assert (h == 0.0).all() and not np.signbit(h).any()
    assert lib.spmv_bicgstab_dir_multi(0, k, sa._ptr(s), sa._ptr(s), sa._ptr(s), sa._ptr(s), None, k, None, k, None, k,
                                       0, st) == 0
    torch.cuda.synchronize()


def test_argument_errors(torch_dev):
    """Every refusal, and that a refused call writes nothing."""
    torch, dev = torch_dev
    lib = sa.hip_lib()
    n, k = 300, 3
    blk = [torch.full((n, k), 1.0 + i, dtype=torch.float64, device=dev) for i in range(6)]
    s = torch.ones(k, dtype=torch.float64, device=dev)
    out = torch.full((2 * k,), -3.0, dtype=torch.float64, device=dev)
    need = lib.spmv_dot_multi_ws_bytes(n, 2 * k)
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    st = _stream(torch, dev)
    p = sa._ptr
    before = [b.clone() for b in blk]

    ok = [n, k, p(s), p(s), p(s), p(s), p(blk[0]), k, p(blk[1]), k, p(blk[2]), k, p(blk[3]), k, p(blk[4]), k, p(blk[5]),
          k, p(out), p(ws), need, 0, st]
    bad = [(0, -1), (1, 0), (2, None), (3, None), (4, None), (5, None), (6, None), (8, None), (10, None), (12, None),
           (14, None), (16, None), (7, k - 1), (9, k - 1), (11, k - 1), (13, k - 1), (15, k - 1), (17, k - 1),
           (18, None), (19, None), (20, need - 8)]
    for pos, val in bad:
        args = list(ok)
        args[pos] = val
        assert lib.spmv_bicgstab_update_dot_multi(*args) == sa.OTHER_ERROR, pos
    args = list(ok)
    args[8], args[9], args[17] = p(blk[5]), k, k + 1  # Sh == R with two leading dimensions
    assert lib.spmv_bicgstab_update_dot_multi(*args) == sa.OTHER_ERROR

    ok = [n, k, p(blk[0]), k, p(blk[1]), k, p(blk[2]), k, p(out), p(ws), need, 0, st]
    for pos, val in [(0, -1), (1, 0), (2, None), (4, None), (6, None), (3, k - 1), (5, k - 1), (7, k - 1), (8, None),
                     (9, None), (10, need - 8)]:
        args = list(ok)
        args[pos] = val
        assert lib.spmv_dot2_multi(*args) == sa.OTHER_ERROR, pos

    ok = [n, k, p(s), p(s), p(s), p(s), p(blk[0]), k, p(blk[1]), k, p(blk[2]), k, 0, st]
    for pos, val in [(0, -1), (1, 0), (2, None), (3, None), (4, None), (5, None), (6, None), (8, None), (10, None),
                     (7, k - 1), (9, k - 1), (11, k - 1)]:
        args = list(ok)
        args[pos] = val
        assert lib.spmv_bicgstab_dir_multi(*args) == sa.OTHER_ERROR, pos
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(blk, before)) and bool((out == -3.0).all())
    assert not ws.any()


# ------------------------------------------------------------ the grid clamps
BIG = 4_194_305


@functools.lru_cache(maxsize=None)
def big_block(seed):
    return host_block(BIG, 50 + seed, 3)


@pytest.mark.parametrize("n,k", [(524_287, 1), (524_287, 3), (524_288, 1), (524_288, 3), (524_289, 1), (524_289, 3),
                                 (4_194_304, 1), (4_194_304, 3), (4_194_305, 1), (4_194_305, 3)])
def test_at_the_grid_clamps(torch_dev, n, k):
    """The dot tree stops growing at n = 524,288 (a thread's two-row loop then
    runs again) and the update grid at n = 4,194,304: the same checks there.
    k = 1 runs the update with Sh == R and dot2 with C == A, k = 3 apart."""
    torch, dev = torch_dev
    lib = sa.hip_lib()
    assert lib.spmv_dot_multi_ws_bytes(524_288, 1) == lib.spmv_dot_multi_ws_bytes(BIG, 1)
    assert lib.spmv_dot_multi_ws_bytes(524_288 - 512, 1) < lib.spmv_dot_multi_ws_bytes(524_288, 1)
    six = [big_block(s) for s in range(6)]
    run_update(torch, dev, n, k, "tight", k == 1, _scalars(60 + k, k), blocks=six)
    run_dir(torch, dev, n, k, "tight", _scalars(70 + k, k), blocks=six[:3])
    run_dot2(torch, dev, n, k, "tight", k == 1, blocks=six[3:])


# ----------------------------------------------------------------- the solver
@functools.lru_cache(maxsize=None)
def _matrix(case):
    m = upwind(*case)
    return m, scipy_csr(m)


def _bits(t):
    import torch

    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("fmt", ["csr", "ell", "sell"])
@pytest.mark.parametrize("case", CASES)
def test_solver(torch_dev, case, fmt):
    torch, dev = torch_dev
    m, A = _matrix(case)
    n = m.n_rows
    ops = {bs: it.build_operator(m, 0, 1, fmt, dev, align=64, bjacobi=bs) for bs in (None, 2)}
    for k in (1, 3, 8, 9):
        Bh = rhs(n, k)
        B = torch.from_numpy(Bh).to(dev)
        for bs, op in ops.items():
            X, its, rel = it.bicgstab_multi(op, B, tol=TOL, maxit=MAXIT, check_every=10)
            mine = true_rel(A, Bh, X.cpu().numpy())
            print(f"{m.label} {fmt} k={k} bjacobi={bs}: its {its}, rel max {rel.max():.3g}, true {mine.max():.3g}")
            assert its < MAXIT and (rel <= REL_BOUND).all() and (mine <= REL_BOUND).all()
            assert np.allclose(rel, mine, rtol=1e-3, atol=1e-14)
            X2, its2, rel2 = it.bicgstab_multi(op, B, tol=TOL, maxit=MAXIT, check_every=10)
            assert its2 == its and torch.equal(_bits(X), _bits(X2)) and same_bits(rel, rel2)  # two runs, same bits
    for bs, op in ops.items():
        Bh = rhs(n, 9, 4)
        B = torch.from_numpy(Bh).to(dev)
        X, its, rel = it.bicgstab_multi(op, B, tol=0.0, maxit=20)
        assert its == 20 and bool((X[:, 4] == 0.0).all()) and rel[4] == 0.0 and np.isfinite(rel).all()
        for j in (0, 3, 8):  # column independence: the same 20 iterations on one column
            Xj, _, relj = it.bicgstab_multi(op, B[:, j:j + 1].contiguous(), tol=0.0, maxit=20)
            assert torch.equal(_bits(Xj[:, 0]), _bits(X[:, j])) and relj[0] == rel[j]
        x, its, rel = it.bicgstab(op, B[:, 0].contiguous(), tol=TOL, maxit=MAXIT, check_every=10)
        mine = true_rel(A, Bh[:, :1], x.cpu().numpy()[:, None])[0]
        assert its < MAXIT and x.shape == (n,) and rel <= REL_BOUND and mine <= REL_BOUND
        x2 = it.bicgstab(op, B[:, 0].contiguous(), tol=TOL, maxit=MAXIT, check_every=10)[0]
        assert torch.equal(_bits(x), _bits(x2))


@pytest.mark.parametrize("kw", [dict(split=True), dict(overlap=True)], ids=["split", "overlap"])
def test_bicgstab_split_and_overlap(torch_dev, kw):
    torch, dev = torch_dev
    m, A = _matrix(CASES[0])
    bh = rhs(m.n_rows, 1)
    b = torch.from_numpy(bh[:, 0].copy()).to(dev)
    x1 = it.bicgstab(it.build_operator(m, 0, 1, "csr", dev, align=64), b, tol=TOL, maxit=MAXIT)[0].cpu().numpy()
    for bs in (None, 2):
        op = it.build_operator(m, 0, 1, "csr", dev, align=64, bjacobi=bs, **kw)
        x, its, rel = it.bicgstab(op, b, tol=TOL, maxit=MAXIT)
        assert its < MAXIT and rel <= REL_BOUND and true_rel(A, bh, x.cpu().numpy()[:, None])[0] <= REL_BOUND
        assert np.abs(x.cpu().numpy() - x1).max() <= 1e-6 * np.abs(x1).max()
    with pytest.raises(sa.SpmvError):
        it.bicgstab_multi(op, torch.from_numpy(bh).to(dev))


def _tiny(rows):
    a = np.array(rows, dtype=np.float64)
    r, c = np.nonzero(a)
    return sa.Coo(a.shape[0], a.shape[1], r.astype(np.int32), c.astype(np.int32), a[r, c], False, "tiny")


def test_breakdowns(torch_dev):
    """tests/test_bicgstab.py's two cases on the device: the column stands
    still (rv = 0) or stagnates (t.s = 0), finite, and rel shows it."""
    torch, dev = torch_dev
    op = it.build_operator(_tiny([[0, 1], [-1, 0]]), 0, 1, "csr", dev, align=64)
    x, its, rel = it.bicgstab(op, torch.tensor([1.0, 0.0], dtype=torch.float64, device=dev), maxit=25)
    assert its == 25 and rel == 1.0 and bool((x == 0.0).all())
    op = it.build_operator(_tiny([[1, 2], [0, 1]]), 0, 1, "csr", dev, align=64)
    B = torch.tensor([[1.0, 0.0], [1.0, 1.0]], dtype=torch.float64, device=dev)
    X, its, rel = it.bicgstab_multi(op, B, maxit=25)
    assert its == 25 and rel[0] == 0.5 and np.array_equal(X.cpu().numpy()[:, 0], [0.5, 0.5])
    assert bool(torch.isfinite(X).all()) and np.isfinite(rel).all()


def test_chebyshev_is_refused(torch_dev):
    torch, dev = torch_dev
    m, _ = _matrix(CASES[2])
    op = it.build_operator(m, 0, 1, "csr", dev, align=64, chebyshev=3, cheb_bounds=(0.1, 2.0))
    B = torch.ones(m.n_rows, 2, dtype=torch.float64, device=dev)
    for call in (lambda: it.bicgstab_multi(op, B), lambda: it.bicgstab(op, B[:, 0].contiguous())):
        with pytest.raises(sa.SpmvError):
            call()
    assert it.bicgstab_multi(op, B, precond=False, maxit=5)[1] == 5  # the operator itself is fine


# -------------------------------------------------------------------- capture
def test_graph_capture(torch_dev):
    """One iteration's vector kernels (dot_multi, axpy_ratio_multi, dot2,
    update-dot, dir) captured on a single stream, a linear graph, and replayed:
    the bits of the eager calls."""
    torch, dev = torch_dev
    lib = sa.hip_lib()
    n, k = 5000, 5
    rng = np.random.default_rng(77)
    start = [torch.from_numpy(rng.uniform(-1, 1, (n, k))).to(dev) for _ in range(7)]  # R0 V T Ph X R P
    rho = torch.from_numpy(rng.uniform(0.5, 2.0, k)).to(dev)
    ws = _ws(torch, dev, n, k)
    p = sa._ptr

    def iteration(R0, V, T, Ph, X, R, P, rv, tst, s_new):
        st = _stream(torch, dev)
        rcs = [lib.spmv_dot_multi(n, k, p(R0), k, p(V), k, p(rv), p(ws), ws.numel(), 0, st),
               lib.spmv_axpy_ratio_multi(n, k, p(rho), p(rv), -1.0, p(V), k, p(R), k, 0, st),
               lib.spmv_dot2_multi(n, k, p(T), k, p(R), k, p(T), k, p(tst), p(ws), ws.numel(), 0, st),
               lib.spmv_bicgstab_update_dot_multi(n, k, p(rho), p(rv), p(tst), p(tst) + 8 * k, p(Ph), k, p(R), k,
                                                  p(T), k, p(R0), k, p(X), k, p(R), k, p(s_new), p(ws), ws.numel(),
                                                  0, st),
               lib.spmv_bicgstab_dir_multi(n, k, p(s_new), p(rv), p(tst) + 8 * k, p(tst), p(V), k, p(R), k, p(P), k,
                                           0, st)]
        assert rcs == [0] * 5, lib.spmv_last_error().decode()

    def state():
        return [t.clone() for t in start] + [torch.zeros(k, dtype=torch.float64, device=dev),
                                             torch.zeros(2 * k, dtype=torch.float64, device=dev),
                                             torch.zeros(2 * k, dtype=torch.float64, device=dev)]

    eager = state()
    iteration(*eager)
    torch.cuda.synchronize()
    held = state()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        iteration(*held)
    torch.cuda.synchronize()
    for t, s in zip(held, state()):  # whatever the capture did, start again
        t.copy_(s)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, held):
        assert torch.equal(_bits(a), _bits(b))
    assert bool((eager[4] != start[4]).any()) and bool((eager[6] != start[6]).any())


# ---------------------------------------------------------- existing solvers
def _old_cg_multi(torch, op, B, maxit):
    """iterate._cg_multi's loop as the parent commit has it, written out."""
    kk, rows, nv = op.kernels, op.rows, B.shape[1]
    send = torch.zeros(op.pad, nv, dtype=torch.float64, device=B.device)
    P, X, R = send[:rows], torch.zeros_like(B), B.clone()
    P.copy_(B)
    AP = torch.zeros_like(B)
    ws = kk.dot_multi_ws(rows, nv)
    rr, rr_new, pAp = (torch.zeros(nv, dtype=torch.float64, device=B.device) for _ in range(3))
    kk.dot_multi(rows, R, R, rr, ws)
    for _ in range(maxit):
        kk.spmm(send, AP)
        kk.dot_multi(rows, P, AP, pAp, ws)
        kk.axpy_ratio_multi(rows, rr, pAp, 1.0, P, X)
        kk.axpy_ratio_multi(rows, rr, pAp, -1.0, AP, R)
        kk.dot_multi(rows, R, R, rr_new, ws)
        kk.xpay_ratio_multi(rows, rr_new, rr, R, P)
        rr, rr_new = rr_new, rr
    return X


def _old_pcg(torch, op, B, maxit, multi):
    """iterate._pcg's loop for a block-Jacobi preconditioner, written out;
    multi False: cg's form, the single-vector product on ld = 1 blocks."""
    kk, rows, nv, M = op.kernels, op.rows, B.shape[1], op.precond

    def zeros(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=B.device)

    send, ap = (zeros(op.pad, nv), zeros(rows, nv)) if multi else (zeros(op.pad), zeros(rows))
    P, AP = (send[:rows], ap) if multi else (send[:rows].unsqueeze(1), ap.unsqueeze(1))
    X, R, Z = torch.zeros_like(B), B.clone(), torch.zeros_like(B)
    ws, pws = kk.dot_multi_ws(rows, nv), kk.precond_ws(M, rows, nv)
    pAp, s, s_new = zeros(nv), zeros(2 * nv), zeros(2 * nv)
    kk.precond_apply_dot(M, rows, R, Z, s, pws)
    P.copy_(Z)
    for _ in range(maxit):
        (kk.spmm if multi else kk.spmv)(send, ap)
        kk.dot_multi(rows, P, AP, pAp, ws)
        kk.axpy_ratio_multi(rows, s[:nv], pAp, 1.0, P, X)
        kk.axpy_ratio_multi(rows, s[:nv], pAp, -1.0, AP, R)
        kk.precond_apply_dot(M, rows, R, Z, s_new, pws)
        kk.xpay_ratio_multi(rows, s_new[:nv], s[:nv], Z, P)
        s, s_new = s_new, s
    return X


def _old_cg(torch, op, b, maxit):
    """iterate._cg's loop, written out: the single-vector kernels."""
    kk, rows = op.kernels, op.rows
    send = torch.zeros(op.pad, dtype=torch.float64, device=b.device)
    p, x, r, Ap = send[:rows], torch.zeros_like(b), b.clone(), torch.zeros_like(b)
    p.copy_(b)
    ws = kk.dot_ws(rows)
    rr, rr_new, pAp = (torch.zeros(1, dtype=torch.float64, device=b.device) for _ in range(3))
    kk.dot(rows, r, r, rr, ws)
    for _ in range(maxit):
        kk.spmv(send, Ap)
        kk.dot(rows, p, Ap, pAp, ws)
        kk.axpy_ratio(rows, rr, pAp, 1.0, p, x)
        kk.axpy_ratio(rows, rr, pAp, -1.0, Ap, r)
        kk.dot(rows, r, r, rr_new, ws)
        kk.xpay_ratio(rows, rr_new, rr, r, p)
        rr, rr_new = rr_new, rr
    return x


def test_existing_solvers_keep_their_bits(torch_dev):
    """cg_multi and cg, with and without a preconditioner, launch what they
    launched before this solver existed: the loops of the parent commit written
    out over the same kernels give the same bits (the symmetric matrix of the
    first grid)."""
    torch, dev = torch_dev
    m = upwind(48, 48, 0.0, 0.0)
    B = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, (m.n_rows, 3))).to(dev)
    b = B[:, 0].contiguous()
    for bs in (None, 2):
        op = it.build_operator(m, 0, 1, "csr", dev, align=64, bjacobi=bs)
        X1 = it.cg_multi(op, B, tol=0.0, maxit=25)[0].clone()
        x1 = it.cg(op, b, tol=0.0, maxit=25)[0].clone()
        if bs is None:
            X0, x0 = _old_cg_multi(torch, op, B, 25), _old_cg(torch, op, b, 25)
        else:
            X0, x0 = _old_pcg(torch, op, B, 25, True), _old_pcg(torch, op, b.unsqueeze(1), 25, False)[:, 0]
        torch.cuda.synchronize()
        assert torch.equal(_bits(X0), _bits(X1)) and bool((X1 != 0).any())
        assert torch.equal(_bits(x0), _bits(x1)) and bool((x1 != 0).any())
