"""Kernels at the sizes where their own constants change their control flow
(tests/thresholds.py builds the matrices), on the MI355X:

  sell_split_fix_kernel   chunk runs around 65,536 + 1 and 2 * 65,536 + 1,
                          where a coarse pass of its run-end search ends on
                          the run's end; followed by other runs and as the
                          last run
  csr_tiled_kernel        tiles owning 1024 / 1025 / 65,536 / 65,537 rows: the
                          LDS offset table, the big-tile plan and its bitmap,
                          row_ptr from global memory, with and without a plan
  the vector kernels      at, just above and well above the sizes at which
                          their stage-1 grids stop growing (vec.hip: 1024
                          workgroups of the dot at n = 2,097,152, 4096 of the
                          updates at 4,194,304; vec_multi.hip: 1024 at 524,288
                          and 4096 at 4,194,304)

Every output starts as NaN (or lies between guard elements), every SpMV is
checked with tests/exact.py's two rules, bit-exact on the integer copy and
within (n_i + 2) 2^-53 sum |a_ij x_j| on the wide-range copy, and runs twice
with the same bits: nothing here uses atomics.

Vector bounds, against np.longdouble references: a dot product of n rounded
products summed in any order, (n + 2) 2^-53 sum |a b|; the ratio updates, one
rounding each for the quotient, the product and the sum plus one ulp for the
device's quotient, 4 2^-53 (|y| + |c x|) (both as test_iterate_multi_gpu.py);
scale_rsqrt, one rounding each for the root, the reciprocal and the product
plus one ulp of slack for the device's operations, 4 2^-53 |x / sqrt(s)|.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import exact
import spmv_amd as sa
import thresholds as th
from test_iterate_multi_gpu import GUARD, U, _dot, _place, _stream

pytestmark = pytest.mark.gpu

LD = np.longdouble
_worst = {}  # kernel -> largest error / bound seen


def note(what, ratio):
    _worst[what] = max(_worst.get(what, 0.0), float(ratio))


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    yield torch, torch.device("cuda:0")
    if _worst:  # the measured figures (pytest -s)
        print("\nlargest error / bound per kernel: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(_worst.items())))


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def run_twice(torch, dev, dm, m, x, what):
    """Two runs into NaN-filled outputs: the same bits; returns the first."""
    xd = torch.from_numpy(np.array(x, order="C")).to(dev)
    ys = []
    for _ in range(2):
        y = torch.full((m.n_rows,), float("nan"), dtype=torch.float64, device=dev)
        dm.run(xd, y)
        torch.cuda.synchronize()
        ys.append(y.cpu().numpy())
    assert same_bits(ys[0], ys[1]), f"{what}: two runs differ"
    return ys[0]


# ------------------------------------------------------------ 1. SELL split
BASE = {"xwin": False}  # the hot-column rule picks no table here (test_thresholds.py): spmv_sell_run_split
SELL_CASES = [(R, 32, 1, False, 1, BASE) for R in th.SELL_RS] + [
    (65_500, 64, 1, False, 1, BASE),                          # W = 16 segments, the small-matrix main kernel
    (65_500, 32, 2, False, 2, BASE),                          # ki = 2, split = 2
    (65_500, 32, 1, False, 1, {"xwin": True}),                # x windows: chunks and main workgroups in one grid
    (65_500, 32, 1, False, 1, {"xwin": False, "hot": 64}),    # spmv_sell_run_hot
    (65_500, 32, 1, True, 1, BASE),                           # the last run in chunk order
    (65_537, 32, 1, True, 1, BASE),
]


def _sell_id(case):
    R, C, T, last, ki, kw = case
    return f"R{R}-C{C}-T{T}-ki{ki}-{'last' if last else 'followed'}-" + "-".join(f"{k}{v}" for k, v in kw.items())


@pytest.mark.parametrize("case", SELL_CASES, ids=[_sell_id(c) for c in SELL_CASES])
def test_sell_split_run_lengths(torch_dev, case):
    """The long run's rows get their own R chunk partials and nothing else:
    a run end found late adds the following slices' partials (every row of
    theirs is full), one found early drops chunks; either changes the integer
    sums.  The rows of the small runs (1, 2, W - 1, W, W + 1, 65 chunks) and of
    the tail are in the same comparison."""
    torch, dev = torch_dev
    R, C, T, last, ki, kw = case
    runs, e, (mr, x, ref, bound) = th.sell_case(R, C, T, last, ki)
    assert R in runs and (runs[-1] == R) == last
    what = f"sell {_sell_id(case)}"
    for m, xin in ((e.m, e.x), (mr, x)):
        dm = sa.to_device(m, "sell", dev, C=C, sigma=C, ki=ki, split=T, **kw)
        p = dm.params
        assert p["n_chunks"] == sum(runs) and p["split_T"] == T and p["ki"] == ki, p
        assert p["H"] == kw.get("hot", 0), p
        if kw["xwin"]:
            assert p["kernel"] == "sell_xwin_kernel" and "x windows" in p["plan"], p
        y = run_twice(torch, dev, dm, m, xin, what)
        if m is e.m:
            exact.assert_exact(y, e.ref, what)
        else:
            note("sell split", exact.assert_fp64(y, mr, x, ref=ref, bound=bound, what=what))
        del dm


# ------------------------------------------------------------ 2. tiled CSR
@pytest.mark.parametrize("hot", [0, 64])
@pytest.mark.parametrize("order", sorted(th.TILE_ORDERS))
def test_csr_tiled_owned_row_thresholds(torch_dev, order, hot):
    """Tiles owning 1024, 1025, 65,536 and 65,537 rows (asserted by the
    constructor), the last of them followed by another tile or the matrix's
    last: with the big-tile plan exactly the 1025- and 65,536-row tiles are
    listed and the 65,537-row tile falls back to row_ptr while a plan is
    attached; without it both read row_ptr.  Same bits either way, and every
    row without entries is +0.0."""
    torch, dev = torch_dev
    owned, under_test, e, (mr, x, ref, bound) = th.tiles_case(order)
    assert [int(owned[t]) for t in under_test] == [1024, 1025, 65536, 65537]
    want_big = int(np.count_nonzero((owned > th.ROW_CAP) & (owned <= th.BIG_ROW_CAP)))
    assert want_big == 2
    empty = np.bincount(e.m.row, minlength=e.m.n_rows) == 0
    got = {}
    for bigplan in (True, False):
        what = f"csr variant 4 hot {hot} bigplan {bigplan} on {order}"
        for m, xin in ((e.m, e.x), (mr, x)):
            dm = sa.to_device(m, "csr", dev, variant=4, hot=hot, bigplan=bigplan)
            p = dm.params
            assert p["kernel"] == "csr_tiled_kernel" and p["H"] == hot, p
            assert p["big_tiles"] == (want_big if bigplan else 0), p
            y = run_twice(torch, dev, dm, m, xin, what)
            if m is e.m:
                exact.assert_exact(y, e.ref, what)
            else:
                note("csr tiled", exact.assert_fp64(y, mr, x, ref=ref, bound=bound, what=what))
            assert (y[empty] == 0.0).all() and not np.signbit(y[empty]).any(), f"{what}: an empty row is not +0.0"
            got[bigplan, m is e.m] = y
            del dm
    for integer in (True, False):
        assert same_bits(got[True, integer], got[False, integer]), f"hot {hot} on {order}: bigplan changes bits"


# ------------------------------------------------------ 3. vector kernels
@functools.lru_cache(maxsize=None)
def host_block(n, seed, k=1):
    """(n, k) uniform(-1, 1) without zeros ((n,) for k = 1); made once, never changed."""
    a = np.random.default_rng(100 * seed + n % 991).uniform(-1.0, 1.0, (n, k) if k > 1 else n)
    a[a == 0.0] = 0.5
    a.setflags(write=False)
    return a


def guarded(torch, dev, body, fill=None):
    """body (or NaN / `fill` of that length) between two GUARD elements on
    each side -> (buffer, address of the live part): 16-byte aligned."""
    n = body if isinstance(body, int) else body.size
    buf = np.full(n + 4, np.nan if fill is None else fill)
    buf[:2] = GUARD
    buf[-2:] = GUARD
    if not isinstance(body, int):
        buf[2:-2] = body
    t = torch.from_numpy(buf).to(dev)
    return t, t.data_ptr() + 16


def live(t):
    """The live part of a guarded buffer after checking its guards."""
    h = t.cpu().numpy()
    assert (h[:2] == GUARD).all() and (h[-2:] == GUARD).all(), "a guard element was written"
    return h[2:-2]


def ratio(err, bound):
    """Largest err / bound after asserting err <= bound everywhere."""
    err, bound = np.atleast_1d(np.asarray(err, np.float64)), np.atleast_1d(np.asarray(bound, np.float64))
    assert (err <= bound).all(), (float(err.max()), float(bound[np.argmax(err - bound)]))
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


@pytest.mark.parametrize("n", [2_097_152, 2_097_153, 5_000_011])
def test_dot_at_the_grid_clamp(torch_dev, n):
    """spmv_dot's stage 1 reaches its 1024 workgroups at n = 2,097,152: from
    there on a thread's loop takes more than one pair of elements."""
    torch, dev = torch_dev
    lib = sa.hip_lib()
    a, b = host_block(n, 1), host_block(n, 2)
    ta, tb = torch.from_numpy(a.copy()).to(dev), torch.from_numpy(b.copy()).to(dev)
    assert lib.spmv_dot_ws_bytes(n) == 8 * 1024 and lib.spmv_dot_ws_bytes(2_097_152 - 2048) == 8 * 1023
    ws = torch.empty(lib.spmv_dot_ws_bytes(n), dtype=torch.uint8, device=dev)
    out, po = guarded(torch, dev, 2)
    for k in range(2):
        assert lib.spmv_dot(n, sa._ptr(ta), sa._ptr(tb), po + 8 * k, sa._ptr(ws), ws.numel(), 0, _stream(torch, dev)) == 0
    torch.cuda.synchronize()
    got = live(out)
    assert got.view(np.int64)[0] == got.view(np.int64)[1]
    prod = a.astype(LD) * b.astype(LD)
    note("dot", ratio(abs(LD(got[0]) - prod.sum()), (n + 2) * U * float(np.abs(prod).sum())))
    assert same_bits(ta.cpu().numpy(), a) and same_bits(tb.cpu().numpy(), b)


@pytest.mark.parametrize("layout", ["tight", "padded"])
@pytest.mark.parametrize("k", [1, 8, 9])
@pytest.mark.parametrize("n", [524_288, 524_289, 1_572_869])
def test_dot_multi_at_the_grid_clamp(torch_dev, n, k, layout):
    """G(n) stops growing at n = 524,288 (1024 workgroups of two rows per
    thread): above it a thread's two-row loop runs again.  The bound, two calls
    with the same bits, and the column rule where G is clamped: column j of the
    wide call has the bits of the k = 1 call on a contiguous copy of it."""
    torch, dev = torch_dev
    lib = sa.hip_lib()
    assert lib.spmv_dot_multi_ws_bytes(n, 1) == 8 * 1024 and lib.spmv_dot_multi_ws_bytes(524_288 - 512, 1) == 8 * 1023
    a, b = host_block(n, 3, 9), host_block(n, 4, 9)
    ta, pa, lda, _ = _place(torch, dev, a, n, k, layout, 11)
    tb, pb, ldb, _ = _place(torch, dev, b, n, k, layout, 12)
    before = (ta.clone(), tb.clone())
    wide = _dot(torch, dev, n, k, pa, lda, pb, ldb)
    again = _dot(torch, dev, n, k, pa, lda, pb, ldb)
    assert same_bits(wide, again)
    assert torch.equal(ta, before[0]) and torch.equal(tb, before[1])  # inputs untouched
    prod = a[:, :k].astype(LD) * b[:, :k].astype(LD)
    assert np.isfinite(wide).all()
    note("dot_multi", ratio(np.abs(wide.astype(LD) - prod.sum(axis=0)), (n + 2) * U * np.abs(prod).sum(axis=0)))
    for j in range(k):
        ca = torch.from_numpy(np.ascontiguousarray(a[:, j])).to(dev)
        cb = torch.from_numpy(np.ascontiguousarray(b[:, j])).to(dev)
        one = _dot(torch, dev, n, 1, ca.data_ptr(), 1, cb.data_ptr(), 1)
        assert one.view(np.int64)[0] == wide.view(np.int64)[j], (n, k, layout, j)


def test_bjacobi_apply_dot_at_the_grid_clamp(torch_dev):
    """The fused apply shares dot_multi_blocks: at n = 524,289 (bs = 3 blocks
    straddle every workgroup, k = 3) its r.z and r.r have spmv_dot_multi's
    bits and meet its bound, and Z has the host statement's bits.  The inverse
    is held to the rule of test_precond_gpu.test_create against
    precond_cases.dense_blocks."""
    from precond_cases import dense_blocks
    from test_precond_gpu import U52, check_sums, host_inverse, residuals, run_apply

    torch, dev = torch_dev
    n, bs, k = 524_289, 3, 3
    i = np.arange(n, dtype=np.int64)
    col = (i // bs * bs)[:, None] + np.arange(bs)[None, :]
    val = np.random.default_rng(19).uniform(-1.0, 1.0, (n, bs))
    val[col == i[:, None]] += 4.0  # dominant diagonal: no singular block
    keep = (col < n).ravel()
    m = sa.Coo(n, n, np.repeat(i, bs)[keep].astype(np.int32), col.ravel()[keep].astype(np.int32), val.ravel()[keep],
               False, "3 x 3 blocks")
    M = sa.BlockJacobi.from_coo(m, bs, dev)
    assert M.info()["singular_blocks"] == 0
    inv = M.inverse().cpu().numpy()
    D = dense_blocks(m, bs)
    e_dev = residuals(D, inv, bs)
    assert (e_dev <= 8 * residuals(D, host_inverse(m, bs)[0], bs).max() + bs * U52).all()
    for layout in ("tight", "padded"):
        rd, zd, R, Z, out = run_apply(torch, dev, M, inv, n, bs, k, layout, True)
        check_sums(torch, dev, n, k, rd, zd, R, Z, out)


UPDATE_N = 4_194_304 + 1 + 256  # the update grids stop at 4096 workgroups of 4 rows per thread: n = 4,194,304


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("what", ["axpy", "xpay"])
def test_ratio_updates_multi_past_the_grid_clamp(torch_dev, what, k):
    """n = 4,194,561: every thread's unrolled loop runs once more for some
    rows and its remainder loop for others.  Tight layout; X, the two rows
    behind Y's live part and the guard elements keep their bits."""
    torch, dev = torch_dev
    lib = sa.hip_lib()
    n = UPDATE_N
    x, y0 = host_block(n, 5, 8)[:, :k], host_block(n, 6, 8)[:, :k]

    def place(h, extra):  # n live rows, two more rows, two guards
        buf = np.full((n + 2) * k + 2, extra)
        buf[: n * k] = h.ravel()
        buf[-2:] = GUARD
        return buf

    bx, by = place(x, 0.375), place(y0, -1.5)
    tx, ty = torch.from_numpy(bx).to(dev), torch.from_numpy(by).to(dev)
    rng = np.random.default_rng(50 + k)
    num = rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)
    den = rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)
    dn, dd = torch.from_numpy(num).to(dev), torch.from_numpy(den).to(dev)
    if what == "axpy":
        rc = lib.spmv_axpy_ratio_multi(n, k, sa._ptr(dn), sa._ptr(dd), -1.0, sa._ptr(tx), k, sa._ptr(ty), k, 0,
                                       _stream(torch, dev))
    else:
        rc = lib.spmv_xpay_ratio_multi(n, k, sa._ptr(dn), sa._ptr(dd), sa._ptr(tx), k, sa._ptr(ty), k, 0,
                                       _stream(torch, dev))
    assert rc == 0, lib.spmv_last_error().decode()
    torch.cuda.synchronize()
    assert same_bits(tx.cpu().numpy(), bx)
    after = ty.cpu().numpy()
    assert same_bits(after[n * k:], by[n * k:])  # rows >= n, guards
    y1 = after[: n * k].reshape(n, k)
    c = (-1.0 if what == "axpy" else 1.0) * (num.astype(LD) / den.astype(LD))
    worst = 0.0
    for lo in range(0, n, 1 << 20):  # in slices: the longdouble copies stay small
        xs, ys, got = (a[lo:lo + (1 << 20)].astype(LD) for a in (x, y0, y1))
        keep, scaled = (ys, c * xs) if what == "axpy" else (xs, c * ys)
        worst = max(worst, ratio(np.abs(got - (keep + scaled)), 4 * U * (np.abs(keep) + np.abs(scaled))))
    note(f"{what}_ratio_multi", worst)


@pytest.mark.parametrize("n", [1, 255, 4_194_304, UPDATE_N])
def test_single_vector_kernels_at_the_grid_clamp(torch_dev, n):
    """spmv_axpy_ratio, spmv_xpay_ratio, spmv_scale_rsqrt and spmv_gather at
    the 4096-workgroup clamp of their grid (n = 4,194,304), above it and at
    the smallest sizes; y between guard elements, x unchanged bit for bit."""
    torch, dev = torch_dev
    lib = sa.hip_lib()
    s = _stream(torch, dev)
    x, y0 = host_block(n, 7), host_block(n, 8)
    tx = torch.from_numpy(x.copy()).to(dev)
    num, den = 3.0, -7.0
    dn = torch.tensor([num], dtype=torch.float64, device=dev)
    dd = torch.tensor([den], dtype=torch.float64, device=dev)
    xl, yl = x.astype(LD), y0.astype(LD)
    c = LD(num) / LD(den)

    ty, py = guarded(torch, dev, y0)
    assert lib.spmv_axpy_ratio(n, sa._ptr(dn), sa._ptr(dd), -1.0, sa._ptr(tx), py, 0, s) == 0
    torch.cuda.synchronize()
    note("axpy_ratio", ratio(np.abs(live(ty) - (yl - c * xl)), 4 * U * (np.abs(yl) + np.abs(c * xl))))

    ty, py = guarded(torch, dev, y0)
    assert lib.spmv_xpay_ratio(n, sa._ptr(dn), sa._ptr(dd), sa._ptr(tx), py, 0, s) == 0
    torch.cuda.synchronize()
    note("xpay_ratio", ratio(np.abs(live(ty) - (xl + c * yl)), 4 * U * (np.abs(xl) + np.abs(c * yl))))

    ds = torch.tensor([7.0], dtype=torch.float64, device=dev)
    ty, py = guarded(torch, dev, n)
    assert lib.spmv_scale_rsqrt(n, sa._ptr(ds), sa._ptr(tx), py, 0, s) == 0
    torch.cuda.synchronize()
    want = xl / np.sqrt(LD(7.0))
    note("scale_rsqrt", ratio(np.abs(live(ty) - want), 4 * U * np.abs(want)))

    order = np.random.default_rng(n).permutation(n).astype(np.int32)
    to = torch.from_numpy(order).to(dev)
    ty, py = guarded(torch, dev, n)
    assert lib.spmv_gather(n, sa._ptr(to), sa._ptr(tx), py, 0, s) == 0
    torch.cuda.synchronize()
    assert same_bits(live(ty), x[order])
    assert same_bits(tx.cpu().numpy(), x) and np.array_equal(to.cpu().numpy(), order)
