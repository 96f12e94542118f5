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
  coo_staged_kernel       tiles spanning RC, RC + 1, 32 (RC + 1 - FW) and one
                          more row (RC = 1024 or 250; FW = 16 or 48 words):
                          the key-change table, the two bitmaps that fill
                          s_start to its last word, the binary searches; for
                          the carry pass at 2, 4 and 8 lanes and both tile
                          sizes, with x windows, with the hot table, and for
                          the single pass; single-pass tails of 1, 2, 79 and
                          80 entries, one on the lone last entry, and the
                          refusal of 81; the accumulate form under a HYB tail
                          at spans of 1024, 1025 and 40,000 rows
  coo_carry_kernel        runs of 1, 7, 8, 9, 255, 256, 257, 511, 512 and 513
                          continuation tiles (tile order up to 7, the wave
                          path from 8, rounds of 256), heads on the last lane
                          of a wave and of a workgroup, two in one wave, the
                          last run ending on the last tile: behind the tiled
                          CSR (fp64 and fp32 values), COO, a HYB tail and the
                          tiled CMRS, whose k-major carries end on the array's
                          last element
  x windows               a COO tile and a CMRS strip run spanning exactly
                          kStagedXwinCap = 2048 columns (staged in LDS), 2049
                          (gathered from global memory) and one, in one launch

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


# ------------------------------------------ 4. the staged COO / CMRS family
def run_both(torch_dev, e, real, fmt, kw, what, label, plan_check=None, ref_of=None):
    """The integer copy (bit-exact) and the real copy (the fp64 bound) through
    sa.to_device(m, fmt, **kw), each twice into NaN; -> {is integer copy: y}."""
    torch, dev = torch_dev
    mr, x, ref, bound = real
    out = {}
    for m, xin in ((e.m, e.x), (mr, x)):
        dm = sa.to_device(m, fmt, dev, **kw)
        if plan_check is not None:
            plan_check(dm)
        y = run_twice(torch, dev, dm, m, xin, what)
        if m is e.m:
            exact.assert_exact(y, e.ref, what)
        else:
            mm, rr, bb = (mr, ref, bound) if ref_of is None else ref_of()
            note(label, exact.assert_fp64(y, mm, x, ref=rr, bound=bb, what=what))
        out[m is e.m] = y
        del dm
    return out


def empty_rows_are_plus_zero(y, m, what):
    empty = np.bincount(m.row, minlength=m.n_rows) == 0
    assert empty.any() and (y[empty] == 0.0).all() and not np.signbit(y[empty]).any(), f"{what}: an empty row is not +0.0"


SPAN_RUNS = [(name, {} if th.SPAN_CASES[name][0] == "single" else {"coo_tail": False})
             for name in sorted(th.SPAN_CASES) if name != "wide-L4"]


@pytest.mark.parametrize("name,kw", SPAN_RUNS, ids=[n for n, _ in SPAN_RUNS])
def test_coo_staged_row_paths_at_their_spans(torch_dev, name, kw):
    """Tiles spanning RC, RC + 1, 32 (RC + 1 - FW) and 32 (RC + 1 - FW) + 1
    rows (asserted by the constructor, with the lanes, the tile and the RC
    the launch takes), one of them once more behind a continued first row;
    their last rows run into the next tile (a carry, or a single-pass tail of
    up to 80), in the -final cases the last of them closes the matrix and
    owns the trailing empty rows.  An off-by-one at either line moves one
    row's entry or runs over s_start: both change the integer sums."""
    launch, lanes, tile, final = th.SPAN_CASES[name]
    info, e, real = th.coo_span_case(name)
    assert info["rc"] == th.coo_row_cap(launch, lanes) and info["tile"] == tile and info["lanes"] == lanes
    assert sorted(set(info["spans"])) == list(info["edges"])

    def plan_check(dm):
        p = dm.params
        assert p["kernel"] == "coo_staged_kernel" and p["H"] == 0 and bool(p["single_pass"]) == (launch == "single"), p

    what = f"coo {name}"
    ys = run_both(torch_dev, e, real, "coo", kw, what, "coo single pass" if launch == "single" else "coo carry pass",
                  plan_check)
    for y in ys.values():
        empty_rows_are_plus_zero(y, e.m, what)


def test_coo_staged_row_paths_with_x_windows_and_hot_table(torch_dev):
    """One matrix (4 lanes, 512-entry tiles, spans around 1024 and 32,288)
    through the x-window launch and the hot-column launch, both RC = 1024, and
    the plain carry pass, RC = 250, whose bitmap and search paths the same
    tiles take: the same bits from all three."""
    info, e, real = th.coo_span_case("wide-L4")
    assert info["rc"] == th.COO_ROW_CAP == th.coo_row_cap("hot", 4) and info["lanes"] == 4 and info["tile"] == th.TILE
    assert [th.staged_row_path(s, th.coo_row_cap("carry", 4), th.TILE) for s in info["edges"]] == [
        "bitmap", "bitmap", "search", "search"]
    want = {"plain": 0, "xwin": 0, "hot": 64}
    kws = {"plain": {"coo_tail": False}, "xwin": {"xwin": True, "coo_tail": False}, "hot": {"hot": 64}}
    got = {}
    for form, kw in kws.items():
        def plan_check(dm, form=form):
            p = dm.params
            assert p["H"] == want[form] and not p["single_pass"], p
            assert ("x windows" in p["plan"]) == (form == "xwin") and (p["xcap"] > 0) == (form == "xwin"), p

        got[form] = run_both(torch_dev, e, real, "coo", kw, f"coo wide-L4 {form}", f"coo {form} launch", plan_check)
        for y in got[form].values():
            empty_rows_are_plus_zero(y, e.m, form)
    for integer in (True, False):
        assert same_bits(got["plain"][integer], got["xwin"][integer]), "x windows change bits"
        assert same_bits(got["plain"][integer], got["hot"][integer]), "the hot table changes bits"


def test_coo_single_pass_tails_at_the_cap(torch_dev):
    """Tails of 80, 2, 79 and 1 entries (the last on nnz - 1 of an odd nnz):
    the default plan is the single pass.  With one tail of 81 the single pass
    is refused by name and the default falls back to the carry pass."""
    torch, dev = torch_dev
    plan, e, real = th.coo_tail_case(False)
    assert plan.max() == th.COO_TAIL_CAP and e.m.nnz % 2 == 1

    def single(dm):
        assert dm.params["single_pass"] and dm.params["H"] == 0, dm.params

    run_both(torch_dev, e, real, "coo", {}, "coo tails up to 80", "coo single pass", single)
    run_both(torch_dev, e, real, "coo", {"coo_tail": True}, "coo tails up to 80, forced", "coo single pass", single)
    plan, e, real = th.coo_tail_case(True)
    assert plan.max() == th.COO_TAIL_CAP + 1
    with pytest.raises(sa.SpmvError, match=f"more than {th.COO_TAIL_CAP} entries"):
        sa.to_device(e.m, "coo", dev, coo_tail=True)

    def carry(dm):
        assert not dm.params["single_pass"] and dm.params["H"] == 0, dm.params

    run_both(torch_dev, e, real, "coo", {}, "coo tail of 81", "coo carry pass", carry)


HYB_FORMS = {"single-pass tail": {}, "carry pass": {"coo_tail": False}, "hot table": {"hot": 64},
             "no x windows": {"xwin": False}}


@pytest.mark.parametrize("form", sorted(HYB_FORMS))
def test_hyb_tail_accumulate_at_its_spans(torch_dev, form):
    """The accumulate kernel (4 lanes, 1,536-entry tiles, RC = 1024) under an
    ELL part of K = 2: tail tiles spanning 1024, 1025 (twice) and 40,000 rows,
    asserted on hyb_build's tail_row.  A row without tail entries keeps its
    ELL sum: the integer check sees a zero written over it."""
    info, e, real = th.hyb_tail_case()
    assert info["spans"] == (th.COO_ROW_CAP, th.COO_ROW_CAP + 1, th.COO_ROW_CAP + 1, 40_000)
    kw = HYB_FORMS[form]

    def plan_check(dm):
        p = dm.params
        assert p["K"] == th.HYB_K and p["tail_nnz"] == e.m.nnz - th.HYB_K * e.m.n_rows and p["H"] == kw.get("hot", 0), p
        assert ("tails" in dm.arrays) == (form in ("single-pass tail", "no x windows")), sorted(dm.arrays)
        assert ("win" in dm.arrays) == (form == "single-pass tail"), sorted(dm.arrays)

    y = run_both(torch_dev, e, real, "hyb", dict(kw, hyb_k=th.HYB_K), f"hyb {form}", "hyb tail (accumulate)", plan_check)
    assert (y[True][info["no_tail"]] == e.ref[info["no_tail"]]).all()


@functools.lru_cache(maxsize=None)
def f32_reference(tile):
    """The real copy of carry_case(tile) as csrf32 stores it, with its reference and bound."""
    _, _, (mr, x, _, _) = th.carry_case(tile)
    m32 = exact.rounded_f32(mr)
    return m32, exact.exact_reference(m32, x), exact.fp64_bound(m32, x)


CARRY_CONSUMERS = [
    ("csr", th.TILE, {"variant": 4, "hot": 0}, "csr_tiled_kernel"),
    ("csr", th.TILE, {"variant": 4, "hot": 64}, "csr_tiled_kernel"),
    ("csrf32", th.TILE, {"variant": 4, "hot": 0}, None),
    ("coo", th.TILE, {"coo_tail": False}, "coo_staged_kernel"),
    ("coo", th.BIG_TILE, {"coo_tail": False}, "coo_staged_kernel"),
    ("coo", th.TILE, {"xwin": True, "coo_tail": False}, "coo_staged_kernel"),
    ("coo", th.TILE, {"hot": 64}, "coo_staged_kernel"),
    ("hyb", th.BIG_TILE, {"hyb_k": th.HYB_K, "coo_tail": False}, None),
    ("cmrs", th.TILE, {"cmrs_variant": 1, "h": 8}, "cmrs_tiled_kernel"),
    ("cmrs", th.TILE, {"cmrs_variant": 1, "h": 64}, "cmrs_tiled_kernel"),
]


def _consumer_id(c):
    return f"{c[0]}-tile{c[1]}-" + "-".join(f"{k}{v}" for k, v in c[2].items())


@pytest.mark.parametrize("consumer", CARRY_CONSUMERS, ids=[_consumer_id(c) for c in CARRY_CONSUMERS])
def test_carry_runs_at_the_wave_path_lines(torch_dev, consumer):
    """coo_carry_kernel behind each of its callers, on rows that continue over
    exactly 1, 7, 8, 9, 255, 256, 257 (and with 512-entry tiles 511, 512, 513)
    tiles, placed as the constructor asserts: a run read one tile short or
    long, a second round not taken, or a load past the last tile changes the
    integer sum of a long row."""
    fmt, tile, kw, kernel = consumer
    info, e, real = th.carry_case(tile)
    lengths = {n for _, n in info["runs"]}
    assert {7, 8, 9, th.CARRY_ROUND - 1, th.CARRY_ROUND, th.CARRY_ROUND + 1} <= lengths
    assert (2 * th.CARRY_ROUND + 1 in lengths) == (tile == th.TILE) and sum(info["runs"][-1]) == info["tiles"]

    def plan_check(dm):
        p = dm.params
        assert p["H"] == kw.get("hot", 0), p
        if kernel is not None:
            assert p["kernel"] == kernel, p
        if fmt == "coo":
            assert not p["single_pass"] and ("x windows" in p["plan"]) == bool(kw.get("xwin")), p
        if fmt == "csrf32":
            assert p["variant"] == 4, p
        if fmt == "hyb":
            assert "tails" not in dm.arrays and p["tail_nnz"] > th.CARRY_ROUND * th.BIG_TILE, p

    ref_of = (lambda: f32_reference(tile)) if fmt == "csrf32" else None
    run_both(torch_dev, e, real, fmt, kw, f"carry runs behind {_consumer_id(consumer)}", f"carry pass behind {fmt}",
             plan_check, ref_of)


@pytest.mark.parametrize("fmt", ["coo", "cmrs"])
def test_staged_x_window_cap(torch_dev, fmt):
    """One launch with a window of exactly 2048 columns (staged in LDS), one of
    2049 (gathered from global memory), one of a single column and narrow
    ones, by the restated window kernels; the same bits without windows."""
    spans, e, real = th.window_case(fmt)
    assert sorted(set(spans.tolist())) == [1, 100, th.XWIN_CAP, th.XWIN_CAP + 1]
    kw = {"coo_tail": False} if fmt == "coo" else {"cmrs_variant": 0, "h": th.CMRS_WINDOW_H}
    kernel = "coo_staged_kernel" if fmt == "coo" else "cmrs_staged_kernel"

    def windows(dm):
        p = dm.params
        assert p["kernel"] == kernel and p["xcap"] == th.XWIN_CAP and "x windows" in p["plan"] and p["H"] == 0, p

    def none(dm):
        assert dm.params["kernel"] == kernel and "x windows" not in dm.params["plan"], dm.params

    on = run_both(torch_dev, e, real, fmt, dict(kw, xwin=True), f"{fmt} x windows at the cap", f"{fmt} x-window cap", windows)
    off = run_both(torch_dev, e, real, fmt, dict(kw, xwin=False), f"{fmt} without x windows", f"{fmt} x-window cap", none)
    for integer in (True, False):
        assert same_bits(on[integer], off[integer]), f"{fmt}: x windows change bits"
