"""The CSR x-window kernel's prologue and argument order (csrc/csr.hip,
csr_xwin_kernel): its leading arguments arrive preloaded in SGPRs in a fixed
order, the window's row offsets and x range are addressed from wave-uniform
bases with 32-bit lane offsets, and the first 512 offsets are requested before
the window's bounds are known.

Every case compares the CSR plan's y with the 16-bit window-relative copy on,
bit for bit, with the same plan with the copy off, and both with the oracle by
the parity rule, on y pre-filled with NaN.  x is a shuffled ramp of distinct
values and n_rows, the number of row groups, the groups per window and the
window cap differ in every case, so a swapped or misread argument changes y.
The shapes are the prologue's edges: one row group minus / plus one row (the
clamp of a row past n_rows), 0 / 1 / 2 / an odd number of entries, a window
that spans exactly the cap and one column more (global gathers, no copy), a
window of more rows than one pass of offsets holds, short rows (the unpipelined
schedule), and enough windows for the XCD-contiguous placement.  The csr16 and
csrf32 formats run the same kernel with their own column / value sources.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import spmv_amd as sa
from oracle import oracle

pytestmark = pytest.mark.gpu

CAP = 2048  # kCsrXwinCap: columns of an x window in LDS, and what one pass of the copy holds


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch, torch.device("cuda:0")


def distinct_x(n, seed):
    """n distinct values in (-1, 1), shuffled."""
    n = max(n, 1)
    return (np.random.default_rng(seed).permutation(n).astype(np.float64) + 0.25) / n * 2.0 - 1.0


def _with_ref(m, seed):
    x = distinct_x(m.n_cols, seed)
    ref = oracle.file_order_spmv(m.n_rows, m.row, m.col, m.val, x)
    x.setflags(write=False)
    ref.setflags(write=False)
    return m, x, ref


def _coo(n_rows, n_cols, lens, lo, width, seed, label, edges=None):
    """Row r holds lens[r] distinct sorted columns of [lo[r], lo[r] + width): one
    per stratum of width // lens[r] columns, at a random place inside it.
    edges = (first, last): the matrix's first entry sits in column `first`, its
    last in column `last`."""
    rng = np.random.default_rng(seed)
    lens = np.broadcast_to(np.asarray(lens, dtype=np.int64), (n_rows,))
    lo = np.broadcast_to(np.asarray(lo, dtype=np.int64), (n_rows,))
    row = np.repeat(np.arange(n_rows, dtype=np.int32), lens)
    k = np.arange(row.size) - np.repeat(np.cumsum(lens) - lens, lens)  # place in its row
    step = np.repeat(width // np.maximum(lens, 1), lens)
    col = np.repeat(lo, lens) + k * step + rng.integers(0, 1 << 30, row.size) % step
    if edges is not None:
        col[0], col[-1] = edges
    assert col.size == 0 or (0 <= col.min() and col.max() < n_cols)
    val = rng.uniform(-1.0, 1.0, row.size)
    return sa.Coo(n_rows, n_cols, row, col.astype(np.int32), val, False, label)


@functools.lru_cache(maxsize=None)
def rows_case(n_rows):
    """About 67 entries per row (58..76): with 4 lanes per row one row group is
    64 rows of about 4,300 entries, three chunks of 1,536, the pipelined schedule."""
    lens = np.random.default_rng(100 + n_rows).integers(58, 77, n_rows)
    return _with_ref(_coo(n_rows, 1500, lens, 0, 1500, n_rows, f"{n_rows} rows x ~64"), 200 + n_rows)


@functools.lru_cache(maxsize=None)
def nnz_case(nnz):
    """nnz entries in the first rows of a 3 x 7 matrix (nnz <= 2), or 65 rows of
    about 64 entries with an odd total."""
    if nnz == "odd":
        lens = np.random.default_rng(7).integers(58, 77, 65)
        lens[-1] -= 1 - (int(lens.sum()) & 1)
        m = _coo(65, 1400, lens, 0, 1400, 8, "65 rows, odd nnz")
        assert m.nnz & 1
        return _with_ref(m, 9)
    lens = np.array([min(nnz, 1), max(nnz - 1, 0), 0])
    return _with_ref(_coo(3, 7, lens, 2, 5, 10 + nnz, f"3 x 7, nnz {nnz}"), 20 + nnz)


@functools.lru_cache(maxsize=None)
def span_case(span):
    """One window (60 rows x 64 entries, 4 lanes per row) whose columns run from
    100 to 100 + span - 1 exactly."""
    m = _coo(60, 4000, 64, 100, span - 64, span, f"one window spanning {span}", edges=(100, 100 + span - 1))
    assert m.col.min() == 100 and m.col.max() == 100 + span - 1
    return _with_ref(m, 31)


@functools.lru_cache(maxsize=None)
def tall_case():
    """1,100 rows x ~64 entries over 1,800 columns: with xwin_rows = 1024 and 4
    lanes per row a window is 16 row groups, 1,025 offsets, three passes of 512;
    the second window holds the 76 rows that are left (18 groups in all)."""
    lens = np.random.default_rng(41).integers(58, 77, 1100)
    return _with_ref(_coo(1100, 1800, lens, 0, 1800, 42, "1,100 rows, 1,024-row windows"), 43)


@functools.lru_cache(maxsize=None)
def short_case():
    """300 rows x 8 entries: 2 lanes per row, one-group windows of one chunk,
    the unpipelined schedule (MODE 0)."""
    return _with_ref(_coo(300, 1000, 8, (np.arange(300) // 128) * 100, 700, 51, "300 rows x 8"), 52)


@functools.lru_cache(maxsize=None)
def many_windows_case(per_row):
    """2,050 windows of 64 rows (xwin_rows = 64, 4 lanes per row); window w reads
    columns [16 w, 16 w + 1,500): neighbouring windows overlap widely and the
    cap is far above twice the rows of a window, so the plan's rule places the
    windows XCD-contiguously (csr_xwin_remap_rule).  2,050 = 8 x 256 + 2: two
    XCDs get one window more than the others."""
    n_rows = 2050 * 64
    lo = (np.arange(n_rows) // 64) * 16
    return _with_ref(_coo(n_rows, 2050 * 16 + 1500, per_row, lo, 1500, 61, f"2,050 windows x {per_row}/row"), 62)


def run(torch, dev, dm, m, x):
    xd = torch.from_numpy(np.array(x, order="C")).to(dev)
    y = torch.full((max(m.n_rows, 1),), float("nan"), dtype=torch.float64, device=dev)
    dm.run(xd, y)
    torch.cuda.synchronize()
    return y.cpu().numpy()[: m.n_rows]


def assert_parity(m, y, x, ref, rel=1e-6):
    bad = oracle.parity(y, ref, m.row, m.col, m.val, x, m.n_rows, rel=rel)
    assert bad.size == 0, f"{m.label}: {bad.size} bad rows, first {bad[:5]}: got {y[bad[:5]]} want {ref[bad[:5]]}"


def same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


def check(torch, dev, case, **kw):
    """(plan with the copy off, plan with it on): same bits, both at parity."""
    m, x, ref = case
    try:
        sa.set_option("csr_col16", 0)
        off = sa.to_device(m, "csr", dev, **kw)
        sa.set_option("csr_col16", 1)
        on = sa.to_device(m, "csr", dev, **kw)
    finally:
        sa.set_option("csr_col16", None)
    assert off.params["index16"] == 0
    y_off, y_on = run(torch, dev, off, m, x), run(torch, dev, on, m, x)
    assert same_bits(y_off, y_on), f"{m.label}: the 16-bit copy changes y"
    assert_parity(m, y_off, x, ref)
    assert_parity(m, y_on, x, ref)
    return off, on, y_on


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 129])
def test_rows_around_a_group(torch_dev, n_rows):
    torch, dev = torch_dev
    off, on, _ = check(torch, dev, rows_case(n_rows), lanes=4)
    assert on.params["kernel"] == "csr_xwin_kernel" and on.params["index16"] == 1
    assert 1300 < on.params["xcap"] <= 1500


@pytest.mark.parametrize("xwin_rows", [0, 1024], ids=["default-windows", "1024-row-windows"])
@pytest.mark.parametrize("nnz", [0, 1, 2, "odd"])
def test_few_entries_and_odd_count(torch_dev, nnz, xwin_rows):
    torch, dev = torch_dev
    _, on, _ = check(torch, dev, nnz_case(nnz), xwin_rows=xwin_rows)
    if nnz in (0, 1):
        assert on.params["index16"] == 0  # no pair to load below 2 entries
    if nnz == "odd":
        assert on.params["index16"] == 1 and on.params["kernel"] == "csr_xwin_kernel"


@pytest.mark.parametrize("span", [CAP, CAP + 1])
def test_window_at_the_cap(torch_dev, span):
    """A window of exactly 2,048 columns is copied to LDS in one pass (the
    clamped lane offset reaches entry 2,047); one column more and the window
    is gathered from global memory, without a 16-bit copy."""
    torch, dev = torch_dev
    off, on, _ = check(torch, dev, span_case(span), lanes=4)
    assert on.params["kernel"] == "csr_xwin_kernel"
    assert on.params["index16"] == (1 if span <= CAP else 0)
    if span <= CAP:
        assert on.params["xcap"] == CAP


def test_window_of_more_rows_than_one_pass(torch_dev):
    torch, dev = torch_dev
    _, on, _ = check(torch, dev, tall_case(), lanes=4, xwin_rows=1024)
    assert on.params["index16"] == 1 and on.params["lanes"] == 4


def test_short_rows(torch_dev):
    torch, dev = torch_dev
    _, on, _ = check(torch, dev, short_case())
    assert on.params["lanes"] == 2 and on.params["kernel"] == "csr_xwin_kernel"


@pytest.mark.parametrize("per_row", [4, 33], ids=["one-chunk", "pipelined"])
def test_xcd_contiguous_windows(torch_dev, per_row):
    """The rule's own choice (remap on) against the round-robin placement
    forced: placement only, the same bits.  33 entries per row make 2,112 per
    window, two chunks of 1,536: the pipelined schedule; 4 per row the other."""
    torch, dev = torch_dev
    case = many_windows_case(per_row)
    m, x, _ = case
    _, on, y = check(torch, dev, case, lanes=4, xwin_rows=64)
    assert on.params["xcap"] > 2 * 64
    try:
        sa.set_option("xwin_remap", 0)
        assert same_bits(run(torch, dev, on, m, x), y), "placement changes y"
    finally:
        sa.set_option("xwin_remap", None)


@pytest.mark.parametrize("n_rows", [65, 129])
def test_forced_remap_on_few_windows(torch_dev, n_rows):
    """2 and 3 windows placed XCD-contiguously: fewer windows than XCDs."""
    torch, dev = torch_dev
    m, x, _ = rows_case(n_rows)
    _, on, y = check(torch, dev, rows_case(n_rows), lanes=4)
    try:
        sa.set_option("xwin_remap", 1)
        assert same_bits(run(torch, dev, on, m, x), y), "placement changes y"
    finally:
        sa.set_option("xwin_remap", None)


@pytest.mark.parametrize("fmt", ["csr16", "csrf32"])
@pytest.mark.parametrize("which", ["rows129", "tall", "short"])
def test_other_column_and_value_sources(torch_dev, fmt, which):
    """Col16 (csr16) and fp32 values with Col32 (csrf32) through the same
    kernel.  Both sum the same products in the same order as the CSR plan:
    its bits — csrf32 on the matrix it stores, the values rounded to fp32 —
    and the oracle's parity on that matrix."""
    torch, dev = torch_dev
    case, kw = {"rows129": (rows_case(129), dict(lanes=4)), "tall": (tall_case(), dict(lanes=4, xwin_rows=1024)),
                "short": (short_case(), {})}[which]
    m, x, ref = case
    if fmt == "csrf32":
        m = sa.Coo(m.n_rows, m.n_cols, m.row, m.col, m.val.astype(np.float32).astype(np.float64), False, m.label)
        ref = oracle.file_order_spmv(m.n_rows, m.row, m.col, m.val, x)
    dm = sa.to_device(m, fmt, dev, **kw)
    assert "win" in dm.arrays
    y = run(torch, dev, dm, m, x)
    assert_parity(m, y, x, ref)
    assert same_bits(y, run(torch, dev, sa.to_device(m, "csr", dev, **kw), m, x)), f"{fmt} differs from the CSR plan"
