"""CSR x-window plans with the plan-owned 16-bit window-relative column copy
(SPMV_OPT_CSR_COL16, spmv_plan_info.index16 = 1 on a CSR plan).

Every case builds three plans of one matrix — the switch off, the switch on,
and variant 3 with global x gathers — and wants the same bits of y from all
three, plus the oracle's parity rule (tests/test_gpu_parity.py).  The copy
only changes where a column comes from, never a product or the order of a
sum, so nothing weaker than bit equality is right.

A window also loads entries of its neighbours (the lead-in entries before its
first 32-entry-aligned chunk, the partner of a pair that straddles its range
end); their 16-bit offsets are relative to ANOTHER window's base, so the
kernel bounds every LDS gather to the running window.  The disjoint-window
matrices below make those offsets differ wildly from the running window's.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import spmv_amd as sa
from conftest import GOLDEN, golden_cases
from oracle import oracle

pytestmark = pytest.mark.gpu

CASES = [c["name"] for c in golden_cases()]


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch, torch.device("cuda:0")


def distinct_x(n, seed):
    """n distinct values in (-1, 1), shuffled."""
    n = max(n, 1)
    x = (np.random.default_rng(seed).permutation(n).astype(np.float64) + 0.25) / n * 2.0 - 1.0
    assert np.unique(x).size == n
    return x


def _with_ref(m, seed):
    x = distinct_x(m.n_cols, seed)
    ref = oracle.file_order_spmv(m.n_rows, m.row, m.col, m.val, x)
    x.setflags(write=False)
    ref.setflags(write=False)
    return m, x, ref


@functools.lru_cache(maxsize=None)
def cantlike():
    return _with_ref(sa.gen_cantlike(0), 3)


@functools.lru_cache(maxsize=None)
def golden(name):
    return _with_ref(sa.read_mtx(GOLDEN / f"{name}.mtx"), 5)


@functools.lru_cache(maxsize=None)
def disjoint(stride, width, odd):
    """1,000 rows of 37..91 entries; the 64 rows of window k take their columns
    from [stride·k, stride·k + width).  Row lengths are random, so the row
    offsets of the windows are no multiples of 32; the last row is trimmed by
    one entry where needed so that nnz is odd / even as asked."""
    rng = np.random.default_rng(17)
    n_rows, rpw = 1000, 64
    lens = rng.integers(37, 92, n_rows)
    if (int(lens.sum()) & 1) != int(odd):
        lens[-1] -= 1
    n_win = (n_rows + rpw - 1) // rpw
    row = np.repeat(np.arange(n_rows, dtype=np.int32), lens)
    col = np.concatenate([np.sort(rng.choice(width, n, replace=False)) + stride * (r // rpw)
                          for r, n in enumerate(lens)]).astype(np.int32)
    val = rng.uniform(-1.0, 1.0, row.size)
    m = sa.Coo(n_rows, stride * n_win, row, col, val, False, f"disjoint windows {stride}/{width} nnz {row.size}")
    ptr = np.concatenate([[0], np.cumsum(lens)])
    assert (m.nnz & 1) == int(odd) and all(ptr[k] % 32 for k in range(rpw, n_rows, rpw))
    return _with_ref(m, 19)


@functools.lru_cache(maxsize=None)
def wide_random():
    return _with_ref(sa.gen_random(2000, 200000, 0, 60), 23)


@functools.lru_cache(maxsize=None)
def banded(interior):
    """20,000 rows x 16 entries, columns row - 8 .. row + 7 modulo n; interior:
    without the first and last 8 rows, the ones whose band wraps around."""
    n = 20_000
    r0, r1 = (8, n - 8) if interior else (0, n)
    ptr, col, val = sa.gen_banded_csr(n, r0, r1)
    row = np.repeat(np.arange(r1 - r0, dtype=np.int32), np.diff(ptr))
    return _with_ref(sa.Coo(r1 - r0, n, row, col, val, False, f"banded rows {r0}..{r1} of {n} x 16"), 29)


def c_info(dm):
    """spmv_plan_get_info asked again (dm.params holds the answer at creation)."""
    pi = sa.PlanInfo()
    assert sa.hip_lib().spmv_plan_get_info(dm.plan, ctypes.byref(pi)) == sa.SUCCESS
    return {name: getattr(pi, name) for name, _ in pi._fields_}


def three_plans(dev, m, **kw):
    """(switch off, switch on, variant 3 with global gathers)."""
    try:
        sa.set_option("csr_col16", 0)
        off = sa.to_device(m, "csr", dev, **kw)
        sa.set_option("csr_col16", 1)
        on = sa.to_device(m, "csr", dev, **kw)
    finally:
        sa.set_option("csr_col16", None)
    kw3 = {k: v for k, v in kw.items() if k == "lanes"}
    v3 = sa.to_device(m, "csr", dev, variant=3, xwin=False, **kw3)
    assert off.params["index16"] == 0 and v3.params["index16"] == 0
    if on.params["index16"]:
        assert "16-bit window column offsets" in on.params["plan"] and on.params["kernel"] == "csr_xwin_kernel"
        assert on.params["owned_bytes"] >= off.params["owned_bytes"] + 2 * m.nnz
    else:
        assert on.params["owned_bytes"] == off.params["owned_bytes"] and on.params["plan"] == off.params["plan"]
    return off, on, v3


def run(torch, dev, dm, m, x):
    xd = torch.from_numpy(np.array(x, order="C")).to(dev)
    y = torch.full((max(m.n_rows, 1),), float("nan"), dtype=torch.float64, device=dev)
    dm.run(xd, y)
    torch.cuda.synchronize()
    return y.cpu().numpy()[: m.n_rows]


def assert_same_bits(ys, label):
    for name, y in zip(("switch on", "variant 3"), ys[1:]):
        assert np.array_equal(ys[0].view(np.int64), y.view(np.int64)), f"{label}: {name} differs from switch off"


def assert_parity(m, y, x, ref):
    bad = oracle.parity(y, ref, m.row, m.col, m.val, x, m.n_rows, rel=1e-6)
    assert bad.size == 0, f"{bad.size} bad rows, first {bad[:5]}: got {y[bad[:5]]} want {ref[bad[:5]]}"


def check(torch, dev, m, x, ref, **kw):
    plans = three_plans(dev, m, **kw)
    ys = [run(torch, dev, dm, m, x) for dm in plans]
    assert_same_bits(ys, m.label)
    assert_parity(m, ys[1], x, ref)
    return plans


@pytest.mark.parametrize("lanes", [0, 2, 16])
def test_cantlike(torch_dev, lanes):
    torch, dev = torch_dev
    m, x, ref = cantlike()
    off, on, _ = check(torch, dev, m, x, ref, lanes=lanes)
    assert on.params["index16"] == 1
    assert on.params["owned_bytes"] - off.params["owned_bytes"] >= 2 * m.nnz


@pytest.mark.parametrize("name", CASES)
def test_golden_fixtures(torch_dev, name):
    torch, dev = torch_dev
    m, x, ref = golden(name)
    _, on, _ = check(torch, dev, m, x, ref)
    if m.nnz < 2:
        assert on.params["index16"] == 0


# (1500, 1400) are the figures of the request for this test: there the window
# table (which counts a window's lead-in entries, columns of the window
# before) spans about 2,900 columns from the second window on, more than the
# 2,048 of the LDS cap, so the plan keeps the int32 columns: the fallback must
# give the same bits.  (1000, 900) keeps every window under the cap with the
# lead-in included, so the copy IS built and the neighbours' offsets (up to
# ~1,900, relative to the previous window's base) meet the bound: window 0
# spans 900 columns and gathers the straddling partner of window 1's first
# entry, whose offset is about 1,000 or more.
@pytest.mark.parametrize("odd", [False, True], ids=["even", "odd"])
@pytest.mark.parametrize("stride,width", [(1500, 1400), (1000, 900)])
def test_disjoint_windows(torch_dev, stride, width, odd):
    torch, dev = torch_dev
    m, x, ref = disjoint(stride, width, odd)
    _, on, _ = check(torch, dev, m, x, ref, lanes=4)
    # (4 lanes per row and a small matrix: one-group windows of 256/4 = 64 rows)
    assert on.params["index16"] == (1 if stride + width <= 2048 else 0)


@pytest.mark.parametrize("odd", [False, True], ids=["even", "odd"])
@pytest.mark.parametrize("stride,width", [(1500, 1400), (1000, 900)])
def test_disjoint_windows_nonfinite_x(torch_dev, stride, width, odd):
    """±inf and NaN in x: a never-summed entry whose gather is bounded reads
    another x value than the int32 path does; y must not notice.  The rows
    that gather a planted value are non-finite in the oracle too (the parity
    rule says nothing there: the class must agree); the others keep the rule."""
    torch, dev = torch_dev
    m, x0, _ = disjoint(stride, width, odd)
    x = np.array(x0)
    # the first and last column of windows 0-2, and a few anywhere
    planted = [0, width - 1, stride, stride + width - 1, 2 * stride, 2 * stride + width - 1, 5 * stride + 7,
               9 * stride + width // 2]
    for i, c in enumerate(planted):
        x[c] = (np.inf, -np.inf, np.nan)[i % 3]
    with np.errstate(invalid="ignore"):
        ref = oracle.file_order_spmv(m.n_rows, m.row, m.col, m.val, x)
    plans = three_plans(dev, m, lanes=4)
    ys = [run(torch, dev, dm, m, x) for dm in plans]
    assert_same_bits(ys, m.label)
    fin = np.isfinite(ref)
    assert 0 < fin.sum() < m.n_rows
    assert np.array_equal(np.isfinite(ys[1]), fin)
    keep = fin[m.row]
    xf = np.where(np.isfinite(x), x, 0.0)  # the kept rows gather no planted column
    bad = oracle.parity(ys[1][fin], ref[fin], np.cumsum(fin)[m.row[keep]] - 1, m.col[keep], m.val[keep], xf,
                        int(fin.sum()), rel=1e-6)
    assert bad.size == 0


def test_windows_wider_than_cap(torch_dev):
    torch, dev = torch_dev
    m, x, ref = wide_random()
    _, on, _ = check(torch, dev, m, x, ref)
    assert on.params["index16"] == 0


@pytest.mark.parametrize("xwin_rows", [0, 256], ids=["one-group", "two-group"])
@pytest.mark.parametrize("interior", [False, True], ids=["whole", "interior"])
def test_banded(torch_dev, interior, xwin_rows):
    """L = 2, R = 4: one-group windows of one chunk (the small-matrix rule,
    MODE 0) and two-group windows (MODE 3, the next group's chunk pipelined).
    The whole matrix's first and last windows hold the rows whose band wraps
    around, 20,000 columns wide: no copy, the plan runs as before.  Without
    those rows every window fits and the copy is built."""
    torch, dev = torch_dev
    m, x, ref = banded(interior)
    _, on, _ = check(torch, dev, m, x, ref, xwin_rows=xwin_rows)
    assert on.params["lanes"] == 2 and on.params["index16"] == int(interior)


def test_multi_and_transposed_leave_the_plan(torch_dev):
    """run_multi and the transposed run read the caller's int32 columns: right
    results, and spmv_plan_get_info says what it said."""
    torch, dev = torch_dev
    m, x, ref = cantlike()
    try:
        sa.set_option("csr_col16", 1)
        dm = sa.to_device(m, "csr", dev)
    finally:
        sa.set_option("csr_col16", None)
    before = c_info(dm)
    assert before["index16"] == 1
    k = 3
    X = np.stack([x, x[::-1], 0.5 * x], axis=1)
    Y = torch.full((m.n_rows, k), float("nan"), dtype=torch.float64, device=dev)
    dm.run_multi(torch.from_numpy(np.ascontiguousarray(X)).to(dev), Y)
    xt = distinct_x(m.n_rows, 31)
    dm.prepare_transpose("scatter")
    yt = torch.full((m.n_cols,), float("nan"), dtype=torch.float64, device=dev)
    dm.run_t(torch.from_numpy(xt).to(dev), yt)
    torch.cuda.synchronize()
    assert c_info(dm) == before
    Yh = Y.cpu().numpy()
    for j in range(k):
        xj = np.ascontiguousarray(X[:, j])
        assert_parity(m, Yh[:, j], xj, ref if j == 0 else oracle.file_order_spmv(m.n_rows, m.row, m.col, m.val, xj))
    ref_t = oracle.file_order_spmv(m.n_cols, m.col, m.row, m.val, xt)
    bad = oracle.parity(yt.cpu().numpy(), ref_t, m.col, m.row, m.val, xt, m.n_cols, rel=1e-6)
    assert bad.size == 0
    assert_parity(m, run(torch, dev, dm, m, x), x, ref)  # and the forward run still uses its copy
