"""The transposed product y = A^T x on the GPU (spmv_plan_prepare_transpose /
spmv_plan_run_t through DeviceMatrix.prepare_transpose / run_t), both modes.

Reference for every y: the oracle on the swapped COO,
oracle.file_order_spmv(n_cols, col, row, val, x), judged by oracle.parity
(rel=1e-6); any fp64 summation order meets it by many orders of magnitude.
x is seeded uniform(-1, 1); y is 3 entries longer than n_cols, NaN in the live
part and 12345.0 in the tail, which must come back bitwise unchanged.  One x
and one reference per matrix are shared by every test that uses it.
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
MODES = ("scatter", "copy")
SENTINEL = 12345.0
TAIL = 3
CSR_PLANS = [{}, {"lanes": 2}, {"lanes": 64}, {"variant": 1}, {"variant": 4}]
PLAN_IDS = ["-".join(f"{k}{v}" for k, v in kw.items()) or "default" for kw in CSR_PLANS]


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch, torch.device("cuda:0")


def _with_ref(m, seed):
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, max(m.n_rows, 1))
    ref = oracle.file_order_spmv(m.n_cols, m.col, m.row, m.val, np.ascontiguousarray(x[: m.n_rows]))
    x.setflags(write=False)
    ref.setflags(write=False)
    return m, x, ref


@functools.lru_cache(maxsize=None)
def golden(name):
    return _with_ref(sa.read_mtx(GOLDEN / f"{name}.mtx"), 7)


@functools.lru_cache(maxsize=None)
def cantlike():
    return _with_ref(sa.gen_cantlike(0), 11)


@functools.lru_cache(maxsize=None)
def rmat():
    return _with_ref(sa.gen_rmat(100_000, 1_000_000, scale=17, seed=1), 13)


def coo(n_rows, n_cols, row, col, val):
    return sa.Coo(n_rows, n_cols, np.asarray(row, np.int32), np.asarray(col, np.int32), np.asarray(val, np.float64))


def to_dev(torch, dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the shared x stays read-only


def new_y(torch, dev, m):
    y = torch.full((m.n_cols + TAIL,), SENTINEL, dtype=torch.float64, device=dev)
    y[: m.n_cols] = float("nan")
    return y


def assert_yt(m, x, ref, y):
    """y (numpy, n_cols + TAIL) against the shared reference; the tail bit by bit."""
    xs = np.ascontiguousarray(x[: m.n_rows])
    assert not np.isnan(y[: m.n_cols]).any(), "NaN left in y"
    bad = oracle.parity(y[: m.n_cols], ref, m.col, m.row, m.val, xs, m.n_cols, rel=1e-6)
    assert bad.size == 0, f"{bad.size} bad columns, first {bad[:5]}: got {y[bad[:5]]} want {ref[bad[:5]]}"
    assert np.array_equal(y[m.n_cols:].view(np.int64), np.full(TAIL, SENTINEL).view(np.int64)), "tail of y written"


def run_t(torch, dev, dm, m, x):
    y = new_y(torch, dev, m)
    dm.run_t(to_dev(torch, dev, x), y)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def check_mode(torch, dev, dm, m, x, ref, mode):
    dm.prepare_transpose(mode)
    info = dm.transpose_info
    assert info["mode"] == mode
    assert_yt(m, x, ref, run_t(torch, dev, dm, m, x))
    return info


def assert_run_still_right(torch, dev, dm, m):
    """A forward run on the same plan."""
    x = sa.ramp_x(m.n_cols)
    y = torch.full((max(m.n_rows, 1),), float("nan"), dtype=torch.float64, device=dev)
    dm.run(torch.from_numpy(x).to(dev), y)
    torch.cuda.synchronize()
    yh = y.cpu().numpy()[: m.n_rows]
    y_ref = oracle.file_order_spmv(m.n_rows, m.row, m.col, m.val, x)
    assert oracle.parity(yh, y_ref, m.row, m.col, m.val, x, m.n_rows, rel=1e-6).size == 0


# ------------------------------------------------------------ 1. fixtures
@pytest.mark.parametrize("kw", CSR_PLANS, ids=PLAN_IDS)
@pytest.mark.parametrize("name", CASES)
def test_golden_fixtures(torch_dev, name, kw):
    torch, dev = torch_dev
    m, x, ref = golden(name)
    dm = sa.to_device(m, "csr", dev, **kw)
    assert dm.transpose_supported
    for mode in MODES:
        info = check_mode(torch, dev, dm, m, x, ref, mode)
        if mode == "scatter":
            assert info["blocks"] == (m.n_rows + 127) // 128 and info["cap"] > 0
            assert info["kernel"] == "csr_t_window_kernel"
        else:
            assert info["owned_bytes"] >= 12 * m.nnz + 8 * (m.n_cols + 1)


# ----------------------------------------------------------- 2. cant-like
def test_cantlike(torch_dev):
    torch, dev = torch_dev
    m, x, ref = cantlike()
    dm = sa.to_device(m, "csr", dev)
    info = check_mode(torch, dev, dm, m, x, ref, "scatter")
    assert info["lds_blocks"] == info["blocks"] > 0 and info["flush_entries"] > 0
    check_mode(torch, dev, dm, m, x, ref, "copy")


# --------------------------------------------------------- 3. skewed rows
@pytest.mark.parametrize("kw", [{}, {"variant": 3}, {"variant": 4, "hot": 4096}],
                         ids=["default", "variant3", "variant4-hot4096"])
def test_rmat(torch_dev, kw):
    """The hot = 4096 plan owns a renumbered column copy; the transposed run
    must read the caller's columns."""
    torch, dev = torch_dev
    m, x, ref = rmat()
    dm = sa.to_device(m, "csr", dev, **kw)
    if kw.get("hot"):
        assert dm.params["H"] > 0 and "hot-column table" in dm.params["plan"]
    info = check_mode(torch, dev, dm, m, x, ref, "scatter")
    assert info["lds_blocks"] < info["blocks"]
    check_mode(torch, dev, dm, m, x, ref, "copy")


# ------------------------------------------------------------ 4. cap edge
def test_cap_edge(torch_dev):
    torch, dev = torch_dev
    m0, _, _ = golden("n67")
    d0 = sa.to_device(m0, "csr", dev)
    d0.prepare_transpose("scatter")
    cap = d0.transpose_info["cap"]
    assert cap > 1
    for last, lds_blocks in ((cap - 1, 1), (cap, 0)):  # span cap: LDS; span cap + 1: global atomics
        m, x, ref = _with_ref(coo(1, cap + 8, [0, 0], [0, last], [1.5, -2.25]), 3)
        dm = sa.to_device(m, "csr", dev)
        info = check_mode(torch, dev, dm, m, x, ref, "scatter")
        assert (info["blocks"], info["lds_blocks"]) == (1, lds_blocks)
        assert info["flush_entries"] == (cap if lds_blocks else 0)
        check_mode(torch, dev, dm, m, x, ref, "copy")


# --------------------------------------------------------- 5. mixed matrix
def test_mixed_blocks(torch_dev):
    """1,000 x 100,000: row i holds columns i..i+7, row 500 also column 99,999,
    so one block of eight spans more than the cap."""
    torch, dev = torch_dev
    rows = np.repeat(np.arange(1000), 8)
    cols = rows + np.tile(np.arange(8), 1000)
    rows, cols = np.append(rows, 500), np.append(cols, 99_999)
    vals = np.random.default_rng(5).uniform(-1.0, 1.0, rows.size)
    m, x, ref = _with_ref(coo(1000, 100_000, rows, cols, vals), 17)
    dm = sa.to_device(m, "csr", dev)
    info = check_mode(torch, dev, dm, m, x, ref, "scatter")
    assert info["blocks"] == 8 and 0 < info["lds_blocks"] < info["blocks"]
    check_mode(torch, dev, dm, m, x, ref, "copy")


# ---------------------------------------------------------- 6. copy bits
def _host_transpose(m):
    ptr, col, val = sa.csr_from_coo(m)
    return sa.csr_transpose(m.n_rows, m.n_cols, ptr, col, val)


@pytest.mark.parametrize("name", ["ragged_shuffled", "duplicates", "n67", "wide"])
def test_copy_mode_bits(torch_dev, name):
    """Copy mode: reproducible, and the bits of a forward CSR plan with default
    options over the host-built A^T (csr_from_coo is stable, so the row-sorted
    COO of A^T reproduces the same three arrays)."""
    torch, dev = torch_dev
    m, x, ref = golden(name)
    dm = sa.to_device(m, "csr", dev)
    dm.prepare_transpose("copy")
    y1, y2 = run_t(torch, dev, dm, m, x), run_t(torch, dev, dm, m, x)
    assert_yt(m, x, ref, y1)
    assert np.array_equal(y1.view(np.int64), y2.view(np.int64))
    t_ptr, t_col, t_val = _host_transpose(m)
    coo_t = coo(m.n_cols, m.n_rows, np.repeat(np.arange(m.n_cols), np.diff(t_ptr)), t_col, t_val)
    fwd = sa.to_device(coo_t, "csr", dev)
    y = torch.full((m.n_cols,), float("nan"), dtype=torch.float64, device=dev)
    fwd.run(to_dev(torch, dev, x), y)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy().view(np.int64), y1[: m.n_cols].view(np.int64))


@pytest.mark.parametrize("name", ["ragged_shuffled", "duplicates", "colmajor", "wide"])
def test_dev_csr_transpose_equals_host(torch_dev, name):
    torch, dev = torch_dev
    m, _, _ = golden(name)
    dm = sa.to_device(m, "csr", dev)
    d_ptr, d_col, d_val = (t.cpu().numpy() for t in sa.dev_csr_transpose(dm))
    t_ptr, t_col, t_val = _host_transpose(m)
    assert np.array_equal(d_ptr, t_ptr)
    assert np.array_equal(d_col, t_col)
    assert np.array_equal(d_val.view(np.int64), t_val.view(np.int64))


def test_dev_csr_transpose_refuses_a_bad_column(torch_dev):
    torch, dev = torch_dev
    m, _, _ = golden("n67")
    dm = sa.to_device(m, "csr", dev)
    bad = sa.DeviceMatrix("csr", m.n_rows, m.n_cols - 1, m.nnz, dev, arrays=dm.arrays)  # the last column is out of range
    assert int(dm.arrays["col"].max()) == m.n_cols - 1
    with pytest.raises(sa.SpmvError) as e:
        sa.dev_csr_transpose(bad)
    assert e.value.rc == sa.OTHER_ERROR


# ---------------------------------------------------------- 7. lifecycle
def test_lifecycle(torch_dev):
    torch, dev = torch_dev
    m, x, ref = golden("ragged_shuffled")
    dm = sa.to_device(m, "csr", dev)
    owned = sa.plan_info(dm)["owned_bytes"]
    info = dm.transpose_info
    assert info["mode"] is None and info["owned_bytes"] == 0
    y = new_y(torch, dev, m)
    before = y.clone()
    with pytest.raises(sa.SpmvError) as e:
        dm.run_t(to_dev(torch, dev, x), y)
    assert e.value.rc == sa.OTHER_ERROR
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int64), before.view(torch.int64)), "a refused run wrote y"
    assert_run_still_right(torch, dev, dm, m)

    s = check_mode(torch, dev, dm, m, x, ref, "scatter")
    assert s["owned_bytes"] == 8 * s["blocks"] > 0
    dm.prepare_transpose("scatter")  # the same mode again: a no-op
    assert dm.transpose_info == s
    assert_run_still_right(torch, dev, dm, m)

    c = check_mode(torch, dev, dm, m, x, ref, "copy")
    assert c["owned_bytes"] >= 12 * m.nnz + 8 * (m.n_cols + 1)
    assert (c["blocks"], c["lds_blocks"], c["flush_entries"], c["cap"]) == (0, 0, 0, 0)
    assert c["kernel"].startswith("csr_")
    assert_run_still_right(torch, dev, dm, m)

    dm.prepare_transpose(None)
    info = dm.transpose_info
    assert info["mode"] is None and info["owned_bytes"] == 0 and info["kernel"] == ""
    with pytest.raises(sa.SpmvError) as e:
        dm.run_t(to_dev(torch, dev, x), y)
    assert e.value.rc == sa.OTHER_ERROR
    assert_run_still_right(torch, dev, dm, m)

    pi = sa.PlanInfo()
    assert sa.hip_lib().spmv_plan_get_info(dm.plan, ctypes.byref(pi)) == sa.SUCCESS
    assert pi.owned_bytes == owned == sa.plan_info(dm)["owned_bytes"]
    assert sa.hip_lib().spmv_plan_prepare_transpose(dm.plan, 3) == sa.OTHER_ERROR  # unknown mode
    check_mode(torch, dev, dm, m, x, ref, "copy")  # destroyed with the plan


def test_null_vectors_refused(torch_dev):
    torch, dev = torch_dev
    m, x, _ = golden("ragged_shuffled")
    dm = sa.to_device(m, "csr", dev)
    dm.prepare_transpose("scatter")
    lib = sa.hip_lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    xd, y = to_dev(torch, dev, x), new_y(torch, dev, m)
    assert lib.spmv_plan_run_t(dm.plan, None, y.data_ptr(), st) == sa.OTHER_ERROR
    assert lib.spmv_plan_run_t(dm.plan, xd.data_ptr(), None, st) == sa.OTHER_ERROR
    assert b"NULL" in lib.spmv_last_error()


# ----------------------------------------------------------- 8. refusals
@pytest.mark.parametrize("fmt", ["coo", "ell", "sell", "cmrs", "sell16"])
def test_refused_formats(torch_dev, fmt):
    torch, dev = torch_dev
    m, _, _ = golden("ragged_shuffled")
    kw = {"ell_max_padding": None} if fmt == "ell" else {}
    dm = sa.to_device(m, fmt, dev, **kw)
    assert dm.transpose_supported is False
    for mode in MODES:
        with pytest.raises(sa.SpmvError) as e:
            dm.prepare_transpose(mode)
        assert e.value.rc == sa.OTHER_ERROR
    assert dm.transpose_info["mode"] is None
    assert_run_still_right(torch, dev, dm, m)


# --------------------------------------------------------------- 9. graph
@pytest.mark.parametrize("mode", MODES)
def test_graph_capture(torch_dev, mode):
    """One run_t captured on a single stream (no parallel branches), replayed,
    x overwritten in place, replayed again."""
    torch, dev = torch_dev
    m, x, ref = golden("ragged_shuffled")
    m2, x2, ref2 = _with_ref(m, 23)
    dm = sa.to_device(m, "csr", dev)
    dm.prepare_transpose(mode)
    xd = to_dev(torch, dev, x)
    y = new_y(torch, dev, m)
    dm.run_t(xd, y)  # first-call setup outside the capture
    torch.cuda.synchronize()
    y[: m.n_cols] = float("nan")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dm.run_t(xd, y)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert_yt(m, x, ref, y.cpu().numpy())
    xd.copy_(to_dev(torch, dev, x2))
    y[: m.n_cols] = float("nan")
    g.replay()
    torch.cuda.synchronize()
    assert_yt(m2, x2, ref2, y.cpu().numpy())
