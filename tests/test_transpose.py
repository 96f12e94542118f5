"""The transposed product y = A^T x, the parts that need no GPU: the C-ABI
symbols and their NULL answers, the host builder spmv_csr_transpose against a
numpy restatement, the host loop spmv_cpu_csr_t against the oracle and run_t's
argument checks.

Reference for every y: the oracle on the swapped COO,
oracle.file_order_spmv(n_cols, col, row, val, x), judged by oracle.parity
(rel=1e-6).  x is seeded uniform(-1, 1); y is 3 entries longer than n_cols,
NaN in the live part and 12345.0 in the tail, which must come back bitwise
unchanged.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import spmv_amd as sa
from conftest import GOLDEN, golden_cases
from oracle import oracle

CASES = [c["name"] for c in golden_cases()]
SENTINEL = 12345.0
TAIL = 3

HIP_NEW = ("spmv_plan_transpose_supported", "spmv_plan_prepare_transpose", "spmv_plan_get_transpose_info",
           "spmv_plan_run_t", "spmv_dev_csr_transpose")
HOST_NEW = ("spmv_csr_transpose", "spmv_cpu_csr_t")


def make_xy(m, seed=0):
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, max(m.n_rows, 1))
    y = np.full(m.n_cols + TAIL, SENTINEL)
    y[: m.n_cols] = np.nan
    return x, y


def assert_yt(m, x, y):
    """y[:n_cols] against the oracle on the swapped COO; the tail bit by bit."""
    xs = np.ascontiguousarray(x[: m.n_rows])
    ref = oracle.file_order_spmv(m.n_cols, m.col, m.row, m.val, xs)
    bad = oracle.parity(y[: m.n_cols], ref, m.col, m.row, m.val, xs, m.n_cols, rel=1e-6)
    assert bad.size == 0, f"{bad.size} bad columns, first {bad[:5]}: got {y[bad[:5]]} want {ref[bad[:5]]}"
    assert np.array_equal(y[m.n_cols:].view(np.int64), np.full(TAIL, SENTINEL).view(np.int64)), "tail of y written"


def test_case_set():
    assert {"all_empty", "one", "tall", "wide", "duplicates"} <= set(CASES)


def test_symbols_exported_and_bound():
    hip = ctypes.CDLL(str(sa.LIB_DIR / "libspmv_hip.so"))
    host = ctypes.CDLL(str(sa.LIB_DIR / "libspmv_host.so"))
    for name in HIP_NEW:
        assert name in sa.HIP_SYMBOLS and hasattr(hip, name)
        assert getattr(sa.hip_lib(), name).argtypes == sa.HIP_SYMBOLS[name][1]
    for name in HOST_NEW:
        assert name in sa.HOST_SYMBOLS and hasattr(host, name)
        assert getattr(sa.host_lib(), name).argtypes == sa.HOST_SYMBOLS[name][1]
    assert ctypes.sizeof(sa.TransposeInfo) == 8 + 4 * 8 + 64
    assert sa.TRANSPOSE_MODES == {None: 0, "scatter": 1, "copy": 2}


def test_null_plan_answers():
    lib = sa.hip_lib()
    assert lib.spmv_plan_transpose_supported(None) == 0
    info = sa.TransposeInfo()
    for what, rc in {
        "run_t": lib.spmv_plan_run_t(None, None, None, None),
        "prepare": lib.spmv_plan_prepare_transpose(None, 1),
        "info": lib.spmv_plan_get_transpose_info(None, ctypes.byref(info)),
    }.items():
        assert rc == sa.OTHER_ERROR, what
    for call in (lambda: lib.spmv_plan_run_t(None, None, None, None),
                 lambda: lib.spmv_plan_prepare_transpose(None, 1),
                 lambda: lib.spmv_plan_get_transpose_info(None, ctypes.byref(info))):
        call()
        assert b"NULL" in lib.spmv_last_error()


@pytest.mark.parametrize("name", CASES)
def test_csr_transpose_golden(name):
    m = sa.read_mtx(GOLDEN / f"{name}.mtx")
    ptr, col, val = sa.csr_from_coo(m)
    t_ptr, t_col, t_val = sa.csr_transpose(m.n_rows, m.n_cols, ptr, col, val)
    rowids = np.repeat(np.arange(m.n_rows, dtype=np.int32), np.diff(ptr))
    o = np.argsort(col, kind="stable")
    want_ptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=m.n_cols))]).astype(np.int64)
    assert t_ptr.dtype == np.int64 and t_col.dtype == np.int32 and t_val.dtype == np.float64
    assert np.array_equal(t_ptr, want_ptr)
    assert np.array_equal(t_col, rowids[o])
    assert np.array_equal(t_val.view(np.int64), val[o].view(np.int64))


def test_csr_transpose_refuses_bad_input():
    m = sa.read_mtx(GOLDEN / "n67.mtx")
    ptr, col, val = sa.csr_from_coo(m)
    for bad_col in (m.n_cols, -1):
        c = col.copy()
        c[len(c) // 2] = bad_col
        with pytest.raises(sa.SpmvError) as e:
            sa.csr_transpose(m.n_rows, m.n_cols, ptr, c, val)
        assert e.value.rc == sa.OTHER_ERROR
    f = sa.host_lib().spmv_csr_transpose
    t_ptr = np.zeros(m.n_cols + 1, np.int64)
    t_col = np.zeros(m.nnz, np.int32)
    t_val = np.zeros(m.nnz)
    good = [m.n_rows, m.n_cols, ptr.ctypes.data, col.ctypes.data, val.ctypes.data, t_ptr.ctypes.data,
            t_col.ctypes.data, t_val.ctypes.data]
    assert f(*good) == sa.SUCCESS
    for i in range(2, 8):  # every array NULL in turn
        args = list(good)
        args[i] = None
        assert f(*args) == sa.OTHER_ERROR, i
    assert f(-1, *good[1:]) == sa.OTHER_ERROR
    assert f(m.n_rows, -1, *good[2:]) == sa.OTHER_ERROR


@pytest.mark.parametrize("name", CASES)
def test_cpu_csr_t_golden(name):
    m = sa.read_mtx(GOLDEN / f"{name}.mtx")
    ptr, col, val = sa.csr_from_coo(m)
    x, y = make_xy(m)
    sa.cpu_csr_t(m.n_rows, m.n_cols, ptr, col, val, x, y)
    assert not np.isnan(y).any()
    assert_yt(m, x, y)
    if m.nnz == 0:
        assert not y[: m.n_cols].any()
    # deterministic: a second run gives the same bits
    y2 = np.full_like(y, SENTINEL)
    sa.cpu_csr_t(m.n_rows, m.n_cols, ptr, col, val, x, y2)
    assert np.array_equal(y.view(np.int64), y2.view(np.int64))


def test_all_empty_gives_zeros():
    m = sa.read_mtx(GOLDEN / "all_empty.mtx")
    ptr, col, val = sa.csr_from_coo(m)
    x, y = make_xy(m)
    sa.cpu_csr_t(m.n_rows, m.n_cols, ptr, col, val, x, y)
    assert m.n_cols > 0 and not y[: m.n_cols].any()
    assert np.array_equal(y[m.n_cols:], np.full(TAIL, SENTINEL))


def test_cpu_csr_t_refuses_bad_input():
    m = sa.read_mtx(GOLDEN / "n67.mtx")
    ptr, col, val = sa.csr_from_coo(m)
    x, y = make_xy(m)
    c = col.copy()
    c[-1] = m.n_cols
    with pytest.raises(sa.SpmvError) as e:
        sa.cpu_csr_t(m.n_rows, m.n_cols, ptr, c, val, x, y)
    assert e.value.rc == sa.OTHER_ERROR
    assert np.array_equal(y[m.n_cols:], np.full(TAIL, SENTINEL))
    for bad_x, bad_y in ((x[:-1], y), (x, y[: m.n_cols - 1]), (x.astype(np.float32), y), (x, y[::2]), (list(x), y)):
        with pytest.raises(sa.SpmvError) as e:
            sa.cpu_csr_t(m.n_rows, m.n_cols, ptr, col, val, bad_x, bad_y)
        assert e.value.rc == sa.OTHER_ERROR


def test_run_t_checks_arguments_before_the_c_call():
    """A bare DeviceMatrix (no plan, nothing on a device): every bad argument
    is an SpmvError(OTHER_ERROR) raised in Python."""
    import torch

    dm = sa.DeviceMatrix("csr", 4, 6, 4, "cuda:0", plan=None)
    assert dm.transpose_supported is False
    gx = torch.zeros(4, dtype=torch.float64)
    gy = torch.zeros(6, dtype=torch.float64)
    bad = {
        "cpu tensors, no plan": (gx, gy),
        "x dtype": (torch.zeros(4, dtype=torch.float32), gy),
        "y dtype": (gx, torch.zeros(6, dtype=torch.float32)),
        "x too short": (torch.zeros(3, dtype=torch.float64), gy),
        "y too short": (gx, torch.zeros(5, dtype=torch.float64)),
        "x strided": (torch.zeros(8, dtype=torch.float64)[::2], gy),
        "y strided": (gx, torch.zeros(12, dtype=torch.float64)[::2]),
        "not a tensor": (np.zeros(4), gy),
    }
    for what, (x, y) in bad.items():
        with pytest.raises(sa.SpmvError) as e:
            dm.run_t(x, y)
        assert e.value.rc == sa.OTHER_ERROR, what
    # a tensor on the right device type but no plan: still refused in Python
    mx = torch.zeros(4, dtype=torch.float64, device="meta")
    with pytest.raises(sa.SpmvError) as e:
        dm.run_t(mx, mx)
    assert e.value.rc == sa.OTHER_ERROR
    for call in (lambda: dm.prepare_transpose("scatter"), lambda: dm.prepare_transpose("sideways"),
                 lambda: dm.transpose_info):
        with pytest.raises(sa.SpmvError) as e:
            call()
        assert e.value.rc == sa.OTHER_ERROR
