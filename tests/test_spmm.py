"""Multi-vector SpMV Y = A·X, the parts that need no GPU: the C-ABI symbols
and their NULL-plan answers, the host loop spmv_cpu_csr_multi against the
oracle (per column, the project's 1e-6 per-row criterion), the byte model and
run_multi's argument checks.

Layout under test (include/spmv.h): X[c*ldx + j], Y[i*ldy + j], j < k.  Every
Y starts as NaN in the k live columns and 12345.0 in the ldy - k padding
columns; the padding must come back bitwise unchanged.
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


def make_xy(m, k, ldx, ldy, seed=0):
    rng = np.random.default_rng(seed)
    Xbuf = np.full((max(m.n_cols, 1), ldx), 777.0)
    Xbuf[:, :k] = rng.uniform(-1.0, 1.0, (max(m.n_cols, 1), k))
    Ybuf = np.full((max(m.n_rows, 1), ldy), SENTINEL)
    Ybuf[:, :k] = np.nan
    return Xbuf, Ybuf


def assert_columns(m, X, Y, k):
    for j in range(k):
        x = np.ascontiguousarray(X[: m.n_cols, j])
        y_ref = oracle.file_order_spmv(m.n_rows, m.row, m.col, m.val, x)
        bad = oracle.parity(Y[: m.n_rows, j], y_ref, m.row, m.col, m.val, x, m.n_rows, rel=1e-6)
        assert bad.size == 0, f"column {j}: {bad.size} bad rows, first {bad[:5]}"


def test_null_plan_answers():
    lib = sa.hip_lib()
    assert lib.spmv_plan_run_multi(None, 1, None, 1, None, 1, None) == sa.OTHER_ERROR
    assert b"NULL" in lib.spmv_last_error()
    assert lib.spmv_plan_multi_supported(None) == 0


def test_symbols_exported_and_bound():
    for name in ("spmv_plan_run_multi", "spmv_plan_multi_supported"):
        assert name in sa.HIP_SYMBOLS
        assert getattr(sa.hip_lib(), name).argtypes == sa.HIP_SYMBOLS[name][1]
    assert "spmv_cpu_csr_multi" in sa.HOST_SYMBOLS
    assert hasattr(ctypes.CDLL(str(sa.LIB_DIR / "libspmv_host.so")), "spmv_cpu_csr_multi")
    assert hasattr(ctypes.CDLL(str(sa.LIB_DIR / "libspmv_hip.so")), "spmv_plan_run_multi")


@pytest.mark.parametrize("padded", [False, True], ids=["contiguous", "padded"])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("name", CASES)
def test_cpu_csr_multi_golden(name, k, padded):
    m = sa.read_mtx(GOLDEN / f"{name}.mtx")
    ptr, col, val = sa.csr_from_coo(m)
    ldx, ldy = (k + 3, k + 1) if padded else (k, k)
    Xbuf, Ybuf = make_xy(m, k, ldx, ldy)
    sa.cpu_csr_multi(m.n_rows, ptr, col, val, Xbuf[:, :k], Ybuf[:, :k])
    if m.n_rows > 0:
        assert_columns(m, Xbuf, Ybuf, k)
    assert np.array_equal(Ybuf[:, k:].view(np.int64), np.full((Ybuf.shape[0], ldy - k), SENTINEL).view(np.int64))
    if m.n_rows == 0:  # nothing to write: the live columns keep their NaN
        assert np.isnan(Ybuf[:, :k]).all()


def test_cpu_csr_multi_refuses_bad_arguments():
    m = sa.read_mtx(GOLDEN / "n67.mtx")
    ptr, col, val = sa.csr_from_coo(m)
    X = np.ones((m.n_cols, 4))
    Y = np.zeros((m.n_rows, 4))
    f = sa.host_lib().spmv_cpu_csr_multi
    args = (m.n_rows, ptr.ctypes.data, col.ctypes.data, val.ctypes.data)
    assert f(*args, 0, X.ctypes.data, 4, Y.ctypes.data, 4) == sa.OTHER_ERROR  # k = 0
    assert f(*args, 4, X.ctypes.data, 3, Y.ctypes.data, 4) == sa.OTHER_ERROR  # ldx < k
    assert f(*args, 4, X.ctypes.data, 4, Y.ctypes.data, 3) == sa.OTHER_ERROR  # ldy < k
    assert not Y.any()  # refused before anything was written
    with pytest.raises(sa.SpmvError) as e:
        sa.cpu_csr_multi(m.n_rows, ptr, col, val, X, Y, k=0)
    assert e.value.rc == sa.OTHER_ERROR


def test_bytes_alg_multi():
    # 12·nnz + 4·(N+1) + 8·k·(N+M) = 48,088,596 + 249,808 + 3,996,864 on the
    # cant-like matrix at k = 4 (the 52.3 MB of the byte model)
    assert sa.bytes_alg_multi(62451, 62451, 4007383, 4) == 52_335_268
    assert sa.bytes_alg_multi(62451, 62451, 4007383, 8) == 56_332_132
    assert sa.bytes_alg_multi(62451, 62451, 4007383, 1) == sa.bytes_alg(62451, 62451, 4007383)
    assert sa.bytes_alg_multi(7, 5, 11, 1) == sa.bytes_alg(7, 5, 11)


def test_run_multi_checks_arguments_before_the_c_call():
    """A bare DeviceMatrix (no plan, nothing on a device): every bad argument
    is an SpmvError(OTHER_ERROR) raised in Python."""
    import torch

    dm = sa.DeviceMatrix("csr", 4, 4, 4, "cuda:0", plan=None)
    assert dm.multi_supported is False
    good = torch.zeros(4, 2, dtype=torch.float64)
    bad = {
        "cpu tensors": (good, good.clone()),
        "dtype": (torch.zeros(4, 2, dtype=torch.float32), good),
        "rank": (torch.zeros(4, dtype=torch.float64), good),
        "rank3": (good, torch.zeros(4, 2, 1, dtype=torch.float64)),
        "k differs": (torch.zeros(4, 3, dtype=torch.float64), good),
        "inner stride": (torch.zeros(4, 4, dtype=torch.float64)[:, ::2], good),
        "row stride": (torch.as_strided(torch.zeros(8, dtype=torch.float64), (4, 2), (1, 1)), good),
        "too few rows": (torch.zeros(3, 2, dtype=torch.float64), good),
        "not a tensor": (np.zeros((4, 2)), good),
    }
    for what, (X, Y) in bad.items():
        with pytest.raises(sa.SpmvError) as e:
            dm.run_multi(X, Y)
        assert e.value.rc == sa.OTHER_ERROR, what
