"""The multi-vector transposed product Y = A^T X, the parts that need no GPU:
the C-ABI symbols and their NULL-plan answers, the host loop
spmv_cpu_csr_t_multi (per column against the oracle on the swapped COO and
bit for bit against spmv_cpu_csr_t), its refusals, run_t_multi's argument
checks and the sanitizer harness tests/san/transpose_multi_harness.c.

Layout under test (include/spmv.h): X[r*ldx + j], Y[c*ldy + j], j < k.  X's
gaps hold NaN; Y's gaps and a 3-row tail hold 12345.0 and must come back
bitwise unchanged; Y's live part starts as NaN.
"""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import spmv_amd as sa
from conftest import GOLDEN, golden_cases
from oracle import oracle

REPO = Path(__file__).resolve().parents[1]
CASES = [c["name"] for c in golden_cases()]
SENTINEL = 12345.0
TAIL = 3

HIP_NEW = ("spmv_plan_run_t_multi", "spmv_plan_get_transpose_multi_info")
HOST_NEW = ("spmv_cpu_csr_t_multi",)


def make_xy(m, k, ldx, ldy, seed=0):
    rng = np.random.default_rng(seed)
    Xbuf = np.full((max(m.n_rows, 1), ldx), np.nan)
    Xbuf[:, :k] = rng.uniform(-1.0, 1.0, (Xbuf.shape[0], k))
    Ybuf = np.full((m.n_cols + TAIL, ldy), SENTINEL)
    Ybuf[: m.n_cols, :k] = np.nan
    return Xbuf, Ybuf


def untouched(m, Ybuf, k):
    """Y's gaps (j >= k) and its tail rows, bit for bit."""
    want = np.full(Ybuf.shape, SENTINEL).view(np.int64)
    got = Ybuf.view(np.int64)
    return np.array_equal(got[:, k:], want[:, k:]) and np.array_equal(got[m.n_cols:], want[m.n_cols:])


def test_symbols_exported_and_bound():
    hip = ctypes.CDLL(str(sa.LIB_DIR / "libspmv_hip.so"))
    host = ctypes.CDLL(str(sa.LIB_DIR / "libspmv_host.so"))
    for name in HIP_NEW:
        assert name in sa.HIP_SYMBOLS and hasattr(hip, name)  # found by its C name
        assert getattr(sa.hip_lib(), name).argtypes == sa.HIP_SYMBOLS[name][1]
    for name in HOST_NEW:
        assert name in sa.HOST_SYMBOLS and hasattr(host, name)
        assert getattr(sa.host_lib(), name).argtypes == sa.HOST_SYMBOLS[name][1]
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert sa.HIP_SYMBOLS["spmv_plan_run_t_multi"] == (ctypes.c_int, [vp, i32, vp, i64, vp, i64, vp])
    assert sa.HIP_SYMBOLS["spmv_plan_get_transpose_multi_info"] == \
        (ctypes.c_int, [vp, ctypes.POINTER(sa.TransposeMultiInfo)])
    assert sa.HOST_SYMBOLS["spmv_cpu_csr_t_multi"] == (ctypes.c_int, [i64, i64, vp, vp, vp, i32, vp, i64, vp, i64])
    assert ctypes.sizeof(sa.TransposeMultiInfo) == 120 == 8 + 4 * 4 + 4 * 8 + 64


def test_null_plan_answers():
    lib = sa.hip_lib()
    info = sa.TransposeMultiInfo()
    for call in (lambda: lib.spmv_plan_run_t_multi(None, 1, None, 1, None, 1, None),
                 lambda: lib.spmv_plan_get_transpose_multi_info(None, ctypes.byref(info))):
        assert call() == sa.OTHER_ERROR
        assert b"NULL" in lib.spmv_last_error()


@pytest.mark.parametrize("k", [1, 3, 8, 9])
@pytest.mark.parametrize("name", CASES)
def test_cpu_csr_t_multi_golden(name, k):
    m = sa.read_mtx(GOLDEN / f"{name}.mtx")
    ptr, col, val = sa.csr_from_coo(m)
    Xbuf, Ybuf = make_xy(m, k, k + 1, k + 2)
    sa.cpu_csr_t_multi(m.n_rows, m.n_cols, ptr, col, val, Xbuf[:, :k], Ybuf[:, :k])
    assert untouched(m, Ybuf, k), "Y's gaps or tail written"
    assert not np.isnan(Ybuf[: m.n_cols, :k]).any(), "NaN left in Y (or X's gaps read)"
    for j in range(k):
        x = np.ascontiguousarray(Xbuf[: m.n_rows, j])
        got = np.ascontiguousarray(Ybuf[: m.n_cols, j])
        ref = oracle.file_order_spmv(m.n_cols, m.col, m.row, m.val, x)
        bad = oracle.parity(got, ref, m.col, m.row, m.val, x, m.n_cols, rel=1e-6)
        assert bad.size == 0, f"column {j}: {bad.size} bad entries, first {bad[:5]}"
        x1 = np.ascontiguousarray(Xbuf[:, j])
        y1 = np.full(m.n_cols, np.nan)
        sa.cpu_csr_t(m.n_rows, m.n_cols, ptr, col, val, x1, y1)
        assert np.array_equal(got.view(np.int64), y1.view(np.int64)), f"column {j} differs from cpu_csr_t"
    if m.nnz == 0:
        assert not Ybuf[: m.n_cols, :k].any()


def test_cpu_csr_t_multi_refuses_bad_input():
    m = sa.read_mtx(GOLDEN / "n67.mtx")
    ptr, col, val = sa.csr_from_coo(m)
    k = 4
    X = np.ones((m.n_rows, k))
    Y = np.full((m.n_cols, k), SENTINEL)
    f = sa.host_lib().spmv_cpu_csr_t_multi
    P = {"ptr": ptr.ctypes.data, "col": col.ctypes.data, "val": val.ctypes.data, "X": X.ctypes.data,
         "Y": Y.ctypes.data}

    def call(n_rows=m.n_rows, n_cols=m.n_cols, k=k, ldx=k, ldy=k, **null):
        a = {**P, **null}
        return f(n_rows, n_cols, a["ptr"], a["col"], a["val"], k, a["X"], ldx, a["Y"], ldy)

    for what, rc in {
        "n_rows < 0": call(n_rows=-1), "n_cols < 0": call(n_cols=-1), "k = 0": call(k=0), "k < 0": call(k=-2),
        "ldx < k": call(ldx=k - 1), "ldy < k": call(ldy=k - 1), "NULL row_ptr": call(ptr=None),
        "NULL col": call(col=None), "NULL val": call(val=None), "NULL X": call(X=None), "NULL Y": call(Y=None),
    }.items():
        assert rc == sa.OTHER_ERROR, what
    assert np.array_equal(Y, np.full_like(Y, SENTINEL)), "a refused call wrote Y"
    for bad_col in (m.n_cols, -1):
        c = col.copy()
        c[-1] = bad_col
        assert call(col=c.ctypes.data) == sa.OTHER_ERROR, bad_col
    assert call() == sa.SUCCESS
    # the wrapper's own checks
    for bad_X, bad_Y, kk in ((X[:-1], Y, None), (X, Y[:-1], None), (X.astype(np.float32), Y, None),
                             (X[:, 0], Y, None), (X[:, ::2], Y[:, :2], None), (X, Y, 0), (X, Y, k + 1),
                             (list(X), Y, None)):
        with pytest.raises(sa.SpmvError) as e:
            sa.cpu_csr_t_multi(m.n_rows, m.n_cols, ptr, col, val, bad_X, bad_Y, k=kk)
        assert e.value.rc == sa.OTHER_ERROR


def test_run_t_multi_checks_arguments_before_the_c_call():
    """A bare DeviceMatrix (no plan, nothing on a device): every bad argument
    is an SpmvError(OTHER_ERROR) raised in Python."""
    import torch

    dm = sa.DeviceMatrix("csr", 4, 6, 4, "cuda:0", plan=None)
    gX = torch.zeros(4, 2, dtype=torch.float64)
    gY = torch.zeros(6, 2, dtype=torch.float64)
    f64 = torch.float64
    bad = {
        "wrong device (cpu tensors)": (gX, gY),
        "X dtype": (torch.zeros(4, 2, dtype=torch.float32), gY),
        "Y dtype": (gX, torch.zeros(6, 2, dtype=torch.float32)),
        "X 1-D": (torch.zeros(4, dtype=f64), gY),
        "Y 1-D": (gX, torch.zeros(6, dtype=f64)),
        "k differs": (torch.zeros(4, 3, dtype=f64), gY),
        "X too few rows": (torch.zeros(3, 2, dtype=f64), gY),
        "Y too few rows": (gX, torch.zeros(5, 2, dtype=f64)),
        "X inner stride": (torch.zeros(4, 4, dtype=f64)[:, ::2], gY),
        "Y inner stride": (gX, torch.zeros(6, 4, dtype=f64)[:, ::2]),
        "X row stride": (torch.as_strided(torch.zeros(8, dtype=f64), (4, 2), (1, 1)), gY),
        "Y row stride": (gX, torch.as_strided(torch.zeros(8, dtype=f64), (6, 2), (1, 1))),
        "not a tensor": (np.zeros((4, 2)), gY),
    }
    for what, (X, Y) in bad.items():
        with pytest.raises(sa.SpmvError) as e:
            dm.run_t_multi(X, Y)
        assert e.value.rc == sa.OTHER_ERROR, what
    # well-formed tensors on the matrix's own device, but no plan: refused in Python
    bare = sa.DeviceMatrix("csr", 4, 6, 4, "cpu", plan=None)
    with pytest.raises(sa.SpmvError) as e:
        bare.run_t_multi(gX, gY)
    assert e.value.rc == sa.OTHER_ERROR and "no plan" in str(e.value)
    with pytest.raises(sa.SpmvError) as e:
        dm.transpose_multi_info
    assert e.value.rc == sa.OTHER_ERROR


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc with libasan")
def test_transpose_multi_harness_under_asan_ubsan():
    """spmv_cpu_csr_t_multi compiled with ASan + UBSan into a stand-alone
    program and driven over the fixtures with exactly-sized allocations."""
    subprocess.run(["make", "-C", str(REPO), "build/san/transpose_multi_harness"], check=True, capture_output=True)
    fixtures = sorted(str(p) for p in (REPO / "tests" / "golden").glob("*.mtx"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=99", OMP_NUM_THREADS="4")
    r = subprocess.run([str(REPO / "build" / "san" / "transpose_multi_harness"), *fixtures], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert f"transpose multi harness: {len(fixtures)} files clean" in r.stdout
