"""The multi-vector symmetric product Y = (S + S^T - diag S) X, the parts that
need no GPU: the C-ABI symbols and their NULL-plan answers, the host loop
spmv_cpu_csr_sym_multi (exactly against an int64 reference on the expansion and
bit for bit against spmv_cpu_csr_sym per column), its refusals,
run_sym_multi's argument checks and the sanitizer harness
tests/san/symmetric_multi_harness.c.

Layout under test (include/spmv.h): X[c*ldx + j], Y[i*ldy + j], j < k.  X's
gaps hold NaN; Y's gaps and a 3-row tail hold 12345.0 and must come back
bitwise unchanged; Y's live part starts as NaN.
"""
from __future__ import annotations

import ctypes
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import exact
import spmv_amd as sa
from conftest import GOLDEN, REPO
from test_symmetric import SQUARE

SENTINEL = 12345.0
TAIL = 3
KMAX = 17

HIP_NEW = ("spmv_plan_run_sym_multi", "spmv_plan_get_symmetric_multi_info")
HOST_NEW = ("spmv_cpu_csr_sym_multi",)


def integer_half_multi(m, seed, kmax=KMAX):
    """test_symmetric.integer_half for kmax vectors -> (the half storage m with
    integer values, integer X[n, kmax], int64 reference of the symmetric
    product).  exact.integerize sizes |value| < 2^a and |x| < 2^b from the
    EXPANDED matrix's longest row; every column of X is bounded by the same b,
    so every product and partial sum of every column is exact in fp64."""
    ex = exact.integerize(sa.expand_symmetric(m), seed)
    half = sa.Coo(m.n_rows, m.n_cols, m.row, m.col, np.array(ex.m.val[: m.nnz]), m.symmetric, m.label)
    e = sa.expand_symmetric(half)
    assert (np.abs(e.val) < (1 << ex.a)).all()
    X_i = exact._signed_ints(np.random.default_rng(seed + 1), (max(m.n_rows, 1), kmax), ex.b)
    assert (np.abs(X_i) < (1 << ex.b)).all()
    ref = exact.int_spmv(m.n_rows, e.row, e.col, e.val.astype(np.int64), X_i[: m.n_cols])
    assert (np.abs(ref) < (1 << 53)).all()
    X = X_i.astype(np.float64)
    for a in (X, ref):
        a.setflags(write=False)
    return half, X, ref


@functools.lru_cache(maxsize=None)
def int_fixture(name):
    return integer_half_multi(sa.read_mtx(GOLDEN / f"{name}.mtx"), seed=51)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ------------------------------------------------------------------ symbols
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
    assert sa.HIP_SYMBOLS["spmv_plan_run_sym_multi"] == (ctypes.c_int, [vp, i32, vp, i64, vp, i64, vp])
    assert sa.HIP_SYMBOLS["spmv_plan_get_symmetric_multi_info"] == \
        (ctypes.c_int, [vp, ctypes.POINTER(sa.SymmetricMultiInfo)])
    assert sa.HOST_SYMBOLS["spmv_cpu_csr_sym_multi"] == (ctypes.c_int, [i64, vp, vp, vp, i32, vp, i64, vp, i64])
    # mode, reserved; cap_cols[4]; window_blocks[4], flush_entries[4]; long_rows, segments, multi_owned_bytes; kernel
    assert ctypes.sizeof(sa.SymmetricMultiInfo) == 2 * 4 + 4 * 4 + 2 * 4 * 8 + 3 * 8 + 64


def test_null_plan_answers():
    lib = sa.hip_lib()
    info = sa.SymmetricMultiInfo()
    for call in (lambda: lib.spmv_plan_run_sym_multi(None, 1, None, 1, None, 1, None),
                 lambda: lib.spmv_plan_get_symmetric_multi_info(None, ctypes.byref(info))):
        assert call() == sa.OTHER_ERROR
        assert b"NULL" in lib.spmv_last_error()


# ---------------------------------------------------- spmv_cpu_csr_sym_multi
@pytest.mark.parametrize("k", [1, 3, 8, 17])
@pytest.mark.parametrize("name", SQUARE)
def test_cpu_csr_sym_multi_is_exact_on_integers(name, k):
    half, X, ref = int_fixture(name)
    n = half.n_rows
    ptr, col, val = sa.csr_from_coo(half)
    ldx, ldy = k + 1, k + 3
    Xbuf = np.full((max(n, 1), ldx), np.nan)
    Xbuf[:, :k] = X[:, :k]
    Ybuf = np.full((n + TAIL, ldy), SENTINEL)
    Ybuf[:n, :k] = np.nan
    before = Ybuf.copy()
    sa.cpu_csr_sym_multi(n, ptr, col, val, Xbuf[:, :k], Ybuf[:, :k])
    Y = Ybuf[:n, :k].copy()
    exact.assert_exact(Y, ref[:, :k], f"{name} k={k}")  # also: no NaN left, so X's gaps were not read
    Ybuf[:n, :k] = np.nan
    assert np.array_equal(bits(Ybuf), bits(before)), "Y's gaps or tail written"
    for j in range(k):
        y1 = np.full(n, np.nan)
        sa.cpu_csr_sym(n, ptr, col, val, np.ascontiguousarray(X[:, j]), y1)
        assert np.array_equal(bits(Y[:, j]), bits(y1)), f"column {j} differs from cpu_csr_sym"
    # ld == k: the same bits
    Yp = np.full((n, k), np.nan)
    sa.cpu_csr_sym_multi(n, ptr, col, val, np.ascontiguousarray(X[:, :k]), Yp)
    assert np.array_equal(bits(Yp), bits(Y))


def test_cpu_csr_sym_multi_refuses_bad_input():
    m = sa.read_mtx(GOLDEN / "symmetric_lower.mtx")
    n = m.n_rows
    ptr, col, val = sa.csr_from_coo(m)
    k = 4
    X = np.ones((n, k))
    Y = np.full((n, k), SENTINEL)
    f = sa.host_lib().spmv_cpu_csr_sym_multi
    P = {"ptr": ptr.ctypes.data, "col": col.ctypes.data, "val": val.ctypes.data, "X": X.ctypes.data,
         "Y": Y.ctypes.data}

    def call(n=n, k=k, ldx=k, ldy=k, **null):
        a = {**P, **null}
        return f(n, a["ptr"], a["col"], a["val"], k, a["X"], ldx, a["Y"], ldy)

    for what, rc in {
        "n < 0": call(n=-1), "k = 0": call(k=0), "k < 0": call(k=-2), "ldx < k": call(ldx=k - 1),
        "ldy < k": call(ldy=k - 1), "NULL row_ptr": call(ptr=None), "NULL col": call(col=None),
        "NULL val": call(val=None), "NULL X": call(X=None), "NULL Y": call(Y=None),
    }.items():
        assert rc == sa.OTHER_ERROR, what
    for bad_col in (n, -1):  # in the last entry: refused before Y is touched
        c = col.copy()
        c[-1] = bad_col
        assert call(col=c.ctypes.data) == sa.OTHER_ERROR, bad_col
    assert np.array_equal(Y, np.full_like(Y, SENTINEL)), "a refused call wrote Y"
    assert call() == sa.SUCCESS
    # the wrapper's own checks
    for bad_X, bad_Y, kk in ((X[:-1], Y, None), (X, Y[:-1], None), (X.astype(np.float32), Y, None),
                             (X[:, 0], Y, None), (X[:, ::2], Y[:, :2], None), (X, Y, 0), (X, Y, k + 1),
                             (list(X), Y, None)):
        with pytest.raises(sa.SpmvError) as e:
            sa.cpu_csr_sym_multi(n, ptr, col, val, bad_X, bad_Y, k=kk)
        assert e.value.rc == sa.OTHER_ERROR


def test_run_sym_multi_checks_arguments_before_the_c_call():
    """A bare DeviceMatrix (no plan, nothing on a device): every bad argument
    is an SpmvError(OTHER_ERROR) raised in Python."""
    import torch

    dm = sa.DeviceMatrix("csr", 6, 6, 4, "cuda:0", plan=None)
    f64 = torch.float64
    gX = torch.zeros(6, 2, dtype=f64)
    gY = torch.zeros(6, 2, dtype=f64)
    bad = {
        "wrong device (cpu tensors)": (gX, gY),
        "X dtype": (torch.zeros(6, 2, dtype=torch.float32), gY),
        "Y dtype": (gX, torch.zeros(6, 2, dtype=torch.float32)),
        "X 1-D": (torch.zeros(6, dtype=f64), gY),
        "Y 1-D": (gX, torch.zeros(6, dtype=f64)),
        "k differs": (torch.zeros(6, 3, dtype=f64), gY),
        "X too few rows": (torch.zeros(5, 2, dtype=f64), gY),
        "Y too few rows": (gX, torch.zeros(5, 2, dtype=f64)),
        "X inner stride": (torch.zeros(6, 4, dtype=f64)[:, ::2], gY),
        "Y inner stride": (gX, torch.zeros(6, 4, dtype=f64)[:, ::2]),
        "X row stride": (torch.as_strided(torch.zeros(8, dtype=f64), (6, 2), (1, 1)), gY),
        "Y row stride": (gX, torch.as_strided(torch.zeros(8, dtype=f64), (6, 2), (1, 1))),
        "not a tensor": (np.zeros((6, 2)), gY),
    }
    for what, (X, Y) in bad.items():
        with pytest.raises(sa.SpmvError) as e:
            dm.run_sym_multi(X, Y)
        assert e.value.rc == sa.OTHER_ERROR, what
    wide = sa.DeviceMatrix("csr", 4, 6, 4, "cpu", plan=None)
    with pytest.raises(sa.SpmvError) as e:
        wide.run_sym_multi(gX, gY)
    assert e.value.rc == sa.OTHER_ERROR and "square" in str(e.value)
    # well-formed tensors on the matrix's own device, but no plan: refused in Python
    bare = sa.DeviceMatrix("csr", 6, 6, 4, "cpu", plan=None)
    with pytest.raises(sa.SpmvError) as e:
        bare.run_sym_multi(gX, gY)
    assert e.value.rc == sa.OTHER_ERROR and "no plan" in str(e.value)
    with pytest.raises(sa.SpmvError) as e:
        dm.symmetric_multi_info
    assert e.value.rc == sa.OTHER_ERROR


# ---------------------------------------------------------------- sanitizer
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc with libasan")
def test_symmetric_multi_harness_under_asan_ubsan():
    """spmv_cpu_csr_sym_multi compiled with ASan + UBSan into a stand-alone
    program (its own main, nothing preloaded) and driven over the fixtures
    with exactly-sized allocations."""
    subprocess.run(["make", "-C", str(REPO), "build/san/symmetric_multi_harness"], check=True, capture_output=True)
    fixtures = sorted(str(p) for p in GOLDEN.glob("*.mtx"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=99", OMP_NUM_THREADS="4")
    r = subprocess.run([str(REPO / "build" / "san" / "symmetric_multi_harness"), *fixtures], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "symmetric multi harness:" in r.stdout and "files clean" in r.stdout
