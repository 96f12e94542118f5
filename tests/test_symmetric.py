"""The symmetric product y = (S + S^T - diag S) x from half-stored matrices,
the parts that need no GPU: the host expansion spmv_coo_symmetrize against a
numpy restatement and a dense product, the host loop spmv_cpu_csr_sym exactly
against an int64 reference, the C-ABI symbols and their NULL answers,
run_sym's argument checks, the drivers' flag parsing and the sanitizer
harness (tests/san/symmetric_harness.c, a stand-alone program).
"""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import exact
import spmv_amd as sa
from conftest import GOLDEN, REPO, golden_cases
from oracle import oracle

HIP_NEW = ("spmv_plan_symmetric_supported", "spmv_plan_prepare_symmetric", "spmv_plan_get_symmetric_info",
           "spmv_plan_run_sym")
HOST_NEW = ("spmv_coo_symmetrize", "spmv_cpu_csr_sym")


def _is_square(name):
    m = sa.read_mtx(GOLDEN / f"{name}.mtx")
    return m.n_rows == m.n_cols


SQUARE = [c["name"] for c in golden_cases() if _is_square(c["name"])]


def coo(n, row, col, val):
    return sa.Coo(n, n, np.asarray(row, np.int32), np.asarray(col, np.int32), np.asarray(val, np.float64))


def numpy_expand(m):
    """The definition, restated: the entries, then the mirror of every
    off-diagonal entry, both in input order."""
    off = m.row != m.col
    return (np.concatenate([m.row, m.col[off]]), np.concatenate([m.col, m.row[off]]),
            np.concatenate([m.val, m.val[off]]))


def assert_expansion(m):
    e = sa.expand_symmetric(m)
    row, col, val = numpy_expand(m)
    assert (e.n_rows, e.n_cols) == (m.n_rows, m.n_cols) and e.symmetric is False
    assert e.row.dtype == np.int32 and e.col.dtype == np.int32 and e.val.dtype == np.float64
    assert np.array_equal(e.row, row) and np.array_equal(e.col, col)
    assert np.array_equal(e.val.view(np.int64), val.view(np.int64))
    return e


def integer_half(m, seed):
    """-> (the half storage m with integer values, integer x, int64 reference
    of the symmetric product).  exact.integerize sizes |value| < 2^a and
    |x| < 2^b from the EXPANDED matrix's longest row, so every product and
    partial sum of the symmetric product is exact in fp64; the half keeps the
    values drawn for its own entries, and the reference is int64 arithmetic on
    its expansion."""
    ex = exact.integerize(sa.expand_symmetric(m), seed)
    half = sa.Coo(m.n_rows, m.n_cols, m.row, m.col, np.array(ex.m.val[: m.nnz]), m.symmetric, m.label)
    e = sa.expand_symmetric(half)
    assert (np.abs(e.val) < (1 << ex.a)).all()
    ref = exact.int_spmv(m.n_rows, e.row, e.col, e.val.astype(np.int64), ex.x.astype(np.int64))
    assert (np.abs(ref) < (1 << 53)).all()
    return half, ex.x, ref


def dense_sym(m):
    s = np.zeros((m.n_rows, m.n_cols))
    np.add.at(s, (m.row, m.col), m.val)
    return s + s.T - np.diag(np.diag(s))


# ------------------------------------------------------ spmv_coo_symmetrize
def test_symbols_exported_and_bound():
    hip = ctypes.CDLL(str(sa.LIB_DIR / "libspmv_hip.so"))
    host = ctypes.CDLL(str(sa.LIB_DIR / "libspmv_host.so"))
    for name in HIP_NEW:
        assert name in sa.HIP_SYMBOLS and hasattr(hip, name)
        assert getattr(sa.hip_lib(), name).argtypes == sa.HIP_SYMBOLS[name][1]
    for name in HOST_NEW:
        assert name in sa.HOST_SYMBOLS and hasattr(host, name)
        assert getattr(sa.host_lib(), name).argtypes == sa.HOST_SYMBOLS[name][1]
    assert ctypes.sizeof(sa.SymmetricInfo) == 8 + 5 * 8 + 64
    assert sa.SYMMETRIC_MODES == {None: 0, "fused": 1, "expand": 2}


def test_symmetric_lower_fixture():
    m = sa.read_mtx(GOLDEN / "symmetric_lower.mtx")
    assert (m.n_rows, m.n_cols, m.nnz) == (50, 50, 179) and m.symmetric
    assert (m.row >= m.col).all()
    diag = int((m.row == m.col).sum())
    e = assert_expansion(m)
    assert e.nnz == 2 * 179 - diag
    assert np.array_equal(e.row[:179], m.row) and np.array_equal(e.col[179:], m.row[m.row != m.col])
    x = np.random.default_rng(3).uniform(-1.0, 1.0, 50)
    y = oracle.file_order_spmv(50, e.row, e.col, e.val, x)
    want = dense_sym(m) @ x
    assert np.allclose(y, want, rtol=1e-13, atol=1e-13)
    assert np.allclose(dense_sym(m), dense_sym(m).T)


def test_upper_and_mixed():
    up = coo(4, [0, 0, 1, 2, 3], [0, 3, 2, 2, 3], [1.0, 2.0, 3.0, 4.0, 5.0])
    e = assert_expansion(up)
    assert e.nnz == 7
    assert e.row.tolist() == [0, 0, 1, 2, 3, 3, 2] and e.col.tolist() == [0, 3, 2, 2, 3, 0, 1]
    assert e.val.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 2.0, 3.0]
    # an entry stored on both sides counts as listed: (0, 2) and (2, 0) both mirror
    mixed = coo(3, [0, 2, 1, 2], [2, 0, 1, 1], [1.5, 2.5, 7.0, -1.0])
    e = assert_expansion(mixed)
    assert e.nnz == 7
    a = dense_sym(mixed)
    assert a[0, 2] == a[2, 0] == 4.0 and a[1, 1] == 7.0 and a[1, 2] == a[2, 1] == -1.0


def test_diagonal_only_is_unchanged():
    d = coo(5, [0, 2, 4, 2], [0, 2, 4, 2], [1.0, 2.0, 3.0, 4.0])
    e = assert_expansion(d)
    assert e.nnz == 4 and np.array_equal(e.row, d.row) and np.array_equal(e.val, d.val)


def test_duplicates_each_count():
    m = coo(3, [1, 1, 1, 2], [0, 0, 1, 2], [1.0, 2.0, 3.0, 4.0])
    e = assert_expansion(m)
    assert e.nnz == 6
    assert e.row.tolist() == [1, 1, 1, 2, 0, 0] and e.col.tolist() == [0, 0, 1, 2, 1, 1]
    assert e.val.tolist() == [1.0, 2.0, 3.0, 4.0, 1.0, 2.0]
    m = sa.read_mtx(GOLDEN / "duplicates.mtx")
    if m.n_rows == m.n_cols:
        assert_expansion(m)


@pytest.mark.parametrize("name", SQUARE)
def test_square_fixtures(name):
    m = sa.read_mtx(GOLDEN / f"{name}.mtx")
    e = assert_expansion(m)
    x = np.random.default_rng(5).uniform(-1.0, 1.0, max(m.n_cols, 1))[: m.n_cols]
    y = oracle.file_order_spmv(m.n_rows, e.row, e.col, e.val, x)
    if m.n_rows <= 2000:
        assert np.allclose(y, dense_sym(m) @ x, rtol=1e-12, atol=1e-12)


def test_empty_and_count_only():
    e = assert_expansion(coo(7, [], [], []))
    assert e.nnz == 0
    assert sa.expand_symmetric(coo(0, [], [], [])).nnz == 0
    f = sa.host_lib().spmv_coo_symmetrize
    row = np.array([1, 2, 2], np.int32)
    col = np.array([0, 2, 1], np.int32)
    z = ctypes.c_int64(-1)
    # the count-only call reads no values and writes nothing but the count
    assert f(3, 3, row.ctypes.data, col.ctypes.data, None, ctypes.byref(z), None, None, None) == sa.SUCCESS
    assert z.value == 5
    assert f(3, 0, None, None, None, ctypes.byref(z), None, None, None) == sa.SUCCESS and z.value == 0


def test_refuses_bad_input():
    f = sa.host_lib().spmv_coo_symmetrize
    val = np.ones(2)
    z = ctypes.c_int64(-1)
    for r, c in (([0, 3], [0, 0]), ([0, 1], [0, 3]), ([-1, 1], [0, 0]), ([0, 1], [0, -1])):
        row, col = np.array(r, np.int32), np.array(c, np.int32)
        assert f(3, 2, row.ctypes.data, col.ctypes.data, val.ctypes.data, ctypes.byref(z), None, None, None) \
            == sa.OTHER_ERROR
        with pytest.raises(sa.SpmvError) as e:
            sa.expand_symmetric(coo(3, r, c, [1.0, 1.0]))
        assert e.value.rc == sa.OTHER_ERROR
    row = col = np.zeros(2, np.int32)
    assert f(-1, 2, row.ctypes.data, col.ctypes.data, val.ctypes.data, ctypes.byref(z), None, None, None) \
        == sa.OTHER_ERROR
    assert f(3, -1, row.ctypes.data, col.ctypes.data, val.ctypes.data, ctypes.byref(z), None, None, None) \
        == sa.OTHER_ERROR
    assert f(3, 2, row.ctypes.data, col.ctypes.data, val.ctypes.data, None, None, None, None) == sa.OTHER_ERROR
    with pytest.raises(sa.SpmvError):
        sa.expand_symmetric(sa.Coo(2, 3, row, col, val))  # not square


def test_cantlike_lower_expands_to_the_full_matrix():
    lower, full = sa.gen_cantlike(2), sa.gen_cantlike(0)
    assert lower.nnz == 2_034_917 and lower.symmetric
    e = sa.expand_symmetric(lower)
    assert e.nnz == full.nnz == 4_007_383
    oe, of = np.lexsort((e.col, e.row)), np.lexsort((full.col, full.row))
    assert np.array_equal(e.row[oe], full.row[of]) and np.array_equal(e.col[oe], full.col[of])
    assert np.array_equal(e.val[oe].view(np.int64), full.val[of].view(np.int64))


# --------------------------------------------------------- spmv_cpu_csr_sym
TAIL, SENTINEL = 3, 12345.0


def cpu_sym(m, x):
    ptr, col, val = sa.csr_from_coo(m)
    y = np.full(m.n_rows + TAIL, SENTINEL)
    y[: m.n_rows] = np.nan
    sa.cpu_csr_sym(m.n_rows, ptr, col, val, x, y)
    assert np.array_equal(y[m.n_rows:].view(np.int64), np.full(TAIL, SENTINEL).view(np.int64)), "tail of y written"
    return y[: m.n_rows]


@pytest.mark.parametrize("name", SQUARE)
def test_cpu_csr_sym_is_exact_on_integers(name):
    """Integer data sized from the EXPANDED matrix's longest row: every product
    and partial sum is exact, so y equals the int64 reference."""
    half, x, ref = integer_half(sa.read_mtx(GOLDEN / f"{name}.mtx"), seed=31)
    exact.assert_exact(cpu_sym(half, x), ref, name)


def test_cpu_csr_sym_against_the_oracle():
    m = sa.read_mtx(GOLDEN / "symmetric_lower.mtx")
    e = sa.expand_symmetric(m)
    x = np.random.default_rng(9).uniform(-1.0, 1.0, m.n_cols)
    y = cpu_sym(m, x)
    ref = oracle.file_order_spmv(m.n_rows, e.row, e.col, e.val, x)
    assert oracle.parity(y, ref, e.row, e.col, e.val, x, m.n_rows, rel=1e-6).size == 0
    assert not cpu_sym(coo(4, [], [], []), np.ones(4)).any()


def test_cpu_csr_sym_refuses_bad_input():
    m = sa.read_mtx(GOLDEN / "symmetric_lower.mtx")
    ptr, col, val = sa.csr_from_coo(m)
    x, y = np.ones(50), np.zeros(50)
    for bad in (50, -1):
        c = col.copy()
        c[-1] = bad
        with pytest.raises(sa.SpmvError) as e:
            sa.cpu_csr_sym(50, ptr, c, val, x, y)
        assert e.value.rc == sa.OTHER_ERROR
    for bx, by in ((x[:-1], y), (x, y[:-1]), (x.astype(np.float32), y), (x, y[::2]), (list(x), y)):
        with pytest.raises(sa.SpmvError) as e:
            sa.cpu_csr_sym(50, ptr, col, val, bx, by)
        assert e.value.rc == sa.OTHER_ERROR
    f = sa.host_lib().spmv_cpu_csr_sym
    assert f(-1, ptr.ctypes.data, col.ctypes.data, val.ctypes.data, x.ctypes.data, y.ctypes.data) == sa.OTHER_ERROR
    assert f(50, None, col.ctypes.data, val.ctypes.data, x.ctypes.data, y.ctypes.data) == sa.OTHER_ERROR
    assert f(50, ptr.ctypes.data, col.ctypes.data, val.ctypes.data, x.ctypes.data, None) == sa.OTHER_ERROR
    assert f(50, ptr.ctypes.data, col.ctypes.data, val.ctypes.data, None, y.ctypes.data) == sa.OTHER_ERROR


# ------------------------------------------------------ C-ABI without a plan
def test_null_plan_answers():
    lib = sa.hip_lib()
    assert lib.spmv_plan_symmetric_supported(None) == 0
    info = sa.SymmetricInfo()
    for call in (lambda: lib.spmv_plan_run_sym(None, None, None, None),
                 lambda: lib.spmv_plan_prepare_symmetric(None, 1),
                 lambda: lib.spmv_plan_get_symmetric_info(None, ctypes.byref(info))):
        assert call() == sa.OTHER_ERROR
        assert b"NULL" in lib.spmv_last_error()


def test_run_sym_checks_arguments_before_the_c_call():
    """A bare DeviceMatrix (no plan, nothing on a device): every bad argument
    is an SpmvError(OTHER_ERROR) raised in Python."""
    import torch

    dm = sa.DeviceMatrix("csr", 6, 6, 4, "cuda:0", plan=None)
    assert dm.symmetric_supported is False
    g = torch.zeros(6, dtype=torch.float64)
    bad = {
        "cpu tensors, no plan": (g, g.clone()),
        "x dtype": (torch.zeros(6, dtype=torch.float32), g),
        "y dtype": (g, torch.zeros(6, dtype=torch.float32)),
        "x too short": (torch.zeros(5, dtype=torch.float64), g),
        "y too short": (g, torch.zeros(5, dtype=torch.float64)),
        "x strided": (torch.zeros(12, dtype=torch.float64)[::2], g),
        "y strided": (g, torch.zeros(12, dtype=torch.float64)[::2]),
        "not a tensor": (np.zeros(6), g),
    }
    for what, (x, y) in bad.items():
        with pytest.raises(sa.SpmvError) as e:
            dm.run_sym(x, y)
        assert e.value.rc == sa.OTHER_ERROR, what
    mx = torch.zeros(6, dtype=torch.float64, device="meta")
    with pytest.raises(sa.SpmvError) as e:
        dm.run_sym(mx, mx)
    assert e.value.rc == sa.OTHER_ERROR
    wide = sa.DeviceMatrix("csr", 4, 6, 4, "cuda:0", plan=None)
    with pytest.raises(sa.SpmvError) as e:
        wide.run_sym(g, g.clone())
    assert e.value.rc == sa.OTHER_ERROR
    for call in (lambda: dm.prepare_symmetric("fused"), lambda: dm.prepare_symmetric("sideways"),
                 lambda: dm.symmetric_info):
        with pytest.raises(sa.SpmvError) as e:
            call()
        assert e.value.rc == sa.OTHER_ERROR


def test_build_operator_has_the_switch():
    import inspect

    import iterate

    p = inspect.signature(iterate.build_operator).parameters["expand_symmetric"]
    assert p.default is False


# ------------------------------------------------------------------ drivers
def _run(prog, *args):
    exe = REPO / "bin" / prog
    if not exe.exists():
        subprocess.run(["make", "-C", str(REPO), prog], check=True, capture_output=True)
    return subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=300)


def test_driver_flags_without_a_gpu():
    """Bad arguments stop with code 4 before the device is looked at; good ones
    get as far as the device check (1 on a GPU-less host)."""
    import torch

    mtx = str(GOLDEN / "symmetric_lower.mtx")
    for prog in ("coo", "ell", "sigma_c", "cmrs"):
        r = _run(prog, "--matrix", mtx, "--symmetric", "fused")
        assert r.returncode == 4, (prog, r.stdout, r.stderr)
        assert "--symmetric" in r.stderr
    for args in (("--symmetric", "sideways"), ("--symmetric",), ("--symmetric", "fused", "--expand-symmetric"),
                 ("--symmetric", "fused", "--gpus", "2"), ("--symmetric", "expand", "--relabel", "yes")):
        r = _run("csr", "--matrix", mtx, *args)
        assert r.returncode == 4, (args, r.stdout, r.stderr)
    if torch.cuda.is_available():
        return
    for prog, args in (("csr", ("--symmetric", "fused")), ("csr", ("--symmetric", "expand")),
                       ("csr", ("--expand-symmetric",)), ("ell", ("--expand-symmetric",)),
                       ("coo", ("--expand-symmetric",))):
        r = _run(prog, "--matrix", mtx, *args)
        assert r.returncode == 1, (prog, args, r.stdout, r.stderr)


# ---------------------------------------------------------------- sanitizer
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc with libasan")
def test_symmetric_harness_under_asan_ubsan():
    """tests/san/symmetric_harness.c: a stand-alone program (its own main, the
    host sources compiled in with ASan + UBSan), exactly sized buffers."""
    subprocess.run(["make", "-C", str(REPO), "build/san/symmetric_harness"], check=True, capture_output=True)
    fixtures = sorted(str(p) for p in GOLDEN.glob("*.mtx"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:exitcode=99",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=99", OMP_NUM_THREADS="4")
    r = subprocess.run([str(REPO / "build" / "san" / "symmetric_harness"), *fixtures], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "symmetric harness:" in r.stdout and "files clean" in r.stdout
