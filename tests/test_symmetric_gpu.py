"""The symmetric product y = (S + S^T - diag S) x on the GPU
(spmv_plan_prepare_symmetric / spmv_plan_run_sym through
DeviceMatrix.prepare_symmetric / run_sym), both modes, on the stored half S.

References, all on the host-expanded COO sa.expand_symmetric(S):
  - the oracle's file-order sum, judged by oracle.parity(rel=1e-6);
  - an int64 reference on integer data sized from the expanded matrix's
    longest row (tests/exact.py through test_symmetric.integer_half): equality;
  - the fp64 forward-error bound (n_i + 2) 2^-53 sum |a_ij x_j| on wide-range
    data (tests/exact.py), which both modes must meet.
y is 3 entries longer than n, NaN in the live part and 12345.0 in the tail,
which must come back bitwise unchanged.  One x and one reference per matrix
are shared by every test that uses it.

The matrices are the smallest at which each path's edges occur: the square
fixtures; n = 129 (one full block and a one-row block, empty rows); an upper
triangle (the window lies above the block's rows); a 3,000-row lower triangle
with a dense first column (unions past the 2,048-column cap: the wide path,
beside banded blocks on the window path); the lower triangle of the
100,000-row R-MAT (duplicates, empty rows, almost entirely the wide path); the
cant-like lower triangle (every block a window block); n = 0 and nnz = 0.
"""
from __future__ import annotations

import ctypes
import functools
import subprocess

import numpy as np
import pytest

import exact
import spmv_amd as sa
from conftest import GOLDEN, REPO
from oracle import oracle
from test_symmetric import SQUARE, integer_half

pytestmark = pytest.mark.gpu

MODES = ("fused", "expand")
SENTINEL = 12345.0
TAIL = 3
CSR_PLANS = [{}, {"lanes": 2}, {"lanes": 64}, {"variant": 1}, {"variant": 4}]
PLAN_IDS = ["-".join(f"{k}{v}" for k, v in kw.items()) or "default" for kw in CSR_PLANS]
GENERATED = ("n129", "upper", "dense_column", "rmat_tril", "cantlike2")
EDGE = ("symmetric_lower", "duplicates") + GENERATED  # the matrices of the exact / bound / repeat checks


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch, torch.device("cuda:0")


def coo(n, row, col, val, label=""):
    return sa.Coo(n, n, np.asarray(row, np.int32), np.asarray(col, np.int32), np.asarray(val, np.float64), True, label)


@functools.lru_cache(maxsize=None)
def half(key: str) -> sa.Coo:
    """The stored half S."""
    rng = np.random.default_rng(sum(map(ord, key)))
    if key == "n129":  # diagonal plus random lower entries; rows 5, 64 and 127 left empty
        r = rng.integers(1, 129, 600)
        c = (rng.random(600) * r).astype(np.int64)  # c < r
        row, col = np.concatenate([np.arange(129), r]), np.concatenate([np.arange(129), c])
        keep = ~np.isin(row, (5, 64, 127))
        return coo(129, row[keep], col[keep], rng.uniform(-1, 1, int(keep.sum())), key)
    if key == "upper":  # strictly above the rows of every block but the diagonal band
        n = 700
        row = np.repeat(np.arange(n), 6)
        col = np.minimum(row + np.tile([0, 1, 2, 130, 300, 517], n), n - 1)
        return coo(n, row, col, rng.uniform(-1, 1, row.size), key)
    if key == "dense_column":  # column 0 dense: rows from 2,048 on have unions past the cap
        n = 3000
        i = np.arange(n)
        row = np.concatenate([i, i, i[3:], i[7:]])
        col = np.concatenate([np.zeros(n, np.int64), i, i[3:] - 3, i[7:] - 7])
        return coo(n, row, col, rng.uniform(-1, 1, row.size), key)
    if key == "rmat_tril":
        m = sa.gen_rmat(100_000, 1_000_000, scale=17, seed=1)
        keep = m.row >= m.col
        return coo(100_000, m.row[keep], m.col[keep], m.val[keep], key)
    if key == "cantlike2":
        return sa.gen_cantlike(2)
    return sa.read_mtx(GOLDEN / f"{key}.mtx")


@functools.lru_cache(maxsize=None)
def case(key: str):
    """-> (S, expansion, x, oracle reference of the expansion on x)."""
    m = half(key)
    e = sa.expand_symmetric(m)
    x = np.random.default_rng(7).uniform(-1.0, 1.0, max(m.n_rows, 1))
    ref = oracle.file_order_spmv(m.n_rows, e.row, e.col, e.val, np.ascontiguousarray(x[: m.n_cols]))
    for a in (x, ref):
        a.setflags(write=False)
    return m, e, x, ref


@functools.lru_cache(maxsize=None)
def int_case(key: str):
    return integer_half(half(key), seed=41)


@functools.lru_cache(maxsize=None)
def real_case(key: str):
    """Wide-range values on the half, wide-range x; the extended-precision
    reference and the fp64 bound of the expansion."""
    m = half(key)
    rng = np.random.default_rng(43)
    mr = sa.Coo(m.n_rows, m.n_cols, m.row, m.col, exact.wide_range(rng, m.nnz), True, m.label)
    x = exact.wide_range(rng, m.n_cols)
    e = sa.expand_symmetric(mr)
    return mr, x, exact.exact_reference(e, x), exact.fp64_bound(e, x)


def to_dev(torch, dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the shared x stays read-only


def new_y(torch, dev, n):
    y = torch.full((n + TAIL,), SENTINEL, dtype=torch.float64, device=dev)
    y[:n] = float("nan")
    return y


def run_sym(torch, dev, dm, x):
    """-> y[:n] (numpy); the tail checked bit by bit."""
    n = dm.n_rows
    y = new_y(torch, dev, n)
    dm.run_sym(to_dev(torch, dev, x), y)
    torch.cuda.synchronize()
    yh = y.cpu().numpy()
    assert np.array_equal(yh[n:].view(np.int64), np.full(TAIL, SENTINEL).view(np.int64)), "tail of y written"
    assert not np.isnan(yh[:n]).any(), "NaN left in y"
    return yh[:n]


def assert_parity(e, x, ref, y):
    xs = np.ascontiguousarray(x[: e.n_cols])
    bad = oracle.parity(y, ref, e.row, e.col, e.val, xs, e.n_rows, rel=1e-6)
    assert bad.size == 0, f"{bad.size} bad rows, first {bad[:5]}: got {y[bad[:5]]} want {ref[bad[:5]]}"


def check_mode(torch, dev, dm, key, mode):
    m, e, x, ref = case(key)
    dm.prepare_symmetric(mode)
    info = dm.symmetric_info
    assert info["mode"] == mode
    assert_parity(e, x, ref, run_sym(torch, dev, dm, x))
    return info


def expected_fused(m, cap=2048):
    """(blocks, window blocks, flush entries) of fused mode, restated: per
    block of 128 rows the union of its column range and its own rows; a union
    of at most cap columns is a window block and flushes its span, a wider one
    flushes its rows; a block without entries does nothing."""
    n = m.n_rows
    blocks = (n + 127) // 128
    lo, hi = np.full(blocks, n, np.int64), np.full(blocks, -1, np.int64)
    np.minimum.at(lo, m.row // 128, m.col)
    np.maximum.at(hi, m.row // 128, m.col)
    has = hi >= 0
    r0 = np.arange(blocks, dtype=np.int64) * 128
    r1 = np.minimum(r0 + 128, n)
    span = np.maximum(hi, r1 - 1) - np.minimum(lo, r0) + 1
    win = has & (span <= cap)
    return blocks, int(win.sum()), int(span[win].sum() + (r1 - r0)[has & ~win].sum())


def csr_order_expansion(m):
    """The host statement of expand mode: the expansion of the CSR-ordered
    entries (the order the plan holds them in) as CSR."""
    ptr, col, val = sa.csr_from_coo(m)
    rows = np.repeat(np.arange(m.n_rows, dtype=np.int32), np.diff(ptr))
    e = sa.expand_symmetric(sa.Coo(m.n_rows, m.n_cols, rows, col, val))
    return e, sa.csr_from_coo(e)


# ------------------------------------------------------------ 1. fixtures
@pytest.mark.parametrize("kw", CSR_PLANS, ids=PLAN_IDS)
@pytest.mark.parametrize("name", SQUARE)
def test_golden_fixtures(torch_dev, name, kw):
    torch, dev = torch_dev
    m = half(name)
    dm = sa.to_device(m, "csr", dev, **kw)
    assert dm.symmetric_supported
    for mode in MODES:
        info = check_mode(torch, dev, dm, name, mode)
        if mode == "fused":
            assert info["blocks"] == (m.n_rows + 127) // 128 and info["cap"] == 2048
            assert info["owned_bytes"] == 8 * info["blocks"]
            assert (info["blocks"], info["window_blocks"], info["flush_entries"]) == expected_fused(m)
            assert info["kernel"] == "csr_sym_window_kernel"
        else:
            assert info["nnz_expanded"] == case(name)[1].nnz
            assert info["owned_bytes"] >= 12 * info["nnz_expanded"] + 8 * (m.n_rows + 1)


def test_case_set():
    assert {"symmetric_lower", "duplicates", "all_empty", "one", "n67"} <= set(SQUARE)


# ------------------------------------------------- 2.-6. the path edges
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", GENERATED)
def test_generated(torch_dev, key, mode):
    torch, dev = torch_dev
    m = half(key)
    dm = sa.to_device(m, "csr", dev)
    info = check_mode(torch, dev, dm, key, mode)
    if mode != "fused":
        assert info["nnz_expanded"] == case(key)[1].nnz
        return
    blocks = (m.n_rows + 127) // 128
    assert info["owned_bytes"] == 8 * blocks
    assert (info["blocks"], info["window_blocks"], info["flush_entries"]) == expected_fused(m)
    if key == "n129":
        assert (info["blocks"], info["window_blocks"]) == (2, 2)
    elif key == "upper":
        assert info["window_blocks"] == blocks  # every union spans at most 127 + 517 + 1 columns
    elif key == "dense_column":
        # block b's union is [0, 128 b + 127]: 2,048 columns at b = 15, the last that fits
        assert (info["blocks"], info["window_blocks"]) == (24, 16)
    elif key == "rmat_tril":
        assert 0 < info["window_blocks"] < blocks // 8  # almost entirely the wide path
    elif key == "cantlike2":
        assert info["window_blocks"] == blocks > 0 and info["flush_entries"] > 0


def test_rmat_tril_reads_the_callers_columns(torch_dev):
    """The hot = 4096 plan owns a renumbered column copy; the symmetric run
    must read the caller's columns."""
    torch, dev = torch_dev
    dm = sa.to_device(half("rmat_tril"), "csr", dev, variant=4, hot=4096)
    assert dm.params["H"] > 0 and "hot-column table" in dm.params["plan"]
    for mode in MODES:
        check_mode(torch, dev, dm, "rmat_tril", mode)


# ------------------------------------------------------ 7. n = 0, nnz = 0
@pytest.mark.parametrize("mode", MODES)
def test_empty(torch_dev, mode):
    torch, dev = torch_dev
    m = coo(300, [], [], [])
    dm = sa.to_device(m, "csr", dev)
    dm.prepare_symmetric(mode)
    info = dm.symmetric_info
    if mode == "fused":
        assert (info["blocks"], info["window_blocks"], info["flush_entries"], info["owned_bytes"]) == (3, 0, 0, 24)
    else:
        assert info["nnz_expanded"] == 0
    y = run_sym(torch, dev, dm, np.ones(300))
    assert not y.any()
    m0 = coo(0, [], [], [])
    d0 = sa.to_device(m0, "csr", dev)
    assert d0.symmetric_supported
    d0.prepare_symmetric(mode)
    y = torch.full((TAIL,), SENTINEL, dtype=torch.float64, device=dev)
    d0.run_sym(torch.zeros(1, dtype=torch.float64, device=dev), y)
    torch.cuda.synchronize()
    assert (y.cpu().numpy() == SENTINEL).all()
    if mode == "fused":
        assert d0.symmetric_info["owned_bytes"] == 0


# -------------------------------------------------- exact and bounded checks
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", EDGE)
def test_exact_on_integers(torch_dev, key, mode):
    """Every product and partial sum is an integer below 2^52 in any order: y
    EQUALS the int64 reference, and two runs are equal."""
    torch, dev = torch_dev
    hm, x, ref = int_case(key)
    dm = sa.to_device(hm, "csr", dev)
    dm.prepare_symmetric(mode)
    y1 = run_sym(torch, dev, dm, x)
    exact.assert_exact(y1, ref, f"{key} {mode}")
    y2 = run_sym(torch, dev, dm, x)
    assert np.array_equal(y1, y2)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", EDGE)
def test_fp64_bound(torch_dev, key, mode):
    """Wide-range data: both modes meet the forward-error bound of the expanded
    matrix; two runs agree within it (fused) or bit for bit (expand)."""
    torch, dev = torch_dev
    mr, x, ref, bound = real_case(key)
    dm = sa.to_device(mr, "csr", dev)
    dm.prepare_symmetric(mode)
    y1 = run_sym(torch, dev, dm, x)
    y2 = run_sym(torch, dev, dm, x)
    for y in (y1, y2):
        bad, worst = exact.fp64_ratio(y, ref, bound)
        print(f"{key} {mode}: largest error / bound = {worst:.3f}")
        assert bad.size == 0, f"{bad.size} rows over the fp64 bound, first {bad[:5]}"
    if mode == "expand":
        assert np.array_equal(y1.view(np.int64), y2.view(np.int64))
    else:
        assert (np.abs(y1 - y2) <= 2 * bound).all()


# ------------------------------------------------------------ expand bits
@pytest.mark.parametrize("key", ["symmetric_lower", "ragged_shuffled", "duplicates", "n129", "dense_column"])
def test_expand_mode_bits(torch_dev, key):
    """Expand mode: the device-built CSR of A equals the host's element for
    element, and the run has the bits of a default forward CSR plan over it."""
    torch, dev = torch_dev
    m, _, x, _ = case(key)
    dm = sa.to_device(m, "csr", dev)
    dm.prepare_symmetric("expand")
    e, (h_ptr, h_col, h_val) = csr_order_expansion(m)
    d_ptr, d_col, d_val = dm.symmetric_arrays()
    assert np.array_equal(d_ptr, h_ptr) and np.array_equal(d_col, h_col)
    assert np.array_equal(d_val.view(np.int64), h_val.view(np.int64))
    y1 = run_sym(torch, dev, dm, x)
    fwd = sa.to_device(e, "csr", dev)
    y = torch.full((m.n_rows,), float("nan"), dtype=torch.float64, device=dev)
    fwd.run(to_dev(torch, dev, x), y)
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy().view(np.int64), y1.view(np.int64))
    info = dm.symmetric_info
    assert info["owned_bytes"] == 12 * e.nnz + 8 * (m.n_rows + 1) + sa.plan_info(fwd)["owned_bytes"]
    assert info["kernel"] == fwd.kernel
    dm.prepare_symmetric("fused")
    with pytest.raises(sa.SpmvError) as err:
        dm.symmetric_arrays()
    assert err.value.rc == sa.OTHER_ERROR


# ------------------------------------------------------- memory contract
@pytest.mark.parametrize("key", ["symmetric_lower", "n129", "dense_column"])
def test_fused_offset_buffers(torch_dev, key):
    """x and y one element into larger buffers (8-byte alignment only): NaN
    around x must not enter a result, the guards around y stay bit for bit."""
    torch, dev = torch_dev
    m, e, x, ref = case(key)
    n = m.n_rows
    dm = sa.to_device(m, "csr", dev)
    dm.prepare_symmetric("fused")
    xb = torch.full((n + 4,), float("nan"), dtype=torch.float64, device=dev)
    xb[1: n + 1] = to_dev(torch, dev, x[:n])
    yb = torch.full((n + 4,), SENTINEL, dtype=torch.float64, device=dev)
    yb[1: n + 1] = float("nan")
    xv, yv = xb[1:], yb[1:]
    assert xv.data_ptr() % 16 == 8 and yv.data_ptr() % 16 == 8
    dm.run_sym(xv, yv)
    torch.cuda.synchronize()
    yh = yb.cpu().numpy()
    guards = np.concatenate([yh[:1], yh[n + 1:]])
    assert np.array_equal(guards.view(np.int64), np.full(4, SENTINEL).view(np.int64)), "a guard of y was written"
    assert not np.isnan(yh[1: n + 1]).any()
    assert_parity(e, x, ref, yh[1: n + 1])


# --------------------------------------------------------------- graph
@pytest.mark.parametrize("mode", MODES)
def test_graph_capture(torch_dev, mode):
    """One run_sym captured on a single stream (no parallel branches),
    replayed, x overwritten in place, replayed again."""
    torch, dev = torch_dev
    m, e, x, ref = case("dense_column")
    x2 = np.random.default_rng(23).uniform(-1.0, 1.0, m.n_rows)
    ref2 = oracle.file_order_spmv(m.n_rows, e.row, e.col, e.val, x2)
    dm = sa.to_device(m, "csr", dev)
    dm.prepare_symmetric(mode)
    xd = to_dev(torch, dev, x)
    y = new_y(torch, dev, m.n_rows)
    dm.run_sym(xd, y)  # first-call setup outside the capture
    torch.cuda.synchronize()
    y[: m.n_rows] = float("nan")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dm.run_sym(xd, y)
    torch.cuda.synchronize()
    for xs, rs in ((x, ref), (x2, ref2)):
        xd.copy_(to_dev(torch, dev, xs))
        y[: m.n_rows] = float("nan")
        g.replay()
        torch.cuda.synchronize()
        yh = y.cpu().numpy()
        assert np.array_equal(yh[m.n_rows:], np.full(TAIL, SENTINEL))
        assert_parity(e, xs, rs, yh[: m.n_rows])


# ----------------------------------------------------------- lifecycle
def assert_forward_and_transposed_still_right(torch, dev, dm, m):
    """run and run_t on the same plan treat S literally, as before."""
    x = sa.ramp_x(m.n_cols)
    y = torch.full((m.n_rows,), float("nan"), dtype=torch.float64, device=dev)
    dm.run(torch.from_numpy(x).to(dev), y)
    torch.cuda.synchronize()
    y_ref = oracle.file_order_spmv(m.n_rows, m.row, m.col, m.val, x)
    assert oracle.parity(y.cpu().numpy(), y_ref, m.row, m.col, m.val, x, m.n_rows, rel=1e-6).size == 0
    y[:] = float("nan")
    dm.run_t(torch.from_numpy(x).to(dev), y)
    torch.cuda.synchronize()
    t_ref = oracle.file_order_spmv(m.n_cols, m.col, m.row, m.val, x)
    assert oracle.parity(y.cpu().numpy(), t_ref, m.col, m.row, m.val, x, m.n_cols, rel=1e-6).size == 0


def test_lifecycle(torch_dev):
    """fused -> expand -> None -> fused; the forward and transposed runs and
    their byte reports are not touched."""
    torch, dev = torch_dev
    key = "dense_column"
    m, e, x, ref = case(key)
    dm = sa.to_device(m, "csr", dev)
    dm.prepare_transpose("scatter")
    owned, t_info = sa.plan_info(dm)["owned_bytes"], dm.transpose_info
    info = dm.symmetric_info
    assert info["mode"] is None and info["owned_bytes"] == 0 and info["kernel"] == ""
    y = new_y(torch, dev, m.n_rows)
    before = y.clone()
    with pytest.raises(sa.SpmvError) as err:
        dm.run_sym(to_dev(torch, dev, x), y)
    assert err.value.rc == sa.OTHER_ERROR
    torch.cuda.synchronize()
    assert torch.equal(y.view(torch.int64), before.view(torch.int64)), "a refused run wrote y"

    f = check_mode(torch, dev, dm, key, "fused")
    assert f["owned_bytes"] == 8 * f["blocks"] == 8 * 24
    dm.prepare_symmetric("fused")  # the same mode again: a no-op
    assert dm.symmetric_info == f
    assert_forward_and_transposed_still_right(torch, dev, dm, m)

    x_info = check_mode(torch, dev, dm, key, "expand")
    assert x_info["owned_bytes"] >= 12 * e.nnz + 8 * (m.n_rows + 1)
    assert (x_info["blocks"], x_info["window_blocks"], x_info["flush_entries"], x_info["cap"]) == (0, 0, 0, 0)
    assert x_info["kernel"].startswith("csr_")
    assert_forward_and_transposed_still_right(torch, dev, dm, m)

    dm.prepare_symmetric(None)
    info = dm.symmetric_info
    assert info["mode"] is None and info["owned_bytes"] == 0 and info["kernel"] == ""
    with pytest.raises(sa.SpmvError) as err:
        dm.run_sym(to_dev(torch, dev, x), y)
    assert err.value.rc == sa.OTHER_ERROR

    assert check_mode(torch, dev, dm, key, "fused") == f
    assert_forward_and_transposed_still_right(torch, dev, dm, m)
    pi = sa.PlanInfo()
    assert sa.hip_lib().spmv_plan_get_info(dm.plan, ctypes.byref(pi)) == sa.SUCCESS
    assert pi.owned_bytes == owned and dm.transpose_info == t_info
    assert sa.hip_lib().spmv_plan_prepare_symmetric(dm.plan, 3) == sa.OTHER_ERROR  # unknown mode
    assert dm.symmetric_info == f  # a refused prepare leaves the plan as it was
    dm.prepare_transpose(None)
    assert dm.symmetric_info == f
    check_mode(torch, dev, dm, key, "expand")  # destroyed with the plan


# ------------------------------------------------------------- refusals
def test_null_vectors_refused(torch_dev):
    torch, dev = torch_dev
    m, _, x, _ = case("symmetric_lower")
    dm = sa.to_device(m, "csr", dev)
    lib = sa.hip_lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    xd, y = to_dev(torch, dev, x), new_y(torch, dev, m.n_rows)
    for mode in MODES:
        dm.prepare_symmetric(mode)
        assert lib.spmv_plan_run_sym(dm.plan, None, y.data_ptr(), st) == sa.OTHER_ERROR
        assert lib.spmv_plan_run_sym(dm.plan, xd.data_ptr(), None, st) == sa.OTHER_ERROR
        assert b"NULL" in lib.spmv_last_error()
    info = sa.SymmetricInfo()
    assert lib.spmv_plan_get_symmetric_info(dm.plan, None) == sa.OTHER_ERROR
    assert lib.spmv_plan_get_symmetric_info(dm.plan, ctypes.byref(info)) == sa.SUCCESS and info.mode == 2


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_refused_not_square(torch_dev, name):
    torch, dev = torch_dev
    m = sa.read_mtx(GOLDEN / f"{name}.mtx")
    assert m.n_rows != m.n_cols
    dm = sa.to_device(m, "csr", dev)
    assert dm.symmetric_supported is False
    for mode in MODES:
        with pytest.raises(sa.SpmvError) as e:
            dm.prepare_symmetric(mode)
        assert e.value.rc == sa.OTHER_ERROR and "square" in str(e.value)
    assert dm.symmetric_info["mode"] is None


@pytest.mark.parametrize("fmt", ["coo", "ell", "sell", "cmrs", "sell16"])
def test_refused_formats(torch_dev, fmt):
    torch, dev = torch_dev
    m = half("symmetric_lower")
    kw = {"ell_max_padding": None} if fmt == "ell" else {}
    dm = sa.to_device(m, fmt, dev, **kw)
    assert dm.symmetric_supported is False
    for mode in MODES:
        with pytest.raises(sa.SpmvError) as e:
            dm.prepare_symmetric(mode)
        assert e.value.rc == sa.OTHER_ERROR
    assert dm.symmetric_info["mode"] is None
    y = new_y(torch, dev, m.n_rows)
    with pytest.raises(sa.SpmvError) as e:
        dm.run_sym(torch.ones(m.n_cols, dtype=torch.float64, device=dev), y)
    assert e.value.rc == sa.OTHER_ERROR


# -------------------------------------------------------------- drivers
def _run(prog, *args):
    exe = REPO / "bin" / prog
    if not exe.exists():
        subprocess.run(["make", "-C", str(REPO), prog], check=True, capture_output=True)
    return subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("mode", MODES)
def test_driver_symmetric(mode):
    r = _run("csr", "--gen", "cantlike", "--symmetric", mode, "--reps", "3", "--warmup", "1", "--strict", "--cpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "\nresult is ok\n" in "\n" + r.stdout and "\ncpu result is ok\n" in r.stdout
    assert f"[symmetric] {mode} over" in r.stdout


def test_driver_symmetric_lower_triangle():
    r = _run("csr", "--gen", "cantlike2", "--symmetric", "fused", "--reps", "3", "--warmup", "1", "--strict",
             "--no-cpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Z=4007383" in r.stdout and "2034917 stored entries expanded to 4007383" in r.stdout
    assert "\nresult is ok\n" in "\n" + r.stdout


def test_driver_expand_symmetric():
    mtx = str(GOLDEN / "symmetric_lower.mtx")
    r = _run("ell", "--matrix", mtx, "--expand-symmetric", "--reps", "3", "--warmup", "1", "--strict", "--cpu")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "179 stored entries expanded to" in r.stdout
    assert "\nresult is ok\n" in "\n" + r.stdout and "\ncpu result is ok\n" in r.stdout
    for prog in ("coo", "csr", "sigma_c", "cmrs"):
        r = _run(prog, "--matrix", mtx, "--expand-symmetric", "--reps", "3", "--warmup", "1", "--strict")
        assert r.returncode == 0, (prog, r.stdout + r.stderr)
        assert "\nresult is ok\n" in "\n" + r.stdout
