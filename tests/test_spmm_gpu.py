"""Multi-vector SpMV Y = A·X on the GPU (spmv_plan_run_multi through
DeviceMatrix.run_multi).

Reference for column j: oracle.file_order_spmv(..., X[:, j]); criterion: the
project's oracle.parity(rel=1e-6), per column.  X is seeded uniform(-1, 1).
Every Y starts as NaN in its k live columns and 12345.0 in its ldy - k padding
columns, which must come back bitwise unchanged.  One X of KMAX columns per
matrix is shared by every k (k uses its first k columns), so each column's
reference is computed once.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import spmv_amd as sa
from conftest import GOLDEN, golden_cases
from oracle import oracle

pytestmark = pytest.mark.gpu

CASES = [c["name"] for c in golden_cases()]
KS = (1, 2, 3, 4, 5, 8, 9, 17)
KMAX = max(KS)
SENTINEL = 12345.0

FMT_PARAMS = [
    ("csr", {}),
    ("csr", {"lanes": 2}),
    ("csr", {"lanes": 64}),
    ("csr", {"variant": 1}),
    ("csr", {"variant": 4}),
    ("ell", {"ki": 1}),
    ("ell", {"ki": 2}),
    ("sell", {"C": 64, "sigma": 1024, "ki": 2}),
    ("sell", {"C": 32, "sigma": 64, "ki": 1}),
    ("sell", {"C": 128, "sigma": 256, "ki": 2}),
    ("sell", {"C": 64, "sigma": 1024, "ki": 2, "split": 2}),
]
IDS = [f"{f}-{'-'.join(f'{k}{v}' for k, v in kw.items()) or 'default'}" for f, kw in FMT_PARAMS]


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch, torch.device("cuda:0")


def _with_refs(m, kmax, seed):
    X = np.random.default_rng(seed).uniform(-1.0, 1.0, (max(m.n_cols, 1), kmax))
    refs = [oracle.file_order_spmv(m.n_rows, m.row, m.col, m.val, np.ascontiguousarray(X[: m.n_cols, j]))
            for j in range(kmax)]
    X.setflags(write=False)
    for r in refs:
        r.setflags(write=False)
    return m, X, refs


@functools.lru_cache(maxsize=None)
def golden(name):
    return _with_refs(sa.read_mtx(GOLDEN / f"{name}.mtx"), KMAX, 7)


@functools.lru_cache(maxsize=None)
def cantlike():
    return _with_refs(sa.gen_cantlike(0), 8, 11)


@functools.lru_cache(maxsize=None)
def rmat():
    return _with_refs(sa.gen_rmat(100_000, 1_000_000, scale=17, seed=1), 3, 13)


def build(dev, m, fmt, **kw):
    if fmt == "ell":
        kw.setdefault("ell_max_padding", None)  # tiny fixtures pad to 64 rows
    return sa.to_device(m, fmt, dev, **kw)


def to_dev(torch, dev, a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)  # a copy: the shared X stays read-only


def run_layout(torch, dev, dm, m, X, k, layout):
    """One run_multi of the first k columns of X in `layout`; returns Y[:n_rows, :k]
    (numpy) after checking the padding columns bit by bit."""
    nc, nr = max(m.n_cols, 1), max(m.n_rows, 1)
    Xk = to_dev(torch, dev, X[:, :k])
    ldx, ldy = (k + 3, k + 1) if layout == "padded" else (k, k)
    if layout == "padded":
        Xbuf = torch.full((nc, ldx), 777.0, dtype=torch.float64, device=dev)
        Xv = Xbuf[:, :k]
        Xv.copy_(Xk)
    elif layout == "offset":  # starts one element into its buffer: 8-byte aligned only
        Xbuf = torch.full((nc * k + 1,), 777.0, dtype=torch.float64, device=dev)
        Xv = Xbuf[1:].view(nc, k)
        Xv.copy_(Xk)
        assert Xv.data_ptr() % 16 == 8
    else:
        Xv = Xk
    Ybuf = torch.full((nr, ldy), SENTINEL, dtype=torch.float64, device=dev)
    Yv = Ybuf[:, :k]
    Yv.fill_(float("nan"))
    dm.run_multi(Xv, Yv)
    torch.cuda.synchronize()
    Yh = Ybuf.cpu().numpy()
    pad = Yh[:, k:]
    assert np.array_equal(pad.view(np.int64), np.full(pad.shape, SENTINEL).view(np.int64)), "padding of Y written"
    return np.ascontiguousarray(Yh[: m.n_rows, :k])


def assert_columns(m, X, refs, Y, k):
    for j in range(k):
        x = np.ascontiguousarray(X[: m.n_cols, j])
        bad = oracle.parity(Y[:, j], refs[j], m.row, m.col, m.val, x, m.n_rows, rel=1e-6)
        assert bad.size == 0, (f"k={k} column {j}: {bad.size} bad rows, first {bad[:5]}: got {Y[bad[:5], j]} "
                               f"want {refs[j][bad[:5]]}")


def assert_run_still_right(torch, dev, dm, m):
    """A plain run on the same matrix (after a refused run_multi)."""
    x = sa.ramp_x(m.n_cols)
    y = torch.full((max(m.n_rows, 1),), float("nan"), dtype=torch.float64, device=dev)
    dm.run(torch.from_numpy(x).to(dev), y)
    torch.cuda.synchronize()
    yh = y.cpu().numpy()[: m.n_rows]
    y_ref = oracle.file_order_spmv(m.n_rows, m.row, m.col, m.val, x)
    assert oracle.parity(yh, y_ref, m.row, m.col, m.val, x, m.n_rows, rel=1e-6).size == 0


# ------------------------------------------------------------ 1. fixtures
@pytest.mark.parametrize("fmt,kw", FMT_PARAMS, ids=IDS)
@pytest.mark.parametrize("name", CASES)
def test_golden_fixtures(torch_dev, name, fmt, kw):
    torch, dev = torch_dev
    m, X, refs = golden(name)
    dm = build(dev, m, fmt, **kw)
    assert dm.multi_supported
    for k in KS:
        for layout in ("contiguous", "padded", "offset"):
            Y = run_layout(torch, dev, dm, m, X, k, layout)
            assert_columns(m, X, refs, Y, k)


# ------------------------------------------------------------ 2. bit rule
@pytest.mark.parametrize("fmt,kw", FMT_PARAMS, ids=IDS)
@pytest.mark.parametrize("name", ["n67", "long_rows", "ragged_shuffled"])
def test_bit_rule(torch_dev, name, fmt, kw):
    """Column j's bits depend on the matrix and input column j only: equal to
    a k = 1 run on a contiguous copy of column j, for every k and layout."""
    torch, dev = torch_dev
    m, X, _ = golden(name)
    dm = build(dev, m, fmt, **kw)
    single = [run_layout(torch, dev, dm, m, np.ascontiguousarray(X[:, j:j + 1]), 1, "contiguous")[:, 0]
              for j in range(9)]
    for k in (2, 3, 8, 9):
        Yc = run_layout(torch, dev, dm, m, X, k, "contiguous")
        Yp = run_layout(torch, dev, dm, m, X, k, "padded")
        assert np.array_equal(Yc.view(np.int64), Yp.view(np.int64)), f"k={k}: padded and contiguous bits differ"
        for j in range(k):
            assert np.array_equal(Yc[:, j].view(np.int64), single[j].view(np.int64)), \
                f"k={k} column {j}: bits differ from the k=1 run"


# ----------------------------------------------------------- 3. cant-like
@pytest.mark.parametrize("fmt", ["csr", "sell", "ell"])
def test_cantlike(torch_dev, fmt):
    torch, dev = torch_dev
    m, X, refs = cantlike()
    dm = build(dev, m, fmt)
    for k in (4, 8):
        Y = run_layout(torch, dev, dm, m, X, k, "contiguous")
        assert_columns(m, X, refs, Y, k)


# --------------------------------------------------------- 4. skewed rows
@pytest.mark.parametrize("fmt,kw", [("csr", {}), ("csr", {"variant": 3}), ("csr", {"variant": 4, "hot": 4096}),
                                    ("sell", {})],
                         ids=["csr-default", "csr-variant3", "csr-variant4-hot4096", "sell"])
def test_skewed_rows(torch_dev, fmt, kw):
    """R-MAT: 44,982 empty rows, longest row 9,775.  The hot = 4096 plan owns a
    renumbered column copy; the multi-vector run must read the original columns."""
    torch, dev = torch_dev
    m, X, refs = rmat()
    dm = build(dev, m, fmt, **kw)
    if kw.get("hot"):
        assert dm.params["H"] > 0 and "hot-column table" in dm.params["plan"]
    Y = run_layout(torch, dev, dm, m, X, 3, "contiguous")
    assert_columns(m, X, refs, Y, 3)


# ----------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("fmt", ["coo", "cmrs", "sell16", "csr16"])
def test_refused_formats(torch_dev, fmt):
    torch, dev = torch_dev
    m, X, _ = golden("ragged_shuffled")
    dm = build(dev, m, fmt)
    assert dm.multi_supported is False
    Xd = to_dev(torch, dev, X[:, :2])
    Y = torch.full((m.n_rows, 2), SENTINEL, dtype=torch.float64, device=dev)
    with pytest.raises(sa.SpmvError) as e:
        dm.run_multi(Xd, Y)
    assert e.value.rc == sa.OTHER_ERROR
    torch.cuda.synchronize()
    assert bool((Y == SENTINEL).all()), "a refused run wrote Y"
    assert_run_still_right(torch, dev, dm, m)


def test_refused_arguments(torch_dev):
    torch, dev = torch_dev
    m, X, _ = golden("ragged_shuffled")
    dm = build(dev, m, "csr")
    lib = sa.hip_lib()
    Xd = to_dev(torch, dev, X[:, :4])
    Y = torch.full((m.n_rows, 4), SENTINEL, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    for what, (k, ldx, ldy) in {"k = 0": (0, 4, 4), "ldx < k": (4, 3, 4), "ldy < k": (4, 4, 3)}.items():
        assert lib.spmv_plan_run_multi(dm.plan, k, Xd.data_ptr(), ldx, Y.data_ptr(), ldy, st) == sa.OTHER_ERROR, what
        assert lib.spmv_last_error()
        assert_run_still_right(torch, dev, dm, m)
    assert lib.spmv_plan_run_multi(dm.plan, 4, None, 4, Y.data_ptr(), 4, st) == sa.OTHER_ERROR  # NULL X, entries
    assert lib.spmv_plan_run_multi(dm.plan, 4, Xd.data_ptr(), 4, None, 4, st) == sa.OTHER_ERROR  # NULL Y, rows
    bad = {
        "ldx < k": (torch.as_strided(Xd, (m.n_cols, 4), (3, 1)), Y),
        "Y inner stride 2": (Xd, torch.full((m.n_rows, 8), SENTINEL, dtype=torch.float64, device=dev)[:, ::2]),
        "X too few rows": (Xd[: m.n_cols - 1], Y),
    }
    for what, (Xb, Yb) in bad.items():
        with pytest.raises(sa.SpmvError) as e:
            dm.run_multi(Xb, Yb)
        assert e.value.rc == sa.OTHER_ERROR, what
        assert_run_still_right(torch, dev, dm, m)
    torch.cuda.synchronize()
    assert bool((Y == SENTINEL).all()), "a refused run wrote Y"


# --------------------------------------------------------------- 6. graph
def test_graph_capture(torch_dev):
    """One run_multi captured on a single stream (no parallel branches),
    replayed, X overwritten in place, replayed again."""
    torch, dev = torch_dev
    m, X, refs = golden("ragged_shuffled")
    dm = build(dev, m, "csr")
    k = 4
    Xd = to_dev(torch, dev, X[:, :k])
    Y = torch.full((m.n_rows, k), float("nan"), dtype=torch.float64, device=dev)
    dm.run_multi(Xd, Y)  # first-call setup outside the capture
    torch.cuda.synchronize()
    Y.fill_(float("nan"))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dm.run_multi(Xd, Y)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert_columns(m, X, refs, Y.cpu().numpy(), k)
    # columns 4..7 of the shared X written over the captured tensor
    Xd.copy_(to_dev(torch, dev, X[:, k:2 * k]))
    Y.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert_columns(m, X[:, k:2 * k], refs[k:2 * k], Y.cpu().numpy(), k)
