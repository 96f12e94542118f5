"""The multi-vector symmetric product Y = (S + S^T - diag S) X on the GPU
(spmv_plan_run_sym_multi through DeviceMatrix.run_sym_multi), both modes, on
the stored half S.

Layout (include/spmv.h): X[c*ldx + j], Y[i*ldy + j], j < k.  Two layouts are
run, those of tests/test_transpose_multi_gpu.py: "plain" (ld == k,
16-byte-aligned bases) and "offset" (bases 8 bytes into larger buffers,
ldx = k + 1, ldy = k + 3; NaN in X's gaps and flanks, 12345.0 in Y's gaps,
flanks and the 3 rows past n).  Y's live part starts as NaN.  After every run
everything of Y's buffer but the live part is compared bit for bit with what
it held before.

References, all on the host-expanded COO sa.expand_symmetric(S): an int64
reference on integer data sized from the expanded matrix's longest row
(test_symmetric_multi.integer_half_multi): equality in every column; the fp64
forward-error bound of tests/exact.py on wide-range data.  One X and one
reference per matrix are shared by every test that uses it.

Matrices: the square fixtures at every k in KS; at k <= 8 the generated ones
of tests/test_symmetric_gpu.py (n129: a one-row last block; upper: windows
above the rows; rmat_tril: almost entirely the wide path; cantlike2: every
block on the window path at every width) and dense_column5000, the dense-column
construction at n = 5,000: 40 blocks, the last of 8 rows, block b's union
spans 128 (b + 1) columns, so with cap_cols = 4,096 / 2,048 / 1,024 / 512 the
first 32 / 16 / 8 / 4 blocks take the window path and the rest the wide path:
both paths run at every width.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import exact
import spmv_amd as sa
import test_symmetric_gpu as sg
from conftest import GOLDEN
from test_symmetric import SQUARE
from test_symmetric_multi import bits, integer_half_multi

pytestmark = pytest.mark.gpu

MODES = sg.MODES
SENTINEL = sg.SENTINEL
TAIL = sg.TAIL
WIDTHS = (1, 2, 4, 8)
KS = (1, 2, 3, 4, 5, 8, 9, 17)  # every width, ragged last blocks, two and three passes
KS8 = tuple(k for k in KS if k <= 8)
LAYOUTS = ("plain", "offset")
GENERATED = ("n129", "upper", "rmat_tril", "cantlike2", "dense_column5000")
SCALES = (1.0, -1.0, 2.0, 0.5, -4.0, 8.0, 0.25, -2.0, 16.0)  # exact scalings: the references scale with them


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch, torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def half(key: str) -> sa.Coo:
    if key == "dense_column5000":  # test_symmetric_gpu's dense_column at n = 5,000
        n = 5000
        rng = np.random.default_rng(5000)
        i = np.arange(n)
        row = np.concatenate([i, i, i[3:], i[7:]])
        col = np.concatenate([np.zeros(n, np.int64), i, i[3:] - 3, i[7:] - 7])
        return sg.coo(n, row, col, rng.uniform(-1, 1, row.size), key)
    return sg.half(key)


@functools.lru_cache(maxsize=None)
def int_case(key: str, kmax: int):
    """-> (half with integer values, X[n, kmax], int64 reference)."""
    return integer_half_multi(half(key), seed=61, kmax=kmax)


@functools.lru_cache(maxsize=None)
def real_case(key: str):
    """Wide-range values on the half and one wide-range x; X's column j is
    SCALES[j] x (powers of two: the reference and the bound scale exactly)."""
    m = half(key)
    rng = np.random.default_rng(47)
    mr = sa.Coo(m.n_rows, m.n_cols, m.row, m.col, exact.wide_range(rng, m.nnz), True, m.label)
    x = exact.wide_range(rng, m.n_cols)
    e = sa.expand_symmetric(mr)
    X = np.stack([s * x for s in SCALES], axis=1)
    X.setflags(write=False)
    return mr, X, exact.exact_reference(e, x), exact.fp64_bound(e, x)


def run_sym_multi(torch, dev, dm, X, k, layout):
    """One run_sym_multi on the first k columns of X (numpy, >= n rows):
    -> Y[:n, :k] as numpy.  Asserts that nothing but Y's live part changed."""
    n = dm.n_rows
    nr, rows_y = max(n, 1), n + TAIL
    Xk = torch.from_numpy(np.array(X[:, :k], order="C")).to(dev)
    if layout == "offset":
        ldx, ldy = k + 1, k + 3
        Xbuf = torch.full((nr * ldx + 2,), float("nan"), dtype=torch.float64, device=dev)
        Xv = Xbuf[1:1 + nr * ldx].view(nr, ldx)[:, :k]
        Ybuf = torch.full((rows_y * ldy + 2,), SENTINEL, dtype=torch.float64, device=dev)
        Yv = Ybuf[1:1 + rows_y * ldy].view(rows_y, ldy)[:, :k]
        assert Xv.data_ptr() % 16 == 8 and Yv.data_ptr() % 16 == 8
    else:
        Xv = torch.full((nr, k), float("nan"), dtype=torch.float64, device=dev)
        Ybuf = torch.full((rows_y * k,), SENTINEL, dtype=torch.float64, device=dev)
        Yv = Ybuf.view(rows_y, k)
        assert Xv.data_ptr() % 16 == 0 and Yv.data_ptr() % 16 == 0
    Xv[:n].copy_(Xk[:n])
    Yv[:n] = float("nan")
    before = Ybuf.clone()
    dm.run_sym_multi(Xv, Yv)
    torch.cuda.synchronize()
    Y = Yv[:n].cpu().numpy().copy()
    Yv[:n] = float("nan")  # then the whole buffer must be what it was: gaps, flanks, rows past n
    assert torch.equal(Ybuf.view(torch.int64), before.view(torch.int64)), f"k={k} {layout}: Y written outside its live part"
    return Y


def assert_exact_twice(torch, dev, dm, X, ref, k, layout, what):
    Y = run_sym_multi(torch, dev, dm, X, k, layout)
    exact.assert_exact(Y, ref[:, :k], what)
    Y2 = run_sym_multi(torch, dev, dm, X, k, layout)  # integer sums are exact in any order
    assert np.array_equal(bits(Y), bits(Y2)), f"{what}: two runs differ"


# ------------------------------------------------ 1. exact on integers
@pytest.mark.parametrize("kw", sg.CSR_PLANS, ids=sg.PLAN_IDS)
@pytest.mark.parametrize("name", SQUARE)
def test_exact_on_integers_fixtures(torch_dev, name, kw):
    torch, dev = torch_dev
    hm, X, ref = int_case(name, 17)
    dm = sa.to_device(hm, "csr", dev, **kw)
    for mode in MODES:
        dm.prepare_symmetric(mode)
        assert dm.symmetric_multi_info["mode"] == mode
        for k in KS:
            for layout in LAYOUTS:
                assert_exact_twice(torch, dev, dm, X, ref, k, layout, f"{name} {kw} {mode} k={k} {layout}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", GENERATED)
def test_exact_on_integers_generated(torch_dev, key, mode):
    torch, dev = torch_dev
    hm, X, ref = int_case(key, 8)
    dm = sa.to_device(hm, "csr", dev)
    dm.prepare_symmetric(mode)
    for k in KS8:
        for layout in LAYOUTS if k in (3, 8) else ("plain",):
            assert_exact_twice(torch, dev, dm, X, ref, k, layout, f"{key} {mode} k={k} {layout}")


# ------------------------------------------- 2. the fp64 bound on real data
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ("symmetric_lower", "duplicates") + GENERATED)
def test_fp64_bound(torch_dev, key, mode):
    """Wide-range data: every column meets the forward-error bound of the
    expanded matrix; two runs agree bit for bit (expand) or within twice the
    bound (fused)."""
    torch, dev = torch_dev
    mr, X, ref, bound = real_case(key)
    dm = sa.to_device(mr, "csr", dev)
    dm.prepare_symmetric(mode)
    for k in (3, 8) if key in GENERATED else (3, 9):
        Y1 = run_sym_multi(torch, dev, dm, X, k, "offset")
        Y2 = run_sym_multi(torch, dev, dm, X, k, "offset")
        for j in range(k):
            for Y in (Y1, Y2):
                bad, worst = exact.fp64_ratio(Y[:, j], SCALES[j] * ref, abs(SCALES[j]) * bound)
                assert bad.size == 0, f"{key} {mode} k={k} column {j}: {bad.size} rows over the fp64 bound, first {bad[:5]}"
            print(f"{key} {mode} k={k} column {j}: largest error / bound = {worst:.3f}")
            if mode == "fused":
                assert (np.abs(Y1[:, j] - Y2[:, j]) <= 2 * abs(SCALES[j]) * bound).all()
        if mode == "expand":
            assert np.array_equal(bits(Y1), bits(Y2))


# ------------------------------------------------------------ 3. expand bits
@pytest.mark.parametrize("key", ["symmetric_lower", "ragged_shuffled", "duplicates", "n129"])
def test_expand_mode_bits(torch_dev, key):
    """Expand mode: column j at any k and either layout has the bits of
    run_multi on a default forward CSR plan over symmetric_arrays(), and the
    same bits when it is run alone."""
    torch, dev = torch_dev
    m = half(key)
    n = m.n_rows
    X = np.random.default_rng(31).uniform(-1.0, 1.0, (n, 9))
    dm = sa.to_device(m, "csr", dev)
    dm.prepare_symmetric("expand")
    a_ptr, a_col, a_val = dm.symmetric_arrays()
    a = sa.Coo(n, n, np.repeat(np.arange(n, dtype=np.int32), np.diff(a_ptr)), a_col, a_val)
    fwd = sa.to_device(a, "csr", dev)
    Yf = torch.full((n, 9), float("nan"), dtype=torch.float64, device=dev)
    fwd.run_multi(torch.from_numpy(X).to(dev), Yf)
    torch.cuda.synchronize()
    want = Yf.cpu().numpy()
    for k in (1, 3, 8, 9):
        for layout in LAYOUTS:
            Y = run_sym_multi(torch, dev, dm, X, k, layout)
            assert np.array_equal(bits(Y), bits(want[:, :k])), f"{key} k={k} {layout}"
    for j in (0, 4, 8):
        for layout in LAYOUTS:
            Y = run_sym_multi(torch, dev, dm, X[:, j:j + 1], 1, layout)
            assert np.array_equal(bits(Y[:, 0]), bits(want[:, j])), f"{key} column {j} alone, {layout}"
    assert dm.symmetric_multi_info["kernel"] == "csr_multi_kernel"


# ------------------------------------------------------------------ 4. info
@pytest.mark.parametrize("key", ["symmetric_lower", "n67", "all_empty"] + list(GENERATED))
def test_info(torch_dev, key):
    torch, dev = torch_dev
    m = half(key)
    blocks = (m.n_rows + 127) // 128
    dm = sa.to_device(m, "csr", dev)
    assert dm.symmetric_multi_info == {"mode": None, "cap_cols": [0] * 4, "window_blocks": [0] * 4,
                                       "flush_entries": [0] * 4, "long_rows": 0, "segments": 0,
                                       "multi_owned_bytes": 0, "kernel": ""}
    dm.prepare_symmetric("fused")
    s_info, p_info, m_info = dm.symmetric_info, sa.plan_info(dm), dm.multi_info
    info = dm.symmetric_multi_info
    caps = info["cap_cols"]
    assert info["mode"] == "fused" and info["kernel"] == "csr_sym_multi_kernel"
    assert all(caps[w] * WIDTHS[w] == caps[0] for w in range(4)), caps  # cap_cols = cap / width
    assert caps[3] >= 128, "the window path must hold a full block's own rows"
    for w in range(4):
        want = sg.expected_fused(m, caps[w])
        assert (blocks, info["window_blocks"][w], info["flush_entries"][w]) == want, (key, w)
    assert (info["long_rows"], info["segments"], info["multi_owned_bytes"]) == (0, 0, 0)
    if key == "cantlike2":
        assert info["window_blocks"] == [488] * 4
    elif key == "rmat_tril":
        assert blocks == 782 and all(0 < info["window_blocks"][w] < blocks // 8 for w in range(4))
    elif key == "dense_column5000":
        # block b's union is [0, 128 b + 127]: it fits while 128 (b + 1) <= cap_cols
        assert blocks == 40 and info["window_blocks"] == [min(c // 128, 40) for c in caps]
        assert all(0 < nb < blocks for nb in info["window_blocks"]), "both paths at every width"
    X = np.ones((max(m.n_rows, 1), 3))
    run_sym_multi(torch, dev, dm, X, 3, "offset")
    assert dm.symmetric_info == s_info and s_info["owned_bytes"] == 8 * blocks, "a multi run changed symmetric_info"
    assert sa.plan_info(dm) == p_info and dm.multi_info == m_info and dm.symmetric_multi_info == info
    dm.prepare_symmetric("expand")
    info = dm.symmetric_multi_info
    assert info == {"mode": "expand", "cap_cols": [0] * 4, "window_blocks": [0] * 4, "flush_entries": [0] * 4,
                    "long_rows": 0, "segments": 0, "multi_owned_bytes": 0, "kernel": "csr_multi_kernel"}


# ------------------------------------------------------------ 5. width edges
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ["dense_column5000", "n129"])
def test_width_edges(torch_dev, key, mode):
    """k = 1, 2, 4, 8 exactly, ragged `live` (3, 5), two and three passes
    (9, 17): each against the columns of ONE 17-column reference, so a pass
    on the wrong X + 8b / Y + 8b or a write to a dead column shows."""
    torch, dev = torch_dev
    hm, X, ref = int_case(key, 17)
    dm = sa.to_device(hm, "csr", dev)
    dm.prepare_symmetric(mode)
    for k in (1, 2, 4, 8, 3, 5, 9, 17):
        for layout in LAYOUTS:
            exact.assert_exact(run_sym_multi(torch, dev, dm, X, k, layout), ref[:, :k], f"{key} {mode} k={k} {layout}")


# -------------------------------------------------------- 6. hot-column plan
def test_rmat_tril_reads_the_callers_columns(torch_dev):
    """The hot = 4096 plan owns a renumbered column copy; the run must read
    the caller's columns, in both modes."""
    torch, dev = torch_dev
    hm, X, ref = int_case("rmat_tril", 8)
    dm = sa.to_device(hm, "csr", dev, variant=4, hot=4096)
    assert dm.params["H"] > 0 and "hot-column table" in dm.params["plan"]
    for mode in MODES:
        dm.prepare_symmetric(mode)
        for k in (3, 8):
            exact.assert_exact(run_sym_multi(torch, dev, dm, X, k, "plain"), ref[:, :k], f"hot {mode} k={k}")


# --------------------------------------------------------------- 7. balanced
@pytest.mark.parametrize("order", ["symmetric first", "multi first"])
def test_balanced_inner_plan(torch_dev, order):
    """prepare_multi("balanced") extends to expand mode's inner plan over A
    (longest row 9,814 entries), whichever prepare comes first."""
    torch, dev = torch_dev
    hm, X, ref = int_case("rmat_tril", 8)
    e = sa.expand_symmetric(hm)
    assert int(np.bincount(e.row).max()) == 9814
    dm = sa.to_device(hm, "csr", dev)
    size = ctypes.sizeof(sa.MultiInfo)
    assert size == 4 * 4 + 8 * 8 + 64
    if order == "symmetric first":
        dm.prepare_symmetric("expand")
        assert dm.symmetric_multi_info["long_rows"] == 0
        dm.prepare_multi("balanced")
    else:
        dm.prepare_multi("balanced")
        dm.prepare_symmetric("expand")
    info = dm.symmetric_multi_info
    assert info["mode"] == "expand" and info["long_rows"] > 0 and info["segments"] > 0 and info["multi_owned_bytes"] > 0
    assert info["kernel"] == "csr_multi_long_kernel"
    mi = dm.multi_info
    assert mi["mode"] == "balanced" and (mi["t_long_rows"], mi["t_segments"], mi["t_owned_bytes"]) == (0, 0, 0)
    for k in (3, 8):
        for layout in LAYOUTS:
            exact.assert_exact(run_sym_multi(torch, dev, dm, X, k, layout), ref[:, :k], f"balanced {order} k={k} {layout}")
    # run_sym through the balanced inner plan is the unbalanced run
    y = sg.run_sym(torch, dev, dm, np.ascontiguousarray(X[:, 0]))
    exact.assert_exact(y, ref[:, 0], "run_sym on a balanced plan")
    # fused mode is unaffected
    dm.prepare_symmetric("fused")
    info = dm.symmetric_multi_info
    assert (info["long_rows"], info["segments"], info["multi_owned_bytes"]) == (0, 0, 0)
    exact.assert_exact(run_sym_multi(torch, dev, dm, X, 8, "plain"), ref, "fused on a balanced plan")
    dm.prepare_symmetric("expand")
    assert dm.symmetric_multi_info["long_rows"] > 0
    dm.prepare_multi(None)
    info = dm.symmetric_multi_info
    assert (info["long_rows"], info["segments"], info["multi_owned_bytes"]) == (0, 0, 0)
    assert info["kernel"] == "csr_multi_kernel" and dm.multi_info["mode"] is None
    assert ctypes.sizeof(sa.MultiInfo) == size
    exact.assert_exact(run_sym_multi(torch, dev, dm, X, 3, "plain"), ref[:, :3], "after prepare_multi(None)")


# ------------------------------------------------------ 8. n = 0, nnz = 0
@pytest.mark.parametrize("mode", MODES)
def test_empty(torch_dev, mode):
    torch, dev = torch_dev
    dm = sa.to_device(sg.coo(300, [], [], []), "csr", dev)
    dm.prepare_symmetric(mode)
    if mode == "fused":
        info = dm.symmetric_multi_info
        assert info["window_blocks"] == [0] * 4 and info["flush_entries"] == [0] * 4
    for k in (1, 3, 9):
        for layout in LAYOUTS:
            assert not run_sym_multi(torch, dev, dm, np.ones((300, k)), k, layout).any()
    d0 = sa.to_device(sg.coo(0, [], [], []), "csr", dev)
    d0.prepare_symmetric(mode)
    for layout in LAYOUTS:
        assert run_sym_multi(torch, dev, d0, np.ones((1, 3)), 3, layout).shape == (0, 3)  # Y's 3 tail rows checked


# --------------------------------------------------------------- 9. graph
@pytest.mark.parametrize("mode", MODES)
def test_graph_capture(torch_dev, mode):
    """One run_sym_multi with ldy > k captured on a single stream (no parallel
    branches), replayed, X overwritten in place, replayed again."""
    torch, dev = torch_dev
    hm, X, ref = int_case("dense_column5000", 17)
    n, k = hm.n_rows, 3
    dm = sa.to_device(hm, "csr", dev)
    dm.prepare_symmetric(mode)
    Xd = torch.from_numpy(np.array(X[:, :k], order="C")).to(dev)
    Ybuf = torch.full((n + TAIL, k + 3), SENTINEL, dtype=torch.float64, device=dev)
    Y = Ybuf[:, :k]
    dm.run_sym_multi(Xd, Y)  # first-call setup outside the capture
    torch.cuda.synchronize()
    Y[:n] = float("nan")
    before = Ybuf.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dm.run_sym_multi(Xd, Y)
    torch.cuda.synchronize()
    for first in (0, 8):  # columns 0..2, then 8..10 written over X in place
        Xd.copy_(torch.from_numpy(np.array(X[:, first:first + k], order="C")).to(dev))
        Y[:n] = float("nan")
        g.replay()
        torch.cuda.synchronize()
        exact.assert_exact(Y[:n].cpu().numpy(), ref[:, first:first + k], f"{mode} replay on columns {first}..")
    Y[:n] = float("nan")
    assert torch.equal(Ybuf.view(torch.int64), before.view(torch.int64)), "Y written outside its live part"


# ----------------------------------------------- 10. lifecycle and refusals
def test_lifecycle(torch_dev):
    """Unprepared: refused, Y untouched.  fused -> expand -> None -> fused with
    run, run_t, run_sym and run_multi of the same plan right throughout."""
    torch, dev = torch_dev
    key, k = "dense_column5000", 5
    hm, X, ref = int_case(key, 17)
    n = hm.n_rows
    e = sa.expand_symmetric(hm)
    dm = sa.to_device(hm, "csr", dev)
    dm.prepare_transpose("scatter")
    Xd = torch.from_numpy(np.array(X[:, :k], order="C")).to(dev)
    Y = torch.full((n, k), float("nan"), dtype=torch.float64, device=dev)
    before = Y.clone()

    def refused():
        with pytest.raises(sa.SpmvError) as err:
            dm.run_sym_multi(Xd, Y)
        assert err.value.rc == sa.OTHER_ERROR and "not prepared" in str(err.value)
        torch.cuda.synchronize()
        assert torch.equal(Y.view(torch.int64), before.view(torch.int64)), "a refused run wrote Y"

    def others_still_right():
        sg.assert_forward_and_transposed_still_right(torch, dev, dm, hm)  # run and run_t treat S literally
        exact.assert_exact(sg.run_sym(torch, dev, dm, np.ascontiguousarray(X[:, 1])), ref[:, 1], "run_sym")
        Yf = torch.full((n, 3), float("nan"), dtype=torch.float64, device=dev)
        dm.run_multi(torch.from_numpy(np.array(X[:, :3], order="C")).to(dev), Yf)
        torch.cuda.synchronize()
        fwd = exact.int_spmv(n, hm.row, hm.col, hm.val.astype(np.int64), X[:, :3].astype(np.int64))
        exact.assert_exact(Yf.cpu().numpy(), fwd, "run_multi")

    refused()
    for mode in ("fused", "expand", None, "fused"):
        dm.prepare_symmetric(mode)
        assert dm.symmetric_multi_info["mode"] == mode
        if mode is None:
            refused()
            continue
        s_info, p_info, t_info = dm.symmetric_info, sa.plan_info(dm), dm.transpose_info
        for layout in LAYOUTS:
            exact.assert_exact(run_sym_multi(torch, dev, dm, X, k, layout), ref[:, :k], f"lifecycle {mode} {layout}")
        assert (dm.symmetric_info, sa.plan_info(dm), dm.transpose_info) == (s_info, p_info, t_info)
        others_still_right()
    assert e.nnz > hm.nnz


def test_bad_arguments_refused(torch_dev):
    """The C call itself: k < 1, leading dimensions below k, NULL X / Y."""
    torch, dev = torch_dev
    m = half("symmetric_lower")
    dm = sa.to_device(m, "csr", dev)
    lib = sa.hip_lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    X = torch.zeros((m.n_rows, 4), dtype=torch.float64, device=dev)
    Y = torch.full((m.n_rows, 4), SENTINEL, dtype=torch.float64, device=dev)
    for mode in MODES:
        dm.prepare_symmetric(mode)
        for what, args in {
            "NULL X": (4, None, 4, Y.data_ptr(), 4), "NULL Y": (4, X.data_ptr(), 4, None, 4),
            "ldx < k": (4, X.data_ptr(), 3, Y.data_ptr(), 4), "ldy < k": (4, X.data_ptr(), 4, Y.data_ptr(), 3),
            "k = 0": (0, X.data_ptr(), 4, Y.data_ptr(), 4), "k < 0": (-1, X.data_ptr(), 4, Y.data_ptr(), 4),
        }.items():
            assert lib.spmv_plan_run_sym_multi(dm.plan, *args, st) == sa.OTHER_ERROR, (mode, what)
            assert lib.spmv_last_error().startswith(b"spmv_plan_run_sym_multi"), (mode, what)
        assert lib.spmv_plan_run_sym_multi(dm.plan, 4, None, 4, Y.data_ptr(), 4, st) == sa.OTHER_ERROR
        assert b"NULL" in lib.spmv_last_error()
    assert lib.spmv_plan_get_symmetric_multi_info(dm.plan, None) == sa.OTHER_ERROR
    torch.cuda.synchronize()
    assert bool((Y == SENTINEL).all()), "a refused call wrote Y"


@pytest.mark.parametrize("fmt", ["coo", "ell", "sell", "cmrs", "sell16"])
def test_refused_formats(torch_dev, fmt):
    torch, dev = torch_dev
    m = half("symmetric_lower")
    kw = {"ell_max_padding": None} if fmt == "ell" else {}
    dm = sa.to_device(m, fmt, dev, **kw)
    X = torch.zeros((m.n_rows, 2), dtype=torch.float64, device=dev)
    Y = torch.full((m.n_rows, 2), SENTINEL, dtype=torch.float64, device=dev)
    with pytest.raises(sa.SpmvError) as e:
        dm.run_sym_multi(X, Y)
    assert e.value.rc == sa.OTHER_ERROR and "not prepared" in str(e.value)
    torch.cuda.synchronize()
    assert bool((Y == SENTINEL).all())
    assert dm.symmetric_multi_info["mode"] is None


@pytest.mark.parametrize("name", ["wide", "tall"])
def test_refused_not_square(torch_dev, name):
    """A non-square CSR plan cannot be prepared: the C call refuses it."""
    torch, dev = torch_dev
    m = sa.read_mtx(GOLDEN / f"{name}.mtx")
    dm = sa.to_device(m, "csr", dev)
    lib = sa.hip_lib()
    rows = max(m.n_rows, m.n_cols)
    X = torch.zeros((rows, 2), dtype=torch.float64, device=dev)
    Y = torch.full((rows, 2), SENTINEL, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    assert lib.spmv_plan_run_sym_multi(dm.plan, 2, X.data_ptr(), 2, Y.data_ptr(), 2, st) == sa.OTHER_ERROR
    assert b"not prepared" in lib.spmv_last_error()
    with pytest.raises(sa.SpmvError) as e:
        dm.run_sym_multi(X, Y)
    assert e.value.rc == sa.OTHER_ERROR and "square" in str(e.value)
    torch.cuda.synchronize()
    assert bool((Y == SENTINEL).all())
