"""The multi-vector transposed product Y = A^T X on the GPU
(spmv_plan_run_t_multi through DeviceMatrix.run_t_multi), both modes.

Layout (include/spmv.h): X[r*ldx + j], Y[c*ldy + j], j < k.  Two layouts are
run: "plain" (ld == k, 16-byte-aligned bases) and "offset" (bases 8 bytes into
larger buffers, ldx = k + 1, ldy = k + 3; NaN in X's gaps and flanks, 12345.0
in Y's gaps, flanks and the 3 rows past n_cols).  Y's live part starts as NaN.
After every run everything of Y's buffer but the live part is compared bit
for bit with what it held before.

References (tests/exact.py): on integerize()'d matrices with integer X every
partial sum in any order is an integer below 2^52, so every column must EQUAL
exact.int_spmv on the swapped COO; on real data every column meets the
textbook bound (n_c + 2) 2^-53 sum|a x| of exact.fp64_bound.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import exact
import spmv_amd as sa
import test_transpose_gpu as tg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch, torch.device("cuda:0")


MODES = tg.MODES
SENTINEL = tg.SENTINEL
TAIL = tg.TAIL
WIDTHS = (1, 2, 4, 8)
KS = (1, 2, 3, 4, 5, 8, 9, 17)  # every width, a ragged last block, three passes
KMAX = 17
LAYOUTS = ("plain", "offset")
FIXTURES = ["n67", "long_rows", "ragged_shuffled", "wide", "tall", "duplicates", "empty_rows", "all_empty"]
SCALES = (1.0, -1.0, 2.0, 0.5, -4.0, 8.0, 0.25, -2.0, 16.0)  # exact scalings: the references scale with them


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def run_t_multi(torch, dev, dm, m, Xt, k, layout):
    """One run_t_multi on the first k columns of Xt (numpy, n_rows x >= k):
    -> Y[:n_cols, :k] as numpy.  Asserts that nothing but Y's live part changed."""
    nr, rows_y = max(m.n_rows, 1), m.n_cols + TAIL
    Xk = torch.from_numpy(np.array(Xt[:, :k], order="C")).to(dev)
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
    Xv[: m.n_rows].copy_(Xk[: m.n_rows])
    Yv[: m.n_cols] = float("nan")
    before = Ybuf.clone()
    dm.run_t_multi(Xv, Yv)
    torch.cuda.synchronize()
    Y = Yv[: m.n_cols].cpu().numpy().copy()
    Yv[: m.n_cols] = float("nan")  # then the whole buffer must be what it was: gaps, flanks, rows past n_cols
    assert torch.equal(Ybuf.view(torch.int64), before.view(torch.int64)), f"k={k} {layout}: Y written outside its live part"
    return Y


@functools.lru_cache(maxsize=None)
def integer_case(key, seed):
    """(Exact, Xt[n_rows, kmax] integer-valued float64, int64 reference A^T Xt);
    kmax = 17 on the fixtures, 8 on the generated matrices (run at k <= 8)."""
    if key in exact.GENERATED:
        return integer_of(exact.generated(key), seed, 8)
    return integer_of(tg.golden(key)[0], seed)


def integer_of(m, seed, kmax=KMAX):
    e = exact.integerize(m, seed=seed)
    Xt_i = exact._signed_ints(np.random.default_rng(seed + 1), (m.n_rows, kmax), e.b)
    ref = exact.int_spmv(m.n_cols, m.col, m.row, e.m.val.astype(np.int64), Xt_i)
    assert (np.abs(ref) < (1 << 53)).all()
    Xt = Xt_i.astype(np.float64)
    Xt.setflags(write=False)
    ref.setflags(write=False)
    return e, Xt, ref


# ------------------------------------------------ 1. exact on integers
@pytest.mark.parametrize("kw", tg.CSR_PLANS, ids=tg.PLAN_IDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_exact_on_integers(torch_dev, name, kw):
    torch, dev = torch_dev
    e, Xt, ref = integer_case(name, 300 + FIXTURES.index(name))
    dm = sa.to_device(e.m, "csr", dev, **kw)
    got = {}
    for mode in MODES:
        dm.prepare_transpose(mode)
        assert dm.transpose_multi_info["mode"] == mode
        for k in KS:
            for layout in LAYOUTS:
                what = f"{name} {kw} {mode} k={k} {layout}"
                Y = run_t_multi(torch, dev, dm, e.m, Xt, k, layout)
                exact.assert_exact(Y, ref[:, :k], what)
                if mode == "scatter":  # integer sums are exact in any order: the atomics give the same bits
                    Y2 = run_t_multi(torch, dev, dm, e.m, Xt, k, layout)
                    assert np.array_equal(bits(Y), bits(Y2)), f"{what}: two runs differ"
                got[mode, k, layout] = Y
    for k in KS:
        for layout in LAYOUTS:
            assert np.array_equal(bits(got["scatter", k, layout]), bits(got["copy", k, layout])), \
                f"{name} {kw} k={k} {layout}: scatter and copy differ"


# ------------------------------------------- 2. the fp64 bound on real data
@functools.lru_cache(maxsize=None)
def real_case(key):
    m = exact.generated(key) if key in exact.GENERATED else tg.golden(key)[0]
    mr, _, xt = exact.realize(m, seed=700 + len(key))
    ref_t = exact.exact_reference(mr, xt, transpose=True)
    bound_t = exact.fp64_bound(mr, xt, transpose=True)
    Xt = np.stack([s * xt for s in SCALES], axis=1)
    Xt.setflags(write=False)
    return mr, xt, Xt, ref_t, bound_t


def assert_bounded(torch, dev, dm, key, ks, layout, what):
    mr, xt, Xt, ref_t, bound_t = real_case(key)
    for k in ks:
        Y = run_t_multi(torch, dev, dm, mr, Xt, k, layout)
        for j in range(k):
            exact.assert_fp64(Y[:, j], mr, xt, transpose=True, ref=SCALES[j] * ref_t, bound=abs(SCALES[j]) * bound_t,
                              what=f"{what} k={k} column {j}")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ["n67", "long_rows", "ragged_shuffled", "cantlike", "rmat"])
def test_fp64_bound(torch_dev, key, mode):
    torch, dev = torch_dev
    dm = sa.to_device(real_case(key)[0], "csr", dev)
    dm.prepare_transpose(mode)
    assert_bounded(torch, dev, dm, key, (3, 9), "offset", f"{key} {mode}")


# ---------------------------------------------------- 3. generated matrices
@pytest.mark.parametrize("kw", [{}, {"variant": 4, "hot": 4096}], ids=["default", "variant4-hot4096"])
@pytest.mark.parametrize("key", ["cantlike", "rmat", "ragged"])
def test_generated(torch_dev, key, kw):
    """LDS accumulators at every width (cant-like), global atomics for wide
    row blocks (R-MAT, ragged); the hot = 4096 plan owns a renumbered column
    copy and the transposed run must read the caller's columns."""
    torch, dev = torch_dev
    e, Xt, ref = integer_case(key, 400 + len(key))
    dm = sa.to_device(e.m, "csr", dev, **kw)
    if kw.get("hot") and key == "rmat":
        assert dm.params["H"] > 0
    for mode in MODES:
        dm.prepare_transpose(mode)
        info, blocks = dm.transpose_multi_info, (e.m.n_rows + 127) // 128
        if mode == "scatter":
            assert info["kernel"] == "csr_t_multi_kernel"
            assert all(0 <= n <= blocks for n in info["lds_blocks"])
            if key == "cantlike":
                assert info["lds_blocks"][3] > 0
            if key == "rmat":
                assert all(n < blocks for n in info["lds_blocks"])
        else:
            assert info["cap_cols"] == [0] * 4 and info["lds_blocks"] == [0] * 4 and info["kernel"] == "csr_multi_kernel"
        for k in (3, 8):
            exact.assert_exact(run_t_multi(torch, dev, dm, e.m, Xt, k, "plain"), ref[:, :k], f"{key} {kw} {mode} k={k}")
        exact.assert_exact(run_t_multi(torch, dev, dm, e.m, Xt, 3, "offset"), ref[:, :3], f"{key} {kw} {mode} offset")


# ------------------------------------------------ 4. the edge of every width
def test_width_edges(torch_dev):
    """One row with entries in columns 0 and `last`: span cap_cols[w] is summed
    in LDS by the kernel of width w, span cap_cols[w] + 1 goes straight to Y."""
    torch, dev = torch_dev
    d0 = sa.to_device(tg.golden("n67")[0], "csr", dev)
    d0.prepare_transpose("scatter")
    caps = d0.transpose_multi_info["cap_cols"]
    assert len(caps) == 4 and all(c > 1 for c in caps)
    assert all(caps[i] * WIDTHS[i] == caps[0] for i in range(4)), caps  # one accumulator size, cap_cols = capM / KV
    for wi, w in enumerate(WIDTHS):
        for last, lds_blocks in ((caps[wi] - 1, 1), (caps[wi], 0)):
            m = tg.coo(1, caps[wi] + 8, [0, 0], [0, last], [3.0, -5.0])
            Xt_i = np.arange(1, w + 1, dtype=np.int64)[None, :] * np.array([[7]])
            ref = exact.int_spmv(m.n_cols, m.col, m.row, m.val.astype(np.int64), Xt_i)
            dm = sa.to_device(m, "csr", dev)
            dm.prepare_transpose("scatter")
            assert dm.transpose_multi_info["lds_blocks"][wi] == lds_blocks, (w, last)
            for k in sorted({w, max(w - 1, 1)}):
                for layout in LAYOUTS:
                    Y = run_t_multi(torch, dev, dm, m, Xt_i.astype(np.float64), k, layout)
                    exact.assert_exact(Y, ref[:, :k], f"width {w} last {last} k={k} {layout}")


def test_mixed_blocks(torch_dev):
    """The 1,000 x 100,000 matrix of test_transpose_gpu.test_mixed_blocks at
    k = 8: seven row blocks sum in LDS, one spans more than every cap."""
    torch, dev = torch_dev
    rows = np.repeat(np.arange(1000), 8)
    cols = rows + np.tile(np.arange(8), 1000)
    rows, cols = np.append(rows, 500), np.append(cols, 99_999)
    e, Xt, ref = integer_of(tg.coo(1000, 100_000, rows, cols, np.ones(rows.size)), 55)
    dm = sa.to_device(e.m, "csr", dev)
    for mode in MODES:
        dm.prepare_transpose(mode)
        if mode == "scatter":
            assert dm.transpose_multi_info["lds_blocks"] == [7] * 4
        for layout in LAYOUTS:
            exact.assert_exact(run_t_multi(torch, dev, dm, e.m, Xt, 8, layout), ref[:, :8], f"mixed {mode} {layout}")


# ------------------------------------------------------- 5. copy-mode bits
@pytest.mark.parametrize("name", ["ragged_shuffled", "duplicates", "n67", "wide"])
def test_copy_mode_bits(torch_dev, name):
    """Copy mode: column j has the bits of run_multi on a default forward CSR
    plan over the host-built A^T, whatever k and the layout."""
    torch, dev = torch_dev
    m = tg.golden(name)[0]
    Xt = np.random.default_rng(31).uniform(-1.0, 1.0, (max(m.n_rows, 1), 9))
    dm = sa.to_device(m, "csr", dev)
    dm.prepare_transpose("copy")
    t_ptr, t_col, t_val = tg._host_transpose(m)
    coo_t = tg.coo(m.n_cols, m.n_rows, np.repeat(np.arange(m.n_cols), np.diff(t_ptr)), t_col, t_val)
    fwd = sa.to_device(coo_t, "csr", dev)
    Yf = torch.full((m.n_cols, 9), float("nan"), dtype=torch.float64, device=dev)
    fwd.run_multi(torch.from_numpy(Xt).to(dev), Yf)
    torch.cuda.synchronize()
    want = Yf.cpu().numpy()
    for k in (3, 8, 9):
        for layout in LAYOUTS:
            Y = run_t_multi(torch, dev, dm, m, Xt, k, layout)
            assert np.array_equal(bits(Y), bits(want[:, :k])), f"{name} k={k} {layout}"


# ----------------------------------------------------------- 6. graph capture
@pytest.mark.parametrize("mode", MODES)
def test_graph_capture(torch_dev, mode):
    """One run_t_multi with ldy > k captured on a single stream, replayed
    twice with Y refilled with NaN in between."""
    torch, dev = torch_dev
    e, Xt, ref = integer_case("ragged_shuffled", 300 + FIXTURES.index("ragged_shuffled"))
    m, k = e.m, 5
    dm = sa.to_device(m, "csr", dev)
    dm.prepare_transpose(mode)
    X = torch.from_numpy(np.array(Xt[:, :k], order="C")).to(dev)
    Ybuf = torch.full((m.n_cols + TAIL, k + 3), SENTINEL, dtype=torch.float64, device=dev)
    Y = Ybuf[:, :k]
    dm.run_t_multi(X, Y)  # first-call setup outside the capture
    torch.cuda.synchronize()
    Y[: m.n_cols] = float("nan")
    before = Ybuf.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dm.run_t_multi(X, Y)
    torch.cuda.synchronize()
    for replay in range(2):
        Y[: m.n_cols] = float("nan")
        g.replay()
        torch.cuda.synchronize()
        exact.assert_exact(Y[: m.n_cols].cpu().numpy(), ref[:, :k], f"{mode} replay {replay}")
    Y[: m.n_cols] = float("nan")
    assert torch.equal(Ybuf.view(torch.int64), before.view(torch.int64)), "Y written outside its live part"


# --------------------------------------------------------------- 7. lifecycle
def test_lifecycle(torch_dev):
    torch, dev = torch_dev
    e, Xt, ref = integer_case("ragged_shuffled", 300 + FIXTURES.index("ragged_shuffled"))
    m, k = e.m, 5
    dm = sa.to_device(m, "csr", dev)
    X = torch.from_numpy(np.array(Xt[:, :k], order="C")).to(dev)
    Y = torch.full((m.n_cols, k), float("nan"), dtype=torch.float64, device=dev)
    before = Y.clone()

    def refused():
        with pytest.raises(sa.SpmvError) as err:
            dm.run_t_multi(X, Y)
        assert err.value.rc == sa.OTHER_ERROR
        torch.cuda.synchronize()
        assert torch.equal(Y.view(torch.int64), before.view(torch.int64)), "a refused run wrote Y"

    refused()  # not prepared
    assert dm.transpose_multi_info == {"mode": None, "cap_cols": [0] * 4, "lds_blocks": [0] * 4, "kernel": ""}
    for mode in ("scatter", "copy", "scatter"):  # switching modes: still right
        dm.prepare_transpose(mode)
        t_info, p_info = dm.transpose_info, sa.plan_info(dm)
        exact.assert_exact(run_t_multi(torch, dev, dm, m, Xt, k, "offset"), ref[:, :k], f"lifecycle {mode}")
        assert dm.transpose_info == t_info and sa.plan_info(dm) == p_info, "a multi run changed the plan's info"
        # the other runs of the same plan
        tg.assert_run_still_right(torch, dev, dm, m)
        y1 = tg.run_t(torch, dev, dm, m, Xt[:, 0])
        exact.assert_exact(y1[: m.n_cols], ref[:, 0], f"run_t after a multi run ({mode})")
        Xf = np.ascontiguousarray(e.x[:, None] * np.array([[1.0, -2.0, 4.0]]))
        Yf = torch.full((m.n_rows, 3), float("nan"), dtype=torch.float64, device=dev)
        dm.run_multi(torch.from_numpy(Xf).to(dev), Yf)
        torch.cuda.synchronize()
        exact.assert_exact(Yf.cpu().numpy(), e.ref[:, None] * np.array([[1, -2, 4]]), f"run_multi after a multi run ({mode})")
    dm.prepare_transpose(None)
    refused()


def test_bad_arguments_refused(torch_dev):
    """The C call itself: NULL X / Y and leading dimensions below k."""
    torch, dev = torch_dev
    m = tg.golden("ragged_shuffled")[0]
    dm = sa.to_device(m, "csr", dev)
    lib = sa.hip_lib()
    st = torch.cuda.current_stream(dev).cuda_stream
    X = torch.zeros((m.n_rows, 4), dtype=torch.float64, device=dev)
    Y = torch.full((m.n_cols, 4), SENTINEL, dtype=torch.float64, device=dev)
    for mode in MODES:
        dm.prepare_transpose(mode)
        for what, args in {
            "NULL X": (4, None, 4, Y.data_ptr(), 4), "NULL Y": (4, X.data_ptr(), 4, None, 4),
            "ldx < k": (4, X.data_ptr(), 3, Y.data_ptr(), 4), "ldy < k": (4, X.data_ptr(), 4, Y.data_ptr(), 3),
            "k = 0": (0, X.data_ptr(), 4, Y.data_ptr(), 4), "k < 0": (-1, X.data_ptr(), 4, Y.data_ptr(), 4),
        }.items():
            assert lib.spmv_plan_run_t_multi(dm.plan, *args, st) == sa.OTHER_ERROR, (mode, what)
            assert lib.spmv_last_error().startswith(b"spmv_plan_run_t_multi"), (mode, what)
        assert lib.spmv_plan_run_t_multi(dm.plan, 4, None, 4, Y.data_ptr(), 4, st) == sa.OTHER_ERROR
        assert b"NULL" in lib.spmv_last_error()
    torch.cuda.synchronize()
    assert bool((Y == SENTINEL).all()), "a refused call wrote Y"


@pytest.mark.parametrize("fmt", ["coo", "ell", "sell", "cmrs", "sell16"])
def test_refused_formats(torch_dev, fmt):
    torch, dev = torch_dev
    m = tg.golden("ragged_shuffled")[0]
    kw = {"ell_max_padding": None} if fmt == "ell" else {}
    dm = sa.to_device(m, fmt, dev, **kw)
    X = torch.zeros((m.n_rows, 2), dtype=torch.float64, device=dev)
    Y = torch.full((m.n_cols, 2), SENTINEL, dtype=torch.float64, device=dev)
    with pytest.raises(sa.SpmvError) as e:
        dm.run_t_multi(X, Y)
    assert e.value.rc == sa.OTHER_ERROR and "not prepared" in str(e.value)
    torch.cuda.synchronize()
    assert bool((Y == SENTINEL).all())
    assert dm.transpose_multi_info["mode"] is None
    tg.assert_run_still_right(torch, dev, dm, m)
