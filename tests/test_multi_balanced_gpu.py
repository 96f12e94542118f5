"""The balanced multi-vector CSR run on the GPU (spmv_plan_prepare_multi through
DeviceMatrix.prepare_multi, then run_multi / run_t_multi).

Reference for column j: oracle.file_order_spmv on X[:, j]; criterion: the
project's oracle.parity(rel=1e-6), per column.  Three layouts: "plain"
(ld == k, 16-byte aligned), "padded" (ldx = k + 3, ldy = k + 1) and "offset"
(both bases 8 bytes into their buffers).  Y starts as NaN in its live part and
12345.0 in its padding columns and in 3 rows past n_rows; after every run
everything but the live part is compared bit for bit with what it held.

The bit rule (include/spmv.h): column j's bits depend on the matrix, the plan
and input column j only; a row of at most long_len entries has the bits of the
unprepared run.  The exact references are those of tests/exact.py.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import exact
import spmv_amd as sa
import test_spmm_gpu as sg
import test_transpose_gpu as tg
from oracle import oracle

pytestmark = pytest.mark.gpu

SENTINEL = sg.SENTINEL
TAIL = 3
KS = (1, 2, 3, 4, 5, 8, 9, 17)
LAYOUTS = ("plain", "padded", "offset")
CSR_PLANS = [{}, {"lanes": 2}, {"lanes": 64}, {"variant": 1}, {"variant": 4}]
PLAN_IDS = ["-".join(f"{k}{v}" for k, v in kw.items()) or "default" for kw in CSR_PLANS]
OPTS = [(4, 8), (0, 3)]
FIXTURES = ["n67", "ragged_shuffled", "long_rows", "empty_rows", "longest_last", "all_empty", "one"]
SCALES = (1.0, -1.0, 2.0, 0.5, -4.0, 8.0, 0.25, -2.0, 16.0)  # exact scalings: the references scale with them


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch, torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def run(torch, dev, dm, m, X, k, layout, transposed=False):
    """One run_multi (or run_t_multi) on the first k columns of X (numpy) ->
    the live part of Y as numpy.  Asserts that nothing else of Y changed."""
    n_in, n_out = (m.n_rows, m.n_cols) if transposed else (m.n_cols, m.n_rows)
    ni, rows_y = max(n_in, 1), n_out + TAIL
    Xk = sg.to_dev(torch, dev, X[:, :k])
    ldx, ldy = (k + 3, k + 1) if layout == "padded" else (k, k)
    off = 1 if layout == "offset" else 0
    Xbuf = torch.full((ni * ldx + off,), float("nan"), dtype=torch.float64, device=dev)
    Xv = Xbuf[off:].view(ni, ldx)[:, :k]
    Xv[:n_in].copy_(Xk[:n_in])
    Ybuf = torch.full((rows_y * ldy + off,), SENTINEL, dtype=torch.float64, device=dev)
    Yv = Ybuf[off:].view(rows_y, ldy)[:, :k]
    assert Xv.data_ptr() % 16 == 8 * off and Yv.data_ptr() % 16 == 8 * off
    Yv[:n_out] = float("nan")
    before = Ybuf.clone()
    (dm.run_t_multi if transposed else dm.run_multi)(Xv, Yv)
    torch.cuda.synchronize()
    Y = Yv[:n_out].cpu().numpy().copy()
    Yv[:n_out] = float("nan")
    assert torch.equal(Ybuf.view(torch.int64), before.view(torch.int64)), f"k={k} {layout}: Y written outside its live part"
    return Y


def row_lens(m):
    return np.bincount(m.row, minlength=m.n_rows)[: m.n_rows] if m.nnz else np.zeros(m.n_rows, np.int64)


def check_counts(dm, m):
    """multi_info's counts are the host planner's for the reported thresholds."""
    info = dm.multi_info
    assert info["mode"] == "balanced"
    ptr, _, _ = sa.csr_from_coo(m)
    c = sa.csr_multi_plan(m.n_rows, ptr, info["long_len"], info["seg_len"], counts_only=True)
    assert (info["long_rows"], info["segments"], info["slots"]) == (c["n_long"], c["n_seg"], c["n_slots"])
    assert info["long_entries"] == int(row_lens(m)[row_lens(m) > info["long_len"]].sum())
    assert info["kernel"] == ("csr_multi_long_kernel" if c["n_seg"] else "csr_multi_kernel")
    return info


# ------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("kw", CSR_PLANS, ids=PLAN_IDS)
@pytest.mark.parametrize("name", FIXTURES)
def test_parity_fixtures(torch_dev, name, kw):
    torch, dev = torch_dev
    m, X, refs = sg.golden(name)
    dm = sa.to_device(m, "csr", dev, **kw)
    for long_len, seg_len in OPTS:
        dm.prepare_multi("balanced", long_len, seg_len)
        info = check_counts(dm, m)
        assert (info["long_len"], info["seg_len"]) == (long_len, seg_len)
        assert (info["segments"] > 0) == bool((row_lens(m) > long_len).any())
        for k in KS:
            for layout in LAYOUTS:
                Y = run(torch, dev, dm, m, X, k, layout)
                assert not np.isnan(Y).any(), f"{name} {kw} ({long_len}, {seg_len}) k={k} {layout}: NaN left in Y"
                sg.assert_columns(m, X, refs, Y, k)


@functools.lru_cache(maxsize=None)
def big_case(key):
    m = tg.golden("long_rows")[0] if key == "long_rows" else exact.generated(key)
    return sg._with_refs(m, 9, 17)


@pytest.mark.parametrize("kw", CSR_PLANS + [{"variant": 4, "hot": 4096}], ids=PLAN_IDS + ["variant4-hot4096"])
@pytest.mark.parametrize("key", ["long_rows", "one_row", "rmat"])
def test_parity_library_rule(torch_dev, key, kw):
    """The library's thresholds; the hot = 4096 plan owns a renumbered column
    copy and the balanced run must read the caller's columns."""
    torch, dev = torch_dev
    m, X, refs = big_case(key)
    dm = sa.to_device(m, "csr", dev, **kw)
    if kw.get("hot") and key == "rmat":
        assert dm.params["H"] > 0
    dm.prepare_multi()
    info = check_counts(dm, m)
    assert info["seg_len"] >= 1 and info["long_len"] >= 1
    assert info["segments"] > 0, (key, kw, info)  # each has a row longer than the rule's threshold at 64 lanes
    for k, layout in ((3, "plain"), (8, "plain"), (8, "offset"), (3, "padded")):
        sg.assert_columns(m, X, refs, run(torch, dev, dm, m, X, k, layout), k)


# ---------------------------------------------------------------- 2. bit rule
@pytest.mark.parametrize("case", [("ragged_shuffled", (4, 8)), ("long_rows", (4, 8)), ("long_rows", (0, 3)),
                                  ("n67", (0, 3)), ("rmat", (None, None)), ("rmat", (16, 64))],
                         ids=lambda c: f"{c[0]}-{c[1][0]}-{c[1][1]}")
def test_bit_rule(torch_dev, case):
    torch, dev = torch_dev
    key, (long_len, seg_len) = case
    m = exact.generated(key) if key in exact.GENERATED else sg.golden(key)[0]
    X = np.random.default_rng(23).uniform(-1.0, 1.0, (max(m.n_cols, 1), 9))
    dm = sa.to_device(m, "csr", dev)
    plain = run(torch, dev, dm, m, X, 9, "plain")  # the unprepared run
    dm.prepare_multi("balanced", long_len, seg_len)
    info = check_counts(dm, m)
    assert info["segments"] > 0
    single = np.stack([run(torch, dev, dm, m, np.ascontiguousarray(X[:, j:j + 1]), 1, "plain")[:, 0] for j in range(9)],
                      axis=1)
    for k in (2, 3, 8, 9):
        for layout in LAYOUTS:
            Y = run(torch, dev, dm, m, X, k, layout)
            assert np.array_equal(bits(Y), bits(single[:, :k])), f"{case} k={k} {layout}: differs from the k = 1 runs"
            Y2 = run(torch, dev, dm, m, X, k, layout)
            assert np.array_equal(bits(Y), bits(Y2)), f"{case} k={k} {layout}: two balanced runs differ"
    short = row_lens(m) <= info["long_len"]
    assert not short.all()
    if key != "n67":
        assert short.any()
    assert np.array_equal(bits(single[short]), bits(plain[short])), f"{case}: a short row's bits changed"


# ------------------------------------------------------------------- 3. exact
EXACT_KEYS = ["rmat", "ragged", "one_row", "empty_runs"]
EXACT_OPTS = [(None, None), (64, 256)]


@functools.lru_cache(maxsize=None)
def integer_case(key):
    e = exact.integerize(exact.generated(key), seed=900 + len(key), k=9)
    return e


@pytest.mark.parametrize("opts", EXACT_OPTS, ids=["rule", "64-256"])
@pytest.mark.parametrize("key", EXACT_KEYS)
def test_exact_on_integers(torch_dev, key, opts):
    torch, dev = torch_dev
    e = integer_case(key)
    dm = sa.to_device(e.m, "csr", dev)
    dm.prepare_multi("balanced", *opts)
    info = check_counts(dm, e.m)
    if opts[0] is not None:
        assert info["segments"] > 0 and info["slots"] > 0
    for k, layout in ((9, "padded"), (8, "plain"), (3, "offset")):
        Y = run(torch, dev, dm, e.m, e.x, k, layout)
        for j in range(k):
            exact.assert_exact(Y[:, j], e.ref[:, j], f"{key} {opts} k={k} {layout} column {j}")


@functools.lru_cache(maxsize=None)
def real_case(key):
    mr, x, _ = exact.realize(exact.generated(key), seed=700 + len(key))
    ref, bound = exact.exact_reference(mr, x), exact.fp64_bound(mr, x)
    X = np.stack([s * x for s in SCALES], axis=1)
    X.setflags(write=False)
    return mr, x, X, ref, bound


@pytest.mark.parametrize("opts", EXACT_OPTS, ids=["rule", "64-256"])
@pytest.mark.parametrize("key", EXACT_KEYS)
def test_fp64_bound(torch_dev, key, opts):
    """|y - ref| <= (n_i + 2) 2^-53 sum|a x| on wide-range real data."""
    torch, dev = torch_dev
    mr, x, X, ref, bound = real_case(key)
    dm = sa.to_device(mr, "csr", dev)
    dm.prepare_multi("balanced", *opts)
    for k, layout in ((9, "offset"), (8, "plain")):
        Y = run(torch, dev, dm, mr, X, k, layout)
        for j in range(k):
            exact.assert_fp64(Y[:, j], mr, x, ref=SCALES[j] * ref, bound=abs(SCALES[j]) * bound,
                              what=f"{key} {opts} k={k} {layout} column {j}")


# --------------------------------------------------------------- 4. lifecycle
def test_lifecycle(torch_dev):
    torch, dev = torch_dev
    m, X, refs = sg.golden("long_rows")
    dm = sa.to_device(m, "csr", dev)
    dm.prepare_transpose("scatter")
    p_info, t_info, tm_info = sa.plan_info(dm), dm.transpose_info, dm.transpose_multi_info
    none = dm.multi_info
    assert none["mode"] is None and none["owned_bytes"] == 0 and none["kernel"] == ""
    assert all(v == 0 for k, v in none.items() if k not in ("mode", "kernel"))
    plain = run(torch, dev, dm, m, X, 5, "padded")

    dm.prepare_multi("balanced", 4, 8)
    info = check_counts(dm, m)
    assert info["owned_bytes"] > 0 and info["segments"] > 0 and info["slots"] > 0
    assert (info["t_long_rows"], info["t_segments"], info["t_owned_bytes"]) == (0, 0, 0)
    assert sa.plan_info(dm) == p_info and dm.transpose_info == t_info and dm.transpose_multi_info == tm_info
    bal = run(torch, dev, dm, m, X, 5, "padded")
    sg.assert_columns(m, X, refs, bal, 5)
    assert not np.array_equal(bits(bal), bits(plain)), "the balanced run did not change any long row's order"
    dm.prepare_multi("balanced", 4, 8)  # a no-op
    assert dm.multi_info == info
    assert np.array_equal(bits(run(torch, dev, dm, m, X, 5, "padded")), bits(bal))

    # bad options: refused, the plan runs on in its mode
    lib = sa.hip_lib()
    for mode, long_len, seg_len in ((1, -2, 8), (1, 4, 0), (1, 4, -3), (2, 4, 8), (-1, -1, -1)):
        o = sa.MultiOpts(long_len, seg_len)
        assert lib.spmv_plan_prepare_multi(dm.plan, mode, ctypes.byref(o)) == sa.OTHER_ERROR, (mode, long_len, seg_len)
        assert lib.spmv_last_error().startswith(b"spmv_plan_prepare_multi")
        assert dm.multi_info == info
    with pytest.raises(sa.SpmvError) as err:
        dm.prepare_multi("balanced", 4, 0)
    assert err.value.rc == sa.OTHER_ERROR
    assert np.array_equal(bits(run(torch, dev, dm, m, X, 5, "padded")), bits(bal))

    dm.prepare_multi("balanced", 0, 3)  # other options: rebuilt
    info2 = check_counts(dm, m)
    assert info2 != info and info2["segments"] > info["segments"]
    sg.assert_columns(m, X, refs, run(torch, dev, dm, m, X, 5, "padded"), 5)
    tg.assert_run_still_right(torch, dev, dm, m)  # the single-vector run of the same plan

    dm.prepare_multi(None)
    assert dm.multi_info == none
    assert np.array_equal(bits(run(torch, dev, dm, m, X, 5, "padded")), bits(plain)), "the unprepared bits did not return"
    assert sa.plan_info(dm) == p_info and dm.transpose_info == t_info
    # bad options on an unprepared plan: still unprepared
    o = sa.MultiOpts(-5, 1)
    assert lib.spmv_plan_prepare_multi(dm.plan, 1, ctypes.byref(o)) == sa.OTHER_ERROR
    assert dm.multi_info == none
    assert np.array_equal(bits(run(torch, dev, dm, m, X, 5, "padded")), bits(plain))


def test_matrix_without_long_rows(torch_dev):
    """No row over the threshold: no tables, no bytes, the unprepared bits."""
    torch, dev = torch_dev
    m, X, refs = sg.cantlike()
    dm = sa.to_device(m, "csr", dev)
    plain = run(torch, dev, dm, m, X, 8, "plain")
    dm.prepare_multi()
    info = check_counts(dm, m)
    assert (info["long_rows"], info["segments"], info["slots"], info["owned_bytes"]) == (0, 0, 0, 0)
    assert np.array_equal(bits(run(torch, dev, dm, m, X, 8, "plain")), bits(plain))


@pytest.mark.parametrize("fmt", ["coo", "ell", "sell", "cmrs", "sell16"])
def test_refused_formats(torch_dev, fmt):
    torch, dev = torch_dev
    m = sg.golden("ragged_shuffled")[0]
    dm = sg.build(dev, m, fmt)
    with pytest.raises(sa.SpmvError) as e:
        dm.prepare_multi()
    assert e.value.rc == sa.OTHER_ERROR and "CSR" in str(e.value)
    with pytest.raises(sa.SpmvError):
        dm.prepare_multi(None)
    assert dm.multi_info["mode"] is None
    sg.assert_run_still_right(torch, dev, dm, m)


# ----------------------------------------------------------- 5. graph capture
def test_graph_capture(torch_dev):
    """A balanced run_multi at k = 8 (row, segment and finish kernels) captured
    on one stream; the replays have the eager run's bits."""
    torch, dev = torch_dev
    m, X, refs = sg.golden("long_rows")
    k = 8
    dm = sa.to_device(m, "csr", dev)
    dm.prepare_multi("balanced", 4, 8)
    assert dm.multi_info["slots"] > 0
    eager = run(torch, dev, dm, m, X, k, "padded")
    Xd = sg.to_dev(torch, dev, X[:, :k])
    Ybuf = torch.full((m.n_rows + TAIL, k + 1), SENTINEL, dtype=torch.float64, device=dev)
    Y = Ybuf[:, :k]
    dm.run_multi(Xd, Y)  # first-call setup outside the capture
    torch.cuda.synchronize()
    Y[: m.n_rows] = float("nan")
    before = Ybuf.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dm.run_multi(Xd, Y)
    torch.cuda.synchronize()
    for replay in range(2):
        Y[: m.n_rows] = float("nan")
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(Y[: m.n_rows].cpu().numpy()), bits(eager)), f"replay {replay}"
    Y[: m.n_rows] = float("nan")
    assert torch.equal(Ybuf.view(torch.int64), before.view(torch.int64)), "Y written outside its live part"


# -------------------------------------------------------- 6. transposed copy
@pytest.mark.parametrize("first", ["transpose", "multi"])
@pytest.mark.parametrize("key", ["ragged_shuffled", "long_rows", "rmat"])
def test_transposed_copy(torch_dev, key, first):
    torch, dev = torch_dev
    m = exact.generated(key) if key in exact.GENERATED else tg.golden(key)[0]
    opts = (None, None) if key == "rmat" else (4, 8)
    ptr, col, val = sa.csr_from_coo(m)
    k = 9
    Xt = np.random.default_rng(41).uniform(-1.0, 1.0, (max(m.n_rows, 1), k))
    want = np.full((m.n_cols, k), np.nan)
    sa.cpu_csr_t_multi(m.n_rows, m.n_cols, ptr, col, val, np.ascontiguousarray(Xt[: m.n_rows]), want)

    dm = sa.to_device(m, "csr", dev)
    if first == "transpose":
        dm.prepare_transpose("copy")
        t_info = dm.transpose_info
        dm.prepare_multi("balanced", *opts)
    else:
        dm.prepare_multi("balanced", *opts)
        dm.prepare_transpose("copy")
        t_info = dm.transpose_info
    assert dm.transpose_info == t_info  # the inner plan's new bytes are reported by multi_info only
    info = check_counts(dm, m)
    assert info["t_segments"] > 0 and info["t_long_rows"] > 0 and info["t_owned_bytes"] > 0

    # the same product by a forward plan over the host-built A^T, prepared the same way
    t_ptr, t_col, t_val = sa.csr_transpose(m.n_rows, m.n_cols, ptr, col, val)
    coo_t = tg.coo(m.n_cols, m.n_rows, np.repeat(np.arange(m.n_cols), np.diff(t_ptr)), t_col, t_val)
    fwd = sa.to_device(coo_t, "csr", dev)
    fwd.prepare_multi("balanced", *opts)
    f_info = fwd.multi_info
    assert (info["t_long_rows"], info["t_segments"], info["t_owned_bytes"]) == \
        (f_info["long_rows"], f_info["segments"], f_info["owned_bytes"])
    for kk, layout in ((9, "offset"), (8, "plain"), (3, "padded")):
        Y = run(torch, dev, dm, m, Xt, kk, layout, transposed=True)
        for j in range(kk):
            x = np.ascontiguousarray(Xt[: m.n_rows, j])
            bad = oracle.parity(np.ascontiguousarray(Y[:, j]), np.ascontiguousarray(want[:, j]), m.col, m.row, m.val, x,
                                m.n_cols, rel=1e-6)
            assert bad.size == 0, f"{key} k={kk} {layout} column {j}: {bad.size} bad entries, first {bad[:5]}"
        Yf = run(torch, dev, fwd, coo_t, Xt, kk, layout)
        assert np.array_equal(bits(Y), bits(Yf)), f"{key} k={kk} {layout}: differs from the forward plan over A^T"

    if first == "transpose":  # either call ends it
        dm.prepare_transpose(None)
        after = dm.multi_info
        assert after["mode"] == "balanced" and after["segments"] == info["segments"]
    else:
        dm.prepare_multi(None)
        after = dm.multi_info
        assert after["mode"] is None
        fwd.prepare_multi(None)  # the inner plan is unprepared again: a default forward plan's bits
        Y = run(torch, dev, dm, m, Xt, 8, "plain", transposed=True)
        assert np.array_equal(bits(Y), bits(run(torch, dev, fwd, coo_t, Xt, 8, "plain")))
        dm.prepare_transpose(None)
    assert (after["t_long_rows"], after["t_segments"], after["t_owned_bytes"]) == (0, 0, 0)
    assert dm.transpose_info["mode"] is None and dm.transpose_info["owned_bytes"] == 0
