"""The row-block core (csrc/rowblock.h) and its eight kernels at their own
constants, on the MI355X: csr_t_window_kernel, csr_t_multi_kernel<1, 2, 4, 8>
(csrc/transpose.hip), csr_sym_window_kernel and csr_sym_multi_kernel<1, 2, 4, 8>
(csrc/symmetric.hip), through spmv_plan_run_t, spmv_plan_run_t_multi,
spmv_plan_run_sym and spmv_plan_run_sym_multi.  tests/thresholds.py builds the
matrices and says what it delivered (tests/test_thresholds.py checks that
without a GPU):

  the stream family   blocks of 1 .. 5,121 entries on both sides of every loop
                      bound of rb_stream's two forms, laid out for rb_row_of's
                      search, wave_run_add's scan and the DPP rounds; last
                      blocks of 1, 2 and 127 rows
  the cap family      column spans and union windows of exactly every cap and
                      one more, every accumulator word hit, neighbouring
                      windows overlapping; launches above 64 KiB of dynamic LDS
  the dropped family  entries in columns -1, n and n + 1, which the scatter and
                      fused runs drop and the copy and expand modes refuse
  the builders        spmv_dev_csr_from_coo and spmv_dev_csr_transpose refuse
                      an index past n without writing past their offsets

Every output starts as NaN between guard elements that are compared bit for
bit, every input is compared bit for bit afterwards.  Every product and width
is checked with both rules of tests/exact.py: equality with an int64 reference
on the integer copy, and |y - ref| <= (n_i + 2) 2^-53 sum |a x| on the
wide-range copy, a bound that holds for any order of the sums, an LDS
accumulator flushed into y included.  The sums come from atomics: "the same
bits twice" is asserted for the integer copy only.
"""
from __future__ import annotations

import numpy as np
import pytest

import exact
import spmv_amd as sa
import thresholds as th
from test_iterate_multi_gpu import GUARD, _place

pytestmark = pytest.mark.gpu

# hot = 64 (a table exists on the tiled path only): the runs must read the caller's columns, not the renumbered copy
PLANS = [{}, {"variant": 4, "hot": 64}, {"variant": 4}]
PLAN_IDS = ["default", "variant4-hot64", "variant4"]
LAYOUTS = ("tight", "padded")
_worst = {}  # kernel -> largest error / bound seen


def note(what, ratio):
    _worst[what] = max(_worst.get(what, 0.0), float(ratio))


@pytest.fixture(scope="module")
def torch_dev():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    yield torch, torch.device("cuda:0")
    if _worst:  # the measured figures (pytest -s)
        print("\nlargest error / bound per kernel: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(_worst.items())))


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ------------------------------------------------------------ the runs
def run_vec(torch, dev, run, x, n_out, lead=2):
    """One single-vector run: x and a NaN-filled y are views `lead` elements
    into larger buffers, y between GUARD elements -> y (numpy).  The guards
    and x must keep their bits."""
    xb = np.full(x.size + 2 * lead, GUARD)
    xb[lead:lead + x.size] = x
    yb = np.full(n_out + 2 * lead, GUARD)
    yb[lead:lead + n_out] = np.nan
    xt, yt = torch.from_numpy(xb).to(dev), torch.from_numpy(yb).to(dev)
    run(xt[lead:lead + x.size], yt[lead:lead + n_out])
    torch.cuda.synchronize()
    yh = yt.cpu().numpy()
    assert np.array_equal(bits(yh[:lead]), bits(yb[:lead])) and np.array_equal(bits(yh[-lead:]), bits(yb[-lead:])), \
        "a guard element of y was written"
    assert np.array_equal(bits(xt.cpu().numpy()), bits(xb)), "x was written"
    return yh[lead:lead + n_out].copy()


def _view(torch, t, ptr, n, k, ld):
    """The (n, k) live part of a buffer placed by _place, as a strided view."""
    off = (ptr - t.data_ptr()) // 8
    return torch.as_strided(t, (n, k), (ld, 1), off)


def place8(torch, dev, host, n, k, layout, fill_seed):
    """_place with 8 rows of padding in front of the live part (and one more
    element in the padded layout) and 8 behind it: for the dropped family,
    where a bounds check that failed would address the row before the first
    or the rows behind the last, still inside the buffer."""
    ld = k if layout == "tight" else k + 3
    off = 8 * ld + (0 if layout == "tight" else 1)
    rows = n + 8
    buf = np.random.default_rng(fill_seed).uniform(-1.0, 1.0, off + rows * ld + 2)
    buf[off:off + rows * ld].reshape(rows, ld)[:n, :k] = host[:n, :k]
    mask = np.zeros(buf.shape, bool)
    mask[off:off + rows * ld].reshape(rows, ld)[:n, :k] = True
    buf[:2] = GUARD
    buf[-2:] = GUARD
    t = torch.from_numpy(buf).to(dev)
    return t, t.data_ptr() + 8 * off, ld, mask


def run_block(torch, dev, run, X, n_in, n_out, k, layout, seed, place=_place):
    """One multi-vector run on the first k columns of X in `layout` -> Y[n_out,
    k] (numpy).  Y's live part starts as NaN; its padding columns, the two rows
    behind it and its guards, and all of X's buffer, must keep their bits."""
    tx, px, ldx, _ = place(torch, dev, X, n_in, k, layout, seed)
    ty, py, ldy, mask = place(torch, dev, np.full((max(n_out, 1), k), np.nan), n_out, k, layout, seed + 1)
    x_before, y_before = tx.cpu().numpy(), ty.cpu().numpy()
    run(_view(torch, tx, px, n_in, k, ldx), _view(torch, ty, py, n_out, k, ldy))
    torch.cuda.synchronize()
    yh = ty.cpu().numpy()
    assert np.array_equal(bits(yh[~mask]), bits(y_before[~mask])), f"k={k} {layout}: Y written outside its live part"
    assert np.array_equal(bits(tx.cpu().numpy()), bits(x_before)), f"k={k} {layout}: X was written"
    return yh[mask].reshape(n_out, k)


def kernel_of(family, k, layout, j):
    """The kernel that computes column j of a k-vector call (launch_scatter_multi, launch_fused_multi)."""
    if family == "t" and k == 1 and layout == "tight":
        return "csr_t_window_kernel"  # k == 1 with ldx == ldy == 1 is the single-vector launch
    return f"csr_{'t' if family == 't' else 'sym'}_multi_kernel<{th.pass_widths(k)[j // 8][1]}>"


def check_products(torch, dev, family, dms, case, what, ks=th.RB_KS, layouts=LAYOUTS, single=True, label="", lead=2,
                   place=_place, name=None, before=None):
    """The single-vector run (single) and the multi-vector runs at every k and
    layout on the integer copy (dms[True]) and the wide-range copy (dms[False])
    of `case` (thresholds.transposed_case / symmetric_case); before(dm) is
    called in front of every run."""
    for integer, dm in dms.items():
        m = case["mi"] if integer else case["mr"]
        X = case["Xi"] if integer else case["X"]
        n_in, n_out = (m.n_rows, m.n_cols) if family == "t" else (m.n_rows, m.n_rows)
        one, many = (dm.run_t, dm.run_t_multi) if family == "t" else (dm.run_sym, dm.run_sym_multi)
        first = f"csr_{'t' if family == 't' else 'sym'}_window_kernel"
        runs = [(None, None)] * bool(single) + [(k, layout) for k in ks for layout in layouts]
        for k, layout in runs:
            tag = f"{what} {'integer' if integer else 'real'} " + ("single" if k is None else f"k={k} {layout}")

            def go():
                if before is not None:
                    before(dm)
                if k is None:
                    return run_vec(torch, dev, one, np.ascontiguousarray(X[:, 0]), n_out, lead)[:, None]
                return run_block(torch, dev, many, X, n_in, n_out, k, layout, 10 * k + len(layout), place)

            Y = go()
            kk = 1 if k is None else k
            if integer:
                exact.assert_exact(Y, case["ref_i"][:, :kk], tag)
                # integer sums are exact in any order: the atomics give the same bits
                assert np.array_equal(bits(Y), bits(go())), f"{tag}: two runs differ"
                continue
            for j in range(kk):
                s = th.RB_SCALES[j]
                r = exact.assert_fp64(Y[:, j], m, None, ref=s * case["ref"], bound=abs(s) * case["bound"],
                                      what=f"{tag} column {j}")
                note(name or (first if k is None else kernel_of(family, k, layout, j)) + label, r)


def plans_of(dev, case, kw):
    return {integer: sa.to_device(case["mi"] if integer else case["mr"], "csr", dev, **kw) for integer in (True, False)}


def assert_transpose_info(dm, expect):
    info, multi = dm.transpose_info, dm.transpose_multi_info
    assert (info["mode"], info["cap"], info["blocks"]) == ("scatter", th.T_CAP, expect["blocks"]), info
    assert (info["lds_blocks"], info["flush_entries"]) == (expect["lds_blocks"], expect["flush_entries"]), info
    assert multi["cap_cols"] == [th.T_MULTI_CAP // w for w in th.T_WIDTHS] and multi["kernel"] == "csr_t_multi_kernel"
    assert multi["lds_blocks"] == expect["multi_lds_blocks"], multi


def assert_symmetric_info(dm, expect):
    info, multi = dm.symmetric_info, dm.symmetric_multi_info
    assert (info["mode"], info["cap"], info["blocks"]) == ("fused", th.S_CAP, expect["blocks"]), info
    assert (info["window_blocks"], info["flush_entries"]) == (expect["window_blocks"], expect["flush_entries"]), info
    assert multi["cap_cols"] == [th.S_MULTI_CAP // w for w in th.T_WIDTHS] and multi["kernel"] == "csr_sym_multi_kernel"
    assert multi["window_blocks"] == expect["multi_window_blocks"], multi
    assert multi["flush_entries"] == expect["multi_flush_entries"], multi


def check_hot(dm, kw):
    if kw.get("hot"):
        assert dm.params["H"] == kw["hot"] and "hot-column table" in dm.params["plan"], dm.params


# ------------------------------------------------------ 1. the stream family
STREAMS = [(nr, lower) for nr in th.RB_LAST_ROWS for lower in (False, True)]
STREAM_IDS = [f"nr{nr}-{'lower' if lower else 'rect'}" for nr, lower in STREAMS]


@pytest.mark.parametrize("kw", PLANS, ids=PLAN_IDS)
@pytest.mark.parametrize("last_nr,lower", STREAMS, ids=STREAM_IDS)
def test_stream_family_transposed(torch_dev, last_nr, lower, kw):
    """Y = A^T X in scatter mode: blocks of every entry count of
    RB_ENTRY_COUNTS (the per-thread loops of csr_t_window_kernel, the uniform
    loops of csr_t_multi_kernel<KV>, the end of the stream inside a quad for KV
    >= 4), every layout of the rows, a last block of 1, 2 or 127 rows.  A step
    or a row taken wrongly moves, drops or repeats an entry: the integer sums
    change.  Copy mode once per matrix, as a cross-check of the references."""
    torch, dev = torch_dev
    info, case, _ = th.stream_case(last_nr, lower)
    assert {E for _, E, _ in info["under"]} == set(th.RB_ENTRY_COUNTS) and info["last_nr"] == last_nr
    expect = th.expected_transpose_info(th.t_windows(case["mi"].n_rows, case["mi"].n_cols, *th.csr_of(case["mi"])[:2]))
    assert expect["lds_blocks"] == expect["blocks"] - len(info["empty"]) == expect["multi_lds_blocks"][3]  # all narrow
    dms = plans_of(dev, case, kw)
    for dm in dms.values():
        check_hot(dm, kw)
        dm.prepare_transpose("scatter")
        assert_transpose_info(dm, expect)
    check_products(torch, dev, "t", dms, case, f"stream nr={last_nr} {'lower' if lower else 'rect'} {kw} scatter")
    if not kw:
        for dm in dms.values():
            dm.prepare_transpose("copy")
        check_products(torch, dev, "t", dms, case, f"stream nr={last_nr} copy", ks=(9,), layouts=("tight",),
                       name="copy mode (inner forward plan)")


@pytest.mark.parametrize("kw", PLANS, ids=PLAN_IDS)
@pytest.mark.parametrize("last_nr", th.RB_LAST_ROWS)
def test_stream_family_symmetric(torch_dev, last_nr, kw):
    """Y = (S + S^T - diag S) X in fused mode on the lower-triangular twin:
    the uniform stream of all five kernels, wave_run_add over rows that end on
    lanes 62, 63 and 0 of a wave and over a row across whole steps, rb_row_of
    in last blocks of 1, 2 and 127 rows (searched for the lanes past the end
    too).  Expand mode once per matrix."""
    torch, dev = torch_dev
    info, _, case = th.stream_case(last_nr, True)
    m = case["mi"]
    expect = th.expected_symmetric_info(m.n_rows, th.sym_windows(m.n_rows, *th.csr_of(m)[:2]))
    assert expect["window_blocks"] == expect["blocks"] - len(info["empty"]) == expect["multi_window_blocks"][3]
    dms = plans_of(dev, case, kw)
    for dm in dms.values():
        check_hot(dm, kw)
        dm.prepare_symmetric("fused")
        assert_symmetric_info(dm, expect)
    check_products(torch, dev, "s", dms, case, f"stream nr={last_nr} {kw} fused")
    if not kw:
        for dm in dms.values():
            dm.prepare_symmetric("expand")
        check_products(torch, dev, "s", dms, case, f"stream nr={last_nr} expand", ks=(9,), layouts=("tight",),
                       name="expand mode (inner forward plan)")


# --------------------------------------------------------- 2. the cap family
@pytest.mark.parametrize("kw", PLANS, ids=PLAN_IDS)
def test_cap_family_transposed(torch_dev, kw):
    """Column spans of 1,024 .. 8,193: for every width both sides of its cap,
    every word of the accumulator hit, so a zero fill or a flush that stops
    short, skips or repeats a stretch, or an LDS allocation one block short,
    changes a sum; csr_t_multi_kernel<1> at span 8,192 launches with 67,600
    bytes of dynamic LDS.  The plan must report the blocks and flush entries
    the constructor promised, before every run."""
    torch, dev = torch_dev
    info, case = th.cap_case()
    dms = plans_of(dev, case, kw)
    for dm in dms.values():
        check_hot(dm, kw)
        dm.prepare_transpose("scatter")
    # before every run: the plan reports what the constructor promised, so no run passes on another path
    check_products(torch, dev, "t", dms, case, f"cap {kw} scatter",
                   before=lambda dm: assert_transpose_info(dm, info["expect"]))
    if not kw:
        for dm in dms.values():
            dm.prepare_transpose("copy")
        check_products(torch, dev, "t", dms, case, "cap copy", ks=(9,), layouts=("tight",),
                       name="copy mode (inner forward plan)")


@pytest.mark.parametrize("kw", PLANS, ids=PLAN_IDS)
def test_cap_family_symmetric(torch_dev, kw):
    """Union windows of 512 .. 4,097 columns in a lower form (the window ends
    on the block's last row) and an upper form (it starts at r0), diagonal-only
    blocks between them and a last block whose span equals its 77 rows: for
    every width both sides of its cap; the k = 1 call runs csr_sym_multi_kernel<1>
    on its own cap of 4,096 columns, with 66,576 bytes of dynamic LDS."""
    torch, dev = torch_dev
    info, case = th.sym_cap_case()
    dms = plans_of(dev, case, kw)
    for dm in dms.values():
        check_hot(dm, kw)
        dm.prepare_symmetric("fused")
    check_products(torch, dev, "s", dms, case, f"cap {kw} fused",
                   before=lambda dm: assert_symmetric_info(dm, info["expect"]))
    if not kw:
        for dm in dms.values():
            dm.prepare_symmetric("expand")
        check_products(torch, dev, "s", dms, case, "cap expand", ks=(9,), layouts=("tight",),
                       name="expand mode (inner forward plan)")


# ----------------------------------------------------- 3. the dropped family
def csr_plan(torch, dev, n, arrays):
    """A CSR plan over hand-uploaded arrays (the host builder refuses a column
    outside [0, n)): no hot table, whose builder refuses such a column too, and
    no x windows; the forward run is never called."""
    ptr, col, val = arrays
    dm = sa.DeviceMatrix("csr", n, n, int(col.size), dev)
    dm.arrays = dict(row_ptr=torch.from_numpy(np.array(ptr)).to(dev), col=torch.from_numpy(np.array(col)).to(dev),
                     val=torch.from_numpy(np.array(val)).to(dev))
    sa._plan_csr(dm, hot=0, xwin=False, variant=1)
    assert dm.params["H"] == 0
    return dm


@pytest.mark.parametrize("family", ["t", "s"], ids=["transposed", "symmetric"])
def test_dropped_columns(torch_dev, family):
    """Entries in columns -1, n and n + 1 (the middle, the first and the last
    entry of a row, in window blocks and in blocks wider than every cap, and a
    block of nothing else): the scatter and the fused runs give the sums of
    the matrix without them and write no guard element; copy and expand mode
    refuse the matrix with SPMV_OTHER_ERROR and leave the plan as it was.
    Before its fix sym_block gave the probe row 29 products instead of 19
    (tests/test_thresholds.py has the model); csr_t_range_kernel recorded
    ranges [-1, n + 1], whose flush wrote y[-1], y[n] and y[n + 1]."""
    torch, dev = torch_dev
    info, csr, t, s = th.dropped_case()
    case = t if family == "t" else s
    n = case["mi"].n_rows
    dms = {integer: csr_plan(torch, dev, n, csr[family, integer]) for integer in (True, False)}
    for dm in dms.values():
        assert dm.nnz == case["mi"].nnz + info["dropped"]
        if family == "t":
            dm.prepare_transpose("scatter")
            valid = th.csr_of(case["mi"])
            assert_transpose_info(dm, th.expected_transpose_info(th.t_windows(n, n, valid[0], valid[1])))
        else:
            dm.prepare_symmetric("fused")
            assert_symmetric_info(dm, th.expected_symmetric_info(n, info["windows"]))
    # x and y 8 elements into their buffers: a bounds check that failed would still read and write inside them
    check_products(torch, dev, family, dms, case, f"dropped {family}", label=" (dropped columns)", lead=8, place=place8)
    for dm in dms.values():
        with pytest.raises(sa.SpmvError) as err:
            dm.prepare_transpose("copy") if family == "t" else dm.prepare_symmetric("expand")
        assert err.value.rc == sa.OTHER_ERROR and "out of range" in str(err.value)
    if family == "s":  # a refused prepare leaves the plan as it was: fused mode still runs
        assert dms[True].symmetric_info["mode"] == "fused"
        y = run_vec(torch, dev, dms[True].run_sym, np.ascontiguousarray(case["Xi"][:, 0]), n, lead=8)
        exact.assert_exact(y, case["ref_i"][:, 0], "dropped s after the refused expand")


# ------------------------------------------------------------ 4. the builders
def _guarded_offsets(torch, dev, n):
    """n + 1 offsets with 8 guard entries behind them."""
    buf = np.full(n + 1 + 8, -1, np.int64)
    buf[n + 1:] = 0x7ABCDEF012345678
    return torch.from_numpy(buf).to(dev), buf


def test_builders_refuse_an_index_past_n_inside_their_offsets(torch_dev):
    """spmv_dev_csr_from_coo with a row index of n + 1 and
    spmv_dev_csr_transpose with a column of n_cols + 2: SPMV_OTHER_ERROR, and
    the 8 entries behind the n + 1 offsets keep their bits.  Before the fix the
    bad index stayed the sort key and row_ptr_from_sorted_kernel wrote the
    offsets up to it, into those entries."""
    torch, dev = torch_dev
    lib = sa.hip_lib()
    m = sa.gen_random(100, 90, 1, 5, seed=3)
    n, nc = m.n_rows, m.n_cols
    row = m.row.copy()
    row[m.nnz // 2] = n + 1
    ptr, col, val = sa.csr_from_coo(m)
    bad_col = col.copy()
    bad_col[m.nnz // 3] = nc + 2
    out_col = torch.empty(m.nnz, dtype=torch.int32, device=dev)
    out_val = torch.empty(m.nnz, dtype=torch.float64, device=dev)
    dims = sa.DeviceMatrix("csr", n, nc, m.nnz, dev).dims()
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in
         dict(row=row, col=m.col, val=m.val, ptr=ptr, bad_col=bad_col, cval=val, good_row=m.row, good_col=col).items()}

    offs, before = _guarded_offsets(torch, dev, n)
    rc = lib.spmv_dev_csr_from_coo(dims, sa._ptr(d["row"]), sa._ptr(d["col"]), sa._ptr(d["val"]), sa._ptr(offs),
                                   sa._ptr(out_col), sa._ptr(out_val))
    torch.cuda.synchronize()
    assert rc == sa.OTHER_ERROR and b"row index out of range" in lib.spmv_last_error()
    assert np.array_equal(offs.cpu().numpy()[n + 1:], before[n + 1:]), "spmv_dev_csr_from_coo wrote past row_ptr[n]"

    offs, before = _guarded_offsets(torch, dev, nc)
    rc = lib.spmv_dev_csr_transpose(dims, sa._ptr(d["ptr"]), sa._ptr(d["bad_col"]), sa._ptr(d["cval"]), sa._ptr(offs),
                                    sa._ptr(out_col), sa._ptr(out_val))
    torch.cuda.synchronize()
    assert rc == sa.OTHER_ERROR and b"column index out of range" in lib.spmv_last_error()
    assert np.array_equal(offs.cpu().numpy()[nc + 1:], before[nc + 1:]), "spmv_dev_csr_transpose wrote past t_ptr[n_cols]"

    # valid input into the same guarded buffers: the host builders' arrays, the guards untouched
    offs, before = _guarded_offsets(torch, dev, n)
    assert lib.spmv_dev_csr_from_coo(dims, sa._ptr(d["good_row"]), sa._ptr(d["col"]), sa._ptr(d["val"]), sa._ptr(offs),
                                     sa._ptr(out_col), sa._ptr(out_val)) == sa.SUCCESS
    torch.cuda.synchronize()
    h = offs.cpu().numpy()
    assert np.array_equal(h[: n + 1], ptr) and np.array_equal(h[n + 1:], before[n + 1:])
    assert np.array_equal(out_col.cpu().numpy(), col) and np.array_equal(bits(out_val.cpu().numpy()), bits(val))
    offs, before = _guarded_offsets(torch, dev, nc)
    assert lib.spmv_dev_csr_transpose(dims, sa._ptr(d["ptr"]), sa._ptr(d["good_col"]), sa._ptr(d["cval"]), sa._ptr(offs),
                                      sa._ptr(out_col), sa._ptr(out_val)) == sa.SUCCESS
    torch.cuda.synchronize()
    t_ptr, t_col, t_val = sa.csr_transpose(n, nc, ptr, col, val)
    h = offs.cpu().numpy()
    assert np.array_equal(h[: nc + 1], t_ptr) and np.array_equal(h[nc + 1:], before[nc + 1:])
    assert np.array_equal(out_col.cpu().numpy(), t_col) and np.array_equal(bits(out_val.cpu().numpy()), bits(t_val))
