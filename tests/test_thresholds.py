"""The constructors of tests/thresholds.py deliver the chunk runs and owned-row
counts they promise, the host's spmv_csr_tiled_bigplan draws its two lines
(1024 and 65,536 owned rows) where csr_tiled_kernel draws them, and the
matrices fit tests/exact.py's integer check.  No GPU.

Also the record of why the SELL cases are the sharp ones: the host
restatement of sell_split_fix_kernel's run-end search finds every run's end,
and its earlier form (lo kept after a coarse pass without a match) reported
c + 65,537 for exactly the run lengths [65,474, 65,536] and, one pass
further, c + 131,073 for [131,010, 131,072].
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import exact
import spmv_amd as sa
import thresholds as th


# --------------------------------------------------------------- SELL runs
@pytest.mark.parametrize("R,C,T,last,ki", [(65_500, 32, 1, False, 1), (65_537, 32, 1, True, 1), (65_500, 64, 1, False, 1),
                                           (65_500, 32, 2, False, 2), (131_073, 32, 1, False, 1)])
def test_sell_run_matrix_delivers_its_runs(R, C, T, last, ki):
    m, runs = th.sell_run_matrix(R, C, T, 99, last, ki)
    W = 1024 // C
    small = [1, 2, W - 1, W, W + 1, 65]
    assert runs[:6] == small and sum(runs) == sum(small) + R + 99
    assert (runs[-1] == R) if last else (runs[6] == R and sum(runs[7:]) == 99 and len(runs) > 7)
    lens = np.bincount(m.row, minlength=m.n_rows)
    assert lens.max() == T * (R + 1) and (lens == 0).any() and m.n_rows % C == 5
    long_row = int(np.argmax(lens))
    cols = m.col[m.row == long_row]
    assert np.unique(cols).size == cols.size  # distinct columns
    assert th.sell_run_matrix(R, C, T, 99, last, ki)[0] is m  # made once


def _chunk_slice(runs):
    return np.repeat(np.arange(len(runs), dtype=np.int32), runs)


@pytest.mark.parametrize("R", th.SELL_RS)
@pytest.mark.parametrize("last", [False, True])
def test_fix_pass_search_restated(R, last):
    """The corrected search finds the end of every run; the earlier one was
    wrong exactly in the two windows, by 1 to 63 chunks too late: chunks of
    the next slices, or past the partial sums when the run is the last."""
    small = list(th.small_runs(32))
    runs = small + ([40, 40, 19, R] if last else [R, 40, 40, 19])
    cs = _chunk_slice(runs)
    starts = np.concatenate(([0], np.cumsum(runs)[:-1]))
    for c, r in zip(starts, runs):
        assert th.fix_pass_end(int(c), cs) == c + r, (c, r)
    c = int(starts[runs.index(R)])
    broken = 65_474 <= R <= 65_536 or 131_010 <= R <= 131_072
    old = th.fix_pass_end(c, cs, fixed=False)
    assert (old != c + R) == broken
    if broken:
        assert old == c + (R + 62) // th.FIX_PASS * th.FIX_PASS + 1 and 1 <= old - (c + R) <= 63


def test_fix_pass_search_every_length_near_the_windows():
    for R in list(range(65_400, 65_620)) + list(range(130_990, 131_140)) + [1, 63, 64, 65, 66, 1024, 65_409]:
        cs = _chunk_slice([3, R, 99])
        assert th.fix_pass_end(3, cs) == 3 + R, R
        assert th.fix_pass_end(0, cs) == 3 and th.fix_pass_end(3 + R, cs) == 3 + R + 99
        assert th.fix_pass_end(0, _chunk_slice([R])) == R, R  # the last run: no probe matches past n_chunks


@pytest.mark.parametrize("R,C,T,last,ki,c_bits", [(65_500, 32, 1, False, 1, 16), (65_536, 32, 1, False, 1, 17),
                                                  (65_500, 32, 2, False, 2, 17), (131_073, 32, 1, False, 1, 18)])
def test_sell_cases_fit_the_integer_check(R, C, T, last, ki, c_bits):
    """exact.integerize accepts the long row: c = ceil(log2(T (R + 1) + 1)) bits
    for the sums (17 for the lengths from 65,535 on) leave a = (52 - c) // 2 and
    b = 52 - c - a for the values and x."""
    runs, e, (mr, x, ref, bound) = th.sell_case(R, C, T, last, ki)
    assert c_bits == math.ceil(math.log2(T * (R + 1) + 1))
    assert (e.a, e.b) == ((52 - c_bits) // 2, 52 - c_bits - (52 - c_bits) // 2)
    if c_bits == 17:
        assert (e.a, e.b) == (17, 18)
    assert e.ref.shape == (e.m.n_rows,) and ref.shape == bound.shape == (mr.n_rows,)
    assert th.sell_case(R, C, T, last, ki)[1] is e  # computed once
    # the host's SELL loop agrees with both references
    ptr, col, val = sa.csr_from_coo(e.m)
    s = sa.sell_build(e.m.n_rows, ptr, col, val, C=C, sigma=C, ki=ki)
    y = np.full(e.m.n_rows, np.nan)
    rc = sa.host_lib().spmv_cpu_sell(e.m.n_rows, C, ki, s["n_slices"], sa._ptr(s["slice_ptr"]), sa._ptr(s["perm"]),
                                     sa._ptr(s["col"]), sa._ptr(s["val"]), sa._ptr(np.ascontiguousarray(e.x)), sa._ptr(y), 0)
    assert rc == 0
    exact.assert_exact(y, e.ref, "spmv_cpu_sell")


def test_sell_cases_get_no_hot_column_table_by_rule():
    """The library's hot-column rule (hot=None) leaves these matrices without
    a table, padding included: the GPU cases without a `hot` keyword take the
    plain split run (spmv_sell_run_split), the one with hot=64 the other."""
    _, e, _ = th.sell_case(65_500, 32, 1, False, 1)
    ptr, col, val = sa.csr_from_coo(e.m)
    s = sa.sell_build(e.m.n_rows, ptr, col, val, C=32, sigma=32, ki=1)
    assert sa.hot_columns(e.m.n_cols, s["col"][: s["stored"]], 0)[0] == 0
    assert sa.hot_columns(e.m.n_cols, s["col"][: s["stored"]], 64)[0] == 64


# ------------------------------------------------------------- tiled CSR
@pytest.mark.parametrize("order", sorted(th.TILE_ORDERS))
def test_tile_rows_matrix_delivers_its_owned_rows(order):
    owned, under_test, e, _ = th.tiles_case(order)
    m = e.m
    assert [int(owned[t]) for t in under_test] == [1024, 1025, 65536, 65537]
    rest = np.delete(owned, under_test)
    assert set(rest.tolist()) == {0, 1}  # the separators: one 512-entry row, or none inside a longer row
    assert owned.sum() == m.n_rows
    assert (under_test[-1] == owned.size - 1) == (order == "final")
    assert (m.nnz % th.TILE == 0) == (order == "final")
    # the definition once more, by a plain loop over the rows' first offsets
    ptr = np.concatenate(([0], np.cumsum(np.bincount(m.row, minlength=m.n_rows))))
    first = np.minimum(ptr[:-1] // th.TILE, owned.size - 1)  # rows behind the last entry: the last tile's
    assert np.array_equal(np.bincount(first, minlength=owned.size), owned)
    assert exact.integerize(m, seed=1).a == 20  # the longest row: 1536 entries, c = 11


@pytest.mark.parametrize("order", sorted(th.TILE_ORDERS))
def test_bigplan_draws_both_lines(order):
    """cap 1024: the tiles owning 1024 rows (offsets staged in LDS) and 65,537
    rows (row_ptr from global memory) get no list, those owning 1025 and 65,536
    list exactly their rows with entries, with the right [a, b) halves."""
    owned, under_test, e, _ = th.tiles_case(order)
    m = e.m
    ptr = np.ascontiguousarray(sa.csr_from_coo(m)[0], dtype=np.int64)
    L = sa.host_lib()
    n = L.spmv_csr_tiled_bigplan(m.n_rows, sa._ptr(ptr), th.TILE, 1024, None)
    tiles = owned.size
    assert n > tiles
    plan = np.full(n, -12345, np.int32)
    assert L.spmv_csr_tiled_bigplan(m.n_rows, sa._ptr(ptr), th.TILE, 1024, sa._ptr(plan)) == n
    index = plan[:tiles]
    listed = (owned > 1024) & (owned <= 65536)
    assert np.array_equal(index >= 0, listed) and (index[~listed] == -1).all()
    assert [bool(listed[t]) for t in under_test] == [False, True, True, False]
    assert sorted(index[listed].tolist()) == list(range(int(listed.sum())))
    own_lo = np.searchsorted(ptr[:m.n_rows], np.arange(tiles, dtype=np.int64) * th.TILE, side="left")
    for t in np.flatnonzero(listed):
        kb = int(index[t])
        beg, end = int(plan[tiles + kb]), int(plan[tiles + kb + 1])
        assert beg % 2 == 0 and end > beg  # int2 items, 8-byte aligned
        items = plan[beg:end].reshape(-1, 2)
        rel = items[:, 0].astype(np.int64)
        a = items[:, 1].astype(np.int64) & 0xFFFF
        b = (items[:, 1].astype(np.int64) >> 16) & 0xFFFF
        t0, t1 = t * th.TILE, min((t + 1) * th.TILE, m.nnz)
        rows = own_lo[t] + np.arange(owned[t])
        ra = ptr[rows] - t0
        rb = np.minimum(ptr[rows + 1], t1) - t0
        keep = ra < rb  # the owned rows with entries
        assert np.array_equal(rel, np.flatnonzero(keep))
        assert np.array_equal(a, ra[keep]) and np.array_equal(b, rb[keep])
        assert rel.tolist() == [0, owned[t] - 1] and a.tolist() == [0, 1] and b.tolist() == [1, th.TILE]
    # with the cap above every tile no tile is listed
    assert L.spmv_csr_tiled_bigplan(m.n_rows, sa._ptr(ptr), th.TILE, 65536, None) == tiles + 1 + (tiles + 1) % 2


def test_references_are_shared():
    a = th.tiles_case("followed")
    assert th.tiles_case("followed")[2] is a[2] and not a[2].ref.flags.writeable
