"""The constructors of tests/thresholds.py deliver the chunk runs and owned-row
counts they promise, the host's spmv_csr_tiled_bigplan draws its two lines
(1024 and 65,536 owned rows) where csr_tiled_kernel draws them, and the
matrices fit tests/exact.py's integer check.  No GPU.

Also the record of why the SELL cases are the sharp ones: the host
restatement of sell_split_fix_kernel's run-end search finds every run's end,
and its earlier form (lo kept after a coarse pass without a match) reported
c + 65,537 for exactly the run lengths [65,474, 65,536] and, one pass
further, c + 131,073 for [131,010, 131,072].

The staged family (coo_staged_kernel, coo_carry_kernel, coo_tail_kernel,
cmrs_tiled_kernel and the two window kernels): every constant and launch rule
that tests/thresholds.py restates is held against the defining line of the
sources (test_restated_constants_match_the_sources: the plan reports none of
them, so a stale restatement would otherwise fail no test); the constructors
deliver the tile spans, tails, carry runs, placements and x windows they
promise; a numpy model of coo_carry_kernel gives the int64 reference on the
carry arrays of carry_run_matrix, plain and k-major, and four one-line
mutations of it do not; a word count of coo_staged_kernel's three row paths
stays inside s_start[RC + 1] at every span under test and leaves it when the
bitmap path's upper line moves one row up.

The row-block core (rowblock.h, transpose.hip, symmetric.hip), at the end of
the file: its constants, window rules, width rule and LDS sizes are held
against the sources in the same test; the stream, cap and dropped families
deliver their entry counts, layouts, spans and placements; a numpy model of
rb_row_of equals np.searchsorted on every block and four one-line mutations of
it do not; a numpy model of wave_run_add gives every row its sum on the valid
families under both key rules, and on the dropped family only with the rule
that keeps a dropped entry in its row's run: the earlier rule (key -1) gives
the probe row 29 products instead of 19.
"""
from __future__ import annotations

import math
from pathlib import Path

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


# ------------------------------------ the staged family: restated constants
def test_restated_constants_match_the_sources():
    """Every constant and rule thresholds.py restates, on its defining line of
    csrc/: the plan reports no COO lanes, tile or row cap, so nothing else
    would notice a restatement gone stale."""
    src = Path(sa.__file__).resolve().parent / "csrc"
    text = {f: (src / f).read_text() for f in ("staged.hip", "coo.hip", "common.h", "sell.hip", "rowblock.h",
                                                 "transpose.hip", "symmetric.hip")}
    width_rule = "const int w = live > 4 ? 3 : live > 2 ? 2 : live - 1;"
    lines = {
        "rowblock.h": [
            f"constexpr int kRbRows = {th.RB_ROWS};", "constexpr int kRbPtr = kRbRows + 2;",
            f"constexpr int kRbU = {th.RB_U};", "constexpr int kTWidths[4] = {" + ", ".join(map(str, th.T_WIDTHS)) + "};",
            # rb_row_of: seven guarded steps; rb_stream: the two loop forms and their tails
            "for (int step = kRbRows / 2; step > 0; step >>= 1)", "if (r + step < nr && s_ptr[r + step] <= e)",
            "for (; e0 + kRbU * kBlock <= end; e0 += kRbU * kBlock) {", "for (; e0 < end; e0 += kBlock) {",
            "for (; e + (kRbU - 1) * kBlock < end; e += kRbU * kBlock) {", "for (; e < end; e += kBlock)",
            "for (int i = (int)threadIdx.x; i <= b->nr; i += kBlock)",
        ],
        "transpose.hip": [
            f"constexpr int32_t kTCap = {th.T_CAP};", f"#define SPMV_T_MULTI_CAP {th.T_MULTI_CAP}", width_rule,
            "return (size_t)(kRbPtr + kRbRows * kv + span * kv) * sizeof(double);",
            "if (c >= 0 && c < n_cols) {",  # csr_t_range_kernel: the range of the columns inside [0, n_cols)
            "const bool lds = b.span <= cap;", "const bool lds = span <= cap;",
            "const WindowTally multi = windows_tally(h, blocks, kTMultiCap / kTWidths[w]);",
        ],
        "symmetric.hip": [
            f"constexpr int32_t kSCap = {th.S_CAP};", f"#define SPMV_S_MULTI_CAP {th.S_MULTI_CAP}", width_rule,
            "return (size_t)(kRbPtr + 2 * (span > kRbRows ? span : kRbRows) * kv) * sizeof(double);",
            # csr_sym_range_kernel: the columns inside [0, n), joined with the block's rows
            "if (c >= 0 && c < n) {", "r.x = r0 < r.x ? (int)r0 : r.x;", "r.y = r1 - 1 > r.y ? (int)(r1 - 1) : r.y;",
            "const int32_t cap = kSMultiCap / kTWidths[w];", "const bool window = span <= cap;",
            # wave_run_add: the scan and the run's last lane
            "for (int off = 1; off < kWave; off <<= 1) {", "if (lane >= off && k == key)",
            "if (key >= 0 && (lane == kWave - 1 || next != key))",
        ],
        "common.h": [f"constexpr int kWave = {th.K_WAVE};", f"constexpr int kBlock = {th.K_BLOCK};",
                     f"constexpr int32_t kStagedXwinCap = {th.XWIN_CAP};"],
        "sell.hip": [f"constexpr int kSellFixThreads = {th.FIX_THREADS};", f"int64_t lo = c + 1, step = {th.FIX_STEP};"],
        "coo.hip": [f"int32_t rr[{th.CARRY_SHORT}];", f"const bool lng = head && rr[{th.CARRY_SHORT - 1}] == r;",
                    f"for (int k = 0; k < {th.CARRY_SHORT} && rr[k] == r; ++k)",
                    f"base += {th.CARRY_ROUND // th.K_WAVE} * kWave", "const bool head = t < n_tiles && r >= 0 && prev != r;",
                    "q[u] = i < n_tiles ? carry_row[i] : -2;"],
        "staged.hip": [
            f"constexpr int kCooRowCap = {th.COO_ROW_CAP};", f"constexpr int kCooRowCapShort = {th.COO_ROW_CAP_SHORT};",
            f"constexpr int kCooTailCap = {th.COO_TAIL_CAP};", f"constexpr int kCooR = {th.COO_R};",
            f"constexpr int kTiledRowCap = {th.ROW_CAP};", f"constexpr int kTiledBigRowCap = {th.BIG_ROW_CAP};",
            f"constexpr int kTiledR = {th.TILE // (2 * th.K_BLOCK)};",
            "int64_t csr_tiled_tile(int64_t, int64_t) { return 2 * kBlock * kTiledR; }",
            "int64_t coo_staged_tile() { return 2 * kBlock * kCooR; }",
            # coo_lanes, coo_hot_r, cmrs_tiled_r
            f"return mean >= {th.MEAN_LANES_8} ? 8 : mean >= {th.MEAN_LANES_4} ? 4 : 2;",
            f"return n_rows > 0 && (double)nnz < {th.MEAN_BIG_TILE} * (double)n_rows ? 1 : kCooR;",
            f"return n_rows > 0 && (double)nnz >= {th.MEAN_BIG_TILE} * (double)n_rows ? 3 : 1;",
            # which RC a launch takes: the default, or by lane count
            "int RC = kCooRowCap>",
            "constexpr int RC = LL == 2 ? kCooRowCap : kCooRowCapShort;",
            "go(coo_staged_kernel<LL, R, false, false, true, XGlobal, true, RC>);",
            "go(coo_staged_kernel<LL, RR, false, true>);",
            "go(coo_staged_kernel<LL, RR, false, false, true, XGlobal, false, RC>);",
            "(coo_staged_kernel<decltype(Lc)::value, decltype(Rc)::value, false, false, true, XHot>)",
            "(coo_staged_kernel<4, R, true, false, false, XGlobal, true>)", "(coo_staged_kernel<4, R, true, false>)",
            "(coo_staged_kernel<4, R, true, false, true, XHot>)",
            "const int64_t tile = tails ? coo_staged_tile() : coo_hot_tile(d.n_rows, d.nnz);",
            # the three row paths and their storage
            "__shared__ int32_t s_start[RC + 1];", "heads = span >= 0 && span <= RC;",
            "constexpr int FW = (2 * kBlock * R + 63) / 64 * 2;",
            "if (!heads && span > RC && span <= 32 * (int64_t)(RC + 1 - FW)) {",
            "constexpr int TP = TAIL ? (kCooTailCap + 1) / 2 : 0;",
            "while (k <= kCooTailCap && t1 + k < nnz && row[t1 + k] == last)",
            # the k-major carries, the strip-run geometry and its windows
            "carry_row[(int64_t)g * tiles + tile] = cr;", "int l = spmv_csr_auto_lanes(d.n_rows, d.nnz);",
            "while (l > 1 && l * h > kBlock)", "*G = kBlock / (l * h) > 0 ? kBlock / (l * h) : 1;",
            "const int64_t c0 = b & ~(int64_t)31;",
            "r = block_col_range(col, c0 >= 2 ? c0 - 2 : 0, e + 1 < nz ? e + 1 : nz);",
            "staged = span > 0 && span <= xcap;", "staged = span > 0 && span <= xcap && span <= 8 * kBlock;",
        ],
    }
    for f, want in lines.items():
        for line in want:
            assert text[f].count(line) >= 1, f"update tests/thresholds.py with the kernel: {f} no longer has `{line}`"
    assert th.BIG_TILE == 2 * th.K_BLOCK * th.COO_R and th.TILE == 2 * th.K_BLOCK and th.FIX_PASS == 65_536
    assert 8 * th.K_BLOCK == th.XWIN_CAP  # cmrs_staged_kernel's one-pass window copy holds a window at the cap
    # the derived edges, as the kernels' comments name them
    assert th.first_words(th.TILE) == 16 and th.first_words(th.BIG_TILE) == 48
    assert [th.span_edges(rc, t) for rc in (250, 1024) for t in (th.TILE, th.BIG_TILE)] == [
        (250, 251, 7520, 7521), (250, 251, 6496, 6497), (1024, 1025, 32288, 32289), (1024, 1025, 31264, 31265)]
    assert [th.coo_row_cap(la, L) for la in ("carry", "single") for L in (2, 4, 8)] == [1024, 250, 250] * 2
    assert [th.coo_row_cap(la, 4) for la in ("xwin", "hot", "acc")] == [1024] * 3
    assert [th.coo_lanes(1000, n) for n in (11_999, 12_000, 47_999, 48_000)] == [2, 4, 4, 8]
    assert [th.carry_tile(1000, n) for n in (95_999, 96_000)] == [512, 1536]
    # the row-block core
    assert th.RB_STEP == 1024 and th.RB_PTR == 130 and 1 << th.RB_SEARCH_STEPS == th.RB_ROWS
    assert [th.pass_widths(k) for k in (1, 2, 3, 4, 5, 8, 9)] == [
        [(1, 1)], [(2, 2)], [(3, 4)], [(4, 4)], [(5, 8)], [(8, 8)], [(8, 8), (1, 1)]]
    assert th.pass_widths(17) == [(8, 8), (8, 8), (1, 1)]
    assert th.t_multi_lds(1, 8192) == 67_600 and th.sym_multi_lds(1, 4096) == 66_576  # both above 64 KiB
    assert th.sym_multi_lds(8, 3) == th.sym_multi_lds(8, 128) == (130 + 2 * 128 * 8) * 8  # the wide path's arrays


# ---------------------------------------------------- COO tiles by their span
@pytest.mark.parametrize("name", sorted(th.SPAN_CASES))
def test_coo_span_matrix_delivers_its_spans(name):
    launch, lanes, tile, final = th.SPAN_CASES[name]
    info, e, (mr, x, ref, bound) = th.coo_span_case(name)
    m, rc = e.m, info["rc"]
    lo, lo1, hi, hi1 = info["edges"]
    assert (lo, lo1, hi, hi1) == (rc, rc + 1, 32 * (rc + 1 - th.first_words(tile)), 32 * (rc + 1 - th.first_words(tile)) + 1)
    assert sorted(info["spans"]) == [lo, lo1, lo1, hi, hi1]
    assert [th.staged_row_path(s, rc, tile) for s in (lo, lo1, hi, hi1)] == ["heads", "bitmap", "bitmap", "search"]
    row = np.sort(m.row)
    spans = th.coo_tile_spans(row, tile)
    assert [int(spans[t]) for t in info["under"]] == list(info["spans"])
    for t, s in zip(info["under"], info["spans"]):  # the definition once more, from the entries
        t1 = min((t + 1) * tile, m.nnz)
        assert row[t1 - 1] - row[t * tile - 1] == s and np.unique(row[t * tile:t1]).size <= 3
    assert th.coo_lanes(m.n_rows, m.nnz) == lanes and info["lanes"] == lanes
    if launch == "single":
        plan = th.coo_tail_plan(row)
        assert plan.max() == th.COO_TAIL_CAP and sorted(plan[list(info["under"])])[-2:] == [79, 80]
    else:
        assert th.carry_tile(m.n_rows, m.nnz) == tile
        assert len(th.carry_runs(row, tile)) >= (4 if final else 5)
    lens = np.bincount(m.row, minlength=m.n_rows)
    assert (lens[-37:] == 0).all() and lens[-38] > 0 and (lens == 0).sum() == sum(s - 2 for s in info["spans"]) + 37
    assert (info["under"][-1] == info["tiles"] - 1) == final and (m.nnz % tile == 0) == final
    assert m.nnz <= 2_000_000 and e.a >= 20
    assert th.coo_span_case(name)[1] is e  # made once


def test_span_cases_get_no_hot_column_table_by_rule():
    """hot=None leaves these matrices without a table (as the SELL cases): the
    cases without a `hot` keyword take the launches SPAN_CASES names."""
    for name in ("carry-L4", "wide-L4", "single-L8"):
        m = th.coo_span_case(name)[1].m
        assert sa.hot_columns(m.n_cols, m.col, 0)[0] == 0
    m = th.coo_span_case("wide-L4")[1].m
    assert sa.hot_columns(m.n_cols, m.col, 64)[0] == 64
    for m in (th.carry_case(th.TILE)[1].m, th.hyb_tail_case()[1].m, th.coo_tail_case(False)[1].m):
        assert sa.hot_columns(m.n_cols, m.col, 0)[0] == 0


def test_staged_row_paths_stay_inside_s_start():
    """The words of s_start[RC + 1] the three row paths touch, for a full tile
    at every span under test: within RC + 1, exactly RC + 1 at the bitmap
    path's upper edge, and RC + 2 there if that line lay one row higher."""
    for name, (launch, lanes, tile, final) in th.SPAN_CASES.items():
        rc = th.coo_row_cap(launch, lanes)
        lo, lo1, hi, hi1 = th.span_edges(rc, tile)
        words = [th.staged_lds_words(s, tile, rc, tile) for s in (lo, lo1, hi, hi1)]
        assert words == [rc + 1, (lo1 + 31) // 32 + th.first_words(tile), rc + 1, 0], (name, words)
        assert max(words) <= rc + 1
        assert th.staged_lds_words(hi1, tile, rc, tile, upper=hi1) == rc + 2 > rc + 1, name
        assert th.staged_lds_words(lo1, tile, rc, tile, upper=hi1) <= rc + 1
    assert th.first_words(th.BIG_TILE) <= th.COO_ROW_CAP + 1  # the accumulate kernel: row-first words only


# ------------------------------------------------------- single-pass tails
def test_coo_tail_matrix_delivers_its_tails():
    (plan, e, _), (plan81, e81, _) = th.coo_tail_case(False), th.coo_tail_case(True)
    assert plan.tolist() == [80, 0, 2, 0, 79, 0, 1, 0] and plan81.tolist() == [81, 0, 2, 0, 79, 0, 1, 0]
    m, m81 = e.m, e81.m
    assert m.nnz % 2 == 1 and m.nnz == m81.nnz and m.n_rows == m81.n_rows and np.array_equal(m.col, m81.col)
    assert m.row[-1] == m.row[7 * th.BIG_TILE - 1] != m.row[7 * th.BIG_TILE - 2 - th.BIG_TILE]  # the tail of 1: nnz - 1
    diff = np.flatnonzero(np.bincount(m.row, minlength=m.n_rows) != np.bincount(m81.row, minlength=m.n_rows))
    assert diff.tolist() == [3, 4]
    assert th.coo_tail_case(False)[1] is e


# ---------------------------------------------------------------- HYB tail
def test_hyb_tail_span_matrix_delivers_its_spans():
    info, e, _ = th.hyb_tail_case()
    m = e.m
    lens = np.bincount(m.row, minlength=m.n_rows)
    assert lens.min() == th.HYB_K and info["spans"] == (1024, 1025, 1025, 40_000)
    assert np.array_equal(info["no_tail"], np.flatnonzero(lens == th.HYB_K)) and info["no_tail"].size > 42_000
    ptr, col, val = sa.csr_from_coo(m)
    hb = sa.hyb_build(m.n_rows, ptr, col, val, ki=2, K=th.HYB_K)
    tr = hb["tail_row"][: hb["tail_nnz"]]
    spans = th.coo_tile_spans(tr, th.BIG_TILE)
    assert [int(spans[t]) for t in info["under"]] == [1024, 1025, 1025, 40_000]
    assert [th.staged_row_path(s, th.COO_ROW_CAP, th.BIG_TILE) for s in (1024, 1025, 40_000)] == ["heads", "bitmap", "search"]
    assert th.coo_tail_plan(tr).max() == 80 and len(th.carry_runs(tr, th.BIG_TILE)) >= 4
    assert th.hyb_tail_case()[1] is e


# -------------------------------------------------------------- carry runs
@pytest.mark.parametrize("tile", [th.TILE, th.BIG_TILE])
def test_carry_run_matrix_delivers_its_runs(tile):
    info, e, _ = th.carry_case(tile)
    m = e.m
    want = [1, 7, 8, 9, 255, 256, 257, 511, 512, 513] if tile == th.TILE else [7, 8, 9, 255, 256, 257]
    assert [k for _, k, _ in info["long_rows"]] == want
    runs = th.carry_runs(np.sort(m.row), tile)
    assert runs == info["runs"] == th.carry_runs(np.asarray(sa.csr_from_coo(m)[0]), tile)
    lens = np.bincount(m.row, minlength=m.n_rows)
    for r, k, head in info["long_rows"]:
        assert lens[r] == tile * k + 7 and (head, k) in runs and r % 64 in (0, 63)
    heads = {k: head for _, k, head in info["long_rows"]}
    assert heads[8] % 64 == 0 and heads[9] // 64 == heads[8] // 64  # two wave-path heads in one wave
    assert heads[255] % 64 == 63 and heads[256] % 256 == 255
    assert sum(runs[-1]) == info["tiles"] == -(-m.nnz // tile) and runs[-1][1] == want[-1]
    assert th.carry_tile(m.n_rows, m.nnz) == tile and m.nnz <= 2_000_000
    assert lens.max() > np.bincount(m.col).max()  # integerize sizes its sums by the longest row
    # the HYB tail of the long rows (1,536-entry tiles whatever the matrix) has runs on both sides of 8 and of 256
    ptr, col, val = sa.csr_from_coo(m)
    hb = sa.hyb_build(m.n_rows, ptr, col, val, ki=2, K=th.HYB_K)
    tail = [n for _, n in th.carry_runs(hb["tail_row"][: hb["tail_nnz"]], th.BIG_TILE)]
    assert min(tail) < th.CARRY_SHORT <= max(tail)
    if tile == th.BIG_TILE:
        assert {7, 8, 9, 255, 256, 257} <= set(tail)
    assert th.carry_case(tile)[1] is e


def _model_rows(cr, cv, y0, ref, **kw):
    """Rows where the carry model's y differs from the int64 reference."""
    return exact.exact_bad_rows(th.carry_model(cr, cv, y0.copy(), **kw), ref)


def _stale(cr, cv, n=300):
    """The arrays with n more elements behind them that continue the last
    carry: what an unchecked load past n_tiles may find."""
    return np.concatenate((cr, np.full(n, cr[-1]))), np.concatenate((cv, np.ones(n)))


@pytest.mark.parametrize("tile", [th.TILE, th.BIG_TILE])
def test_carry_model_gives_the_reference(tile):
    """coo_carry_kernel's order of work in numpy, on the carries of the integer
    copy: the COO / CSR layout and, for 512-entry tiles, cmrs_tiled_kernel's
    k-major one at h = 8 and h = 64."""
    _, e, _ = th.carry_case(tile)
    cr, cv, y0 = th.carry_arrays(e.m, e.x, tile)
    assert exact.exact_bad_rows(y0, e.ref).size >= len(th.CARRY_RUNS[tile])  # the carries are needed
    assert _model_rows(cr, cv, y0, e.ref).size == 0
    crs, cvs = _stale(cr, cv)
    assert _model_rows(crs, cvs, y0, e.ref, n_tiles=cr.size).size == 0
    if tile == th.TILE:
        for h in (8, 64):
            kr, kv, ky, tiles = th.cmrs_carry_arrays(e.m, e.x, h, tile)
            assert kr.size == h * tiles and kr[-1] >= 0  # a run ends on the array's last element
            assert exact.exact_bad_rows(ky, e.ref).size > 0 and _model_rows(kr, kv, ky, e.ref).size == 0


@pytest.mark.parametrize("tile", [th.TILE, th.BIG_TILE])
@pytest.mark.parametrize("mutate", ["one_round", "short", "unbounded", "first_head"])
def test_carry_model_mutations_fail_here(tile, mutate):
    """Each one-line mutation of the model changes rows of carry_run_matrix:
    one round only loses the runs of more than 256 tiles (a run of exactly 256
    needs the second round only to find its end), the short path alone every
    run of 9 or more, loads past n_tiles add to the run that ends on the last
    tile, and a wave that serves only its first wave-path head loses the runs
    of 9 and of 255 tiles, whose heads share a wave with the run of 8."""
    info, e, _ = th.carry_case(tile)
    cr, cv, y0 = th.carry_arrays(e.m, e.x, tile)
    crs, cvs = _stale(cr, cv)
    bad = _model_rows(crs, cvs, y0, e.ref, n_tiles=cr.size, mutate=mutate)
    rows = {k: r for r, k, _ in info["long_rows"]}
    if mutate == "one_round":
        assert set(bad) == {r for k, r in rows.items() if k > th.CARRY_ROUND}
    elif mutate == "short":
        assert set(bad) == {r for k, r in rows.items() if k > th.CARRY_SHORT}  # a run of exactly 8: still right
    elif mutate == "unbounded":
        assert bad.tolist() == [info["long_rows"][-1][0]]
    else:
        long_heads = [(r, hd) for r, k, hd in info["long_rows"] if k >= th.CARRY_SHORT]
        later = {r for i, (r, hd) in enumerate(long_heads) if any(h2 // th.K_WAVE == hd // th.K_WAVE for _, h2 in long_heads[:i])}
        assert set(bad) == later == {rows[9], rows[th.CARRY_ROUND - 1]}


def test_carry_model_mutations_on_one_row():
    """What exact.generated("one_row") could tell before: its one run (39
    continuation tiles of 512 entries, 13 of 1,536) stays inside the first
    round, and it is the only one, so a wave path that stops after one round
    or serves one head per wave passes it: no matrix of the suite had run the
    second round or two wave-path heads in one wave.  It has no run of 7, 8 or
    9 tiles either.  Its run is longer than 8 and ends on the last tile, so
    the other two mutations already change it."""
    e = exact.integerize(exact.generated("one_row"), seed=5)
    for tile, run in ((th.TILE, 39), (th.BIG_TILE, 13)):
        cr, cv, y0 = th.carry_arrays(e.m, e.x, tile)
        assert th.runs_of(cr) == [(1, run)] and th.CARRY_SHORT < run < th.CARRY_ROUND
        crs, cvs = _stale(cr, cv)
        assert _model_rows(cr, cv, y0, e.ref).size == 0
        assert _model_rows(crs, cvs, y0, e.ref, n_tiles=cr.size, mutate="one_round").size == 0
        assert _model_rows(crs, cvs, y0, e.ref, n_tiles=cr.size, mutate="first_head").size == 0
        assert _model_rows(crs, cvs, y0, e.ref, n_tiles=cr.size, mutate="short").tolist() == [1]
        assert _model_rows(crs, cvs, y0, e.ref, n_tiles=cr.size, mutate="unbounded").tolist() == [1]


# --------------------------------------------------------------- x windows
def test_window_matrices_deliver_their_windows():
    want = [100, 100, 2048, 100, 2049, 100, 1, 100, 100]
    spans, e, _ = th.window_case("coo")
    assert spans.tolist() == want and th.carry_tile(e.m.n_rows, e.m.nnz) == th.TILE
    assert np.array_equal(th.tile_windows(sa.coo_sort_by_row(e.m)[1], th.TILE), spans)
    spans, e, _ = th.window_case("cmrs")
    m, _, G = th.cmrs_window_matrix()
    assert spans.tolist() == want and m is not None and G * th.CMRS_WINDOW_H * len(want) > m.n_rows > G * th.CMRS_WINDOW_H * (len(want) - 1)
    ptr, col, _ = sa.csr_from_coo(m)
    # the entries outside a run that its chunks load widen no window: without them every span is the same
    own = [int(col[ptr[s]:ptr[min(s + G * 8, m.n_rows)]].max() - col[ptr[s]:ptr[min(s + G * 8, m.n_rows)]].min()) + 1
           for s in range(0, m.n_rows, G * 8)]
    assert own == want
    assert th.window_case("cmrs")[1] is e


def test_references_are_shared():
    a = th.tiles_case("followed")
    assert th.tiles_case("followed")[2] is a[2] and not a[2].ref.flags.writeable
    for make in (lambda: th.coo_span_case("carry-L2"), lambda: th.coo_tail_case(True), th.hyb_tail_case,
                 lambda: th.carry_case(th.BIG_TILE), lambda: th.window_case("coo")):
        b = make()
        assert make()[1] is b[1] and make()[2][2] is b[2][2]
        assert not b[1].ref.flags.writeable and not b[1].m.val.flags.writeable and not b[2][0].val.flags.writeable


# ======================================================= the row-block core
# rowblock.h and its eight users (transpose.hip, symmetric.hip): the stream,
# cap and dropped families of tests/thresholds.py deliver what they promise;
# numpy models of rb_row_of and wave_run_add give the reference on them, and
# their one-line mutations (and wave_run_add's earlier key rule) do not.
STREAMS = [(nr, lower) for nr in th.RB_LAST_ROWS for lower in (False, True)]
STREAM_IDS = [f"nr{nr}-{'lower' if lower else 'rect'}" for nr, lower in STREAMS]


@pytest.mark.parametrize("last_nr,lower", STREAMS, ids=STREAM_IDS)
def test_rowblock_stream_matrix_delivers_its_blocks(last_nr, lower):
    m, info = th.rowblock_stream_matrix(last_nr, lower)
    ptr = th.csr_of(m)[0]
    assert np.array_equal(ptr, sa.csr_from_coo(m)[0])
    assert m.n_rows % th.RB_ROWS == last_nr and (m.n_rows == m.n_cols) == lower
    counts = sorted(E for _, E, _ in info["under"])
    assert counts == sorted(2 * th.RB_ENTRY_COUNTS)
    both_sides = lambda line: {line - 1, line, line + 1} <= set(counts)  # noqa: E731
    assert both_sides(th.K_BLOCK) and both_sides(th.RB_STEP) and both_sides(2 * th.RB_STEP)
    assert {th.RB_STEP + th.K_BLOCK - 1, th.RB_STEP + th.K_BLOCK, 5 * th.RB_STEP + 1} <= set(counts)
    for E in th.RB_ENTRY_COUNTS:  # two different layouts per count
        assert len({la for _, e, la in info["under"] if e == E}) == 2
    lens = np.diff(ptr)
    for (b, E, layout), s0 in zip(info["under"], info["starts"]):
        r0 = b * th.RB_ROWS
        mine = lens[r0:r0 + th.RB_ROWS]
        ends = (ptr[r0 + 1:r0 + th.RB_ROWS + 1] - s0)[mine > 0]  # where rows end, from the block's first entry
        if layout == "first":
            assert mine[0] == E and mine[1:].sum() == 0
        elif layout == "last":
            assert mine[-1] == E and mine[:-1].sum() == 0
        elif layout == "middle":
            assert mine[77] == E and mine.sum() == E
        elif layout == "singles":
            assert (mine[: min(E, 127)] == 1).all()
        elif layout == "wave" and E >= 1023:  # a row ends one lane before a wave's last, on it and one past it
            assert {62, 63, 0} <= set(((ends - 1) % th.K_WAVE).tolist())
            assert set(mine[mine > 0][:-1].tolist()) == {63, 64, 65}
        elif layout == "long" and E >= th.RB_LONG_ROW:  # the long row holds a whole unrolled step of the stream
            a, z = ptr[r0 + 5] - s0, ptr[r0 + 6] - s0
            assert z - a == th.RB_LONG_ROW and a % th.RB_STEP == 0 and a + th.RB_STEP < z
        elif layout == "runs":
            assert mine[:40].sum() == 0 and mine[-40:].sum() == 0 and (mine[40:-40] > 0).sum() == min(E, 48)
    assert any(la == "wave" and E >= 1023 for _, E, la in info["under"])
    # the windows: the rules once more by a plain loop, and narrow
    win = info["windows"]
    for b in range(win.shape[0]):
        r0, r1 = b * th.RB_ROWS, min((b + 1) * th.RB_ROWS, m.n_rows)
        c = m.col[ptr[r0]:ptr[r1]]
        if c.size == 0:
            assert tuple(win[b]) == (0, -1) and (b in info["empty"])
        elif lower:
            assert tuple(win[b]) == (min(int(c.min()), r0), max(int(c.max()), r1 - 1))
        else:
            assert tuple(win[b]) == (int(c.min()), int(c.max()))
    assert (win[:, 1] - win[:, 0] + 1).max() < 512
    assert th.rowblock_stream_matrix(last_nr, lower)[0] is m and not m.val.flags.writeable  # made once, read-only


def test_rowblock_cap_matrices_deliver_their_spans():
    m, info = th.rowblock_cap_matrix()
    assert sorted(s for _, s in info["under"]) == [1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193] == sorted(th.T_CAP_SPANS)
    e = info["expect"]
    span = info["windows"][:, 1] - info["windows"][:, 0] + 1
    assert e["lds_blocks"] == int(((span > 0) & (span <= 2048)).sum()) == 4 and e["flush_entries"] == 1024 + 1025 + 2048 + 9
    for w, cap in zip(th.T_WIDTHS, (8192, 4096, 2048, 1024)):
        assert e["multi_lds_blocks"][th.T_WIDTHS.index(w)] == int(((span > 0) & (span <= cap)).sum())
        assert {cap, cap + 1} <= set(span.tolist())  # both sides of the cap of every width
    assert np.bincount(m.col).max() >= 4  # overlapping windows: a column is hit from several blocks
    s, sinfo = th.rowblock_sym_cap_matrix()
    assert sorted(sp for _, sp, kind in sinfo["under"] if kind == "lower") == sorted(th.S_CAP_SPANS)
    assert sorted(sp for _, sp, kind in sinfo["under"] if kind == "upper") == sorted(th.S_CAP_SPANS)
    assert th.S_CAP_SPANS == (512, 513, 1024, 1025, 2048, 2049, 4096, 4097) and s.n_rows == 6221
    se = sinfo["expect"]
    sspan = sinfo["windows"][:, 1] - sinfo["windows"][:, 0] + 1
    rows = np.minimum(th.RB_ROWS, s.n_rows - th.RB_ROWS * np.arange(sspan.size))
    for i, cap in enumerate((4096, 2048, 1024, 512)):
        fit, wide = (sspan > 0) & (sspan <= cap), sspan > cap
        assert se["multi_window_blocks"][i] == int(fit.sum()) and wide.sum() == 2 * (2 * i + 1)
        assert se["multi_flush_entries"][i] == int(sspan[fit].sum() + rows[wide].sum())
    assert (se["window_blocks"], se["flush_entries"]) == (se["multi_window_blocks"][1], se["multi_flush_entries"][1])
    assert sspan[-1] == th.S_CAP_LAST_ROWS == rows[-1]  # the last block: the span equals nr
    # the expansion is what the half describes: every off-diagonal entry once more
    ex = sa.expand_symmetric(s)
    assert ex.nnz == 2 * s.nnz - int((s.row == s.col).sum())


def test_rowblock_cases_fit_the_integer_check():
    """The integer copies fit exact.integerize's budget: |value| < 2^a, |x| <
    2^b with a + b + ceil(log2(longest row or column + 1)) <= 52 on the matrix
    (transposed) or on its expansion (symmetric).  The densest column of the
    cap family is hit from many blocks; the stream family's longest row is the
    5,121-entry block in one row."""
    for nr, lower in STREAMS:
        info, t, s = th.stream_case(nr, lower)
        assert (t["a"], t["b"]) == (19, 20) and (s is None) == (not lower)  # c = 13: 5,121 entries in one row
        assert t["ref_i"].shape == (t["mi"].n_cols, th.RB_KMAX) and not t["ref_i"].flags.writeable
        if s is not None:
            assert s["a"] + s["b"] + 13 <= 52 and s["ref_i"].shape == (s["mi"].n_rows, th.RB_KMAX)
    _, t = th.cap_case()
    densest = int(np.bincount(t["mi"].col).max())
    assert densest >= 4 and t["a"] + t["b"] + math.ceil(math.log2(max(densest, 65) + 1)) <= 52
    _, s = th.sym_cap_case()
    ex = sa.expand_symmetric(s["mi"])
    longest = int(np.bincount(ex.row).max())
    # a row of the 4,097-column window: its diagonal and 31 or 32 of the 3,969 far columns, mirrored entries besides
    assert longest >= 32 and s["a"] + s["b"] + math.ceil(math.log2(longest + 1)) <= 52 and s["a"] >= 20
    assert th.cap_case()[1] is t and th.sym_cap_case()[1] is s  # computed once


# ------------------------------------------------------- rb_row_of, modelled
def _row_search(m, mutate=None, lanes="uniform"):
    """-> (entries whose modelled row differs from searchsorted, of them the
    ones that are lanes past the block's end, the rows the model gave them)."""
    ptr = th.csr_of(m)[0]
    wrong = past = 0
    rows = []
    for b in range(th.rb_blocks(m.n_rows)):
        r0, nr = b * th.RB_ROWS, min(th.RB_ROWS, m.n_rows - b * th.RB_ROWS)
        s_ptr = ptr[r0:r0 + nr + 1]
        if s_ptr[0] == s_ptr[nr]:
            continue
        e = th.uniform_lanes(int(s_ptr[0]), int(s_ptr[nr])).ravel()
        want = np.searchsorted(s_ptr[:nr], e, side="right") - 1
        got = th.rb_row_of(s_ptr, nr, e, mutate)
        bad = got != want
        wrong += int(bad.sum())
        past += int((bad & (e >= s_ptr[nr])).sum())
        rows += [(nr, int(g)) for g in np.unique(got[bad])]
    return wrong, past, rows


@pytest.mark.parametrize("last_nr,lower", STREAMS, ids=STREAM_IDS)
def test_row_search_model_gives_the_row(last_nr, lower):
    """The seven guarded steps equal np.searchsorted(s_ptr[:nr], e, "right") - 1
    for every entry id a block's stream hands out, the ids past the block's end
    in its last partial step included (sym_block searches for those too)."""
    m = th.rowblock_stream_matrix(last_nr, lower)[0]
    assert _row_search(m)[0] == 0


def test_row_search_mutations_fail_here():
    """Each one-line mutation gives a wrong row on these matrices:
      <= to <         the first entry of every row that follows an entry
      six steps       without step 64 the rows from 64 on ("last", "middle",
                      "singles"); without step 1 the odd rows
      r + step <= nr  s_ptr[nr] is the block's end, above every entry, and in a
                      full block no step reaches r + step = 128: the mutation
                      can only move the lanes past the end of the SHORT last
                      block (1, 2 and 127 rows), to row nr, one past the block.
                      sym_block searches for those lanes and then ignores them,
                      so the guard protects no result today; the model keeps
                      the three last blocks able to see it."""
    totals = {}
    for nr, lower in STREAMS:
        m = th.rowblock_stream_matrix(nr, lower)[0]
        for mutate in ("less", "guard", "six_front", "six_back"):
            wrong, past, rows = _row_search(m, mutate)
            assert wrong > 0, (mutate, nr, lower)
            totals[mutate] = totals.get(mutate, 0) + wrong
            if mutate == "guard":
                assert wrong == past and all(got == n for n, got in rows)
                assert {n for n, _ in rows} == {nr}  # the short last block alone
            elif mutate == "six_front":
                assert past < wrong
    assert min(totals.values()) > 100


# ---------------------------------------------------- wave_run_add, modelled
def _row_counts(m):
    """x = 1, every value 1: a row's sum is the number of its entries inside [0, n)."""
    ptr, col, _ = th.csr_of(m)
    ok = (col >= 0) & (col < m.n_cols)
    return ptr, col, ok.astype(np.float64), np.bincount(m.row[ok], minlength=m.n_rows).astype(np.float64)


@pytest.mark.parametrize("last_nr", th.RB_LAST_ROWS)
def test_wave_scan_model_on_the_valid_families(last_nr):
    """Without a dropped entry both key rules give every row its sum: on the
    lower stream matrices (rows ending on lanes 62, 63 and 64, a row across
    whole steps, blocks that end inside a wave) and on the cap family."""
    for m in (th.rowblock_stream_matrix(last_nr, True)[0], th.rowblock_sym_cap_matrix()[0]):
        ptr, col, prod, want = _row_counts(m)
        for fixed in (False, True):
            assert np.array_equal(th.sym_row_sums(m.n_rows, ptr, col, prod, fixed), want)


def test_wave_scan_double_counts_around_a_dropped_lane():
    """The defect on record without a GPU: with key -1 on a dropped entry
    inside a row the scan's step off = 2 adds the lane below the gap into the
    lane above it and both are the last of a run.  The probe row (10 entries,
    a dropped one, 9 more, all 1.0, lanes 0..19 of one wave) gets 29 instead
    of 19; a dropped FIRST or LAST entry of a row breaks no run.  With the
    row's key and a product of 0.0 on the dropped lane every row gets its sum."""
    with_d, valid, info = th.rowblock_dropped_matrix()
    ptr, col, prod, want = _row_counts(with_d)
    assert np.array_equal(want, np.bincount(valid.row, minlength=valid.n_rows))
    assert np.array_equal(th.sym_row_sums(with_d.n_rows, ptr, col, prod, fixed=True), want)
    old = th.sym_row_sums(with_d.n_rows, ptr, col, prod, fixed=False)
    pr = info["probe_row"]
    assert want[pr] == 19.0 and old[pr] == 29.0
    bad = np.flatnonzero(old != want)
    assert pr in bad and (old[bad] > want[bad]).all()
    # the rows that come out wrong are exactly rows with a dropped entry strictly inside them
    out = (with_d.col < 0) | (with_d.col >= with_d.n_cols)
    inner = {int(with_d.row[e]) for e in np.flatnonzero(out)
             if ptr[with_d.row[e]] < e < ptr[with_d.row[e] + 1] - 1 and not out[ptr[with_d.row[e]]:ptr[with_d.row[e] + 1]].all()}
    assert set(bad.tolist()) <= inner and len(bad) >= 4
    # the minimal wave of the issue: ten products of row 5, a dropped lane, nine more
    key = np.full((1, th.K_WAVE), -1)
    p = np.zeros((1, th.K_WAVE))
    key[0, :20], p[0, :20] = 5, 1.0
    key[0, 10], p[0, 10] = -1, 0.0
    acc = np.zeros(8)
    th.wave_run_add(acc, key, p)
    assert acc[5] == 29.0
    key[0, 10] = 5
    acc[:] = 0.0
    th.wave_run_add(acc, key, p)
    assert acc[5] == 19.0


def test_rowblock_dropped_matrix_delivers_its_entries():
    with_d, valid, info = th.rowblock_dropped_matrix()
    n = with_d.n_rows
    out = (with_d.col < 0) | (with_d.col >= n)
    assert sorted(np.unique(with_d.col[out]).tolist()) == [-1, n, n + 1] and info["dropped"] == out.sum() == with_d.nnz - valid.nnz
    ptr = th.csr_of(with_d)[0]
    first = out[ptr[:-1][np.diff(ptr) > 0]]
    last = out[ptr[1:][np.diff(ptr) > 0] - 1]
    assert first.sum() >= 4 and last.sum() >= 4  # dropped first and last entries of rows
    span = info["windows"][:, 1] - info["windows"][:, 0] + 1
    blocks = with_d.row[out] // th.RB_ROWS
    assert {info["only"], info["window_block"], *info["wide"]} <= set(blocks.tolist())
    assert (span[list(info["wide"])] > th.T_MULTI_CAP).all() and 0 < span[info["window_block"]] < 512
    # the host statements refuse the matrix: they cannot supply the reference
    y = np.zeros(n)
    with pytest.raises(sa.SpmvError):
        sa.cpu_csr_sym(n, ptr, with_d.col, with_d.val, np.ones(n), y)
    with pytest.raises(sa.SpmvError):
        sa.cpu_csr_t(n, n, ptr, with_d.col, with_d.val, np.ones(n), y)
    # the cases: the valid matrix's references, and CSR arrays that hold its values at the valid entries
    cinfo, csr, t, s = th.dropped_case()
    for (kind, integer), (p, c, v) in csr.items():
        case = t if kind == "t" else s
        assert np.array_equal(v[~out], (case["mi"] if integer else case["mr"]).val) and (v[out] != 0.0).all()
        assert p is ptr or np.array_equal(p, ptr)
    assert th.dropped_case()[2] is t
