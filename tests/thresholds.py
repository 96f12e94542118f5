"""Matrices that land on the kernels' own size thresholds: TEST
INFRASTRUCTURE ONLY (tests/test_thresholds.py, tests/test_thresholds_gpu.py).

The matrix families of tests/exact.py never reach the sizes at which a kernel
changes its control flow; those sizes are named only by the kernels' sources.
Two constructors put a matrix exactly there and say what they delivered, so a
test can assert that it ran the case it meant:

  sell_run_matrix   a SELL split plan whose chunk runs have given lengths.
                    sell_split_fix_kernel (csrc/sell.hip) finds a run's end by
                    coarse passes of 1024 probes 64 apart and one fine pass of
                    64: the lengths around 65,536 + 1 and 2 * 65,536 + 1 are
                    where a coarse pass ends exactly on the run's end.
  tile_rows_matrix  a CSR matrix whose 512-entry tiles own given numbers of
                    rows.  csr_tiled_kernel (csrc/staged.hip) stages the
                    offsets of up to 1024 owned rows in LDS, lists the rows of
                    a tile of up to 65,536 in a big-tile plan, and reads
                    row_ptr from global memory beyond that;
                    spmv_csr_tiled_bigplan (host/formats.c) draws the same two
                    lines.

The staged family (csrc/staged.hip, csrc/coo.hip) has its own constructors,
with the kernels' constants and launch rules restated below (the plan reports
none of them; tests/test_thresholds.py holds every restated line against the
sources):

  coo_span_matrix       COO tiles that span given numbers of rows (prev, last]:
                        coo_staged_kernel takes its key-change table up to RC
                        rows, the row-first and span bitmaps (both inside
                        s_start[RC + 1]) up to 32 (RC + 1 - FW), two binary
                        searches per row beyond
  coo_tail_matrix       single-pass tiles whose last rows run 1, 2, 79 and 80
                        entries past the tile (kCooTailCap = 80), one ending
                        on the lone last entry of an odd nnz; or one of 81
  hyb_tail_span_matrix  a HYB tail (the accumulate kernel) whose tiles span
                        1024, 1025 and 40,000 rows
  carry_run_matrix      rows over given numbers of continuation tiles:
                        coo_carry_kernel sums a run of up to 7 in tile order
                        and a run of 8 or more over the wave, 256 tiles a round
  coo_window_matrix,    x windows of exactly kStagedXwinCap = 2048 columns, of
  cmrs_window_matrix    2049 and of one, in one launch

The row-block core (csrc/rowblock.h) and its users, the transposed scatter
kernels and the fused symmetric kernels, have theirs at the end of the file,
again with constants, window rules, the width rule and LDS sizes restated, and
with numpy models of rb_row_of's search and wave_run_add's scan:

  rowblock_stream_matrix   128-row blocks of 1 .. 5,121 entries around every
                           loop bound of rb_stream (steps of 1,024, a tail in
                           steps of 256), in seven row layouts; last blocks of
                           1, 2 and 127 rows; a lower-triangular twin
  rowblock_cap_matrix,     column spans of 1,024 .. 8,193 and union windows of
  rowblock_sym_cap_matrix  512 .. 4,097: every cap of every width and one more
  rowblock_dropped_matrix  valid entries plus columns -1, n and n + 1

None needs a GPU.  The matrices are made once per argument set and never
changed.
"""
from __future__ import annotations

import functools

import numpy as np

import exact
import spmv_amd as sa

FIX_THREADS = 1024      # sell.hip kSellFixThreads
FIX_STEP = 64           # the coarse pass's probe distance
FIX_PASS = FIX_THREADS * FIX_STEP  # chunks one full coarse pass covers: 65,536
TILE = 512              # staged.hip: 2 * kBlock * kTiledR entries per tile
ROW_CAP = 1024          # staged.hip kTiledRowCap
BIG_ROW_CAP = 65536     # staged.hip kTiledBigRowCap
K_BLOCK = 256           # common.h kBlock
K_WAVE = 64             # common.h kWave
COO_ROW_CAP = 1024      # staged.hip kCooRowCap
COO_ROW_CAP_SHORT = 250  # staged.hip kCooRowCapShort
COO_TAIL_CAP = 80       # staged.hip kCooTailCap
COO_R = 3               # staged.hip kCooR
XWIN_CAP = 2048         # common.h kStagedXwinCap
CARRY_SHORT = 8         # coo.hip coo_carry_kernel: rr[8], lng = rr[7] == r
CARRY_ROUND = 4 * K_WAVE  # coo.hip coo_carry_kernel: base += 4 * kWave
BIG_TILE = 2 * K_BLOCK * COO_R  # staged.hip coo_staged_tile(): 1536 entries
MEAN_LANES_8 = 48.0     # staged.hip coo_lanes
MEAN_LANES_4 = 12.0     # staged.hip coo_lanes
MEAN_BIG_TILE = 96.0    # staged.hip coo_hot_r, cmrs_tiled_r


def _freeze(m: sa.Coo) -> sa.Coo:
    for a in (m.row, m.col, m.val):
        a.setflags(write=False)
    return m


# ----------------------------------------------------------- SELL chunk runs
def fix_pass_end(c: int, chunk_slice: np.ndarray, fixed: bool = True) -> int:
    """The run end sell_split_fix_kernel computes for the run starting at chunk
    c, restated on the host (fixed=False: the search before its correction,
    which kept lo after a coarse pass without a match)."""
    n_chunks, s = chunk_slice.size, chunk_slice[c]

    def hits(q):  # probes that find the run's slice (the kernel's q < n_chunks guard)
        return int(np.count_nonzero((q < n_chunks) & (chunk_slice[np.minimum(q, n_chunks - 1)] == s)))

    lo, first = c + 1, True
    while True:
        n = hits(lo + FIX_STEP * np.arange(FIX_THREADS, dtype=np.int64))
        if n < FIX_THREADS:
            if n > 0:
                lo = lo + (n - 1) * FIX_STEP + 1
            elif fixed and not first:
                lo = lo - FIX_STEP + 1
            break
        lo += FIX_PASS
        first = False
    return lo + hits(lo + np.arange(FIX_STEP, dtype=np.int64))


def run_lengths(chunk_slice: np.ndarray) -> list:
    """Lengths of the runs of equal values, in order."""
    if chunk_slice.size == 0:
        return []
    cut = np.flatnonzero(np.diff(chunk_slice)) + 1
    return np.diff(np.concatenate(([0], cut, [chunk_slice.size]))).tolist()


def small_runs(C: int) -> tuple:
    """Run lengths every sell_run_matrix has besides the long one: 1, 2, and
    around W = 1024 / C, the segment count of the fix pass (a run of at most W
    chunks is summed in chunk order, a longer one in W segments), and 65, one
    past the fine pass's 64 probes."""
    W = FIX_THREADS // C
    return (1, 2, W - 1, W, W + 1, 65)


@functools.lru_cache(maxsize=None)
def sell_run_matrix(R: int, C: int, T: int, tail_chunks: int = 99, last: bool = False, ki: int = 1):
    """-> (matrix, expected run lengths).  C-row slices, to be built with
    sigma = C, ki and split = T (T a multiple of ki):

      slice 0         rows of 0..T entries: no chunk
      the small runs  one slice per length r of small_runs(C): one row of
                      T (r + 1) entries among short rows
      the long run    one row of T (R + 1) entries in distinct columns among
                      short rows: exactly R chunks
      the tail        full-width slices, every row T (q + 1) entries long, q
                      at most 40, tail_chunks >= 64 chunks in all: a run end
                      found up to 63 chunks too late adds these rows' non-zero
                      partial sums and still reads inside the partial buffer
      the last slice  5 short rows (the row count is no multiple of C)

    last=True puts the long run behind the tail: the last run in chunk order.
    The expected run lengths come from the host's spmv_sell_split_plan on the
    built SELL structure and are asserted to be the ones meant."""
    assert R >= 1 and T >= 1 and T % ki == 0 and tail_chunks >= FIX_STEP
    rng = np.random.default_rng(R + 7 * C + 13 * T + (1 if last else 0))
    n_cols = T * (R + 1) + 7
    tails = [40] * (tail_chunks // 40) + ([tail_chunks % 40] if tail_chunks % 40 else [])

    def short(n):  # lengths 0..T, at least one empty and one full row
        lens = rng.integers(0, T + 1, n)
        lens[0], lens[-1] = 0, T
        return lens

    def one_long(r):  # a slice's row lengths: the long row in a random place
        lens = short(C)
        lens[rng.integers(1, C - 1)] = T * (r + 1)
        return lens

    slices = [short(C)] + [one_long(r) for r in small_runs(C)]
    body = [one_long(R)]
    tail = [np.full(C, T * (q + 1)) for q in tails]
    slices += tail + body if last else body + tail
    want = list(small_runs(C)) + (tails + [R] if last else [R] + tails)
    lens = np.concatenate(slices + [short(5)]).astype(np.int64)
    n_rows = lens.size
    row = np.repeat(np.arange(n_rows, dtype=np.int32), lens)
    col = np.empty(row.size, np.int32)
    ptr = np.concatenate(([0], np.cumsum(lens)))
    for r in np.flatnonzero(lens):
        col[ptr[r]:ptr[r + 1]] = rng.permutation(n_cols)[: lens[r]]  # distinct columns in every row
    m = _freeze(sa.Coo(n_rows, n_cols, row, col, rng.uniform(-1.0, 1.0, row.size), False,
                       f"SELL run of {R} chunks (C={C}, T={T}, ki={ki}{', last' if last else ''})"))
    cptr, ccol, cval = sa.csr_from_coo(m)
    s = sa.sell_build(n_rows, cptr, ccol, cval, C=C, sigma=C, ki=ki)
    Tp, chunk_slice, chunk_k0 = sa.sell_split_plan(s, T)
    runs = run_lengths(chunk_slice)
    assert Tp == T and runs == want, (runs[:8], want[:8])
    assert np.array_equal(chunk_k0, np.concatenate([T * np.arange(1, r + 1) for r in runs]))
    return m, runs


# the run lengths on both sides of the two windows in which the uncorrected
# search was wrong, [65,474, 65,536] and [131,010, 131,072], and inside them
SELL_RS = (65_473, 65_474, 65_500, 65_536, 65_537, 65_538, 131_040, 131_073)


@functools.lru_cache(maxsize=None)
def sell_case(R: int, C: int = 32, T: int = 1, last: bool = False, ki: int = 1):
    """-> (runs, integer copy with its int64 reference (exact.Exact), (real
    copy, x, reference, bound)); computed once, shared by the CPU and GPU
    tests, never changed."""
    m, runs = sell_run_matrix(R, C, T, 99, last, ki)
    seed = R % 10_007 + 3 * C + 5 * T + (1 if last else 0)
    mr, x, _ = exact.realize(m, seed=seed + 1)
    return runs, exact.integerize(m, seed=seed), (mr, x, exact.exact_reference(mr, x), exact.fp64_bound(mr, x))


# ------------------------------------------------------ tiled CSR owned rows
TILE_NRS = (ROW_CAP, ROW_CAP + 1, BIG_ROW_CAP, BIG_ROW_CAP + 1)
TILE_ORDERS = {"followed": True, "final": False}  # is the 65,537-row tile followed by another, or the matrix's last


@functools.lru_cache(maxsize=None)
def tiles_case(order: str):
    """As sell_case for tile_rows_matrix(TILE_NRS, trailing=TILE_ORDERS[order]):
    -> (owned rows per tile, tiles under test, integer copy, (real copy, x,
    reference, bound))."""
    m, owned, under_test = tile_rows_matrix(TILE_NRS, TILE_ORDERS[order])
    seed = 77 + sorted(TILE_ORDERS).index(order)
    mr, x, _ = exact.realize(m, seed=seed + 10)
    return owned, under_test, exact.integerize(m, seed=seed), (mr, x, exact.exact_reference(mr, x),
                                                              exact.fp64_bound(mr, x))



@functools.lru_cache(maxsize=4)
def tile_rows_matrix(nrs: tuple, trailing: bool = True, n_cols: int = 4096, seed: int = 31):
    """-> (matrix, owned rows per tile, indices of the tiles under test).  For
    every nr >= 2 of nrs one 512-entry tile that owns exactly nr rows: a row
    of 1 entry at the tile's first offset, nr - 2 empty rows, a row of 511
    entries that fills the tile.  In front of each, in turn, a tile that owns
    one 512-entry row, and a 1536-entry row whose first tile owns it and whose
    other two own no row.  trailing: a last, short tile of one 100-entry row
    follows; else the last tile under test is the matrix's last, and its rows
    are the trailing ones.

    A tile owns the rows whose first offset lies in it (csr_tile_rows_kernel:
    own_lo[t] = the first row with row_ptr >= 512 t; the last tile also takes
    the rows behind the last entry): the returned counts are np.searchsorted
    on row_ptr, and the tiles under test are asserted to own nrs."""
    assert all(nr >= 2 for nr in nrs)
    lens, under_test, tile = [], [], 0
    for i, nr in enumerate(nrs):
        sep = [TILE] if i % 2 == 0 else [3 * TILE]
        lens += sep
        tile += sep[0] // TILE
        under_test.append(tile)
        lens += [1] + [0] * (nr - 2) + [TILE - 1]
        tile += 1
    if trailing:
        lens += [100]
    lens = np.asarray(lens, np.int64)
    n_rows, nnz = lens.size, int(lens.sum())
    assert nnz == tile * TILE + (100 if trailing else 0)
    rng = np.random.default_rng(seed)
    m = _freeze(sa.Coo(n_rows, n_cols, np.repeat(np.arange(n_rows, dtype=np.int32), lens),
                       rng.integers(0, n_cols, nnz).astype(np.int32), rng.uniform(-1.0, 1.0, nnz), False,
                       f"tiles owning {list(nrs)} rows"))
    owned = owned_rows(n_rows, np.concatenate(([0], np.cumsum(lens))))
    assert [int(owned[t]) for t in under_test] == list(nrs), (owned.tolist(), under_test)
    return m, owned, tuple(under_test)


def owned_rows(n_rows: int, row_ptr: np.ndarray) -> np.ndarray:
    """Rows every 512-entry tile owns, as csr_tiled_kernel counts them."""
    nnz = int(row_ptr[n_rows])
    tiles = (nnz + TILE - 1) // TILE
    lo = np.searchsorted(row_ptr[:n_rows], np.arange(tiles, dtype=np.int64) * TILE, side="left")
    hi = np.concatenate((lo[1:], [n_rows]))  # the last tile: through n_rows - 1
    return (hi - lo).astype(np.int64)


# ------------------------------------------- staged COO: launch rules restated
def coo_lanes(n_rows: int, nnz: int) -> int:
    """staged.hip coo_lanes: lanes per row of every COO launch but the accumulate one."""
    mean = nnz / n_rows if n_rows > 0 else 0.0
    return 8 if mean >= MEAN_LANES_8 else 4 if mean >= MEAN_LANES_4 else 2


def carry_tile(n_rows: int, nnz: int) -> int:
    """staged.hip coo_hot_r / cmrs_tiled_r: entries per tile of the COO carry
    pass (plain, x windows, hot table) and of the tiled CMRS; the single pass
    and the HYB tail always cut BIG_TILE."""
    return TILE if n_rows > 0 and nnz < MEAN_BIG_TILE * n_rows else BIG_TILE


def coo_row_cap(launch: str, lanes: int) -> int:
    """RC of the coo_staged_kernel instantiation a launch takes (launch_coo_staged,
    launch_coo_staged_hot, launch_coo_staged_acc*): the non-temporal carry pass
    and the single pass pick it by lane count, every other launch has the default."""
    if launch in ("carry", "single"):
        return COO_ROW_CAP if lanes == 2 else COO_ROW_CAP_SHORT
    assert launch in ("xwin", "hot", "acc"), launch
    return COO_ROW_CAP


def first_words(tile: int) -> int:
    """FW of coo_staged_kernel: 32-bit words of a tile's row-first bitmap."""
    return (tile + 63) // 64 * 2


def bitmap_rows(rc: int, tile: int) -> int:
    """The widest span the bitmap path takes: its span bitmap and the row-first
    words then fill s_start[rc + 1] to the last word."""
    return 32 * (rc + 1 - first_words(tile))


def span_edges(rc: int, tile: int) -> tuple:
    """Both sides of the two lines coo_staged_kernel<..., RC = rc> draws."""
    return (rc, rc + 1, bitmap_rows(rc, tile), bitmap_rows(rc, tile) + 1)


def staged_row_path(span: int, rc: int, tile: int, upper: int | None = None) -> str:
    upper = bitmap_rows(rc, tile) if upper is None else upper
    return "heads" if span <= rc else "bitmap" if span <= upper else "search"


def staged_lds_words(span: int, n: int, rc: int, tile: int, upper: int | None = None) -> int:
    """Words of s_start the row phase of a non-accumulate tile of n entries
    touches (the highest index + 1): the key-change table writes [0, span], the
    bitmap path ceil(span / 32) span words and behind them two words per 64
    entries, the search path none."""
    path = staged_row_path(span, rc, tile, upper)
    if path == "heads":
        return span + 1
    if path == "bitmap":
        return (span + 31) // 32 + 2 * ((n + 63) // 64)
    return 0


def coo_tile_spans(row: np.ndarray, tile: int) -> np.ndarray:
    """span of every tile as coo_staged_kernel computes it: rows in (prev, last],
    row[t1 - 1] - (row[t0 - 1] if t0 else -1), over the row-sorted entries."""
    nnz = row.size
    tiles = (nnz + tile - 1) // tile
    last = row[np.minimum((np.arange(tiles, dtype=np.int64) + 1) * tile, nnz) - 1].astype(np.int64)
    return last - np.concatenate(([-1], last[:-1]))


def coo_tail_plan(row: np.ndarray, tile: int = BIG_TILE) -> np.ndarray:
    """coo_tail_kernel restated: for every full tile with entries behind it, how
    many of them continue its last row, counted up to COO_TAIL_CAP + 1."""
    nnz = row.size
    tiles = (nnz + tile - 1) // tile
    out = np.zeros(tiles, np.int64)
    for t in range(tiles):
        t1 = (t + 1) * tile
        if t1 < nnz:
            other = row[t1:t1 + COO_TAIL_CAP + 1] != row[t1 - 1]
            out[t] = int(np.argmax(other)) if other.any() else other.size
    return out


def _sorted_rows(lens: np.ndarray) -> np.ndarray:
    return np.repeat(np.arange(lens.size, dtype=np.int32), lens)


def _span_layout(spans, tile, overs, cont, flen, bulk, final):
    """-> (row lengths, tiles under test, the entries each of their last rows
    runs into the next tile).  `bulk` tile-aligned filler rows of flen entries
    (flen divides the tile), then for every S of spans a separator tile of
    filler and the tile under test: a row of 3 entries at the tile's first
    entry, S - 2 empty rows, a row that fills the tile and runs `over` entries
    on; behind the tile of S == cont a second one whose first entries continue
    that row (first_continues) and which spans S rows after it.  A row that
    ends on the next filler boundary follows each.  The end: a row of 7 and 37
    empty rows; final: the 37 empty rows directly behind the last tile under
    test, which then has no overhang and is the matrix's last tile."""
    assert tile % flen == 0 and all(s >= 2 for s in spans)
    per = tile // flen
    lens, under, ran, pos = [], [], [], 0
    overs = list(overs)

    def filler(k):
        nonlocal pos
        lens.extend([flen] * k)
        pos += k * flen

    filler((bulk + per - 1) // per * per)
    for i, S in enumerate(spans):
        filler(per)
        assert pos % tile == 0
        carried = 0
        for second in ((False, True) if S == cont else (False,)):
            closing = final and i == len(spans) - 1 and (second or S != cont)
            over = 0 if closing else overs.pop(0)
            under.append(pos // tile)
            ran.append(over)
            lens.extend([3] + [0] * (S - 2) + [tile - carried - 3 + over])
            pos += tile - carried + over
            carried = over
        if carried:
            if pos % flen:
                lens.append(-pos % flen)
                pos += lens[-1]
            filler((-pos % tile) // flen)
    if final:
        assert pos % tile == 0 and under[-1] == pos // tile - 1
    lens.extend(([] if final else [7]) + [0] * 37)
    return np.asarray(lens, np.int64), tuple(under), tuple(ran)


CARRY_OVERS = (5, 1, 300, 2, 97)  # entries the last rows of the tiles under test run on: the carries


def tail_overs(tail: int) -> tuple:
    return (tail, 1, tail - 1, 2, 37)


@functools.lru_cache(maxsize=2)
def coo_span_matrix(spans: tuple, tile: int, lanes: int, tail: int | None = None, final: bool = False,
                    cont: int | None = None, n_cols: int = 2000, seed: int = 41):
    """-> (matrix, info).  COO tiles of `tile` entries spanning exactly `spans`
    rows (the span `cont`, by default spans[1], twice: once more behind a
    continued first row), laid out by _span_layout, with as much filler as
    puts the mean row where coo_lanes gives `lanes` and, for the carry pass (tail None), where
    carry_tile gives `tile`; tail: the single pass (always BIG_TILE), whose
    tiles under test have last rows running up to `tail` entries on.  Asserts
    the spans, the lanes, the tile and, for the single pass, the tail plan."""
    single = tail is not None
    cont = spans[1] if cont is None else cont
    assert tile in (TILE, BIG_TILE) and (not single or tile == BIG_TILE)
    if not single and tile == BIG_TILE:
        assert lanes == 8
        target, flen = MEAN_BIG_TILE, tile // 2
    else:
        target, flen = {8: (MEAN_LANES_8, 256), 4: (MEAN_LANES_4, 128), 2: (None, tile)}[lanes]
    overs = tail_overs(tail) if single else CARRY_OVERS
    lens, under, ran = _span_layout(spans, tile, overs, cont, flen, 0, final)
    if target is not None:  # filler rows until the mean row is 4 % above the target
        want = 1.04 * target
        bulk = max(0, int(np.ceil((want * lens.size - lens.sum()) / (flen - want))))
        lens, under, ran = _span_layout(spans, tile, overs, cont, flen, bulk, final)
    n_rows, nnz = lens.size, int(lens.sum())
    row = _sorted_rows(lens)
    wanted = tuple(s for s in spans for _ in range(2 if s == cont else 1))
    got = coo_tile_spans(row, tile)
    assert tuple(int(got[t]) for t in under) == wanted, (got[list(under)], wanted)
    assert coo_lanes(n_rows, nnz) == lanes, (n_rows, nnz, lanes)
    second = under[wanted.index(cont) + 1]
    assert row[second * tile] == row[second * tile - 1]  # first_continues
    if single:
        plan = coo_tail_plan(row)
        assert plan.max() == tail <= COO_TAIL_CAP and tuple(int(plan[t]) for t in under) == ran, (plan.max(), ran)
    else:
        assert carry_tile(n_rows, nnz) == tile, (n_rows, nnz, tile)
        assert all(row[(t + 1) * tile] == row[(t + 1) * tile - 1] for t, o in zip(under, ran) if o)  # carries
    assert (under[-1] == got.size - 1 and nnz % tile == 0) == final
    assert nnz <= 2_000_000
    rng = np.random.default_rng(seed + lanes + tile + (7 if final else 0))
    m = _freeze(sa.Coo(n_rows, n_cols, row, rng.integers(0, n_cols, nnz).astype(np.int32),
                       rng.uniform(-1.0, 1.0, nnz), False,
                       f"COO tiles of {tile} spanning {list(wanted)} rows, {lanes} lanes"
                       f"{', single pass' if single else ''}{', final' if final else ''}"))
    return m, dict(spans=wanted, under=under, ran=ran, lanes=lanes, tile=tile, tiles=int(got.size))


# name: (the launch whose RC places the spans, lanes, tile, final).  "wide-L4"
# serves the x-window and the hot-column launch (RC = 1024 at 4 lanes) and,
# for the bits, the plain carry pass (RC = 250: its bitmap and search paths).
SPAN_CASES = {
    "carry-L2": ("carry", 2, TILE, False),
    "carry-L2-final": ("carry", 2, TILE, True),
    "carry-L4": ("carry", 4, TILE, False),
    "carry-L8": ("carry", 8, TILE, False),
    "carry-L8-big": ("carry", 8, BIG_TILE, False),
    "wide-L4": ("xwin", 4, TILE, False),
    "single-L2": ("single", 2, BIG_TILE, False),
    "single-L2-final": ("single", 2, BIG_TILE, True),
    "single-L4": ("single", 4, BIG_TILE, False),
    "single-L8": ("single", 8, BIG_TILE, False),
}


def _case(m: sa.Coo, seed: int):
    """(integer copy with its int64 reference, (real copy, x, reference, bound))"""
    mr, x, _ = exact.realize(m, seed=seed + 1)
    return exact.integerize(m, seed=seed), (mr, x, exact.exact_reference(mr, x), exact.fp64_bound(mr, x))


@functools.lru_cache(maxsize=None)
def coo_span_case(name: str):
    """-> (info, integer copy, (real copy, x, reference, bound)) of SPAN_CASES[name]:
    the spans RC, RC + 1, 32 (RC + 1 - FW) and one more (final: the upper bitmap
    edge last); computed once, shared by the CPU and GPU tests."""
    launch, lanes, tile, final = SPAN_CASES[name]
    rc = coo_row_cap(launch, lanes)
    e = span_edges(rc, tile)
    spans = (e[1], e[3], e[0], e[2]) if final else e
    m, info = coo_span_matrix(spans, tile, lanes, COO_TAIL_CAP if launch == "single" else None, final, e[1])
    return dict(info, rc=rc, launch=launch, edges=e), *_case(m, 300 + sorted(SPAN_CASES).index(name))


# --------------------------------------------------- single-pass tails at the cap
@functools.lru_cache(maxsize=None)
def coo_tail_matrix(over_cap: bool = False, n_cols: int = 3000):
    """-> (matrix, tail plan).  1,536-entry tiles 0, 2, 4 and 6 end in rows that
    run 80 (over_cap: 81), 2, 79 and 1 entries on; the last of them ends on
    nnz - 1, the lone entry of an odd nnz.  Both forms have the same rows but
    for the two around the first tile end, and the same columns and values."""
    tails = [COO_TAIL_CAP + (1 if over_cap else 0), 2, COO_TAIL_CAP - 1, 1]
    lens = []
    for i, k in enumerate(tails):
        lens += [100, 0, 0, BIG_TILE - 100 + k] + ([BIG_TILE - k] if i < len(tails) - 1 else [])
    lens = np.asarray(lens + [0] * 5, np.int64)
    row, nnz = _sorted_rows(lens), int(lens.sum())
    plan = coo_tail_plan(row)
    assert nnz % 2 == 1 and row[-1] == row[6 * BIG_TILE + BIG_TILE - 1] and nnz == 7 * BIG_TILE + 1
    assert plan.tolist() == [tails[0], 0, 2, 0, COO_TAIL_CAP - 1, 0, 1, 0]
    assert coo_lanes(lens.size, nnz) == 8
    rng = np.random.default_rng(43)
    return _freeze(sa.Coo(lens.size, n_cols, row, rng.integers(0, n_cols, nnz).astype(np.int32),
                          rng.uniform(-1.0, 1.0, nnz), False, f"single-pass tails {tails}")), plan


@functools.lru_cache(maxsize=None)
def coo_tail_case(over_cap: bool = False):
    m, plan = coo_tail_matrix(over_cap)
    return plan, *_case(m, 350 + int(over_cap))


# ------------------------------------------------------ HYB tail: accumulate
HYB_K = 2
HYB_SPANS = (COO_ROW_CAP, COO_ROW_CAP + 1, 40_000)  # the accumulate bitmap has no upper line


@functools.lru_cache(maxsize=None)
def hyb_tail_span_matrix(n_cols: int = 2000):
    """-> (matrix, info).  Every row has HYB_K entries for the ELL part; the
    entries past them are a _span_layout of 1,536-entry tiles spanning
    HYB_SPANS rows (1025 twice, once behind a continued first row), with
    overhangs the single-pass tail plan accepts.  The spans and the tail plan
    are asserted on sa.hyb_build's own tail_row."""
    lens_t, under, ran = _span_layout(HYB_SPANS, BIG_TILE, tail_overs(COO_TAIL_CAP), HYB_SPANS[1], BIG_TILE, 0, False)
    lens = lens_t + HYB_K
    nnz = int(lens.sum())
    rng = np.random.default_rng(47)
    m = _freeze(sa.Coo(lens.size, n_cols, _sorted_rows(lens), rng.integers(0, n_cols, nnz).astype(np.int32),
                       rng.uniform(-1.0, 1.0, nnz), False, f"HYB tail tiles spanning {list(HYB_SPANS)} rows"))
    ptr, col, val = sa.csr_from_coo(m)
    hb = sa.hyb_build(m.n_rows, ptr, col, val, ki=2, K=HYB_K)
    tr = hb["tail_row"][: hb["tail_nnz"]]
    assert hb["K"] == HYB_K and hb["tail_nnz"] == lens_t.sum() and np.array_equal(tr, _sorted_rows(lens_t))
    spans = coo_tile_spans(tr, BIG_TILE)
    wanted = (HYB_SPANS[0], HYB_SPANS[1], HYB_SPANS[1], HYB_SPANS[2])
    assert tuple(int(spans[t]) for t in under) == wanted, (spans[list(under)], wanted)
    plan = coo_tail_plan(tr)
    assert plan.max() == COO_TAIL_CAP and tuple(int(plan[t]) for t in under) == ran
    assert coo_row_cap("acc", 4) == HYB_SPANS[0]
    return m, dict(spans=wanted, under=under, ran=ran, no_tail=np.flatnonzero(lens_t == 0))


@functools.lru_cache(maxsize=None)
def hyb_tail_case():
    m, info = hyb_tail_span_matrix()
    return info, *_case(m, 360)


# ------------------------------------------------------------ carry runs
def carry_rows(row: np.ndarray, tile: int) -> np.ndarray:
    """carry_row of the COO and CSR tile passes over row-sorted entries:
    carry_row[t] = the row of entry t * tile if it continues the row of entry
    t * tile - 1, else -1."""
    tiles = (row.size + tile - 1) // tile
    cr = np.full(tiles, -1, np.int64)
    t0 = np.arange(1, tiles, dtype=np.int64) * tile
    cr[1:] = np.where(row[t0] == row[t0 - 1], row[t0], -1)
    return cr


def runs_of(cr: np.ndarray) -> list:
    """[(head index, run length)] of the runs of equal carries >= 0: what
    coo_carry_kernel's head test (r >= 0 && prev != r) starts a sum for."""
    cr = np.asarray(cr, np.int64)
    cut = np.flatnonzero(np.diff(cr)) + 1
    start = np.concatenate(([0], cut))
    length = np.diff(np.concatenate((start, [cr.size])))
    return [(int(s), int(n)) for s, n in zip(start, length) if cr[s] >= 0]


def carry_runs(row_or_ptr: np.ndarray, tile: int) -> list:
    """runs_of(carry_rows(...)) from the sorted row ids or from row_ptr."""
    a = np.asarray(row_or_ptr)
    row = a if a.dtype == np.int32 else _sorted_rows(np.diff(a))
    return runs_of(carry_rows(row, tile))


def _products(m: sa.Coo, x: np.ndarray):
    order = np.argsort(m.row, kind="stable")
    return m.row[order].astype(np.int64), m.val[order] * np.asarray(x)[m.col[order]]


def carry_arrays(m: sa.Coo, x: np.ndarray, tile: int):
    """What the tile pass hands coo_carry_kernel -> (carry_row, carry_val, y):
    y holds every row's entries of the tile it begins in."""
    row, prod = _products(m, x)
    cr = carry_rows(row, tile)
    tid = np.arange(row.size, dtype=np.int64) // tile
    carried = row == cr[tid]
    return (cr, np.bincount(tid[carried], weights=prod[carried], minlength=cr.size),
            np.bincount(row[~carried], weights=prod[~carried], minlength=m.n_rows))


def cmrs_carry_arrays(m: sa.Coo, x: np.ndarray, h: int, tile: int):
    """cmrs_tiled_kernel's carries restated, k-major: the strip that runs into
    tile t from an earlier one (no strip starts at t's first entry) leaves
    carry[k * tiles + t] for every row key k with entries in the tile, up to
    the next strip's start -> (carry_row, carry_val, y, tiles)."""
    row, prod = _products(m, x)
    nnz = row.size
    tiles = (nnz + tile - 1) // tile
    n_strips = (m.n_rows + h - 1) // h
    ptr = np.concatenate(([0], np.cumsum(np.bincount(row, minlength=m.n_rows))))
    sp = np.concatenate((ptr[: m.n_rows: h], [nnz]))
    assert sp.size == n_strips + 1
    t0 = np.arange(tiles, dtype=np.int64) * tile
    s_lo = np.searchsorted(sp[:n_strips], t0, side="left")  # csr_tile_rows_kernel over strip_ptr
    has = (s_lo > 0) & (sp[s_lo] > t0)
    end = np.minimum(sp[s_lo], t0 + tile)
    j = np.arange(nnz, dtype=np.int64)
    tid = j // tile
    carried = has[tid] & (j < end[tid])
    assert (row[carried] // h == s_lo[tid[carried]] - 1).all()
    idx = (row % h) * tiles + tid
    cr = np.full(h * tiles, -1, np.int64)
    cr[idx[carried]] = row[carried]
    return (cr, np.bincount(idx[carried], weights=prod[carried], minlength=cr.size),
            np.bincount(row[~carried], weights=prod[~carried], minlength=m.n_rows), tiles)


def carry_model(cr, cv, y, n_tiles: int | None = None, mutate: str | None = None):
    """coo_carry_kernel in numpy, y updated in place: the head test, a run of
    up to CARRY_SHORT - 1 tiles added in tile order by the head's thread, a
    longer one lane-strided over the wave in rounds of CARRY_ROUND tiles and
    then the xor butterfly.  cr and cv may be longer than n_tiles (what lies
    behind the arrays).  mutate, one line each:
      "one_round"  the wave path stops after its first round
      "short"      no run takes the wave path: a run of exactly 8 is summed as a
                   short one, and of a longer one only rr[0..7] are read
      "unbounded"  the loads are not held to n_tiles
      "first_head" only the first wave-path head of a wave's 64 tiles is served"""
    assert mutate in (None, "one_round", "short", "unbounded", "first_head")
    cr, cv = np.asarray(cr, np.int64), np.asarray(cv, np.float64)
    n = cr.size if n_tiles is None else n_tiles
    lim = cr.size if mutate == "unbounded" else n

    def load(i):  # the guarded loads: -2 / 0.0 past the limit
        ok = i < lim
        ic = np.minimum(i, cr.size - 1)
        return np.where(ok, cr[ic], -2), np.where(ok, cv[ic], 0.0)

    prev = np.concatenate(([-1], cr[: n - 1]))
    lane = np.arange(K_WAVE, dtype=np.int64)
    served = set()  # waves whose ballot loop has run once
    for t in np.flatnonzero((cr[:n] >= 0) & (prev != cr[:n])):  # the heads, wave by wave in lane order
        rr, vv = load(t + np.arange(CARRY_SHORT, dtype=np.int64))
        r = int(rr[0])
        if rr[CARRY_SHORT - 1] != r or mutate == "short":
            s = 0.0
            for k in range(CARRY_SHORT):
                if rr[k] != r:
                    break
                s += vv[k]
            y[r] += s
            continue
        if mutate == "first_head" and t // K_WAVE in served:
            continue
        served.add(t // K_WAVE)
        s, base = np.zeros(K_WAVE), int(t)
        while True:
            end = np.zeros(K_WAVE, bool)
            for u in range(CARRY_ROUND // K_WAVE):
                q, v = load(base + u * K_WAVE + lane)
                s = s + np.where(q == r, v, 0.0)
                end |= q != r
            if end.any() or mutate == "one_round":
                break
            base += CARRY_ROUND
        off = K_WAVE // 2
        while off:
            s = s + s[lane ^ off]
            off //= 2
        y[r] += s[t % K_WAVE]
    return y


CARRY_N_COLS_STEP = 7919  # a long row's columns: start + 7919 i mod n_cols, distinct while it is no longer than n_cols


@functools.lru_cache(maxsize=None)
def carry_run_matrix(runs: tuple, tile: int, pad: int = 0, trailing: int = 0):
    """-> (matrix, info).  One long row per item of runs, an int k or (k,
    residue, modulus): the row begins 100 entries into a tile behind three rows
    of 5 entries and has tile * k + 7 entries, so it continues over exactly k
    tiles; with (residue, modulus) rows of up to 100 entries in front put the
    run's head (its first continuation tile) at a tile index = residue mod
    modulus.  pad: entries in such rows before everything; trailing: empty
    rows behind the last long row, whose run ends on the matrix's last tile.
    At least 60 empty rows in front of the three short ones place the long
    rows alternately at row ids = 0 and = 63 mod 64, the last at 63: row keys
    0 and h - 1 of a CMRS strip for h = 8 and h = 64, each strip beginning in
    its long row's first tile.  Asserts the runs, the placements and the CMRS
    carries' k-major runs for both h."""
    items = [(it, None, None) if isinstance(it, int) else it for it in runs]
    lens, pos, long_rows = [], 0, []

    def short_rows(n):
        nonlocal pos
        while n > 0:
            lens.append(min(100, n))
            n -= lens[-1]
            pos += lens[-1]

    short_rows(pad)
    for i, (k, res, mod) in enumerate(items):
        T = (pos + 15 - 100 + tile - 1) // tile if pos + 15 > 100 else 0
        while mod is not None and (T + 1) % mod != res:
            T += 1
        short_rows(T * tile + 100 - 15 - pos)
        key = 63 if i % 2 or i == len(items) - 1 else 0
        lens.extend([0] * (60 + (key - (len(lens) + 63)) % 64) + [5, 5, 5])
        assert len(lens) % 64 == key
        pos += 15
        assert pos == T * tile + 100
        long_rows.append((len(lens), k, T + 1))
        lens.append(tile * k + 7)
        pos += lens[-1]
    lens = np.asarray(lens + [0] * trailing, np.int64)
    n_rows, nnz = lens.size, int(lens.sum())
    row = _sorted_rows(lens)
    found = carry_runs(row, tile)
    tiles = (nnz + tile - 1) // tile
    for (r, k, head), (_, res, mod) in zip(long_rows, items):
        assert (head, k) in found and (mod is None or head % mod == res), (r, k, head)
    heads = [hd for _, k, hd in long_rows if k >= CARRY_SHORT]
    assert any(a // K_WAVE == b // K_WAVE for a, b in zip(heads, heads[1:]))  # two wave-path heads in one wave
    assert any(hd % K_WAVE == K_WAVE - 1 for hd in heads) and any(hd % K_BLOCK == K_BLOCK - 1 for hd in heads)
    assert found[-1] == (long_rows[-1][2], long_rows[-1][1]) and sum(found[-1]) == tiles  # ends on the last tile
    assert carry_tile(n_rows, nnz) == tile, (n_rows, nnz, tile)
    n_cols = int(lens.max()) + 12_345
    n_cols += n_cols % CARRY_N_COLS_STEP == 0
    rng = np.random.default_rng(53 + tile)
    col = rng.integers(0, n_cols, nnz).astype(np.int32)
    ptr = np.concatenate(([0], np.cumsum(lens)))
    for r, _, _ in long_rows:
        col[ptr[r]:ptr[r + 1]] = (rng.integers(0, n_cols) + CARRY_N_COLS_STEP * np.arange(lens[r])) % n_cols
        assert np.unique(col[ptr[r]:ptr[r + 1]]).size == min(lens[r], n_cols)
    assert np.bincount(col).max() < lens.max()
    m = _freeze(sa.Coo(n_rows, n_cols, row, col, rng.uniform(-1.0, 1.0, nnz), False,
                       f"rows over {[k for _, k, _ in long_rows]} continuation tiles of {tile}"))
    for h in (8, 64):  # the same runs k-major, one in the last segment ending on the array's last element
        cr, _, _, tl = cmrs_carry_arrays(m, np.ones(n_cols), h, tile)
        assert tl == tiles and cr.size == h * tiles
        kruns = runs_of(cr)
        for r, k, head in long_rows:
            assert ((r % h) * tiles + head, k) in kruns and r % h in (0, h - 1), (h, r, k)
        assert sum(kruns[-1]) == cr.size and kruns[-1][1] == long_rows[-1][1]
    return m, dict(runs=found, long_rows=tuple(long_rows), tiles=tiles, tile=tile)


CARRY_RUNS = {
    TILE: (1, 7, (8, 0, K_WAVE), 9, (CARRY_ROUND - 1, K_WAVE - 1, K_WAVE), (CARRY_ROUND, K_BLOCK - 1, K_BLOCK),
           CARRY_ROUND + 1, 2 * CARRY_ROUND - 1, 2 * CARRY_ROUND, 2 * CARRY_ROUND + 1),
    BIG_TILE: (7, (8, 0, K_WAVE), 9, (CARRY_ROUND - 1, K_WAVE - 1, K_WAVE), (CARRY_ROUND, K_BLOCK - 1, K_BLOCK),
               CARRY_ROUND + 1),
}
CARRY_TRAILING = {TILE: 20_000, BIG_TILE: 0}  # empty rows: a mean row below / above 96 entries


@functools.lru_cache(maxsize=None)
def carry_case(tile: int):
    """-> (info, integer copy, (real copy, x, reference, bound)) of
    carry_run_matrix(CARRY_RUNS[tile], tile, 33, CARRY_TRAILING[tile])."""
    m, info = carry_run_matrix(CARRY_RUNS[tile], tile, 33, CARRY_TRAILING[tile])
    return info, *_case(m, 370 + tile)


# ------------------------------------------------------------- x windows
def tile_windows(col_sorted: np.ndarray, tile: int) -> np.ndarray:
    """tile_window_kernel restated: columns spanned by every tile of the
    row-sorted entries (max - min + 1)."""
    cut = np.arange(0, col_sorted.size, tile)
    return (np.maximum.reduceat(col_sorted, cut).astype(np.int64) - np.minimum.reduceat(col_sorted, cut) + 1)


WINDOW_BASE = 1000  # the column every window of the two matrices below contains


def _window_cols(rng, n, kind):
    """n columns of one tile / strip run: "cap" spans XWIN_CAP columns, "over"
    one more, "one" a single column, else 100; the first and last columns of
    the range both occur."""
    width = {"cap": XWIN_CAP, "over": XWIN_CAP + 1, "one": 1}.get(kind, 100)
    c = WINDOW_BASE + rng.integers(0, width, n)
    c[n // 2], c[n // 2 + 1] = WINDOW_BASE, WINDOW_BASE + width - 1
    return c


WINDOW_KINDS = ("", "", "cap", "", "over", "", "one", "", "")  # per tile / strip run; the last one is short


@functools.lru_cache(maxsize=None)
def coo_window_matrix(n_cols: int = 5000):
    """-> (matrix, window spans).  Rows of 80 entries (a mean row below 96:
    512-entry tiles, with carries); tile 2's columns span exactly 2048, tile
    4's 2049, tile 6's one column, the others 100."""
    rng = np.random.default_rng(59)
    nnz = (len(WINDOW_KINDS) - 1) * TILE + 37
    lens = np.asarray([80] * (nnz // 80) + [nnz % 80], np.int64)
    col = np.concatenate([_window_cols(rng, min(TILE, nnz - t * TILE), kind) for t, kind in enumerate(WINDOW_KINDS)])
    m = _freeze(sa.Coo(lens.size, n_cols, _sorted_rows(lens), col.astype(np.int32), rng.uniform(-1.0, 1.0, nnz),
                       False, "COO x windows of 2048, 2049 and 1 columns"))
    assert carry_tile(m.n_rows, nnz) == TILE and coo_lanes(m.n_rows, nnz) == 8
    spans = tile_windows(sa.coo_sort_by_row(m)[1], TILE)
    assert spans.tolist() == [{"cap": XWIN_CAP, "over": XWIN_CAP + 1, "one": 1}.get(k, 100) for k in WINDOW_KINDS]
    assert len(carry_runs(m.row, TILE)) >= 4
    return m, spans


def cmrs_geometry(n_rows: int, nnz: int, h: int) -> tuple:
    """staged.hip cmrs_geometry -> (L, G): lanes per row, strips per workgroup."""
    L = sa.hip_lib().spmv_csr_auto_lanes(n_rows, nnz)
    while L > 1 and L * h > K_BLOCK:
        L //= 2
    return L, max(K_BLOCK // (L * h), 1)


def cmrs_windows(ptr: np.ndarray, col: np.ndarray, h: int, G: int) -> np.ndarray:
    """cmrs_window_kernel restated: columns spanned by the entries a run of G
    strips loads, from two before its 32-aligned first entry to one past its
    last (0 for a run without entries)."""
    n_rows, nnz = ptr.size - 1, int(ptr[-1])
    sp = np.concatenate((ptr[:n_rows:h], [nnz]))
    n_strips = sp.size - 1
    out = []
    for s0 in range(0, n_strips, G):
        b, e = int(sp[s0]), int(sp[min(s0 + G, n_strips)])
        c = col[max((b & ~31) - 2, 0):min(e + 1, nnz)] if b < e else col[:0]
        out.append(int(c.max()) - int(c.min()) + 1 if c.size else 0)
    return np.asarray(out, np.int64)


CMRS_WINDOW_H = 8


@functools.lru_cache(maxsize=None)
def cmrs_window_matrix(n_cols: int = 5000):
    """-> (matrix, window spans, G).  Rows of 15 entries behind a first row of
    22, so a strip run's first entry is not 32-aligned and its window reaches
    back into the run before; those entries and the one behind each run hold
    WINDOW_BASE, which every run's range contains.  Run 2 spans exactly 2048
    columns, run 4 2049, run 6 one column, the others 100; the last run is
    short."""
    h = CMRS_WINDOW_H
    L, G = cmrs_geometry(1000, 15_000, h)
    n_rows = (len(WINDOW_KINDS) - 1) * G * h + 5
    lens = np.full(n_rows, 15, np.int64)
    lens[0] = 22
    nnz = int(lens.sum())
    assert cmrs_geometry(n_rows, nnz, h) == (L, G)
    ptr0 = np.concatenate(([0], np.cumsum(lens)))
    cut = ptr0[np.minimum(np.arange(len(WINDOW_KINDS) + 1) * G * h, n_rows)]  # the strip runs' entry ranges
    rng = np.random.default_rng(61)
    col = np.concatenate([_window_cols(rng, int(cut[w + 1] - cut[w]), kind) for w, kind in enumerate(WINDOW_KINDS)])
    for b, e in zip(cut[:-1], cut[1:]):
        col[max((b & ~31) - 2, 0):b] = WINDOW_BASE
        if e < nnz:
            col[e] = WINDOW_BASE
    m = _freeze(sa.Coo(n_rows, n_cols, _sorted_rows(lens), col.astype(np.int32), rng.uniform(-1.0, 1.0, nnz), False,
                       "CMRS x windows of 2048, 2049 and 1 columns"))
    ptr, ccol, _ = sa.csr_from_coo(m)
    spans = cmrs_windows(np.asarray(ptr, np.int64), ccol, h, G)
    assert np.array_equal(ptr, ptr0) and (cut[1:-1] % 32 != 0).all()
    assert spans.tolist() == [{"cap": XWIN_CAP, "over": XWIN_CAP + 1, "one": 1}.get(k, 100) for k in WINDOW_KINDS]
    return m, spans, G


@functools.lru_cache(maxsize=None)
def window_case(fmt: str):
    m, spans = (coo_window_matrix() if fmt == "coo" else cmrs_window_matrix()[:2])
    return spans, *_case(m, 380 + len(fmt))


# ===================================================== the row-block core
# csrc/rowblock.h and its users csr_t_window_kernel, csr_t_multi_kernel<KV>
# (csrc/transpose.hip), csr_sym_window_kernel and csr_sym_multi_kernel<KV>
# (csrc/symmetric.hip).  Constants, the window rules, the width rule and the
# LDS sizes restated (tests/test_thresholds.py holds them against the sources),
# then three families:
#
#   rowblock_stream_matrix   blocks of 128 rows whose entry counts sit on both
#                            sides of every loop bound of rb_stream's two forms
#                            (steps of 1,024 entries, a tail in steps of 256),
#                            the entries laid out so that rb_row_of's search,
#                            wave_run_add's scan and the DPP rounds meet their
#                            edges; last blocks of 1, 2 and 127 rows
#   rowblock_cap_matrix,     blocks whose column span (transposed) or union
#   rowblock_sym_cap_matrix  window (symmetric) is exactly every cap and one
#                            more, every column of the span hit
#   rowblock_dropped_matrix  a valid matrix plus entries in columns -1, n and
#                            n + 1, which the scatter and fused runs drop
RB_ROWS = 128                # rowblock.h kRbRows
RB_PTR = RB_ROWS + 2         # rowblock.h kRbPtr
RB_U = 4                     # rowblock.h kRbU
RB_STEP = RB_U * K_BLOCK     # entries of one unrolled step of rb_stream: 1,024
RB_SEARCH_STEPS = 7          # rb_row_of: step = kRbRows / 2, ..., 1
T_CAP = 2048                 # transpose.hip kTCap
T_MULTI_CAP = 8192           # transpose.hip SPMV_T_MULTI_CAP
S_CAP = 2048                 # symmetric.hip kSCap
S_MULTI_CAP = 4096           # symmetric.hip SPMV_S_MULTI_CAP
T_WIDTHS = (1, 2, 4, 8)      # rowblock.h kTWidths
RB_KS = (1, 2, 3, 4, 5, 8, 9)  # vectors per call: live < KV at every width, a second pass of width 1
RB_KMAX = max(RB_KS)
# exact scalings: column j of a real X is SCALES[j] * x, its reference and bound scale with it
RB_SCALES = (1.0, -2.0, 0.5, 4.0, -0.25, 8.0, -1.0, 0.125, -16.0)
# both sides of every bound of `e + 3 * 256 < end` (per thread) and `e0 + 1024 <= end` (uniform), of the
# 256-entry tail steps, of two and of five unrolled steps; E mod 4 takes 1, 2 and 3
RB_ENTRY_COUNTS = (1, 255, 256, 257, 1023, 1024, 1025, 1026, 1279, 1280, 2047, 2048, 2049, 5121)
RB_LAYOUTS = ("first", "last", "middle", "singles", "wave", "long", "runs")
RB_LAST_ROWS = (1, 2, 127)   # rows of the last block: rb_row_of's guard r + step < nr, the tid < nr loads of x
RB_LONG_ROW = 1500           # the "long" layout's row: longer than one unrolled step


def rb_blocks(n_rows: int) -> int:
    return (n_rows + RB_ROWS - 1) // RB_ROWS


def pass_widths(k: int) -> list:
    """launch_scatter_multi / launch_fused_multi: [(live vectors, kernel width)]
    of the ceil(k / 8) passes: live > 4 -> 8, > 2 -> 4, else live."""
    out = []
    for j0 in range(0, k, 8):
        live = min(k - j0, 8)
        out.append((live, 8 if live > 4 else 4 if live > 2 else live))
    return out


def t_multi_lds(kv: int, span: int) -> int:
    """transpose.hip t_multi_lds: dynamic LDS bytes of csr_t_multi_kernel<kv>."""
    return (RB_PTR + RB_ROWS * kv + span * kv) * 8


def sym_multi_lds(kv: int, span: int) -> int:
    """symmetric.hip sym_multi_lds: dynamic LDS bytes of csr_sym_multi_kernel<kv>."""
    return (RB_PTR + 2 * max(span, RB_ROWS) * kv) * 8


def _block_ranges(n_rows, n_cols, ptr, col):
    blocks = rb_blocks(n_rows)
    win = np.empty((blocks, 2), np.int64)
    for b in range(blocks):
        r0, r1 = b * RB_ROWS, min((b + 1) * RB_ROWS, n_rows)
        c = np.asarray(col[ptr[r0]:ptr[r1]], np.int64)
        c = c[(c >= 0) & (c < n_cols)]
        win[b] = (c.min(), c.max()) if c.size else (0, -1)
    return win


def t_windows(n_rows: int, n_cols: int, ptr, col) -> np.ndarray:
    """csr_t_range_kernel restated -> (blocks, 2) {lo, hi}: the range of the
    block's columns inside [0, n_cols); {0, -1} for a block without one."""
    return _block_ranges(n_rows, n_cols, ptr, col)


def sym_windows(n: int, ptr, col) -> np.ndarray:
    """csr_sym_range_kernel restated: the same range joined with the block's
    own rows; {0, -1} for a block without an entry inside [0, n)."""
    win = _block_ranges(n, n, ptr, col)
    for b in range(win.shape[0]):
        if win[b, 1] >= win[b, 0]:
            win[b] = (min(win[b, 0], b * RB_ROWS), max(win[b, 1], min((b + 1) * RB_ROWS, n) - 1))
    return win


def window_tally(win: np.ndarray, cap: int):
    """plan.hip windows_tally -> (blocks that fit, the sum of their spans, the widest of them)."""
    span = win[:, 1] - win[:, 0] + 1
    fit = (span > 0) & (span <= cap)
    return int(fit.sum()), int(span[fit].sum()), int(span[fit].max()) if fit.any() else 0


def expected_transpose_info(win: np.ndarray) -> dict:
    """What prepare_scatter must report for these windows."""
    one = window_tally(win, T_CAP)
    return dict(blocks=win.shape[0], lds_blocks=one[0], flush_entries=one[1],
                multi_lds_blocks=[window_tally(win, T_MULTI_CAP // w)[0] for w in T_WIDTHS],
                multi_widest=[window_tally(win, T_MULTI_CAP // w)[2] for w in T_WIDTHS])


def expected_symmetric_info(n: int, win: np.ndarray) -> dict:
    """What prepare_fused must report: a union past the cap flushes the sums of the block's rows."""
    span = win[:, 1] - win[:, 0] + 1
    rows = np.minimum((np.arange(win.shape[0]) + 1) * RB_ROWS, n) - np.arange(win.shape[0]) * RB_ROWS

    def at(cap):
        fit = window_tally(win, cap)
        return fit[0], fit[1] + int(rows[span > cap].sum()), fit[2]

    one, multi = at(S_CAP), [at(S_MULTI_CAP // w) for w in T_WIDTHS]
    return dict(blocks=win.shape[0], window_blocks=one[0], flush_entries=one[1],
                multi_window_blocks=[m[0] for m in multi], multi_flush_entries=[m[1] for m in multi],
                multi_widest=[m[2] for m in multi])


def csr_of(m: sa.Coo):
    """(row_ptr, col, val) of a row-sorted Coo in numpy: no host builder, so
    columns outside [0, n_cols) pass through."""
    assert (np.diff(m.row) >= 0).all()
    ptr = np.concatenate(([0], np.cumsum(np.bincount(m.row, minlength=m.n_rows)))).astype(np.int64)
    return ptr, m.col, m.val


# ------------------------------------------------------- the models
def rb_row_of(s_ptr: np.ndarray, nr: int, e: np.ndarray, mutate: str | None = None) -> np.ndarray:
    """rowblock.h rb_row_of in numpy for entries e (any shape): seven guarded
    steps over the block's nr + 1 offsets.  mutate, one line each:
      "less"       s_ptr[r + step] < e instead of <=
      "guard"      r + step <= nr instead of < nr
      "six_front"  the search starts at step 32
      "six_back"   the search stops before step 1"""
    assert mutate in (None, "less", "guard", "six_front", "six_back") and s_ptr.size == nr + 1
    steps = [RB_ROWS >> (i + 1) for i in range(RB_SEARCH_STEPS)]
    steps = steps[1:] if mutate == "six_front" else steps[:-1] if mutate == "six_back" else steps
    e = np.asarray(e, np.int64)
    r = np.zeros(e.shape, np.int64)
    for step in steps:
        inside = (r + step <= nr) if mutate == "guard" else (r + step < nr)
        at = s_ptr[np.minimum(r + step, nr)]
        r = r + step * (inside & ((at < e) if mutate == "less" else (at <= e)))
    return r


def uniform_lanes(s0: int, end: int) -> np.ndarray:
    """The entry ids rb_stream<true> hands to its body, wave by wave -> (waves,
    64): the block's entries from s_ptr[0] in order; the last tail step is
    filled with ids past `end` (the lanes that are not live)."""
    count = (end - s0 + K_BLOCK - 1) // K_BLOCK * K_BLOCK if (end - s0) % RB_STEP else end - s0
    return (s0 + np.arange(count, dtype=np.int64)).reshape(-1, K_WAVE)


def wave_run_add(acc: np.ndarray, key: np.ndarray, p: np.ndarray) -> None:
    """symmetric.hip wave_run_add for (waves, 64) keys and products: the
    segmented scan by shuffles from `off` lanes below, then the last lane of
    every run adds its sum to acc[key]."""
    lane = np.arange(K_WAVE)
    p = p.astype(np.float64).copy()
    off = 1
    while off < K_WAVE:
        t, k = p.copy(), key.copy()
        t[:, off:], k[:, off:] = p[:, :-off], key[:, :-off]
        p = np.where((lane >= off) & (k == key), p + t, p)
        off *= 2
    nxt = key.copy()
    nxt[:, :-1] = key[:, 1:]
    last = (key >= 0) & ((lane == K_WAVE - 1) | (nxt != key))
    np.add.at(acc, key[last], p[last])


def sym_row_sums(n: int, ptr, col, prod, fixed: bool) -> np.ndarray:
    """The row sums of sym_block as its accumulator receives them through
    wave_run_add (the mirrored products are not modelled): prod[e] is the
    product of entry e, taken as 0.0 where the entry is dropped.  fixed: a
    dropped entry keeps its row's key; else it gets key -1, the form that
    breaks a run of equal keys in two."""
    acc = np.zeros(n)
    win = sym_windows(n, ptr, col)
    col = np.asarray(col, np.int64)
    for b in range(win.shape[0]):
        if win[b, 1] < win[b, 0]:
            continue
        r0, nr = b * RB_ROWS, min(RB_ROWS, n - b * RB_ROWS)
        s_ptr = np.asarray(ptr[r0:r0 + nr + 1], np.int64)
        e = uniform_lanes(int(s_ptr[0]), int(s_ptr[nr]))
        live = e < s_ptr[nr]
        ec = np.minimum(e, max(int(s_ptr[nr]) - 1, 0))
        kept = live & (col[ec] >= 0) & (col[ec] < n)
        key = np.where(live if fixed else kept, r0 + rb_row_of(s_ptr, nr, e), -1)
        wave_run_add(acc, key, np.where(kept, np.asarray(prod)[ec], 0.0))
    return acc


# ------------------------------------------------ 1. the stream family
def _rb_row_lens(layout: str, E: int) -> np.ndarray:
    """Row lengths of a full block of E entries."""
    lens = np.zeros(RB_ROWS, np.int64)
    if layout == "first":
        lens[0] = E
    elif layout == "last":
        lens[RB_ROWS - 1] = E
    elif layout == "middle":  # row 77 = 64 + 8 + 4 + 1 among empty rows
        lens[77] = E
    elif layout == "singles":  # one entry per row, what is left in the last row
        k = min(E, RB_ROWS - 1)
        lens[:k] = 1
        lens[RB_ROWS - 1] += E - k
    elif layout == "wave":  # rows of 63, 64 and 65: their last entries on lanes 62, 62, 63, 63, 0, 63 of a wave
        r, left = 0, E
        while left > 0:
            lens[r] = min((K_WAVE - 1, K_WAVE, K_WAVE + 1, K_WAVE, K_WAVE + 1, K_WAVE - 1)[r % 6], left)
            left -= lens[r]
            r += 1
    elif layout == "long":  # one row across a whole unrolled step, rows of up to 100 behind it
        lens[5] = min(E, RB_LONG_ROW)
        r, left = 6, E - lens[5]
        while left > 0:
            lens[r] = min(100, left)
            left -= lens[r]
            r += 1
    else:  # "runs": 40 empty rows in front, 40 behind
        assert layout == "runs"
        mid = RB_ROWS - 80
        lens[40:40 + mid] = E // mid
        lens[40:40 + E % mid] += 1
    assert lens.sum() == E
    return lens


def rb_layout_of(j: int, second: bool) -> str:
    """The layout of the block of RB_ENTRY_COUNTS[j] in the first / second pass over the counts."""
    return RB_LAYOUTS[(j + (3 if second else 0)) % len(RB_LAYOUTS)]


RB_LAST_ENTRIES = 300  # the short last block: one tail step of 256 and a partial one


@functools.lru_cache(maxsize=None)
def rowblock_stream_matrix(last_nr: int, lower: bool = False):
    """-> (matrix, info).  Two blocks of 128 rows per E of RB_ENTRY_COUNTS, in
    two different layouts (rb_layout_of); a filler block of 37 entries in front
    of every fourth, so that blocks begin at odd offsets that are no multiple
    of 32; a block without entries behind every fifth; a last block of last_nr
    rows and 300 entries, its first and last row used.  lower=False: 300
    columns, every block in a range of at most 300; lower=True: square, lower
    triangular, row r's columns in [r - 200, r].  Every window stays under 512
    columns, the narrowest cap.  info: under = [(block, E, layout)], empty =
    the blocks without entries, starts = the first offset of every block under
    test."""
    rng = np.random.default_rng(900 + last_nr + (7 if lower else 0))
    lens, under, empty, b = [], [], [], 0
    for i in range(2 * len(RB_ENTRY_COUNTS)):
        j, second = i % len(RB_ENTRY_COUNTS), i >= len(RB_ENTRY_COUNTS)
        if i % 4 == 1:
            f = np.zeros(RB_ROWS, np.int64)
            np.add.at(f, rng.integers(0, RB_ROWS, 37), 1)
            lens.append(f)
            b += 1
        E, layout = RB_ENTRY_COUNTS[j], rb_layout_of(j, second)
        lens.append(_rb_row_lens(layout, E))
        under.append((b, E, layout))
        b += 1
        if i % 5 == 2:
            lens.append(np.zeros(RB_ROWS, np.int64))
            empty.append(b)
            b += 1
    tail = np.zeros(last_nr, np.int64)
    tail[0] = 37 if last_nr > 1 else RB_LAST_ENTRIES
    if last_nr > 2:
        tail[last_nr // 2] = 100
    tail[last_nr - 1] += RB_LAST_ENTRIES - tail.sum()
    lens = np.concatenate(lens + [tail])
    n_rows, nnz = lens.size, int(lens.sum())
    assert n_rows == b * RB_ROWS + last_nr and rb_blocks(n_rows) == b + 1
    row = _sorted_rows(lens)
    if lower:
        n_cols = n_rows
        col = row - (rng.integers(0, 201, nnz) % (row.astype(np.int64) + 1))
    else:
        n_cols = 300
        base, width = rng.integers(0, 100, b + 1), rng.integers(40, 200, b + 1)
        blk = row // RB_ROWS
        col = base[blk] + rng.integers(0, 1 << 30, nnz) % width[blk]
    m = _freeze(sa.Coo(n_rows, n_cols, row, col.astype(np.int32), rng.uniform(-1.0, 1.0, nnz), False,
                       f"row-block stream family, last block of {last_nr} rows{', lower triangle' if lower else ''}"))
    ptr = csr_of(m)[0]
    starts = [int(ptr[blk * RB_ROWS]) for blk, _, _ in under]
    for (blk, E, layout), s in zip(under, starts):
        assert ptr[(blk + 1) * RB_ROWS] - s == E
        assert np.array_equal(np.diff(ptr[blk * RB_ROWS:(blk + 1) * RB_ROWS + 1]), _rb_row_lens(layout, E))
    assert all(ptr[blk * RB_ROWS] == ptr[(blk + 1) * RB_ROWS] for blk in empty) and len(empty) >= 3
    assert ptr[n_rows] - ptr[b * RB_ROWS] == RB_LAST_ENTRIES and lens[b * RB_ROWS] > 0 and lens[-1] > 0
    assert sum(s % 2 == 1 and s % 32 != 0 for s in starts) >= 8 and starts[0] == 0
    assert {E for _, E, _ in under} == set(RB_ENTRY_COUNTS) and {E % 4 for E in RB_ENTRY_COUNTS} == {0, 1, 2, 3}
    for layout in RB_LAYOUTS:  # every layout in a block of at most one tail step and in one of whole unrolled steps
        es = [E for _, E, la in under if la == layout]
        assert min(es) <= K_BLOCK + 1 and max(es) > RB_STEP, (layout, es)
    assert any(la == "long" and E >= RB_LONG_ROW for _, E, la in under)
    win = sym_windows(n_rows, ptr, m.col) if lower else t_windows(n_rows, n_cols, ptr, m.col)
    span = win[:, 1] - win[:, 0] + 1
    assert span.max() < min(S_MULTI_CAP, T_MULTI_CAP) // max(T_WIDTHS) and (span[empty] == 0).all()
    if lower:
        assert (m.col <= m.row).all() and (m.col == m.row).any() and (m.col < m.row).any()
    assert 30_000 < nnz < 60_000
    return m, dict(under=tuple(under), empty=tuple(empty), starts=tuple(starts), last_nr=last_nr, windows=win)


# ------------------------------------------- references shared by the tests
def _int_block(seed: int, rows: int, bits: int) -> np.ndarray:
    return _signed_block(np.random.default_rng(seed), rows, bits)


def _signed_block(rng, rows, bits):
    return exact._signed_ints(rng, (rows, RB_KMAX), bits)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def transposed_case(m: sa.Coo, seed: int) -> dict:
    """Y = A^T X on m, both rules of tests/exact.py: the integer copy with an
    integer X[n_rows, 9] and its int64 reference; the wide-range copy with one
    x, its extended-precision reference and fp64 bound, column j of its X being
    RB_SCALES[j] x (exact scalings: reference and bound scale with them)."""
    e = exact.integerize(m, seed=seed)
    Xi = _int_block(seed + 1, m.n_rows, e.b)
    ref = exact.int_spmv(m.n_cols, m.col, m.row, e.m.val.astype(np.int64), Xi)
    assert (np.abs(ref) < (1 << 53)).all()
    mr, _, xt = exact.realize(m, seed=seed + 2)
    X = np.stack([s * xt for s in RB_SCALES], axis=1)
    Xf = Xi.astype(np.float64)
    _frozen(Xf, ref, X)
    return dict(mi=e.m, Xi=Xf, ref_i=ref, mr=mr, X=X, ref=exact.exact_reference(mr, xt, transpose=True),
                bound=exact.fp64_bound(mr, xt, transpose=True), a=e.a, b=e.b)


def symmetric_case(m: sa.Coo, seed: int) -> dict:
    """Y = (S + S^T - diag S) X on the half m: as transposed_case, the integer
    sizes taken from the expansion's longest row (test_symmetric.integer_half)
    and the reference and bound of the real copy from sa.expand_symmetric."""
    ex = exact.integerize(sa.expand_symmetric(m), seed)
    half = sa.Coo(m.n_rows, m.n_cols, m.row, m.col, np.array(ex.m.val[: m.nnz]), m.symmetric, m.label + " (integer)")
    ei = sa.expand_symmetric(half)
    Xi = _int_block(seed + 1, m.n_rows, ex.b)
    ref = exact.int_spmv(m.n_rows, ei.row, ei.col, ei.val.astype(np.int64), Xi)
    assert (np.abs(ei.val) < (1 << ex.a)).all() and (np.abs(ref) < (1 << 53)).all()
    rng = np.random.default_rng(seed + 2)
    mr = sa.Coo(m.n_rows, m.n_cols, m.row, m.col, exact.wide_range(rng, m.nnz), m.symmetric, m.label + " (wide range)")
    x = exact.wide_range(rng, m.n_cols)
    er = sa.expand_symmetric(mr)
    X = np.stack([s * x for s in RB_SCALES], axis=1)
    Xf = Xi.astype(np.float64)
    _frozen(half.val, Xf, ref, mr.val, X)
    return dict(mi=half, Xi=Xf, ref_i=ref, mr=mr, X=X, ref=exact.exact_reference(er, x), bound=exact.fp64_bound(er, x),
                a=ex.a, b=ex.b)


@functools.lru_cache(maxsize=None)
def stream_case(last_nr: int, lower: bool):
    """-> (info, transposed_case, symmetric_case or None) of rowblock_stream_matrix; made once."""
    m, info = rowblock_stream_matrix(last_nr, lower)
    seed = 500 + 10 * last_nr + (5 if lower else 0)
    return info, transposed_case(m, seed), symmetric_case(m, seed + 3) if lower else None


# ---------------------------------------------------- 2. the cap family
T_CAP_SPANS = tuple(s for c in (1024, 2048, 4096, 8192) for s in (c, c + 1))
S_CAP_SPANS = tuple(s for c in (512, 1024, 2048, 4096) for s in (c, c + 1))


def _spread(total: int, rows: int = RB_ROWS) -> np.ndarray:
    lens = np.full(rows, total // rows, np.int64)
    lens[: total % rows] += 1
    return lens


@functools.lru_cache(maxsize=None)
def rowblock_cap_matrix():
    """-> (matrix, info) for the transposed runs.  One block of 128 rows per
    span of T_CAP_SPANS (both sides of 8,192 / KV for KV = 8, 4, 2, 1 and of
    kTCap): `span` entries over the 128 rows (8,193: 64 a row, eight unrolled
    steps), their columns a permutation of [lo, lo + span), so every
    accumulator word is hit; lo = 61 per block further on, so neighbouring
    windows overlap and several workgroups add to the same outputs.  The wide
    and the narrow spans alternate; a block without entries and a last block of
    5 rows over 9 columns close the matrix.  info: under = [(block, span)],
    expect = what the plan must report (expected_transpose_info)."""
    rng = np.random.default_rng(911)
    order = (8193, 1024, 4097, 2048, 8192, 1025, 4096, 2049)
    assert sorted(order) == sorted(T_CAP_SPANS)
    lens, cols, under = [], [], []
    for b, span in enumerate(order):
        lens.append(_spread(span))
        cols.append(61 * b + rng.permutation(span))
        under.append((b, span))
    lens += [np.zeros(RB_ROWS, np.int64), np.array([3, 0, 4, 0, 5])]
    cols.append(5000 + rng.integers(0, 9, 12))
    cols[-1][:2] = (5000, 5008)
    lens, col = np.concatenate(lens), np.concatenate(cols)
    n_rows, n_cols = lens.size, 61 * len(order) + max(order) + 17
    m = _freeze(sa.Coo(n_rows, n_cols, _sorted_rows(lens), col.astype(np.int32), rng.uniform(-1.0, 1.0, col.size), False,
                       "row blocks spanning every transposed cap and one more column"))
    ptr = csr_of(m)[0]
    win = t_windows(n_rows, n_cols, ptr, m.col)
    span = win[:, 1] - win[:, 0] + 1
    assert [int(span[b]) for b, _ in under] == list(order) and span[len(order)] == 0 and span[-1] == 9
    for b, s in under:
        c = m.col[ptr[b * RB_ROWS]:ptr[(b + 1) * RB_ROWS]]
        assert np.array_equal(np.sort(c), win[b, 0] + np.arange(s))  # every column of the span, once
    assert all(win[b, 1] >= win[b + 1, 0] for b in range(len(order) - 1))  # neighbours overlap
    expect = expected_transpose_info(win)
    small = 1 + 0  # the 9-column last block fits every cap
    assert expect["lds_blocks"] == 3 + small and expect["flush_entries"] == 1024 + 1025 + 2048 + 9
    assert expect["multi_lds_blocks"] == [7 + small, 5 + small, 3 + small, 1 + small]
    assert expect["multi_widest"] == [8192, 4096, 2048, 1024]
    assert [t_multi_lds(w, s) for w, s in zip(T_WIDTHS, expect["multi_widest"])] == [67_600, 68_624, 70_672, 74_768]
    assert t_multi_lds(1, 8192) > 65_536  # more than the default dynamic LDS of a launch
    assert 30_000 < m.nnz < 40_000
    return m, dict(under=tuple(under), expect=expect, windows=win)


S_CAP_LOWER_AT = 40  # the first block of the lower-half forms: r0 = 5,120 >= 4,097 - 128
S_CAP_UPPER_AT = 1   # the first block of the upper-half forms
S_CAP_BLOCKS = 48    # full blocks; a diagonal-only block of S_CAP_LAST_ROWS rows follows
S_CAP_LAST_ROWS = 77
S_CAP_EMPTY = (20, 21)


@functools.lru_cache(maxsize=None)
def rowblock_sym_cap_matrix():
    """-> (half, info) for the symmetric runs; n = 48 * 128 + 77 = 6,221.  The
    union window of a block is its column range joined with its rows:
      lower forms  blocks 40..47, one per span of S_CAP_SPANS: every row its
                   diagonal entry, and the span - 128 columns [r0 + 128 - span,
                   r0) spread over the rows: the window ends on the block's
                   last row
      upper forms  blocks 1..8: the diagonal, and the columns [r0 + 128, r0 +
                   span) spread over the rows: the window starts exactly at r0
      the others   the diagonal only (span 128), blocks 20 and 21 nothing
      the last     77 rows, the diagonal only: the span equals nr
    Every word of every window is hit: the rows' words by their sums, the
    others as a mirrored column.  info: under = [(block, span, form)], expect =
    what the plan must report (expected_symmetric_info)."""
    rng = np.random.default_rng(913)
    n = S_CAP_BLOCKS * RB_ROWS + S_CAP_LAST_ROWS
    form = {S_CAP_LOWER_AT + i: (s, "lower") for i, s in enumerate(S_CAP_SPANS)}
    form.update({S_CAP_UPPER_AT + i: (s, "upper") for i, s in enumerate(S_CAP_SPANS)})
    rows, cols, under = [], [], []
    for b in range(rb_blocks(n)):
        if b in S_CAP_EMPTY:
            continue
        r0, nr = b * RB_ROWS, min(RB_ROWS, n - b * RB_ROWS)
        own = r0 + np.arange(nr)
        rows.append(own)
        cols.append(own)
        if b in form:
            span, kind = form[b]
            far = (r0 + RB_ROWS - span + np.arange(span - RB_ROWS)) if kind == "lower" else (r0 + RB_ROWS + np.arange(span - RB_ROWS))
            rows.append(r0 + np.repeat(np.arange(RB_ROWS), _spread(span - RB_ROWS)))
            cols.append(rng.permutation(far))
            under.append((b, span, kind))
    row, col = np.concatenate(rows), np.concatenate(cols)
    order = np.argsort(row, kind="stable")
    m = _freeze(sa.Coo(n, n, row[order].astype(np.int32), col[order].astype(np.int32), rng.uniform(-1.0, 1.0, row.size),
                       True, "union windows spanning every symmetric cap and one more column"))
    ptr = csr_of(m)[0]
    win = sym_windows(n, ptr, m.col)
    span = win[:, 1] - win[:, 0] + 1
    for b, s, kind in under:
        r0 = b * RB_ROWS
        assert span[b] == s and (win[b, 1] == r0 + RB_ROWS - 1 if kind == "lower" else win[b, 0] == r0), (b, s, kind)
        c = np.unique(m.col[ptr[r0]:ptr[r0 + RB_ROWS]])
        assert np.array_equal(c, win[b, 0] + np.arange(s))  # every column of the window
        mine = slice(ptr[r0], ptr[r0 + RB_ROWS])
        assert ((m.col[mine] <= m.row[mine]) if kind == "lower" else (m.col[mine] >= m.row[mine])).all()
    assert (span[list(S_CAP_EMPTY)] == 0).all() and span[-1] == S_CAP_LAST_ROWS
    rest = np.setdiff1d(np.arange(S_CAP_BLOCKS), [b for b, _, _ in under] + list(S_CAP_EMPTY))
    assert (span[rest] == RB_ROWS).all()
    expect = expected_symmetric_info(n, win)
    live = rb_blocks(n) - len(S_CAP_EMPTY)
    assert expect["window_blocks"] == live - 2 * 3  # 2,049, 4,096 and 4,097 in both forms are past kSCap
    assert expect["multi_window_blocks"] == [live - 2 * 1, live - 2 * 3, live - 2 * 5, live - 2 * 7]
    assert expect["multi_widest"] == [4096, 2048, 1024, 512]
    assert sym_multi_lds(1, 4096) == 66_576 > 65_536 and [sym_multi_lds(w, S_MULTI_CAP // w) for w in T_WIDTHS] == [66_576] * 4
    wide = sum(s > S_CAP for _, s, _ in under)
    assert expect["flush_entries"] == int(span[span <= S_CAP].sum()) + RB_ROWS * wide
    return m, dict(under=tuple(under), expect=expect, windows=win)


@functools.lru_cache(maxsize=None)
def cap_case():
    m, info = rowblock_cap_matrix()
    return info, transposed_case(m, 601)


@functools.lru_cache(maxsize=None)
def sym_cap_case():
    m, info = rowblock_sym_cap_matrix()
    return info, symmetric_case(m, 611)


# ------------------------------------------------- 3. the dropped family
DROP_PROBE_ROW = 5      # of the probe block: 10 entries, a dropped one, 9 more, lanes 0..19 of the block's first wave
DROP_WIDE_COLS = 50     # the wide blocks also hold columns [0, 50): unions past every cap
DROP_WIDE_AT = 66       # first of the two wide blocks: r0 = 8,448 > kTMultiCap


@functools.lru_cache(maxsize=None)
def rowblock_dropped_matrix():
    """-> (matrix with the dropped entries, the same matrix without them,
    info); both as row-sorted Coo, to be turned into CSR by csr_of (the host
    builders refuse such columns).  The valid matrix is the lower-triangular
    stream matrix with a last block of 127 rows, grown to n = 68 * 128 + 3:
      the probe block   (the first block behind the stream matrix) rows 0..4
                        empty, row 5 of 19 entries, rows of 64 behind it
      a block of        dropped entries only (nothing else in its 128 rows)
      two wide blocks   at rows 8,448 on: 1,025 entries near the diagonal and
                        in columns [0, 50), so their unions and column ranges
                        are wider than every cap of both families
    Added entries, columns -1, n and n + 1 in turn, never another value:
      - in the probe block, behind the 10th entry of row 5: the middle of a
        row, inside one wave
      - as the first and as the last entry of rows of a window block of the
        stream matrix, of the probe block and of both wide blocks, and in the
        middle of a long row of each
      - the block of nothing else.
    info: probe_row (global), dropped = their count, windows (symmetric union
    windows, unchanged by the added entries), wide = the wide blocks."""
    base, binfo = rowblock_stream_matrix(127, True)
    rng = np.random.default_rng(917)
    n = (DROP_WIDE_AT + 2) * RB_ROWS + 3
    first = rb_blocks(base.n_rows)
    probe, only = first, first + 1
    assert only < DROP_WIDE_AT - 1
    rows, cols = [base.row.astype(np.int64)], [base.col.astype(np.int64)]
    lens = np.zeros(RB_ROWS, np.int64)
    lens[DROP_PROBE_ROW] = 19
    lens[DROP_PROBE_ROW + 1:DROP_PROBE_ROW + 9] = K_WAVE
    r = probe * RB_ROWS + np.repeat(np.arange(RB_ROWS), lens)
    rows.append(r)
    cols.append(r - rng.integers(0, 150, r.size))
    for b in (DROP_WIDE_AT, DROP_WIDE_AT + 1):
        lens = _rb_row_lens("wave" if b == DROP_WIDE_AT else "long", 1025)
        r = b * RB_ROWS + np.repeat(np.arange(RB_ROWS), lens)
        c = np.where(rng.integers(0, 3, r.size) == 0, rng.integers(0, DROP_WIDE_COLS, r.size), r - rng.integers(0, 150, r.size))
        c[:2] = (0, r[1])
        rows.append(r)
        cols.append(c)
    row, col = np.concatenate(rows), np.concatenate(cols)
    order = np.argsort(row, kind="stable")
    row, col = row[order], col[order]
    val = rng.uniform(-1.0, 1.0, row.size)
    valid = sa.Coo(n, n, row.astype(np.int32), col.astype(np.int32), val, True, "the dropped family without its dropped entries")
    ptr = csr_of(valid)[0]
    bad_cols = (-1, n, n + 1)
    # (entry position the dropped entry goes in front of, its row)
    places = [(int(ptr[probe * RB_ROWS + DROP_PROBE_ROW]) + 10, probe * RB_ROWS + DROP_PROBE_ROW)]
    window_block = next(b for b, E, la in binfo["under"] if la == "wave" and E >= 2048)
    for b in (window_block, probe, DROP_WIDE_AT, DROP_WIDE_AT + 1):
        rws = b * RB_ROWS + np.flatnonzero(np.diff(ptr[b * RB_ROWS:(b + 1) * RB_ROWS + 1]) >= 19)
        for r in (int(rws[0]), int(rws[len(rws) // 2]), int(rws[-1])):
            if r == probe * RB_ROWS + DROP_PROBE_ROW:
                continue
            places += [(int(ptr[r]), r), (int(ptr[r + 1]), r), (int(ptr[r]) + int(ptr[r + 1] - ptr[r]) // 2, r)]
    pos = np.array([p for p, _ in places], np.int64)
    add_row = np.array([r for _, r in places], np.int64)
    add_col = np.array([bad_cols[i % 3] for i in range(len(places))], np.int64)
    add_val = rng.uniform(1.0, 2.0, len(places))
    row_d, col_d, val_d = (np.insert(a, pos, v) for a, v in ((row, add_row), (col, add_col), (val, add_val)))
    lens = np.zeros(RB_ROWS, np.int64)  # the block of dropped entries only: 300 over a few rows
    lens[[0, 3, 64, 127]] = (1, 70, 129, 100)
    r = only * RB_ROWS + np.repeat(np.arange(RB_ROWS), lens)
    at = int(np.searchsorted(row_d, only * RB_ROWS))
    row_d = np.insert(row_d, at, r)
    col_d = np.insert(col_d, at, np.array(bad_cols)[np.arange(r.size) % 3])
    val_d = np.insert(val_d, at, rng.uniform(1.0, 2.0, r.size))
    assert (np.diff(row_d) >= 0).all()
    with_d = sa.Coo(n, n, row_d.astype(np.int32), col_d.astype(np.int32), val_d, True, "valid entries and columns -1, n, n + 1")
    _freeze(valid)
    _freeze(with_d)
    out = (with_d.col < 0) | (with_d.col >= n)
    assert set(np.unique(with_d.col[out]).tolist()) == set(bad_cols) and out.sum() == len(places) + 300
    for a, b_ in ((with_d.row[~out], valid.row), (with_d.col[~out], valid.col), (with_d.val[~out], valid.val)):
        assert np.array_equal(a, b_)  # without them: the valid matrix, entry for entry
    ptr_d = csr_of(with_d)[0]
    pr = probe * RB_ROWS + DROP_PROBE_ROW
    assert ptr_d[pr] == ptr_d[probe * RB_ROWS] and ptr_d[pr + 1] - ptr_d[pr] == 20 and out[ptr_d[pr] + 10]
    assert not out[ptr_d[pr]:ptr_d[pr] + 10].any() and not out[ptr_d[pr] + 11:ptr_d[pr] + 20].any()
    win = sym_windows(n, ptr_d, with_d.col)
    assert np.array_equal(win, sym_windows(n, ptr, valid.col)) and np.array_equal(
        t_windows(n, n, ptr_d, with_d.col), t_windows(n, n, ptr, valid.col))
    span = win[:, 1] - win[:, 0] + 1
    assert span[only] == 0 and ptr_d[(only + 1) * RB_ROWS] - ptr_d[only * RB_ROWS] == 300
    wide = (DROP_WIDE_AT, DROP_WIDE_AT + 1)
    tspan = np.diff(t_windows(n, n, ptr_d, with_d.col), axis=1)[:, 0] + 1
    assert (span[list(wide)] > T_MULTI_CAP).all() and (tspan[list(wide)] > T_MULTI_CAP).all()
    assert span[window_block] < S_MULTI_CAP // 8 and span[probe] < S_MULTI_CAP // 8
    for b in (window_block, probe) + wide:  # each holds a first, a last and a middle dropped entry of a row
        blk = slice(ptr_d[b * RB_ROWS], ptr_d[(b + 1) * RB_ROWS])
        assert out[blk].sum() >= 3
    return with_d, valid, dict(probe_row=pr, dropped=int(out.sum()), windows=win, wide=wide, only=only,
                               window_block=window_block)


@functools.lru_cache(maxsize=None)
def dropped_case():
    """-> (info, (ptr, col, val) per copy with the dropped entries, the cases of
    the valid matrix).  The integer and the real copy of the matrix WITH the
    dropped entries take the valid copy's values at the valid entries and 3.0
    (integer) or the constructor's values (real) at the dropped ones."""
    with_d, valid, info = rowblock_dropped_matrix()
    t, s = transposed_case(valid, 631), symmetric_case(valid, 641)
    out = (with_d.col < 0) | (with_d.col >= with_d.n_cols)
    ptr = csr_of(with_d)[0]

    def arrays(vals, fill):
        v = np.where(out, fill, 0.0)
        v[~out] = vals
        return _frozen(ptr, with_d.col, v)

    csr = {("t", True): arrays(t["mi"].val, 3.0), ("t", False): arrays(t["mr"].val, with_d.val),
           ("s", True): arrays(s["mi"].val, 3.0), ("s", False): arrays(s["mr"].val, with_d.val)}
    return info, csr, t, s
