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

Neither needs a GPU.  The matrices are made once per argument set and never
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
