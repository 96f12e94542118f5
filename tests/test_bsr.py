"""Block CSR on the host (no GPU): sa.bsr_build (spmv_bsr_plan / spmv_bsr_fill)
and sa.cpu_bsr (spmv_cpu_bsr) over the golden fixtures for b = 1..8, sizes that
are no multiple of b, the exact-integer and fp64-bound checks of tests/exact.py,
every refusal the header lists, the byte table of the cant-like matrix and
to_device's fill rule."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import exact
import spmv_amd as sa
from conftest import GOLDEN, golden_cases

CASES = [c["name"] for c in golden_cases()]
BS = tuple(range(1, sa.BSR_MAX_B + 1))


@functools.lru_cache(maxsize=None)
def matrix(key):
    if key == "random301":  # 301 rows: no multiple of 2, 3 or 4; 500 columns: none of 3
        return sa.gen_random(301, 500, 0, 60)
    if key == "random503":  # neither size is a multiple of 2, 3 or 4
        return sa.gen_random(301, 503, 0, 60, seed=2)
    if key == "two_rows":  # fewer rows than a block is high
        return sa.Coo(2, 7, np.array([0, 1, 1, 0], np.int32), np.array([6, 0, 6, 3], np.int32),
                      np.array([1.5, -2.0, 0.25, 4.0]), False, "2 x 7")
    return sa.read_mtx(GOLDEN / f"{key}.mtx")


def build(m, b):
    ptr, col, val = sa.csr_from_coo(m)
    return sa.bsr_build(m.n_rows, m.n_cols, ptr, col, val, b), (ptr, col, val)


def run_cpu(m, b, x):
    s, _ = build(m, b)
    y = np.full(max(m.n_rows, 1), np.nan)
    sa.cpu_bsr(m.n_rows, m.n_cols, b, s["brow_ptr"], s["bcol"], s["bval"], np.ascontiguousarray(x), y)
    return y[: m.n_rows]


def test_sizes_are_no_multiples():
    m = matrix("random301")
    assert all(m.n_rows % b for b in (2, 3, 4)) and m.n_cols % 3
    m = matrix("random503")
    assert all(m.n_rows % b and m.n_cols % b for b in (2, 3, 4))


@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("case", CASES + ["random301", "random503", "two_rows"])
def test_build_reproduces_the_csr(case, b):
    m = matrix(case)
    s, (ptr, col, val) = build(m, b)
    n_brows, n_blocks = s["n_brows"], s["n_blocks"]
    assert n_brows == -(-m.n_rows // b)
    bp, bc, bv = s["brow_ptr"], s["bcol"], s["bval"].reshape(n_blocks, b, b)
    assert bp.dtype == np.int64 and bc.dtype == np.int32 and bp.shape == (n_brows + 1,) and bc.shape == (n_blocks,)
    assert bp[0] == 0 and bp[-1] == n_blocks and (np.diff(bp) >= 0).all()
    # the counts of spmv_bsr_plan are the fill's: distinct (block row, block column) pairs
    pairs = np.unique(np.stack([m.row // b, m.col // b], axis=1), axis=0) if m.nnz else np.zeros((0, 2), np.int64)
    assert n_blocks == len(pairs)
    brow = np.repeat(np.arange(n_brows), np.diff(bp))
    # strictly ascending inside a block row, hence exactly the sorted distinct pairs
    assert np.array_equal(np.stack([brow, bc], axis=1), pairs)
    # scattered back, duplicates summed in CSR order: the CSR itself
    want = np.zeros((n_blocks, b, b))
    slot = {(int(i), int(j)): k for k, (i, j) in enumerate(pairs)}
    rows = np.repeat(np.arange(m.n_rows), np.diff(ptr))
    filled = np.zeros((n_blocks, b, b), bool)
    for r, c, v in zip(rows, col, val):
        k = slot[(r // b, c // b)]
        want[k, r % b, c % b] += v
        filled[k, r % b, c % b] = True
    assert np.array_equal(bv, want)
    # padding slots and slots outside the matrix: +0.0 bit for bit
    assert (bv[~filled].view(np.uint64) == 0).all()
    rr = brow[:, None, None] * b + np.arange(b)[None, :, None] + np.zeros((1, 1, b), np.int64)
    cc = bc.astype(np.int64)[:, None, None] * b + np.arange(b)[None, None, :] + np.zeros((1, b, 1), np.int64)
    assert not filled[(rr >= m.n_rows) | (cc >= m.n_cols)].any()
    assert s["fill"] == (n_blocks * b * b / m.nnz if m.nnz else 0.0)


@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("case", CASES + ["random301", "random503", "two_rows"])
def test_cpu_bsr_exact_on_integer_data(case, b):
    e = exact.integerize(matrix(case), seed=7)
    exact.assert_exact(run_cpu(e.m, b, e.x), e.ref, f"cpu_bsr {case} b={b}")


@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("case", CASES + ["random301", "random503", "two_rows"])
def test_cpu_bsr_within_the_fp64_bound(case, b):
    mr, x, _ = exact.realize(matrix(case), seed=107)
    exact.assert_fp64(run_cpu(mr, b, x), mr, x, what=f"cpu_bsr {case} b={b}")


def test_cpu_bsr_leaves_the_flanks_alone():
    """y past n_rows is not written and x past n_cols is not read (NaN there
    would reach a row through a partial last block column)."""
    m = matrix("random503")
    e = exact.integerize(m, seed=3)
    for b in BS:
        s, _ = build(e.m, b)
        x = np.full(m.n_cols + b, np.nan)
        x[: m.n_cols] = e.x
        y = np.full(m.n_rows + b, -7.0)
        sa.cpu_bsr(m.n_rows, m.n_cols, b, s["brow_ptr"], s["bcol"], s["bval"], x, y)
        exact.assert_exact(y[: m.n_rows], e.ref, f"b={b}")
        assert (y[m.n_rows:] == -7.0).all()


def test_refusals():
    L, P = sa.host_lib(), sa._ptr
    m = matrix("n67")
    ptr, col, val = sa.csr_from_coo(m)
    nbr, nbl = ctypes.c_int64(-5), ctypes.c_int64(-5)
    out = (ctypes.byref(nbr), ctypes.byref(nbl))

    def plan(n_rows=m.n_rows, n_cols=m.n_cols, p=P(ptr), c=P(col), b=3, o=out):
        return L.spmv_bsr_plan(n_rows, n_cols, p, c, b, *o)

    assert plan() == sa.SUCCESS
    nbr.value = nbl.value = -5
    bad_col = col.copy()
    bad_col[-1] = m.n_cols
    neg_col = col.copy()
    neg_col[0] = -1
    for kw in (dict(b=0), dict(b=sa.BSR_MAX_B + 1), dict(n_rows=-1), dict(n_cols=-1), dict(n_cols=2**31 - 8),
               dict(c=P(bad_col)), dict(c=P(neg_col)), dict(p=None), dict(c=None), dict(o=(None, ctypes.byref(nbl))),
               dict(o=(ctypes.byref(nbr), None))):
        assert plan(**kw) == sa.OTHER_ERROR, kw
    assert (nbr.value, nbl.value) == (-5, -5)  # nothing written

    s = sa.bsr_build(m.n_rows, m.n_cols, ptr, col, val, 3)
    bp, bc, bv = (np.full_like(s[k], 99) for k in ("brow_ptr", "bcol", "bval"))

    def fill(n_rows=m.n_rows, n_cols=m.n_cols, p=P(ptr), c=P(col), v=P(val), b=3, o=(P(bp), P(bc), P(bv))):
        return L.spmv_bsr_fill(n_rows, n_cols, p, c, v, b, *o)

    for kw in (dict(b=0), dict(b=9), dict(n_rows=-1), dict(n_cols=-1), dict(n_cols=2**31 - 8), dict(c=P(bad_col)),
               dict(c=P(neg_col)), dict(p=None), dict(c=None), dict(v=None), dict(o=(None, P(bc), P(bv))),
               dict(o=(P(bp), None, P(bv))), dict(o=(P(bp), P(bc), None))):
        assert fill(**kw) == sa.OTHER_ERROR, kw
    assert (bp == 99).all() and (bc == 99).all() and (bv == 99).all()  # nothing written
    assert fill() == sa.SUCCESS and np.array_equal(bp, s["brow_ptr"]) and np.array_equal(bv, s["bval"])

    x, y = np.ones(m.n_cols), np.full(m.n_rows, -7.0)

    def cpu(n_rows=m.n_rows, n_cols=m.n_cols, b=3, n_brows=s["n_brows"], a=(P(bp), P(bc), P(bv)), xx=P(x), yy=P(y)):
        return L.spmv_cpu_bsr(n_rows, n_cols, b, n_brows, *a, xx, yy)

    far = bc.copy()
    far[-1] = -(-m.n_cols // 3)
    for kw in (dict(b=0), dict(b=9), dict(n_rows=-1), dict(n_cols=-1), dict(n_brows=s["n_brows"] + 1),
               dict(n_cols=2**31 - 8), dict(a=(None, P(bc), P(bv))), dict(a=(P(bp), None, P(bv))),
               dict(a=(P(bp), P(bc), None)), dict(a=(P(bp), P(far), P(bv))), dict(xx=None), dict(yy=None)):
        assert cpu(**kw) == sa.OTHER_ERROR, kw
    assert (y == -7.0).all()
    assert cpu() == sa.SUCCESS and not (y == -7.0).all()
    with pytest.raises(sa.SpmvError):
        sa.bsr_build(m.n_rows, m.n_cols, ptr, col, val, 9)


@functools.lru_cache(maxsize=None)
def cantlike_bsr(b):
    m = exact.generated("cantlike")
    return m, build(m, b)[0]


@pytest.mark.parametrize("b,blocks", [(2, 1_336_178), (3, 480_625), (4, 462_393)])
def test_cantlike_byte_table(b, blocks):
    """The table of profiles/bsr/README.md: byte counts, computed here."""
    m, s = cantlike_bsr(b)
    assert (m.n_rows, m.nnz) == (62_451, 4_007_383)
    assert s["n_blocks"] == blocks
    csr = 12 * m.nnz + 8 * (m.n_rows + 1)
    assert csr == 48_588_212
    want = {2: (5_344_712, 48_352_224), 3: (4_325_625, 36_694_044), 4: (7_398_288, 61_160_788)}[b]
    assert (blocks * b * b, sa.bsr_stored_bytes(s)) == want
    assert round(s["fill"], 3) == {2: 1.334, 3: 1.079, 4: 1.846}[b]


def test_fill_rule():
    """bsr_max_fill=None accepts what stores fewer bytes than CSR: the
    cant-like matrix at b = 3 (and, by 0.5 %, at b = 2), not at b = 4, and
    not the tiny fixtures, whose few entries sit alone in their blocks."""
    for b, ok in ((2, True), (3, True), (4, False)):
        m, s = cantlike_bsr(b)
        if ok:
            sa.bsr_check_fill(m.n_rows, m.nnz, s)
        else:
            with pytest.raises(sa.SpmvError, match="not fewer than CSR"):
                sa.bsr_check_fill(m.n_rows, m.nnz, s)
        sa.bsr_check_fill(m.n_rows, m.nnz, s, float("inf"))
        with pytest.raises(sa.SpmvError, match="fill"):
            sa.bsr_check_fill(m.n_rows, m.nnz, s, 1.0)
    # to_device refuses before anything is uploaded (no GPU needed to see it)
    for case in ("colmajor", "n67", "ragged_shuffled"):
        with pytest.raises(sa.SpmvError, match="not fewer than CSR"):
            sa.to_device(matrix(case), "bsr", "cuda:0", block=3)
    for block in (1, 5, 8, True, 3.0):
        with pytest.raises(sa.SpmvError, match="block must be 2, 3 or 4"):
            sa.to_device(matrix("n67"), "bsr", "cuda:0", block=block)
    assert sa.BLOCK_FORMATS == ("bsr",) and "bsr" not in sa.ALL_FORMATS


def test_build_operator_refuses_an_align_that_cuts_block_rows():
    """Several ranks: each blocks its own shard, so align must be a multiple
    of the block size; refused before anything is uploaded."""
    import iterate as it

    m = matrix("n67")
    with pytest.raises(sa.SpmvError, match="align=1024 must be a multiple of the block size"):
        it.build_operator(m, 0, 2, "bsr", "cuda:0", block=3, bsr_max_fill=float("inf"))
    with pytest.raises(sa.SpmvError, match="align=6 must be a multiple"):
        it.build_operator(m, 1, 2, "bsr", "cuda:0", align=6, block=4, bsr_max_fill=float("inf"))
