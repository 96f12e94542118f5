"""Two order-independent checks of an SpMV result: TEST INFRASTRUCTURE ONLY.

oracle.parity(rel=1e-6) is the reference project's acceptance rule; for an
fp64 kernel it is nine to ten orders of magnitude looser than what a correct
kernel delivers, and no relative rule can see a dropped entry whose product
is small against its row.  The two checks here close that gap without
depending on any summation order:

  exact    integerize() gives the matrix small signed integer values and an
           integer x, sized so that every product and every partial sum, in
           ANY order, is an integer below 2^52: fp64 (and the fp32-value
           path) computes it without a single rounding, and the result must
           EQUAL an int64 reference.  A dropped, duplicated or misattributed
           entry, however small, changes the integer.
  bounded  on real data |y_i - ref_i| <= (n_i + 2) * 2^-53 * sum_j |a_ij x_j|,
           the textbook forward-error bound of n_i rounded products summed in
           any order (n_i - 1 additions and one product rounding per term:
           gamma_n <= n u to first order; the + 2 covers the rounding of the
           magnitude itself and of the reference).  No measured constant.
           A value, product or partial sum that passes through fp32 misses it
           by about eight orders of magnitude.

The references never touch the oracle: int64 arithmetic for the first,
extended precision (or an error-free float64 expansion) for the second.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

import spmv_amd as sa

U = 2.0 ** -53  # unit roundoff of fp64


@dataclass
class Exact:
    m: sa.Coo            # the matrix with integer values (float64 storage)
    x: np.ndarray        # float64 (n_cols,) or (n_cols, k): integer-valued forward input
    xt: np.ndarray       # float64 (n_rows,): integer-valued input of the transposed product
    ref: np.ndarray      # int64 (n_rows,) or (n_rows, k): A x
    ref_t: np.ndarray    # int64 (n_cols,): A^T xt
    a: int               # |value| < 2^a
    b: int               # |x| < 2^b


def _signed_ints(rng, shape, bits):
    """Non-zero signed integers |v| < 2^bits, a random bit length per entry
    (so small magnitudes sit next to large ones)."""
    length = rng.integers(1, bits + 1, shape)               # 1..bits
    lo = np.left_shift(np.int64(1), length - 1)             # 2^(length-1)
    mag = lo + (rng.integers(0, 1 << 62, shape) % lo)       # [2^(length-1), 2^length)
    return np.where(rng.integers(0, 2, shape) == 1, -mag, mag).astype(np.int64)


def int_spmv(n_out, out_idx, in_idx, val_i, x_i):
    """y[out] += val * x[in] in int64 (x_i 1-D or 2-D)."""
    y = np.zeros((n_out,) + x_i.shape[1:], np.int64)
    np.add.at(y, out_idx, val_i * x_i[in_idx] if x_i.ndim == 1 else val_i[:, None] * x_i[in_idx])
    return y


def integerize(m: sa.Coo, seed: int, k: int = 1) -> Exact:
    """A copy of m with signed non-zero integer values |v| < 2^a, integer inputs
    |x| < 2^b and int64 references, where a <= 23 (exact in fp32 too) and
    a + b + ceil(log2(longest row or column + 1)) <= 52: every product and
    every partial sum of A x, A X and A^T x, in any order, is exact in fp64."""
    rng = np.random.default_rng(seed)
    longest = 0
    if m.nnz:
        longest = int(max(np.bincount(m.row, minlength=1).max(), np.bincount(m.col, minlength=1).max()))
    c = math.ceil(math.log2(longest + 1))
    assert (1 << c) >= longest + 1
    budget = 52 - c
    a = min(23, budget // 2)
    b = budget - a
    assert a >= 8 and b >= 8, (a, b, longest)
    assert a + b + c <= 52 and a <= 23
    val_i = _signed_ints(rng, m.nnz, a)
    x_i = _signed_ints(rng, (m.n_cols,) if k == 1 else (m.n_cols, k), b)
    xt_i = _signed_ints(rng, m.n_rows, b)
    assert np.all(val_i != 0) and np.all(x_i != 0) and np.all(xt_i != 0)
    assert (np.abs(val_i) < (1 << a)).all() and (np.abs(x_i) < (1 << b)).all() and (np.abs(xt_i) < (1 << b)).all()
    ref = int_spmv(m.n_rows, m.row, m.col, val_i, x_i)
    ref_t = int_spmv(m.n_cols, m.col, m.row, val_i, xt_i)
    assert (np.abs(ref) < (1 << 53)).all() and (np.abs(ref_t) < (1 << 53)).all()
    mi = sa.Coo(m.n_rows, m.n_cols, m.row, m.col, val_i.astype(np.float64), m.symmetric, m.label + " (integer)")
    out = Exact(mi, x_i.astype(np.float64), xt_i.astype(np.float64), ref, ref_t, a, b)
    for arr in (mi.val, out.x, out.xt, ref, ref_t):
        arr.setflags(write=False)
    return out


def exact_bad_rows(y, ref_int):
    """Rows where y != ref (value comparison: -0.0 equals 0.0; NaN never equal)."""
    y = np.asarray(y)
    want = np.asarray(ref_int).astype(np.float64)
    assert y.shape == want.shape, (y.shape, want.shape)
    bad = ~(y == want)
    return np.nonzero(bad if bad.ndim == 1 else bad.any(axis=1))[0]


def assert_exact(y, ref_int, what=""):
    y = np.asarray(y)
    want = np.asarray(ref_int).astype(np.float64)
    assert y.shape == want.shape, (what, y.shape, want.shape)
    nan = np.isnan(y)
    assert not nan.any(), f"{what}: NaN left in y, first at {np.argwhere(nan)[:5].tolist()}"
    if np.array_equal(y, want):
        return
    bad = exact_bad_rows(y, ref_int)
    f = bad[:5]
    raise AssertionError(f"{what}: {bad.size} rows differ from the int64 reference, first {f.tolist()}: "
                         f"got {y[f].tolist()} want {want[f].tolist()} difference {(y[f] - want[f]).tolist()}")


# ------------------------------------------------------------ the matrices
GENERATED = ("ragged", "cantlike", "rmat", "empty_runs", "odd", "one_row")


@functools.lru_cache(maxsize=None)
def generated(key: str) -> sa.Coo:
    """The smallest matrices at which each kernel path's edges still occur."""
    if key == "ragged":  # long ragged rows, x windows that do not fit, carries
        return sa.gen_random(4_000, 50_000, 0, 2_000, seed=21)
    if key == "cantlike":  # the small-matrix SELL kernel, head copies, x windows, CSR16 / SELL16
        return sa.gen_cantlike(0)
    if key == "rmat":  # tiled CSR / COO / CMRS, hot-column tables, hub rows over many tiles, empty rows
        return sa.gen_rmat(100_000, 1_000_000, scale=17, seed=1)
    if key == "empty_runs":  # big-tile plans, the bitmap zero fill
        from test_gpu_parity import _empty_run_matrix

        return _empty_run_matrix()[0]
    if key == "odd":  # an odd entry count: the array's lone last entry
        m = sa.gen_rmat(30_000, 299_999, scale=15, seed=4)
        assert m.nnz % 2 == 1
        return m
    if key == "one_row":  # 3 rows, one of 20,001 entries: carries across many tiles
        rng = np.random.default_rng(5)
        return sa.Coo(3, 5_000, np.full(20_001, 1, np.int32), rng.integers(0, 5_000, 20_001).astype(np.int32),
                      rng.uniform(-1, 1, 20_001), False, "one row of 20,001 entries")
    raise KeyError(key)


# ---------------------------------------------------------------- real data
def _segments(idx, n_out):
    """Stable order by output index, start of every non-empty segment, counts."""
    order = np.argsort(idx, kind="stable")
    counts = np.bincount(idx, minlength=n_out)[:n_out] if idx.size else np.zeros(n_out, np.int64)
    starts = np.concatenate(([0], np.cumsum(counts)[:-1])) if n_out else np.zeros(0, np.int64)
    return order, starts.astype(np.int64), counts.astype(np.int64)


def _io(m, transpose):
    return (m.n_cols, m.col, m.row) if transpose else (m.n_rows, m.row, m.col)


def _reference_longdouble(m, x, transpose):
    n_out, oi, ii = _io(m, transpose)
    order, starts, counts = _segments(oi, n_out)
    ref = np.zeros(n_out, np.longdouble)
    if oi.size:
        p = m.val.astype(np.longdouble)[order] * np.asarray(x, np.float64).astype(np.longdouble)[ii[order]]
        ne = counts > 0
        ref[ne] = np.add.reduceat(p, starts[ne])
    return ref


def _two_product(a, b):
    """Error-free a*b = p + e in float64 (Veltkamp split, Dekker product)."""
    p = a * b
    f = 134217729.0  # 2^27 + 1
    ah = a * f
    ah = ah - (ah - a)
    al = a - ah
    bh = b * f
    bh = bh - (bh - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _reference_fsum(m, x, transpose):
    """The error-free route: every product split into p + e exactly, each row
    summed by math.fsum (correctly rounded)."""
    n_out, oi, ii = _io(m, transpose)
    order, starts, counts = _segments(oi, n_out)
    ref = np.zeros(n_out, np.float64)
    if oi.size:
        p, e = _two_product(m.val[order], np.asarray(x, np.float64)[ii[order]])
        for i in np.nonzero(counts)[0]:
            s, t = starts[i], starts[i] + counts[i]
            ref[i] = math.fsum(np.concatenate((p[s:t], e[s:t])).tolist())
    return ref


def exact_reference(m: sa.Coo, x, transpose: bool = False):
    """A x (or A^T x) to far below fp64_bound: extended precision where the
    platform's long double carries a 64-bit significand (error <= about
    n 2^-64 of the magnitude, 2^-11 of the bound), else correctly rounded."""
    if np.finfo(np.longdouble).nmant >= 63:
        return _reference_longdouble(m, x, transpose)
    return _reference_fsum(m, x, transpose)


def fp64_bound(m: sa.Coo, x, transpose: bool = False):
    """(n_i + 2) * 2^-53 * sum_j |a_ij x_j| per output row."""
    n_out, oi, ii = _io(m, transpose)
    n_i = np.bincount(oi, minlength=n_out)[:n_out] if oi.size else np.zeros(n_out, np.int64)
    mag = np.bincount(oi, weights=np.abs(m.val * np.asarray(x, np.float64)[ii]), minlength=n_out)[:n_out] \
        if oi.size else np.zeros(n_out)
    return (n_i + 2) * U * mag


def fp64_ratio(y, ref, bound):
    """(rows over the bound, largest error / bound over rows with a bound > 0)."""
    y = np.asarray(y, np.float64)
    assert y.shape == ref.shape == bound.shape, (y.shape, ref.shape, bound.shape)
    err = np.abs(y.astype(ref.dtype) - ref).astype(np.float64)
    bad = np.nonzero(~(err <= bound))[0]
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    return bad, worst


def assert_fp64(y, m: sa.Coo, x, transpose: bool = False, ref=None, bound=None, what=""):
    """|y - ref| <= bound on every row; returns the largest error / bound."""
    ref = exact_reference(m, x, transpose) if ref is None else ref
    bound = fp64_bound(m, x, transpose) if bound is None else bound
    y = np.asarray(y, np.float64)
    bad, worst = fp64_ratio(y, ref, bound)
    if bad.size:
        f = bad[:5]
        raise AssertionError(f"{what}: {bad.size} rows over the fp64 bound, first {f.tolist()}: got {y[f].tolist()} "
                             f"want {ref[f].astype(np.float64).tolist()} error "
                             f"{np.abs(y[f] - ref[f]).astype(np.float64).tolist()} bound {bound[f].tolist()}")
    return worst


def rounded_f32(m: sa.Coo) -> sa.Coo:
    """The matrix the fp32-value path (csrf32) stores: values rounded to fp32."""
    return sa.Coo(m.n_rows, m.n_cols, m.row, m.col, m.val.astype(np.float32).astype(np.float64), m.symmetric, m.label)


def wide_range(rng, shape):
    """uniform(-1, 1) * 2^randint(-30, 30): a wide dynamic range."""
    return rng.uniform(-1.0, 1.0, shape) * np.exp2(rng.integers(-30, 31, shape).astype(np.float64))


def realize(m: sa.Coo, seed: int):
    """-> (matrix with wide-range real values, x[n_cols], xt[n_rows])."""
    rng = np.random.default_rng(seed)
    mr = sa.Coo(m.n_rows, m.n_cols, m.row, m.col, wide_range(rng, m.nnz), m.symmetric, m.label + " (wide range)")
    x, xt = wide_range(rng, m.n_cols), wide_range(rng, m.n_rows)
    for arr in (mr.val, x, xt):
        arr.setflags(write=False)
    return mr, x, xt
