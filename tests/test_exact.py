"""The exact-integer and fp64-bound checks of tests/exact.py over the host
library's CPU loops and the oracle's file-order sum (no GPU), and the proof
that both checks can fail.

Matrices: every golden fixture and the generated matrices of exact.GENERATED
(the ones tests/test_exact_gpu.py runs the kernels on).  Per matrix one
integer copy (values, a 3-column X, the transposed input, int64 references)
and one wide-range real copy with its extended-precision references, shared
by every loop.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import exact
import spmv_amd as sa
from conftest import GOLDEN, golden_cases
from oracle import oracle

CASES = [c["name"] for c in golden_cases()]
KEYS = CASES + list(exact.GENERATED)
LOOPS = ("coo", "csr", "ell", "sell", "cmrs", "csr_multi", "csr_t", "oracle")
K = 3


def matrix(key):
    return exact.generated(key) if key in exact.GENERATED else sa.read_mtx(GOLDEN / f"{key}.mtx")


@functools.lru_cache(maxsize=None)
def integer_case(key):
    return exact.integerize(matrix(key), seed=KEYS.index(key), k=K)


@functools.lru_cache(maxsize=None)
def real_case(key):
    mr, x, xt = exact.realize(matrix(key), seed=100 + KEYS.index(key))
    fwd = (exact.exact_reference(mr, x), exact.fp64_bound(mr, x))
    tr = (exact.exact_reference(mr, xt, transpose=True), exact.fp64_bound(mr, xt, transpose=True))
    return mr, x, xt, fwd, tr


def run_loop(loop, m, x, generated=False):
    """y of one CPU loop over m (x: (n_cols,), for csr_multi (n_cols, k), for
    csr_t (n_rows,)); y starts as NaN."""
    L = sa.host_lib()
    P = sa._ptr
    if loop == "oracle":
        return oracle.file_order_spmv(m.n_rows, m.row, m.col, m.val, x)
    ptr, col, val = sa.csr_from_coo(m)
    x = np.ascontiguousarray(x)
    if loop == "csr_t":
        y = np.full(max(m.n_cols, 1), np.nan)
        sa.cpu_csr_t(m.n_rows, m.n_cols, ptr, col, val, x, y)
        return y[: m.n_cols]
    if loop == "csr_multi":
        Y = np.full((max(m.n_rows, 1), x.shape[1]), np.nan)
        sa.cpu_csr_multi(m.n_rows, ptr, col, val, x, Y)
        return Y[: m.n_rows]
    y = np.full(max(m.n_rows, 1), np.nan)
    if loop == "coo":
        r, c, v = sa.coo_sort_by_row(m)
        rc = L.spmv_cpu_coo(m.n_rows, m.nnz, P(r), P(c), P(v), P(x), P(y), 2)
    elif loop == "csr":
        rc = L.spmv_cpu_csr(m.n_rows, P(ptr), P(col), P(val), P(x), P(y), 2)
    elif loop == "ell":
        e = sa.ell_build(m.n_rows, ptr, col, val, ki=2, max_padding=64.0 if generated else None)
        rc = L.spmv_cpu_ell(m.n_rows, e["K"], e["ld"], e["ki"], P(e["col"]), P(e["val"]), P(x), P(y), 2)
    elif loop == "sell":
        s = sa.sell_build(m.n_rows, ptr, col, val, C=64, sigma=1024, ki=2)
        rc = L.spmv_cpu_sell(m.n_rows, s["C"], s["ki"], s["n_slices"], P(s["slice_ptr"]), P(s["perm"]), P(s["col"]),
                             P(s["val"]), P(x), P(y), 2)
    else:
        c = sa.cmrs_build(m.n_rows, ptr, h=8)
        rc = L.spmv_cpu_cmrs(m.n_rows, c["h"], c["n_strips"], P(c["strip_ptr"]), P(c["row_in_strip"]), P(col), P(val),
                             P(x), P(y), 2)
    assert rc == sa.SUCCESS
    return y[: m.n_rows]


ELL_REFUSED = {"rmat", "empty_runs", "odd", "one_row"}  # padding factor over 64, as on the GPU


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("loop", LOOPS)
def test_cpu_loop_exact_and_bounded(loop, key):
    gen = key in exact.GENERATED
    if loop == "ell" and key in ELL_REFUSED:
        with pytest.raises(sa.SpmvError):
            run_loop(loop, integer_case(key).m, integer_case(key).x[:, 0], generated=True)
        return
    e = integer_case(key)
    mr, x, xt, (ref, bound), (ref_t, bound_t) = real_case(key)
    what = f"{loop} on {key}"
    if loop == "csr_t":
        exact.assert_exact(run_loop(loop, e.m, e.xt), e.ref_t, what)
        exact.assert_fp64(run_loop(loop, mr, xt), mr, xt, transpose=True, ref=ref_t, bound=bound_t, what=what)
    elif loop == "csr_multi":
        exact.assert_exact(run_loop(loop, e.m, e.x), e.ref, what)
        Y = run_loop(loop, mr, np.stack([x, -x, 2.0 * x], axis=1))  # exact scalings: the references scale with them
        for j, s in enumerate((1.0, -1.0, 2.0)):
            exact.assert_fp64(Y[:, j], mr, x, ref=s * ref, bound=abs(s) * bound, what=f"{what} column {j}")
    else:
        exact.assert_exact(run_loop(loop, e.m, e.x[:, 0], gen), e.ref[:, 0], what)
        exact.assert_fp64(run_loop(loop, mr, x, gen), mr, x, ref=ref, bound=bound, what=what)


def test_integer_scheme_parameters():
    """The bit budgets the scheme derives (a + b + ceil(log2(longest + 1)) <= 52, a <= 23)."""
    e = integer_case("ragged")
    assert (e.a, e.b) == (20, 21)  # longest row 2,000
    e = integer_case("cantlike")
    assert (e.a, e.b) == (22, 23)
    e = integer_case("one_row")
    assert (e.a, e.b) == (18, 19)  # 20,001 entries: 15 bits
    # small magnitudes next to large ones: every bit length occurs
    v = np.abs(integer_case("ragged").m.val).astype(np.int64)
    assert set(np.floor(np.log2(v)).astype(int).tolist()) == set(range(20))


def test_reference_routes_agree():
    """The extended-precision route and the error-free fsum route give the
    same reference to far below the bound."""
    mr, x, xt, _, _ = real_case("ragged_shuffled")
    for tr, v in ((False, x), (True, xt)):
        a = exact._reference_fsum(mr, v, tr)
        bound = exact.fp64_bound(mr, v, tr)
        if np.finfo(np.longdouble).nmant >= 63:
            b = exact._reference_longdouble(mr, v, tr)
            assert np.all(np.abs(b - a.astype(np.longdouble)).astype(np.float64) <= bound / 2)
        assert np.all(np.abs(exact.exact_reference(mr, v, tr).astype(np.float64) - a) <= bound / 2)


# ------------------------------------------------- the checks can fail
def _long_row(m):
    return int(np.argmax(np.bincount(m.row, minlength=m.n_rows)))


def _without(m, drop):
    keep = np.ones(m.nnz, bool)
    keep[drop] = False
    return sa.Coo(m.n_rows, m.n_cols, m.row[keep], m.col[keep], m.val[keep])


@pytest.mark.parametrize("loop", ["csr", "coo", "sell"])
def test_dropped_small_entry_is_flagged(loop):
    """The smallest-magnitude entry of the longest row missing from the
    matrix the loop runs: exactly that row differs.  Its product is below
    1e-6 of the row's magnitude, so the relative rule cannot see it."""
    e = integer_case("ragged")
    i = _long_row(e.m)
    idx = np.nonzero(e.m.row == i)[0]
    drop = idx[np.argmin(np.abs(e.m.val[idx]))]
    x = np.ascontiguousarray(e.x[:, 0])
    y = run_loop(loop, _without(e.m, drop), x)
    assert exact.exact_bad_rows(y, e.ref[:, 0]).tolist() == [i]
    with pytest.raises(AssertionError, match=rf"1 rows differ from the int64 reference, first \[{i}\]"):
        exact.assert_exact(y, e.ref[:, 0])
    old = oracle.parity(y, e.ref[:, 0].astype(np.float64), e.m.row, e.m.col, e.m.val, x, e.m.n_rows, rel=1e-6)
    assert old.size == 0


def test_duplicated_entry_is_flagged():
    e = integer_case("ragged")
    i = _long_row(e.m)
    j = np.nonzero(e.m.row == i)[0][7]
    m2 = sa.Coo(e.m.n_rows, e.m.n_cols, np.append(e.m.row, e.m.row[j]), np.append(e.m.col, e.m.col[j]),
                np.append(e.m.val, e.m.val[j]))
    y = run_loop("csr", m2, np.ascontiguousarray(e.x[:, 0]))
    assert exact.exact_bad_rows(y, e.ref[:, 0]).tolist() == [i]
    with pytest.raises(AssertionError, match="1 rows differ"):
        exact.assert_exact(y, e.ref[:, 0])


def test_swapped_entries_are_flagged():
    """One entry of row i attributed to row i + 1 and one of row i + 1 to row i."""
    e = integer_case("ragged")
    counts = np.bincount(e.m.row, minlength=e.m.n_rows)
    i = int(np.nonzero((counts[:-1] > 0) & (counts[1:] > 0))[0][0])
    p, q = np.nonzero(e.m.row == i)[0][0], np.nonzero(e.m.row == i + 1)[0][0]
    x = np.ascontiguousarray(e.x[:, 0])
    assert e.m.val[p] * x[e.m.col[p]] != e.m.val[q] * x[e.m.col[q]]
    row = e.m.row.copy()
    row[p], row[q] = i + 1, i
    y = run_loop("csr", sa.Coo(e.m.n_rows, e.m.n_cols, row, e.m.col, e.m.val), x)
    assert exact.exact_bad_rows(y, e.ref[:, 0]).tolist() == [i, i + 1]
    with pytest.raises(AssertionError, match="2 rows differ"):
        exact.assert_exact(y, e.ref[:, 0])


@pytest.mark.parametrize("key", ["ragged", "cantlike"])
def test_fp32_x_is_flagged(key):
    """x rounded to fp32 before the CPU CSR loop: the fp64 bound flags at
    least 99 % of the non-empty rows; the 1e-6 rule flags none of the random
    matrix's."""
    mr, x, _, (ref, bound), _ = real_case(key)
    y = run_loop("csr", mr, x.astype(np.float32).astype(np.float64))
    bad, worst = exact.fp64_ratio(y, ref, bound)
    nonempty = int((np.bincount(mr.row, minlength=mr.n_rows) > 0).sum())
    assert bad.size >= 0.99 * nonempty, (bad.size, nonempty)
    assert worst > 1e4
    with pytest.raises(AssertionError, match="rows over the fp64 bound"):
        exact.assert_fp64(y, mr, x, ref=ref, bound=bound)
    if key == "ragged":
        old = oracle.parity(y, ref.astype(np.float64), mr.row, mr.col, mr.val, x, mr.n_rows, rel=1e-6)
        assert old.size == 0


def test_fp32_values_are_flagged_and_csrf32_reference_is_not():
    """Values rounded to fp32 miss the bound of the unrounded matrix and meet
    the one formed on the rounded values (the csrf32 contract)."""
    mr, x, _, (ref, bound), _ = real_case("ragged")
    m32 = exact.rounded_f32(mr)
    y = run_loop("csr", m32, x)
    bad, _ = exact.fp64_ratio(y, ref, bound)
    assert bad.size >= 0.99 * int((np.bincount(mr.row, minlength=mr.n_rows) > 0).sum())
    exact.assert_fp64(y, m32, x)


def test_one_ulp_is_flagged():
    e = integer_case("ragged_shuffled")
    y = run_loop("csr", e.m, np.ascontiguousarray(e.x[:, 0])).copy()
    exact.assert_exact(y, e.ref[:, 0])
    i = int(np.nonzero(y)[0][3])
    y[i] = np.nextafter(y[i], np.inf)
    assert exact.exact_bad_rows(y, e.ref[:, 0]).tolist() == [i]
    with pytest.raises(AssertionError, match=rf"first \[{i}\]"):
        exact.assert_exact(y, e.ref[:, 0])
    y[i] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        exact.assert_exact(y, e.ref[:, 0])
    # a value comparison: -0.0 equals 0.0
    exact.assert_exact(np.array([-0.0, 3.0]), np.array([0, 3], np.int64))
