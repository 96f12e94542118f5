"""Restarted GMRES on the MI355X: the three basis kernels (csrc/krylov.hip) at
their own edges, and iterate.gmres through libspmv_hip.

Kernels, == on the bits.  spmv_krylov_project_dot's w_out against the host
statement (spmv_cpu_krylov_project) and its c + 1 sums against spmv_dot_multi
with k = 1 on the same columns of the same device buffers; spmv_krylov_combine
and spmv_krylov_normalize against their host statements.  The row counts are
the steps of the dot tree's G(n) = min(ceil(n / 512), 1024): nothing, one
row, a single workgroup's last row, the first row of a second one, and the cap
(1024 * 512 rows, one less, one more).  The widths are the edges of the four
instantiations (1..8, 9..16, 17..24, 25..32 columns) and odd ones in between.
The data is spread over 2^+-30 (tests/exact.py's generator) so that another
summation order changes bits; the exact-integer case holds the sums against
int64 arithmetic.

Every operand lives in a flat buffer of GUARD values, `shift` doubles behind
its start (shift = 1: 8-byte alignment only, no 16-byte loads), with two rows
past n and the padding columns of ld > width left as GUARD; the whole buffer
is compared after the call, so a write outside the statement's elements fails.
The out array and the workspace (exactly the bytes the header asks for) have
guards of their own.

Solver.  The solves of tests/test_gmres.py on build_operator's device
operators: rel <= tol (the solver's own true residual) and a fresh residual in
numpy, the iteration count within one cycle of the numpy double's (GMRES
minimises the residual, so rounding moves the step at which tol is crossed by
a few steps at most; a wrong recurrence is off by factors).
"""
from __future__ import annotations

import numpy as np
import pytest

import iterate as it
import spmv_amd as sa
from exact import wide_range
from iterate_bicgstab_double import scipy_csr, true_rel, upwind
from iterate_gmres_double import BLOCK_SIZES, CASES, MAXIT, RESTARTS, TOL, case_rhs, coo_of, double_count, rotations

pytestmark = pytest.mark.gpu

GUARD = -7.25e300
SMALL_NS = (0, 1, 2, 511, 512, 513)
WIDTHS = (1, 2, 7, 8, 9, 16, 17, 24, 25, 31, 32)
CAP_NS = (1024 * 512 - 1, 1024 * 512 + 1)
CAP_WIDTHS = (1, 9)
MODES = ("apart", "inplace", "column", "null", "copy")


@pytest.fixture(scope="module")
def env():
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    return torch, dev, sa.hip_lib()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


class Window:
    """A (rows + 2, ld) window `shift` doubles into a flat host buffer of GUARD
    values; `live` columns of the first `rows` rows hold data."""

    def __init__(self, rows, live, ld, shift, data):
        self.rows, self.ld, self.shift = rows, ld, shift
        self.flat = np.full(shift + (rows + 2) * ld + 2, GUARD)
        self.view = np.lib.stride_tricks.as_strided(self.flat[shift:], (rows + 2, ld), (8 * ld, 8))
        if live:
            self.view[:rows, :live] = data

    def upload(self, torch, dev):
        self.dev = torch.from_numpy(self.flat).to(dev)
        assert self.dev.data_ptr() % 16 == 0
        return self

    def ptr(self, col=0):
        return self.dev.data_ptr() + 8 * (self.shift + col)

    def column(self, col=0):
        """(rows + 2, 1) host view of one column, for the host statements."""
        return self.view[:, col:col + 1]

    def unchanged_but(self, expected_flat):
        return same_bits(self.dev.cpu().numpy(), expected_flat)


def _guarded(torch, dev, count):
    t = torch.full((count + 4,), float("nan"), dtype=torch.float64, device=dev)
    t[:2] = GUARD
    t[-2:] = GUARD
    return t


def _live(t):
    h = t.cpu().numpy()
    assert (h[:2] == GUARD).all() and (h[-2:] == GUARD).all(), "a guard was overwritten"
    return h[2:-2].copy()


def _stream(torch, dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _values(rng, shape, ints):
    if ints:
        return rng.integers(-3, 4, shape).astype(np.float64)
    v = wide_range(rng, shape)
    v[v == 0.0] = 0.5
    return v


def _coefficients(rng, c, ints):
    h = rng.integers(-3, 4, c).astype(np.float64) if ints else rng.uniform(-2.0, 2.0, c)
    if c > 1:
        h[c // 2] = 0.0
    return h


def _project_ws_doubles(lib, n, c):
    nbytes = lib.spmv_dot_multi_ws_bytes(n, 8 * ((c + 7) // 8) + 1)
    assert nbytes % 8 == 0
    return nbytes // 8


def _project(env, n, c, ldv, shift, mode, ints=False):
    """One spmv_krylov_project_dot call -> (sums (c + 1,), w_out (n,), V (n, c), w (n,)) on the host, after
    every check of bits and guards."""
    torch, dev, lib = env
    rng = np.random.default_rng([n, c, ldv, shift, MODES.index(mode)])
    st = _stream(torch, dev)
    column = mode == "column"
    assert ldv > c or not column
    V = Window(n, c, ldv, shift, _values(rng, (n, c), ints))
    ldw = 1 if mode in ("inplace", "null") else 3
    w = Window(n, 1, ldw, shift, _values(rng, (n, 1), ints))
    h = None if mode in ("null", "copy") else _coefficients(rng, c, ints)
    apart = Window(n, 0, 2, 1 - shift, None) if mode in ("apart", "copy") else None
    out_w = {"apart": apart, "copy": apart, "inplace": w, "column": V, "null": None}[mode]
    out_col = c if column else 0
    # what the host statement leaves
    want = {id(t): t.flat.copy() for t in (V, w, apart) if t is not None}
    if h is not None:
        sa.cpu_krylov_project(n, V.view[:, :c], h, w.column(), out_w.column(out_col), c=c)
    elif out_w is not None:
        out_w.view[:n, 0] = w.view[:n, 0]
    want, host_now = {k: None for k in want}, want
    for t in (V, w, apart):
        if t is not None:
            want[id(t)] = t.flat.copy()  # after the statement
            t.flat[:] = host_now[id(t)]  # the device gets the inputs
            t.upload(torch, dev)
    hd = None if h is None else torch.from_numpy(h).to(dev)
    out = _guarded(torch, dev, c + 1)
    ws = _guarded(torch, dev, _project_ws_doubles(lib, n, c))
    rc = lib.spmv_krylov_project_dot(n, c, V.ptr(), ldv, None if hd is None else hd.data_ptr(), w.ptr(), ldw,
                                     None if out_w is None else out_w.ptr(out_col),
                                     0 if out_w is None else out_w.ld, out.data_ptr() + 16, ws.data_ptr() + 16,
                                     8 * (ws.numel() - 4), 0, st)
    assert rc == sa.SUCCESS, (n, c, ldv, shift, mode, lib.spmv_last_error().decode())
    got = _live(out)
    _live(ws)
    for t in (V, w, apart):
        if t is not None:
            assert t.unchanged_but(want[id(t)]), (n, c, ldv, shift, mode, "a buffer differs from the host statement")
    # the sums, column by column, by spmv_dot_multi on the buffers the call left
    res_w, res_col = (w, 0) if out_w is None else (out_w, out_col)
    ref = _guarded(torch, dev, c + 1)
    dws = torch.empty(max(lib.spmv_dot_multi_ws_bytes(n, 1), 8), dtype=torch.uint8, device=dev)
    for j in range(c + 1):
        a, lda = (V.ptr(j), ldv) if j < c else (res_w.ptr(res_col), res_w.ld)
        rc = lib.spmv_dot_multi(n, 1, a, lda, res_w.ptr(res_col), res_w.ld, ref.data_ptr() + 16 + 8 * j,
                                dws.data_ptr(), dws.numel(), 0, st)
        assert rc == sa.SUCCESS
    assert same_bits(got, _live(ref)), (n, c, ldv, shift, mode, got, _live(ref))
    flat = want[id(res_w)] if out_w is not None else w.flat
    res = np.lib.stride_tricks.as_strided(flat[res_w.shift:], (n + 2, res_w.ld), (8 * res_w.ld, 8))[:n, res_col]
    return got, res.copy(), V.view[:n, :c].copy(), w.view[:n, 0].copy()


def _modes(c, ldv):
    return [m for m in MODES if m != "column" or ldv > c]


@pytest.mark.parametrize("n", SMALL_NS)
def test_project_dot_bits(env, n):
    calls = 0
    for c in WIDTHS:
        for ldv in (c, c + 1):
            for shift in (0, 1):
                for mode in _modes(c, ldv):
                    got, res, V, _ = _project(env, n, c, ldv, shift, mode)
                    calls += 1
                    if n == 0:
                        assert same_bits(got, np.zeros(c + 1))
                    else:  # and they are the sums: a loose check next to the exact-integer one
                        scale = np.abs(V).T @ np.abs(res)
                        assert (np.abs(got[:c] - V.T @ res) <= 1e-12 * scale + 1e-300).all()
    print(f"n = {n}: {calls} calls bit-equal")


@pytest.mark.parametrize("n", CAP_NS)
@pytest.mark.parametrize("c", CAP_WIDTHS)
def test_project_dot_bits_at_the_grid_cap(env, n, c):
    for ldv, shift, mode in ((c, 0, "apart"), (c + 1, 1, "column"), (c + 1, 0, "inplace"), (c, 1, "null")):
        _project(env, n, c, ldv, shift, mode)


@pytest.mark.parametrize("n", (1, 513, 1030))
def test_project_dot_exact_on_integers(env, n):
    """Entries in -3..3: every product and every partial sum is an integer far
    below 2^53, so the tree's order does not matter and the sums are int64's."""
    for c in WIDTHS:
        for mode in ("apart", "column", "null"):
            got, res, V, w = _project(env, n, c, c + 1, c % 2, mode, ints=True)
            Vi, ri = V.astype(np.int64), res.astype(np.int64)
            assert np.array_equal(got[:c], (Vi.T @ ri).astype(np.float64)), (n, c, mode)
            assert got[c] == float(ri @ ri)
            if mode == "null":
                assert np.array_equal(res, w)


def test_project_dot_refusals(env):
    torch, dev, lib = env
    st = _stream(torch, dev)
    n, c = 5, 3
    V = torch.ones(n, c, dtype=torch.float64, device=dev)
    w, o = torch.ones(n, dtype=torch.float64, device=dev), torch.full((n,), GUARD, dtype=torch.float64, device=dev)
    h = torch.ones(c, dtype=torch.float64, device=dev)
    out = torch.full((c + 1,), GUARD, dtype=torch.float64, device=dev)
    ws = torch.empty(lib.spmv_dot_multi_ws_bytes(n, 9), dtype=torch.uint8, device=dev)
    p = sa._ptr
    ok = [n, c, p(V), c, p(h), p(w), 1, p(o), 1, p(out), p(ws), ws.numel(), 0, st]
    for pos, bad in ((0, -1), (1, 0), (1, 33), (2, None), (3, c - 1), (5, None), (6, 0), (7, None), (8, 0), (9, None),
                     (10, None), (11, ws.numel() - 8)):
        args = list(ok)
        args[pos] = bad
        assert lib.spmv_krylov_project_dot(*args) == sa.OTHER_ERROR, pos
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == GUARD).all() and (out.cpu().numpy() == GUARD).all()
    y = np.ones(c)
    okc = [n, c, p(V), c, p(y), p(o), 1, 0, st]
    for pos, bad in ((0, -1), (1, 0), (1, 33), (2, None), (3, c - 1), (4, None), (5, None), (6, 0)):
        args = list(okc)
        args[pos] = bad
        assert lib.spmv_krylov_combine(*args) == sa.OTHER_ERROR, pos
    s = torch.ones(1, dtype=torch.float64, device=dev)
    okn = [n, p(s), p(w), 1, p(o), 1, None, 0, st]
    for pos, bad in ((0, -1), (1, None), (2, None), (3, 0), (4, None), (5, 0)):
        args = list(okn)
        args[pos] = bad
        assert lib.spmv_krylov_normalize(*args) == sa.OTHER_ERROR, pos
    torch.cuda.synchronize()
    assert (o.cpu().numpy() == GUARD).all()


# ------------------------------------------------------- combine, normalize
@pytest.mark.parametrize("n", SMALL_NS + CAP_NS)
def test_combine_bits(env, n):
    torch, dev, lib = env
    st = _stream(torch, dev)
    for c in (WIDTHS if n < 1000 else CAP_WIDTHS):
        for ldv in (c, c + 1):
            for shift in (0, 1):
                for ints in (False, True):
                    rng = np.random.default_rng([n, c, ldv, shift, ints])
                    V = Window(n, c, ldv, shift, _values(rng, (n, c), ints))
                    y = _coefficients(rng, c, ints)
                    t = Window(n, 0, 1 + shift, 1 - shift, None)
                    before = V.flat.copy()
                    V.upload(torch, dev), t.upload(torch, dev)
                    rc = lib.spmv_krylov_combine(n, c, V.ptr(), ldv, sa._ptr(y), t.ptr(), t.ld, 0, st)
                    assert rc == sa.SUCCESS, (n, c, ldv, shift, lib.spmv_last_error().decode())
                    sa.cpu_krylov_combine(n, V.view[:, :c], y, t.column(), c=c)
                    assert t.unchanged_but(t.flat), (n, c, ldv, shift, ints)
                    assert V.unchanged_but(before)
                    if ints:
                        want = V.view[:n, :c].astype(np.int64) @ y.astype(np.int64)
                        assert np.array_equal(t.view[:n, 0], want.astype(np.float64))


@pytest.mark.parametrize("n", SMALL_NS + CAP_NS)
def test_normalize_bits(env, n):
    torch, dev, lib = env
    st = _stream(torch, dev)
    for s in (2.75, 3e-300, 0.0, -1.0):
        for alias in (False, True):
            for with_copy in (False, True):
                for shift in (0, 1):
                    rng = np.random.default_rng([n, alias, with_copy, shift])
                    w = Window(n, 1, 1 + shift, shift, _values(rng, (n, 1), False))
                    v = w if alias else Window(n, 0, 3, 1 - shift, None)
                    copy = Window(n, 0, 1, shift, None) if with_copy else None
                    for t in {id(t): t for t in (w, v, copy) if t is not None}.values():
                        t.upload(torch, dev)
                    sd = torch.tensor([s], dtype=torch.float64, device=dev)
                    rc = lib.spmv_krylov_normalize(n, sd.data_ptr(), w.ptr(), w.ld, v.ptr(), v.ld,
                                                   None if copy is None else copy.ptr(), 0, st)
                    assert rc == sa.SUCCESS, (n, s, alias, lib.spmv_last_error().decode())
                    sa.cpu_krylov_normalize(n, np.array([s]), w.column(), v.column(),
                                            None if copy is None else copy.view[:n, 0])
                    for t in (w, v, copy):
                        if t is not None:
                            assert t.unchanged_but(t.flat), (n, s, alias, with_copy, shift)
                    if s <= 0.0:
                        assert (v.view[:n, 0] == 0.0).all()


# -------------------------------------------------------------------- solver
# the upwind matrices have no block structure (3 x 3 blocks: fill 2.9), which
# to_device's break-even rule refuses unless told that any fill will do
FORMATS = (("csr", {}), ("sell", {}), ("bsr", {"block": 3, "bsr_max_fill": float("inf")}))


def _device_solve(env, m, b, fmt, kw, bs, restart, maxit=MAXIT, **op_kw):
    torch, dev, _ = env
    op = it.build_operator(m, 0, 1, fmt, dev, align=64, bjacobi=bs, **op_kw, **kw)
    x, its, rel = it.gmres(op, torch.from_numpy(b).to(dev), tol=TOL, maxit=maxit, restart=restart)
    return x.cpu().numpy(), its, rel


@pytest.mark.parametrize("fmt,kw", FORMATS)
@pytest.mark.parametrize("case", CASES)
def test_gmres_converges(env, case, fmt, kw):
    m = upwind(*case)
    A, b = scipy_csr(m), case_rhs(case)
    for restart in RESTARTS:
        for bs in BLOCK_SIZES:
            x, its, rel = _device_solve(env, m, b, fmt, kw, bs, restart)
            mine = float(true_rel(A, b[:, None], x[:, None])[0])
            ref = double_count(case, restart, bs)
            print(f"{fmt} {case} restart {restart} bs {bs}: its {its} (double {ref}, difference {its - ref}), "
                  f"rel {rel:.3g}, fresh true_rel {mine:.3g}")
            assert its < MAXIT and np.isfinite(x).all()
            assert rel <= TOL and mine <= TOL
            assert abs(its - ref) <= restart


def test_rotations_where_bicgstab_stands_still(env):
    torch, dev, _ = env
    op = it.build_operator(rotations(), 0, 1, "csr", dev, align=64)
    b = torch.from_numpy(np.random.default_rng(1).uniform(-0.5, 0.5, 64)).to(dev)
    x, its, rel = it.gmres(op, b, tol=TOL, maxit=50, restart=20)
    _, _, rel_b = it.bicgstab(op, b, tol=TOL, maxit=50)
    print(f"rotations: gmres its {its} rel {rel:.3g}, bicgstab rel {rel_b:.3g}")
    assert its <= 2 and rel <= TOL
    assert rel_b > 0.5


def test_end_cases(env):
    torch, dev, _ = env
    op = it.build_operator(coo_of(np.diag(np.arange(1.0, 9.0))), 0, 1, "csr", dev, align=64)
    b = np.zeros(8)
    b[3] = 2.0
    x, its, rel = it.gmres(op, torch.from_numpy(b).to(dev), tol=TOL, maxit=50, restart=5)
    assert its == 1 and rel == 0.0 and np.array_equal(x.cpu().numpy(), b / 4.0)
    x, its, rel = it.gmres(op, torch.zeros(8, dtype=torch.float64, device=dev))
    assert its == 0 and rel == 0.0 and (x.cpu().numpy() == 0.0).all()
    rng = np.random.default_rng(2)
    a = rng.uniform(-1, 1, (12, 12)) + 4.0 * np.eye(12)
    b = rng.uniform(-1, 1, 12)
    op = it.build_operator(coo_of(a), 0, 1, "csr", dev, align=64)
    x, its, rel = it.gmres(op, torch.from_numpy(b).to(dev), tol=TOL, maxit=100, restart=31)
    assert its <= 12 and rel <= TOL
    assert np.linalg.norm(b - a @ x.cpu().numpy()) <= TOL * np.linalg.norm(b)
    with pytest.raises(sa.SpmvError, match="restart"):
        it.gmres(op, torch.from_numpy(b).to(dev), restart=32)
    with pytest.raises(sa.SpmvError):
        it.gmres(op, torch.from_numpy(b))  # a host tensor


def test_two_calls_give_the_same_bits_and_split_operators_solve(env):
    case = CASES[2]
    m = upwind(*case)
    b = case_rhs(case)
    x1, its1, rel1 = _device_solve(env, m, b, "csr", {}, 3, 20)
    x2, its2, rel2 = _device_solve(env, m, b, "csr", {}, 3, 20)
    assert same_bits(x1, x2) and its1 == its2 and rel1 == rel2
    for overlap in (False, True):
        xs, its, rel = _device_solve(env, m, b, "csr", {}, 3, 20, split=True, overlap=overlap)
        assert rel <= TOL and abs(its - its1) <= 20
        assert np.linalg.norm(xs - x1) <= 1e-6 * np.linalg.norm(x1)
