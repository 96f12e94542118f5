"""The binding's operand checks, pinned call by call.

tests/golden/binding_refusals.json records what every call of `table()` gave
BEFORE the checks were folded into shared validators: the exception's type,
its rc and its text.  The replay below asserts the same outcome, entry by
entry, so neither a message nor the order of two checks can move unnoticed.
An entry with a "parent" key is a declared difference: "parent" is the old
outcome, the entry itself the one asserted now (DeviceMatrix.run on a
non-tensor, and cpu_csr_multi's Y-rows and k-columns refusals).

No call reaches a library: hip_lib / host_lib are replaced by a stub whose
every function raises ReachedLibrary(<its name>), which is the recorded
outcome of an accepted call.  The accepted side proper (one-row operands with
an odd row stride, ld > k slices) runs on the real host library at the end.
"""
from __future__ import annotations

import ctypes
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import spmv_amd as sa

FIXTURE = Path(__file__).resolve().parent / "golden" / "binding_refusals.json"
F64 = torch.float64


class ReachedLibrary(Exception):
    """Every check passed: the call got as far as the named C function."""


class _StubLib:
    def __getattr__(self, name):
        def reached(*args):
            raise ReachedLibrary(name)

        return reached


class _StubStream:
    cuda_stream = 0


def outcome(thunk) -> dict:
    try:
        thunk()
    except Exception as e:  # noqa: BLE001 - the type is what is recorded
        return {"type": type(e).__name__, "rc": getattr(e, "rc", None), "message": str(e)}
    return {"type": None, "rc": None, "message": ""}


def _strided_rows(shape, row_bytes):
    """A float64 array whose row stride is row_bytes (not a multiple of 8)."""
    return np.ndarray(shape, np.float64, buffer=bytearray(row_bytes * shape[0] + 64), strides=(row_bytes, 8))


def _device_table(sa):
    """(call, label, thunk) for the six run methods on bare, plan-less objects
    and CPU tensors: nothing touches a device."""
    on_gpu, square, rect = (sa.DeviceMatrix("none", r, 6, 6, dev, plan=None)
                            for r, dev in ((6, "cuda:0"), (6, "cpu"), (4, "cpu")))
    st = _StubStream()
    out = []

    def add(name, label, dm, a, b):
        out.append((name, label, lambda: getattr(dm, name)(a, b, stream=st)))

    def v(n=6, dtype=F64):
        return torch.zeros(n, dtype=dtype)

    gaps = torch.zeros(12, dtype=F64)[::2]
    for name in ("run", "run_t", "run_sym"):
        long_first = (v(6), v(4)) if name == "run" else (v(4), v(6))  # what the 4 x 6 matrix takes
        for label, dm, x, y in (
                ("no plan", square, v(), v()),
                ("wrong device", on_gpu, v(), v()),
                ("x dtype", square, v(dtype=torch.float32), v()),
                ("y dtype", square, v(), v(dtype=torch.float32)),
                ("x too short", square, v(5), v()),
                ("y too short", square, v(), v(5)),
                ("x non-contiguous", square, gaps, v()),
                ("y non-contiguous", square, v(), gaps),
                ("x a numpy array", square, np.zeros(6), v()),
                ("y a numpy array", square, v(), np.zeros(6)),
                ("x a list", square, [0.0] * 6, v()),
                ("x 2-D of 6 entries", square, torch.zeros(6, 1, dtype=F64), v()),
                ("longer y than needed", square, v(), v(9)),
                ("4 x 6: operands as it takes them", rect, *long_first),
                ("4 x 6: operands swapped", rect, *long_first[::-1]),
                ("dtype and too short", square, v(5, torch.float32), v()),
                ("y dtype and x too short", square, v(5), v(dtype=torch.float32)),
                ("too short and non-contiguous", square, v(5), gaps),
                ("non-contiguous and wrong device", on_gpu, gaps, v()),
                ("4 x 6: dtype first", rect, v(dtype=torch.float32), v()),
                ("4 x 6: too short for either", rect, v(3), v(3)),
                ("4 x 6: non-contiguous", rect, gaps, gaps)):
            add(name, label, dm, x, y)

    def m(rows=6, k=2, dtype=F64):
        return torch.zeros(rows, k, dtype=dtype)

    def inner2(rows=6):
        return torch.zeros(rows, 4, dtype=F64)[:, ::2]

    def overlap(rows=6):  # row stride 1 < k = 2
        return torch.as_strided(torch.zeros(2 * rows, dtype=F64), (rows, 2), (1, 1))

    for name in ("run_multi", "run_t_multi", "run_sym_multi"):
        long_first = (m(6), m(4)) if name == "run_multi" else (m(4), m(6))
        for label, dm, X, Y in (
                ("no plan", square, m(), m()),
                ("wrong device", on_gpu, m(), m()),
                ("X dtype", square, m(dtype=torch.float32), m()),
                ("Y dtype", square, m(), m(dtype=torch.float32)),
                ("X 1-D", square, v(), m()),
                ("Y 1-D", square, m(), v()),
                ("k differs", square, m(k=3), m()),
                ("zero columns", square, m(k=0), m(k=0)),
                ("X too few rows", square, m(5), m()),
                ("Y too few rows", square, m(), m(5)),
                ("X inner stride 2", square, inner2(), m()),
                ("Y inner stride 2", square, m(), inner2()),
                ("X row stride < k", square, overlap(), m()),
                ("Y row stride < k", square, m(), overlap()),
                ("X a numpy array", square, np.zeros((6, 2)), m()),
                ("Y a numpy array", square, m(), np.zeros((6, 2))),
                ("column slices of wider tensors", square, torch.zeros(6, 4, dtype=F64)[:, :2],
                 torch.zeros(6, 5, dtype=F64)[:, 1:3]),
                ("one column with inner stride 3", square, torch.zeros(6, 3, dtype=F64)[:, :1],
                 torch.zeros(6, 3, dtype=F64)[:, 2:]),
                ("4 x 6: operands as it takes them", rect, *long_first),
                ("4 x 6: operands swapped", rect, *long_first[::-1]),
                ("X dtype and too few rows", square, m(5, dtype=torch.float32), m()),
                ("X 1-D and Y dtype", square, v(), m(dtype=torch.float32)),
                ("Y 1-D and X too few rows", square, m(5), v()),
                ("k differs and too few rows", square, m(5, k=3), m()),
                ("too few rows and inner stride", square, m(5), inner2()),
                ("inner stride and wrong device", on_gpu, inner2(), m()),
                ("row stride and wrong device", on_gpu, m(), overlap()),
                ("4 x 6: dtype first", rect, m(dtype=torch.float32), m()),
                ("4 x 6: 1-D first", rect, v(), m()),
                ("4 x 6: k differs", rect, m(k=3), m()),
                ("4 x 6: too few rows for either", rect, m(3), m(3)),
                ("4 x 6: inner stride", rect, inner2(), inner2())):
            add(name, label, dm, X, Y)
    return out


def _host_table(sa):
    """(call, label, thunk) for the numpy host statements on a 3-row matrix."""
    ptr = np.array([0, 1, 2, 3], np.int64)
    col = np.array([0, 1, 2], np.int32)
    val = np.ones(3)
    out = []

    def v(n=3, dtype=np.float64):
        return np.zeros(n, dtype)

    def m(rows=3, k=2, dtype=np.float64):
        return np.zeros((rows, k), dtype)

    def inner2(rows=3):
        return np.zeros((rows, 4))[:, ::2]

    def odd(rows=3):
        return _strided_rows((rows, 2), 20)

    gaps = np.zeros(6)[::2]
    for name, call, ny in (("cpu_csr_t", lambda x, y: sa.cpu_csr_t(3, 4, ptr, col, val, x, y), 4),
                           ("cpu_csr_sym", lambda x, y: sa.cpu_csr_sym(3, ptr, col, val, x, y), 3)):
        for label, x, y in (
                ("accepted", v(), v(ny)),
                ("x not an array", [0.0] * 3, v(ny)),
                ("y not an array", v(), [0.0] * ny),
                ("x float32", v(dtype=np.float32), v(ny)),
                ("y float32", v(), v(ny, np.float32)),
                ("x 2-D", m(3, 1), v(ny)),
                ("x non-contiguous", gaps, v(ny)),
                ("y non-contiguous", v(), np.zeros(2 * ny)[::2]),
                ("x too short", v(2), v(ny)),
                ("y too short", v(), v(ny - 1)),
                ("x too short and y float32", v(2), v(ny, np.float32)),
                ("x float32 and too short", v(2, np.float32), v(ny))):
            out.append((name, label, lambda call=call, x=x, y=y: call(x, y)))

    for name, call, ny in (
            ("cpu_csr_multi", lambda X, Y, k=None: sa.cpu_csr_multi(3, ptr, col, val, X, Y, k), 3),
            ("cpu_csr_t_multi", lambda X, Y, k=None: sa.cpu_csr_t_multi(3, 4, ptr, col, val, X, Y, k), 4),
            ("cpu_csr_sym_multi", lambda X, Y, k=None: sa.cpu_csr_sym_multi(3, ptr, col, val, X, Y, k), 3),
            ("cpu_bjacobi_apply_multi",
             lambda X, Y, k=None, inv=m(4, 2): sa.cpu_bjacobi_apply_multi(3, 2, inv, X, Y, k), 3)):
        cases = [
            ("accepted", m(), m(ny)),
            ("column slices of wider arrays", np.zeros((3, 4))[:, :2], np.zeros((ny, 5))[:, 1:3]),
            ("k smaller than either width", m(), m(ny), 1),
            ("X not an array", [[0.0, 0.0]] * 3, m(ny)),
            ("Y not an array", m(), None),
            ("X float32", m(dtype=np.float32), m(ny)),
            ("Y float32", m(), m(ny, dtype=np.float32)),
            ("X 1-D", v(), m(ny)),
            ("Y 1-D", m(), v(ny)),
            ("X inner stride 2", inner2(), m(ny)),
            ("Y inner stride 2", m(), inner2(ny)),
            ("X row stride of 20 bytes", odd(), m(ny)),
            ("Y row stride of 20 bytes", m(), odd(ny)),
            ("X too few rows", m(2), m(ny)),
            ("Y too few rows", m(), m(ny - 1)),
            ("k larger than X's width", m(), m(ny, 3), 3),
            ("k larger than Y's width", m(), m(ny, 1)),
            ("k = 0", m(), m(ny), 0),
            ("Y float32 and X inner stride 2", inner2(), m(ny, dtype=np.float32)),
            ("X inner stride 2 and Y too few rows", inner2(), m(ny - 1)),
            ("Y too few rows and k larger than its width", m(), m(ny - 1, 1)),
        ]
        if name == "cpu_bjacobi_apply_multi":
            short = {"inv": m(3, 2)}
            cases += [("inv too short", m(), m(ny), None, short),
                      ("inv too short and k larger than X's width", m(), m(ny, 3), 3, short)]
        for label, X, Y, *rest in cases:
            k = rest[0] if rest else None
            kw = rest[1] if len(rest) > 1 else {}
            out.append((name, label, lambda call=call, X=X, Y=Y, k=k, kw=kw: call(X, Y, k, **kw)))

    def cheb(R=None, AZ=None, D=None, Zin=None, Zout=None, k=None, inv=None):
        R, D, Zout = (m() if t is None else t for t in (R, D, Zout))
        return lambda: sa.cpu_bjacobi_cheb_step_multi(3, 2, m(4, 2) if inv is None else inv, 0.5, 2.0, R, AZ, D, Zin,
                                                      Zout, k)

    for label, thunk in (
            ("step 0 accepted", cheb()),
            ("general step accepted", cheb(AZ=m(), Zin=m())),
            ("step 0 ignores Zin", cheb(Zin="ignored")),
            ("AZ given without Zin", cheb(AZ=m())),
            ("AZ without Zin comes before R's dtype", cheb(R=m(dtype=np.float32), AZ=m())),
            ("R not an array", cheb(R=[[0.0, 0.0]] * 3)),
            ("AZ float32", cheb(AZ=m(dtype=np.float32), Zin=m())),
            ("D 1-D", cheb(D=v())),
            ("Zin inner stride 2", cheb(AZ=m(), Zin=inner2())),
            ("Zout row stride of 20 bytes", cheb(Zout=odd())),
            ("Zin too few rows", cheb(AZ=m(), Zin=m(2))),
            ("D fewer than k columns", cheb(D=m(3, 1))),
            ("k larger than R's width", cheb(k=3)),
            ("inv too short", cheb(inv=m(3, 2))),
            ("inv too short and Zout too few rows", cheb(Zout=m(2), inv=m(3, 2))),
            ("R too few rows and AZ float32", cheb(R=m(2), AZ=m(dtype=np.float32), Zin=m()))):
        out.append(("cpu_bjacobi_cheb_step_multi", label, thunk))

    def update(blocks=None, scalars=None, k=None):
        b = {**dict.fromkeys(("Ph", "Sh", "T", "X", "R")), **(blocks or {})}
        s = {**dict.fromkeys(("a_num", "a_den", "w_num", "w_den")), **(scalars or {})}
        return lambda: sa.cpu_bicgstab_update_multi(3, *(v(2) if t is None else t for t in s.values()),
                                                    *(m() if t is None else t for t in b.values()), k)

    def direction(blocks=None, scalars=None, k=None):
        b = {**dict.fromkeys(("V", "R", "P")), **(blocks or {})}
        s = {**dict.fromkeys(("rho_new", "rv", "tt", "ts")), **(scalars or {})}
        return lambda: sa.cpu_bicgstab_dir_multi(3, *(v(2) if t is None else t for t in s.values()),
                                                 *(m() if t is None else t for t in b.values()), k)

    for name, make, mid, last, sc in (("cpu_bicgstab_update_multi", update, "T", "R", "a_den"),
                                      ("cpu_bicgstab_dir_multi", direction, "R", "P", "tt")):
        for label, thunk in (
                ("accepted", make()),
                ("k smaller than the width", make(k=1)),
                ("a block not an array", make({mid: [[0.0, 0.0]] * 3})),
                ("a block float32", make({last: m(dtype=np.float32)})),
                ("a block 1-D", make({mid: v()})),
                ("a block with inner stride 2", make({last: inner2()})),
                ("a block with a row stride of 20 bytes", make({mid: odd()})),
                ("a block with too few rows", make({last: m(2)})),
                ("k larger than the width", make(k=3)),
                ("one block narrower than the first", make({last: m(3, 1)})),
                ("a scalar array too short", make(scalars={sc: v(1)})),
                ("a scalar array float32", make(scalars={sc: v(2, np.float32)})),
                ("a scalar array with gaps", make(scalars={sc: np.zeros(4)[::2]})),
                ("a scalar array 2-D", make(scalars={sc: m(2, 1)})),
                ("a scalar not an array", make(scalars={sc: [0.0, 0.0]})),
                ("too few rows and a short scalar array", make({last: m(2)}, {sc: v(1)})),
                ("float32 block after one with too few rows", make({mid: m(2), last: m(dtype=np.float32)}))):
            out.append((name, label, thunk))

    def combine(blocks, C=None, Y=None):
        if C is None:
            C = np.zeros((sum(t.shape[1] for t in blocks), 2))
        return lambda: sa.cpu_block_combine_multi(3, C, blocks, m() if Y is None else Y)

    for label, thunk in (
            ("accepted, 1 block", combine([m()])),
            ("accepted, 3 blocks", combine([m(), m(3, 1), m(3, 8)])),
            ("0 blocks", combine([])),
            ("4 blocks", combine([m()] * 4)),
            ("a 9-column block", combine([m(3, 9)])),
            ("a 0-column block", combine([m(3, 0), m()])),
            ("a block not an array", combine([m(), [[0.0]] * 3], C=np.zeros((3, 2)))),
            ("a block float32", combine([m(dtype=np.float32)])),
            ("a block 1-D", combine([v()], C=np.zeros((1, 2)))),
            ("a block with inner stride 2", combine([inner2()])),
            ("a block with a row stride of 20 bytes", combine([odd()])),
            ("a block with too few rows", combine([m(), m(2)])),
            ("Y too few rows", combine([m()], Y=m(2))),
            ("Y float32", combine([m()], Y=m(dtype=np.float32))),
            ("Y fewer than kc columns", combine([m()], Y=m(3, 1))),
            ("C of the wrong height", combine([m()], C=np.zeros((3, 2)))),
            ("C with 9 columns", combine([m()], C=np.zeros((2, 9)), Y=m(3, 9))),
            ("4 blocks and Y too few rows", combine([m()] * 4, Y=m(2))),
            ("a 9-column block and Y float32", combine([m(3, 9)], Y=m(dtype=np.float32)))):
        out.append(("cpu_block_combine_multi", label, thunk))
    return out


def table(sa):
    return _device_table(sa) + _host_table(sa)


def replay(sa) -> list:
    """Every entry's outcome with both libraries stubbed out."""
    saved = sa.hip_lib, sa.host_lib
    sa.hip_lib = sa.host_lib = _StubLib
    try:
        return [{"call": call, "label": label, **outcome(thunk)} for call, label, thunk in table(sa)]
    finally:
        sa.hip_lib, sa.host_lib = saved


def recorded() -> list:
    """The fixture, {call: [[label, type, rc, message(, parent's three)], ..]}, as replay()'s list."""
    out = []
    for call, rows in json.loads(FIXTURE.read_text()).items():
        for label, kind, rc, message, *parent in rows:
            e = {"call": call, "label": label, "type": kind, "rc": rc, "message": message}
            if parent:
                e["parent"] = dict(zip(("type", "rc", "message"), parent[0]))
            out.append(e)
    return out


def test_every_refusal_is_the_recorded_one():
    want = recorded()
    got = replay(sa)
    assert [(e["call"], e["label"]) for e in got] == [(e["call"], e["label"]) for e in want], \
        "the table and the fixture list different calls"
    declared = [e for e in want if "parent" in e]
    assert {e["call"] for e in declared} == {"run", "cpu_csr_multi"} and len(declared) <= 8
    for g, w in zip(got, want):
        w = {k: v for k, v in w.items() if k != "parent"}
        assert g == w, f'{w["call"]}: {w["label"]}'
    # a declared difference turns a call that got through, or died of an
    # AttributeError, into an SpmvError(OTHER_ERROR): never the other way round
    for e in declared:
        assert e["parent"]["type"] in ("ReachedLibrary", "AttributeError"), e["label"]
        assert (e["type"], e["rc"]) == ("SpmvError", sa.OTHER_ERROR), e["label"]


def test_the_fixture_covers_every_listed_call_and_both_sides():
    want = recorded()
    calls = {e["call"] for e in want}
    assert calls == {"run", "run_multi", "run_t", "run_t_multi", "run_sym", "run_sym_multi", "cpu_csr_t",
                     "cpu_csr_sym", "cpu_csr_multi", "cpu_csr_t_multi", "cpu_csr_sym_multi",
                     "cpu_bjacobi_apply_multi", "cpu_bjacobi_cheb_step_multi", "cpu_bicgstab_update_multi",
                     "cpu_bicgstab_dir_multi", "cpu_block_combine_multi"}
    for call in calls:
        kinds = {e["type"] for e in want if e["call"] == call}
        assert "SpmvError" in kinds, call
        if call.startswith("cpu_"):  # the plan-less run methods end in their "no plan" refusal instead
            assert "ReachedLibrary" in kinds, call
        else:
            assert any("no plan" in e["message"] for e in want if e["call"] == call), call


# ------------------------------------------------------------ accepted side
@pytest.fixture(scope="module")
def integer_matrices():
    """Small integer matrices: every order of summation gives the same bits,
    so the dense product is the exact answer."""
    rng = np.random.default_rng(5)
    out = {}
    for n_rows, n_cols in ((1, 7), (5, 7)):
        A = rng.integers(-3, 4, (n_rows, n_cols)).astype(np.float64)
        A[0, 0] = 2.0  # no empty matrix
        m = sa.Coo(n_rows, n_cols, *(a.astype(np.int32) for a in np.nonzero(A)), A[np.nonzero(A)])
        out[n_rows] = (A, m.n_rows, m.n_cols, *sa.csr_from_coo(m))
    n = 6
    S = np.tril(rng.integers(-3, 4, (n, n))).astype(np.float64)
    S[np.diag_indices(n)] = 4.0
    h = sa.Coo(n, n, *(a.astype(np.int32) for a in np.nonzero(S)), S[np.nonzero(S)])
    out["sym"] = (S + S.T - np.diag(np.diag(S)), S, *sa.csr_from_coo(h))
    one = sa.Coo(1, 1, np.zeros(1, np.int32), np.zeros(1, np.int32), np.full(1, 3.0))
    out["sym1"] = (np.full((1, 1), 3.0), None, *sa.csr_from_coo(one))
    return out


def _block(rng, rows, k, ld):
    """(rows, k) integer-valued slice of a (rows, ld) array: strides[0] is ld
    doubles whatever rows is."""
    buf = np.full((rows, ld), np.nan)
    X = buf[:, 1:1 + k]
    X[:] = rng.integers(-4, 5, (rows, k))
    return X


@pytest.mark.parametrize("k", [1, 2, 3])
def test_one_row_operands_with_an_odd_row_stride_are_accepted(integer_matrices, k):
    """A one-row slice of a wider array has a row stride that says nothing
    about k; the C functions want ld >= k, and the binding passes k."""
    rng = np.random.default_rng(k)
    A, n_rows, n_cols, ptr, col, val = integer_matrices[1]
    X = _block(rng, n_cols, k, 5)
    Y = np.full((1, 7), 99.0)[:, 2:2 + k]  # one row, strides[0] = 7 doubles
    assert Y.shape[0] == 1 and Y.strides[0] == 56
    sa.cpu_csr_multi(n_rows, ptr, col, val, X, Y)
    assert np.array_equal(Y, A @ X)
    X1 = np.full((1, 5), np.nan)[:, 1:1 + k]  # A^T of a one-row matrix: a one-row X
    X1[:] = rng.integers(-4, 5, (1, k))
    Yt = _block(rng, n_cols, k, 9)
    assert X1.strides[0] == 40
    sa.cpu_csr_t_multi(n_rows, n_cols, ptr, col, val, X1, Yt)
    assert np.array_equal(Yt, A.T @ X1)
    A1, _, ptr1, col1, val1 = integer_matrices["sym1"]
    Ys = np.full((1, 7), 99.0)[:, 2:2 + k]
    sa.cpu_csr_sym_multi(1, ptr1, col1, val1, X1, Ys)
    assert np.array_equal(Ys, A1 @ X1)
    # k given and smaller than the one-row operands' width
    Yk = np.full((1, 7), 99.0)[:, 2:2 + k]
    sa.cpu_csr_multi(n_rows, ptr, col, val, X, Yk, k=1)
    assert np.array_equal(Yk[:, :1], (A @ X)[:, :1]) and np.all(Yk[:, 1:] == 99.0)


@pytest.mark.parametrize("k,ld", [(1, 3), (2, 5), (8, 11)])
def test_column_slices_of_wider_arrays_are_accepted(integer_matrices, k, ld):
    rng = np.random.default_rng(ld)
    A, n_rows, n_cols, ptr, col, val = integer_matrices[5]
    X = _block(rng, n_cols, k, ld)
    Ybuf = np.full((n_rows + 2, ld + 1), 99.0)
    sa.cpu_csr_multi(n_rows, ptr, col, val, X, Ybuf[:, :k])
    want = np.full_like(Ybuf, 99.0)
    want[:n_rows, :k] = A @ X
    assert np.array_equal(Ybuf, want)
    Xt = _block(rng, n_rows, k, ld)
    Ybuf = np.full((n_cols + 2, ld + 1), 99.0)
    sa.cpu_csr_t_multi(n_rows, n_cols, ptr, col, val, Xt, Ybuf[:, :k])
    want = np.full_like(Ybuf, 99.0)
    want[:n_cols, :k] = A.T @ Xt
    assert np.array_equal(Ybuf, want)
    Asym, _, ptr, col, val = integer_matrices["sym"]
    Xs = _block(rng, 6, k, ld)
    Ybuf = np.full((6 + 2, ld + 1), 99.0)
    sa.cpu_csr_sym_multi(6, ptr, col, val, Xs, Ybuf[:, :k])
    want = np.full_like(Ybuf, 99.0)
    want[:6, :k] = Asym @ Xs
    assert np.array_equal(Ybuf, want)


# ---------------------------------------------------------------- info dicts
def test_info_dicts_keep_their_keys_and_values():
    """The five *_info properties through one reader: a stub library fills the
    structs, and each dict is what the hand-written conversion gave."""
    filled = {}

    class Lib:
        def __getattr__(self, name):
            def get(plan, ref):
                info = ref._obj
                for i, (field, ctype) in enumerate(type(info)._fields_):
                    if field == "kernel":
                        info.kernel = name.encode()
                    elif field == "mode":
                        info.mode = 1
                    elif issubclass(ctype, ctypes.Array):
                        setattr(info, field, ctype(*range(10 * i, 10 * i + 4)))
                    else:
                        setattr(info, field, 7 + i)
                filled[name] = info
                return sa.SUCCESS

            return get

    dm = sa.DeviceMatrix("csr", 6, 6, 6, "cpu", plan=None)
    saved, sa.hip_lib = sa.hip_lib, Lib
    try:
        for prop in ("multi_info", "transpose_info", "transpose_multi_info", "symmetric_info", "symmetric_multi_info"):
            with pytest.raises(sa.SpmvError) as e:
                getattr(dm, prop)
            assert e.value.rc == sa.OTHER_ERROR and str(e.value) == f"{prop} failed: rc=4 format csr has no plan"
        dm.plan = 1
        assert dm.multi_info == {
            "mode": "balanced", "long_len": 8, "seg_len": 9, "long_rows": 11, "segments": 12, "slots": 13,
            "long_entries": 14, "owned_bytes": 15, "t_long_rows": 16, "t_segments": 17, "t_owned_bytes": 18,
            "kernel": "spmv_plan_get_multi_info"}
        assert dm.transpose_info == {
            "mode": "scatter", "cap": 8, "blocks": 9, "lds_blocks": 10, "flush_entries": 11, "owned_bytes": 12,
            "kernel": "spmv_plan_get_transpose_info"}
        assert dm.transpose_multi_info == {
            "mode": "scatter", "cap_cols": [20, 21, 22, 23], "lds_blocks": [30, 31, 32, 33],
            "kernel": "spmv_plan_get_transpose_multi_info"}
        assert dm.symmetric_info == {
            "mode": "fused", "cap": 8, "blocks": 9, "window_blocks": 10, "flush_entries": 11, "nnz_expanded": 12,
            "owned_bytes": 13, "kernel": "spmv_plan_get_symmetric_info"}
        assert dm.symmetric_multi_info == {
            "mode": "fused", "cap_cols": [20, 21, 22, 23], "window_blocks": [30, 31, 32, 33],
            "flush_entries": [40, 41, 42, 43], "long_rows": 12, "segments": 13, "multi_owned_bytes": 14,
            "kernel": "spmv_plan_get_symmetric_multi_info"}
        for d in (dm.multi_info, dm.transpose_multi_info):
            assert all(type(v) in (int, str, list) for v in d.values())
    finally:
        dm.plan = None
        sa.hip_lib = saved
