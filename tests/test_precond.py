"""Block-Jacobi preconditioned CG — the parts that need no GPU: the host
statement (spmv_bjacobi_build, spmv_cpu_bjacobi_apply_multi), the solvers'
orchestration on the numpy double (one rank and two gloo ranks) and the
refusals of every entry point.  tests/test_precond_gpu.py runs the device
object and the same solvers through libspmv_hip.

Inverse rule.  e(X) = max |I - D_q X| in np.longdouble; the statement passes
when e <= 8 e(np.linalg.inv(D_q)) + bs 2^-52: another elimination order and
fused rounding change the error by a small constant, not by orders of
magnitude.  Enforced on every block LAPACK calls well conditioned (cond below
1e8); a block with a zero row or column must come back as the identity and be
counted.

Solves.  N is the iteration count of a textbook numpy PCG (precond_cases)
with the very same blocks; the solver checks rr every check_every iterations
and its recurrence rounds differently, hence at most N + check_every + N // 10
iterations.  block_congruence(20, 3): N = 78 at bs = 3 on one rank and on two
(the rank boundary, row 576, falls between two nodes); 873 at bs = 4, whose
blocks straddle the nodes; plain CG needs 2,983.  precond=False is therefore
held to 4 N with the N of bs = 3 (312 iterations): 4 x 873 would exceed what
plain CG needs and the statement would say nothing.
"""
from __future__ import annotations

import ctypes
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch

import iterate as it
import spmv_amd as sa
from conftest import GOLDEN, PKG, REPO, golden_cases
from iterate_precond_double import HostBlockJacobi, np_precond_operator
from precond_cases import block_congruence, dense_blocks, lower_half, numpy_pcg_count, rhs, scipy_csr

ALL_BS = tuple(range(1, 17))
U52 = 2.0 ** -52
TOL = 1e-10
CHECK_EVERY = 5


# ------------------------------------------------------------- inverse rule
def residual(D, X):
    """max |I - D_q X_q| per block, in np.longdouble."""
    Dl, Xl = D.astype(np.longdouble), X.astype(np.longdouble)
    eye = np.eye(D.shape[1], dtype=np.longdouble)
    return np.array([np.abs(eye - Dl[q] @ Xl[q]).max() for q in range(D.shape[0])], np.longdouble)


def check_inverse(name, D, inv, singular, bs):
    """The rule of the module docstring on every block; returns the largest
    e / bound over the well-conditioned blocks."""
    nbk = D.shape[0]
    X = inv.reshape(nbk, bs, bs)
    eye = np.eye(bs)
    assert np.isfinite(X).all(), name
    is_eye = np.array([np.array_equal(X[q], eye) for q in range(nbk)])
    plain = np.array([np.array_equal(D[q], eye) for q in range(nbk)])
    worst = 0.0
    for q in range(nbk):
        dead = not np.isfinite(D[q]).all() or (D[q] == 0.0).all(axis=1).any() or (D[q] == 0.0).all(axis=0).any()
        if dead:
            assert is_eye[q], (name, q, "a block with a zero row or column must become the identity")
            continue
        if np.linalg.cond(D[q]) < 1e8:
            assert not is_eye[q] or plain[q], (name, q, "a regular block was replaced")
            e = residual(D[q:q + 1], X[q:q + 1])[0]
            bound = 8 * residual(D[q:q + 1], np.linalg.inv(D[q])[None])[0] + bs * U52
            assert e <= bound, (name, bs, q, float(e), float(bound))
            worst = max(worst, float(e / bound))
    assert singular == int((is_eye & ~plain).sum()), (name, bs, singular)
    return worst


def square_fixtures():
    out = []
    for case in golden_cases():
        if case["n_rows"] == case["n_cols"]:
            out.append(sa.read_mtx(GOLDEN / (case["name"] + ".mtx")))
    return out


def host_inverse(m, bs, col_base=0, half=False):
    ptr, col, val = sa.csr_from_coo(m)
    return sa.bjacobi_build_host(m.n_rows, ptr, col, val, bs, col_base, half)


@pytest.mark.parametrize("bs", ALL_BS)
def test_extraction_and_inverse_on_fixtures(bs):
    fixtures = square_fixtures()
    assert len(fixtures) >= 5
    for m in fixtures + [block_congruence(6, 3)]:
        inv, singular = host_inverse(m, bs)
        assert inv.shape == ((m.n_rows + bs - 1) // bs * bs, bs)
        worst = check_inverse(m.label, dense_blocks(m, bs), inv, singular, bs)
        print(f"bs={bs} {os.path.basename(m.label)}: {singular} singular, max e/bound {worst:.3g}")


@pytest.mark.parametrize("bs", ALL_BS)
def test_symmetric_half_gives_the_full_matrix_inverse(bs):
    """The lower half with symmetric_half against the blocks of the FULL
    matrix; the stored half's own dense extraction agrees with them too."""
    m = block_congruence(6, 3)
    half = lower_half(m)
    D = dense_blocks(m, bs)
    Dh = dense_blocks(half, bs, symmetric_half=True)
    assert np.abs(D - Dh).max() <= 2 * U52 * np.abs(D).max()  # A' is symmetric to the last bit or two
    inv, singular = host_inverse(half, bs, half=True)
    assert singular == 0
    print(f"bs={bs}: max e/bound {check_inverse('lower half', D, inv, singular, bs):.3g}")
    # without the flag the blocks are lower triangular: another inverse
    if bs > 1:
        assert not np.array_equal(inv, host_inverse(half, bs)[0])


@pytest.mark.parametrize("bs", [1, 3, 4, 16])
def test_shard_with_col_base(bs):
    """Rank 1 of 2 in the gathered layout: its own columns start at pad."""
    m = block_congruence(6, 3)
    counts = np.bincount(m.row, minlength=m.n_rows).astype(np.int64)
    layout = it.layout_for(m.n_rows, counts, 2, 8)
    lo, hi = int(layout.bounds[1]), int(layout.bounds[2])
    assert 0 < lo < hi and layout.pad >= hi - lo
    loc = it.local_shard(m, layout, 1)
    inv, singular = host_inverse(loc, bs, col_base=layout.pad)
    worst = check_inverse("shard", dense_blocks(m, bs, lo, hi), inv, singular, bs)
    print(f"bs={bs}: rows {lo}..{hi}, max e/bound {worst:.3g}")
    wrong = host_inverse(loc, bs, col_base=0)[0]  # rank 0's columns are not this rank's diagonal
    assert not np.array_equal(wrong, inv)


@pytest.mark.parametrize("bs", ALL_BS)
def test_tiny_sizes(bs):
    """n = 0, n = 1 and n = bs - 1 < bs: one short block completed with the
    identity."""
    ptr0 = np.zeros(1, np.int64)
    inv, singular = sa.bjacobi_build_host(0, ptr0, np.zeros(0, np.int32), np.zeros(0), bs)
    assert inv.shape == (0, bs) and singular == 0
    for n in sorted({1, bs - 1} - {0}):
        rng = np.random.default_rng(n)
        A = rng.uniform(-1, 1, (n, n)) + n * np.eye(n)
        r, c = np.nonzero(np.ones((n, n)))
        m = sa.Coo(n, n, r.astype(np.int32), c.astype(np.int32), A[r, c].copy(), False, f"dense {n}")
        inv, singular = host_inverse(m, bs)
        assert inv.shape == (bs, bs) and singular == 0
        check_inverse(m.label, dense_blocks(m, bs), inv, singular, bs)
        assert np.array_equal(inv[n:, n:], np.eye(bs - n)) and not inv[:n, n:].any() and not inv[n:, :n].any()


def test_singular_blocks_become_the_identity():
    def build(rows, cols, vals, n, bs):
        m = sa.Coo(n, n, np.array(rows, np.int32), np.array(cols, np.int32), np.array(vals, np.float64), False, "")
        return host_inverse(m, bs)

    inv, singular = build([0, 2], [0, 2], [2.0, 4.0], 3, 1)  # row 1: no diagonal
    assert singular == 1 and np.array_equal(inv[:, 0], [0.5, 1.0, 0.25])
    inv, singular = build([0, 0, 1, 1, 2, 3], [0, 1, 0, 1, 3, 2], [2.0, 0.0, 0.0, 4.0, 5.0, 5.0], 6, 2)
    # block 0 regular, block 1 = [[0, 5], [5, 0]] regular through its pivoting, block 2 all zero
    assert singular == 1
    assert np.array_equal(inv[0:2], [[0.5, 0.0], [0.0, 0.25]])
    assert np.array_equal(inv[2:4], [[0.0, 0.2], [0.2, 0.0]])
    assert np.array_equal(inv[4:6], np.eye(2))
    inv, singular = build([0, 0, 1, 1, 2, 3], [0, 1, 0, 1, 2, 3], [1.0, float("nan"), 2.0, 3.0, 1.0, 1.0], 4, 2)
    assert singular == 1 and np.array_equal(inv, np.tile(np.eye(2), (2, 1)))
    inv, singular = build([0, 0, 1, 1], [0, 1, 0, 1], [1.0, 2.0, 2.0, 4.0], 2, 2)  # rank 1: an exact zero pivot
    assert singular == 1 and np.array_equal(inv, np.eye(2))
    inv, singular = build([0, 1], [0, 1], [float("inf"), 1.0], 2, 2)
    assert singular == 1 and np.array_equal(inv, np.eye(2))


def test_duplicates_add_and_foreign_columns_are_ignored():
    m = sa.Coo(4, 4, np.array([0, 0, 0, 1, 1, 2, 3, 3], np.int32), np.array([0, 0, 3, 1, 2, 2, 3, 0], np.int32),
               np.array([1.0, 3.0, 9.0, 2.0, 9.0, 8.0, 5.0, 9.0]), False, "dup")
    inv, singular = host_inverse(m, 2)
    assert singular == 0 and np.array_equal(inv, [[0.25, 0.0], [0.0, 0.5], [0.125, 0.0], [0.0, 0.2]])
    ptr, col, val = sa.csr_from_coo(m)
    col = col.copy()
    col[col == 3] = np.where(np.arange((col == 3).sum()) % 2 == 0, 2_000_000_000, -5)  # out of range: ignored
    inv, singular = sa.bjacobi_build_host(4, ptr, col, val, 2)
    assert singular == 1 and np.array_equal(inv[2:], np.eye(2))  # row 3 lost its diagonal


# -------------------------------------------------------------------- apply
def fma_chain(inv, R, n, bs):
    """The statement's chain, element by element (math.fma, Python >= 3.13)."""
    Z = np.empty((n, R.shape[1]))
    for i in range(n):
        r0 = i // bs * bs
        nb = min(bs, n - r0)
        for j in range(R.shape[1]):
            s = inv[i, 0] * R[r0, j]
            for c in range(1, nb):
                s = math.fma(inv[i, c], R[r0 + c, j], s)
            Z[i, j] = s
    return Z


@pytest.mark.parametrize("bs", ALL_BS)
def test_host_apply(bs):
    rng = np.random.default_rng(bs)
    for n in (1, bs - 1, 67):
        if n < 1:
            continue
        nbk = (n + bs - 1) // bs
        inv = rng.uniform(-1, 1, (nbk * bs, bs))
        for k, ld in ((1, 1), (3, 3), (5, 8)):
            Rbuf = rng.uniform(-1, 1, (n, ld))
            Rbuf[:, k:] = np.nan  # padding must not be read
            Zbuf = np.full((n + 2, ld), 12345.0)
            sa.cpu_bjacobi_apply_multi(n, bs, inv, Rbuf[:, :k], Zbuf[:, :k])
            assert (Zbuf[n:] == 12345.0).all() and (Zbuf[:, k:] == 12345.0).all()
            Z, R = Zbuf[:n, :k], Rbuf[:, :k]
            if hasattr(math, "fma"):
                assert np.array_equal(Z.view(np.int64), fma_chain(inv, R, n, bs).view(np.int64)), (n, k)
                continue
            for i in range(n):
                r0 = i // bs * bs
                nb = min(bs, n - r0)
                a = inv[i, :nb].astype(np.longdouble)[:, None]
                ref = (a * R[r0:r0 + nb].astype(np.longdouble)).sum(axis=0)
                mag = (np.abs(a) * np.abs(R[r0:r0 + nb]).astype(np.longdouble)).sum(axis=0)
                assert (np.abs(Z[i].astype(np.longdouble) - ref) <= (bs + 1) * 2.0 ** -53 * mag).all(), (n, k, i)


# ------------------------------------------------------------------- solves
GRID, B_NODE = 20, 3


def _solve(rank, world, comm=None):
    """Every case on this rank: {(solver, bs): (iterations, rel, x)} plus the
    unpreconditioned run held to 4 N."""
    m = block_congruence(GRID, B_NODE)
    B = rhs(m.n_rows)
    out = {}
    n3 = None
    for bs in (3, 4):
        op = np_precond_operator(m, rank, world, bs)
        N = numpy_pcg_count(m, B, bs, op.layout.bounds)
        n3 = N if bs == 3 else n3
        Bl = torch.from_numpy(B[op.lo:op.lo + op.rows].copy())
        X, its, rel = it.cg_multi(op, Bl, comm, tol=TOL, maxit=10 * N, check_every=CHECK_EVERY)
        out["multi", bs] = (N, its, rel, X.numpy().copy())
        x, its, rel = it.cg(op, Bl[:, 1].contiguous(), comm, tol=TOL, maxit=10 * N, check_every=CHECK_EVERY)
        out["cg", bs] = (numpy_pcg_count(m, B[:, 1:2], bs, op.layout.bounds), its, np.array([rel]),
                         x.numpy().copy()[:, None])
    X, its, rel = it.cg_multi(op, Bl, comm, tol=TOL, maxit=4 * n3, check_every=CHECK_EVERY, precond=False)
    out["plain", 0] = (n3, its, rel, X.numpy().copy())
    x, its, rel = it.cg(op, Bl[:, 1].contiguous(), comm, tol=TOL, maxit=4 * n3, check_every=CHECK_EVERY, precond=False)
    out["plain cg", 0] = (n3, its, np.array([rel]), x.numpy().copy()[:, None])
    return op.lo, out


def _check_case(key, N, its, rel, X):
    m = block_congruence(GRID, B_NODE)
    A, B = scipy_csr(m), rhs(m.n_rows)
    cols = [1] if key[0].endswith("cg") else [0, 1, 2]
    print(f"{key}: N = {N}, {its} iterations, rel {rel}")
    if key[0].startswith("plain"):
        assert its == 4 * N and not (rel <= TOL).all(), (key, its, rel)  # no preconditioner: far from done
        return
    assert its <= N + CHECK_EVERY + N // 10, (key, its, N)
    assert (rel <= TOL).all()
    for j, c in enumerate(cols):
        res = np.linalg.norm(B[:, c] - A @ X[:, j])
        print(f"   column {c}: true residual {res / np.linalg.norm(B[:, c]):.3g}")
        assert res <= 2e-10 * np.linalg.norm(B[:, c]), (key, c, res)


@pytest.fixture(scope="module")
def one_rank():
    return _solve(0, 1)


def test_pcg_single_rank(one_rank):
    lo, out = one_rank
    assert lo == 0 and out["multi", 3][0] == 78
    for key, (N, its, rel, X) in out.items():
        _check_case(key, N, its, rel, X)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path[:0] = [str(PKG), str(REPO), str(REPO / "tests")]
    import torch.distributed as dist

    import iterate as it2

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        q.put((rank,) + _solve(rank, world, it2.Comm(dist)))
    finally:
        dist.destroy_process_group()


def test_pcg_two_ranks(one_rank):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, lo0, out0), (_, lo1, out1) = res
    assert lo0 == 0 and lo1 == out0["multi", 3][3].shape[0]
    for key in out0:
        N, its, rel, x0 = out0[key]
        assert (N, its) == out1[key][:2] and np.array_equal(rel, out1[key][2])  # the all-reduced scalars
        X = np.concatenate([x0, out1[key][3]])
        _check_case(key, N, its, rel, X)
        if key[0].startswith("plain"):
            continue
        X1 = one_rank[1][key][3]
        for j in range(X.shape[1]):
            d = np.linalg.norm(X[:, j] - X1[:, j]) / np.linalg.norm(X1[:, j])
            print(f"   column {j}: two ranks against one {d:.3g}")
            assert d <= 1e-9, (key, j, d)


def test_pcg_zero_column_split_operator_and_explicit_precond():
    m = block_congruence(8, 3)
    n = m.n_rows
    op = np_precond_operator(m, 0, 1, 3)
    B = torch.zeros(n, 2, dtype=torch.float64)
    B[:, 0] = 1.0
    X, its, rel = it.cg_multi(op, B, tol=TOL, maxit=500, check_every=CHECK_EVERY)
    assert its < 100 and rel[1] == 0.0 and rel[0] <= TOL
    assert (X[:, 1] == 0.0).all() and torch.isfinite(X).all()
    X0, its0, rel0 = it.cg_multi(op, torch.zeros(n, 2, dtype=torch.float64))
    assert its0 == 0 and (rel0 == 0.0).all() and (X0 == 0.0).all()
    x, its0, rel0 = it.cg(op, torch.zeros(n, dtype=torch.float64))
    assert its0 == 0 and rel0 == 0.0 and (x == 0.0).all()
    # an operator without a preconditioner takes one by keyword, and the same iterates come out
    bare = np_precond_operator(m, 0, 1, None)
    assert bare.precond is None
    X2, its2, _ = it.cg_multi(bare, B, tol=TOL, maxit=500, check_every=CHECK_EVERY, precond=op.precond)
    assert its2 == its and torch.equal(X2, X)
    # cg (not cg_multi) runs split operators; the preconditioner comes from the local part
    sp_op = np_precond_operator(m, 0, 1, 3, split=True)
    x, its3, rel3 = it.cg(sp_op, B[:, 0].contiguous(), tol=TOL, maxit=500, check_every=CHECK_EVERY)
    assert its3 <= its + CHECK_EVERY and rel3 <= TOL
    assert np.linalg.norm(x.numpy() - X[:, 0].numpy()) <= 1e-9 * np.linalg.norm(X[:, 0].numpy())


# ---------------------------------------------------------------- refusals
def test_host_refusals():
    lib = sa.host_lib()
    ptr = np.array([0, 1, 2], np.int64)
    col = np.array([0, 1], np.int32)
    val = np.array([2.0, 4.0])
    inv = np.full(4, 7.0)
    s = ctypes.c_int64(-3)
    P = sa._ptr
    ok = (2, P(ptr), P(col), P(val), 2, 0, 0, P(inv), ctypes.byref(s))

    def build(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.spmv_bjacobi_build(*a)

    for bad in (dict(a0=-1), dict(a4=0), dict(a4=17), dict(a4=-1), dict(a5=-1), dict(a1=None), dict(a2=None),
                dict(a3=None), dict(a7=None), dict(a8=None)):
        assert build(**bad) == sa.OTHER_ERROR, bad
    assert (inv == 7.0).all() and s.value == -3  # nothing written
    assert build() == sa.SUCCESS and s.value == 0 and np.array_equal(inv, [0.5, 0.0, 0.0, 0.25])
    R = np.ones((2, 3))
    Z = np.full((2, 3), 7.0)
    ok = (2, 2, P(inv), 3, P(R), 3, P(Z), 3)

    def apply(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return lib.spmv_cpu_bjacobi_apply_multi(*a)

    for bad in (dict(a0=-1), dict(a1=0), dict(a1=17), dict(a3=0), dict(a5=2), dict(a7=2), dict(a2=None), dict(a4=None),
                dict(a6=None)):
        assert apply(**bad) == sa.OTHER_ERROR, bad
    assert (Z == 7.0).all()
    assert apply() == sa.SUCCESS and np.array_equal(Z, [[0.5] * 3, [0.25] * 3])
    for bs in (0, 17):
        with pytest.raises(sa.SpmvError):
            sa.bjacobi_build_host(2, ptr, col, val, bs)
    with pytest.raises(sa.SpmvError):
        sa.cpu_bjacobi_apply_multi(2, 2, inv, R, Z[:, :2])  # Z narrower than k
    with pytest.raises(sa.SpmvError):
        sa.cpu_bjacobi_apply_multi(2, 2, inv[:3], R, Z)  # inv too short


def test_device_entry_points_refuse_before_touching_a_device():
    """Argument errors are reported as such with or without a GPU."""
    lib = sa.hip_lib()
    ptr = (ctypes.c_int64 * 3)(0, 1, 2)
    a = ctypes.addressof(ptr)  # never dereferenced: every call below is refused
    h = ctypes.c_void_p(0)
    d = sa.Dims(2, 2, 2, 0, None)
    for dims, args in ((d, (a, a, a, 0, 0, 0)), (d, (a, a, a, 17, 0, 0)), (d, (a, a, a, 3, -1, 0)),
                       (d, (None, a, a, 3, 0, 0)), (d, (a, None, a, 3, 0, 0)), (d, (a, a, None, 3, 0, 0)),
                       (sa.Dims(-1, 2, 2, 0, None), (a, a, a, 3, 0, 0)), (sa.Dims(2, 2, -1, 0, None), (a, a, a, 3, 0, 0))):
        assert lib.spmv_bjacobi_create(dims, *args, ctypes.byref(h)) == sa.OTHER_ERROR and not h.value
    assert lib.spmv_bjacobi_create(d, a, a, a, 3, 0, 0, None) == sa.OTHER_ERROR
    info = sa.BjacobiInfo()
    assert lib.spmv_bjacobi_get_info(None, ctypes.byref(info)) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_inverse(None, ctypes.byref(h)) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_apply_multi(None, 1, a, 1, a, 1, None) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_apply_dot_multi(None, 1, a, 1, a, 1, a, a, 1 << 20, None) == sa.OTHER_ERROR
    assert lib.spmv_bjacobi_destroy(None) == sa.SUCCESS
    assert lib.spmv_bjacobi_ws_bytes(5000, 3) == 2 * lib.spmv_dot_multi_ws_bytes(5000, 3)
    assert lib.spmv_bjacobi_ws_bytes(0, 0) == 16


@pytest.mark.parametrize("bs", [0, 17, -1, 2.5, True])
def test_python_refusals_before_any_upload(bs, monkeypatch):
    def no_upload(*a, **k):
        raise AssertionError("uploaded before refusing")

    monkeypatch.setattr(sa, "to_device", no_upload)
    monkeypatch.setattr(sa, "_dev_tensor", no_upload)
    m = block_congruence(6, 3)
    with pytest.raises(sa.SpmvError):
        it.build_operator(m, bjacobi=bs)
    with pytest.raises(sa.SpmvError):
        it.build_operator(lower_half(m), symmetric="expand", bjacobi=bs)
    with pytest.raises(sa.SpmvError):
        sa.BlockJacobi.from_coo(m, bs, "cpu")


def test_host_block_jacobi_matches_build_operator_layout():
    """The double's preconditioner of rank 1 equals the blocks of the global
    matrix cut from that rank's rows."""
    m = block_congruence(6, 3)
    op = np_precond_operator(m, 1, 2, 4, align=8)
    assert isinstance(op.precond, HostBlockJacobi) and op.precond.singular == 0
    D = dense_blocks(m, 4, op.lo, op.lo + op.rows)
    check_inverse("rank 1", D, op.precond.inv, 0, 4)
