"""Multi-right-hand-side CG (iterate.cg_multi) — CPU tests.

The orchestration (gathered (world*pad, k) layout, one all-gather per
iteration, one all-reduce per k-vector of scalars, the stopping rule) runs
on one rank and on two gloo ranks with the numpy double of
tests/iterate_multi_double.py; tests/test_iterate_multi_gpu.py runs the same
solver through libspmv_hip on the MI355X.
"""
from __future__ import annotations

import os
import socket
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import iterate as it
import spmv_amd as sa
from conftest import PKG, REPO
from iterate_double import NumpyKernels, laplacian_2d
from iterate_multi_double import NumpyMultiKernels

GRID = 40
K = 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rhs(n):
    """(n, 3): all ones, uniform(-0.5, 0.5), e_0."""
    B = np.zeros((n, K))
    B[:, 0] = 1.0
    B[:, 1] = np.random.default_rng(7).random(n) - 0.5
    B[0, 2] = 1.0
    return B


def _np_operator(m, rank, world, kernels=NumpyMultiKernels, align=64, split=False):
    counts = np.bincount(m.row, minlength=m.n_rows).astype(np.int64)
    layout = it.layout_for(m.n_rows, counts, world, align)
    loc = it.local_shard(m, layout, rank)
    if not split:
        return it.DistOperator(layout, rank, m.n_rows, kernels(loc), "cpu")
    local, remote = it.split_local_remote(loc, layout, rank)
    return it.DistOperator(layout, rank, m.n_rows, kernels(local), "cpu", kernels(remote), False)


def _solve(rank, world, comm=None):
    m = laplacian_2d(GRID)
    op = _np_operator(m, rank, world)
    B = torch.from_numpy(_rhs(m.n_rows)[op.lo:op.lo + op.rows].copy())
    X, its, rel = it.cg_multi(op, B, comm, tol=1e-10, maxit=500, check_every=5)
    return its, rel, op.lo, X.numpy().copy()


def _check_solution(X, its, rel):
    m = laplacian_2d(GRID)
    A = sp.csr_matrix((m.val, (m.row, m.col)), shape=(m.n_rows, m.n_cols))
    B = _rhs(m.n_rows)
    assert its < 500 and rel.shape == (K,) and (rel <= 1e-10).all()
    for j in range(K):
        assert np.linalg.norm(B[:, j] - A @ X[:, j]) <= 2e-10 * np.linalg.norm(B[:, j])


@pytest.fixture(scope="module")
def one_rank():
    return _solve(0, 1)


def test_cg_multi_single_rank(one_rank):
    its, rel, lo, X = one_rank
    assert lo == 0
    _check_solution(X, its, rel)


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


def test_cg_multi_two_ranks(one_rank):
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
    (_, its0, rel0, lo0, x0), (_, its1, rel1, lo1, x1) = res
    assert its0 == its1 and np.array_equal(rel0, rel1)  # every rank sees the all-reduced scalars
    assert lo0 == 0 and lo1 == x0.shape[0]
    X = np.concatenate([x0, x1])
    _check_solution(X, its0, rel0)
    X1 = one_rank[3]
    for j in range(K):
        assert np.linalg.norm(X[:, j] - X1[:, j]) <= 1e-9 * np.linalg.norm(X1[:, j])


def test_cg_multi_zero_column_and_zero_block():
    """A zero right-hand side among others stays exactly zero (the
    den == 0 -> ratio 0 rule) and reports rel 0.0; an all-zero block returns
    at once."""
    m = laplacian_2d(12)
    op = _np_operator(m, 0, 1)
    B = torch.zeros(m.n_rows, 2, dtype=torch.float64)
    B[:, 0] = 1.0
    X, its, rel = it.cg_multi(op, B, tol=1e-10, maxit=200, check_every=5)
    assert its < 200 and rel[1] == 0.0 and rel[0] <= 1e-10
    assert torch.isfinite(X).all() and (X[:, 1] == 0.0).all()
    X, its, rel = it.cg_multi(op, torch.zeros(m.n_rows, 2, dtype=torch.float64))
    assert its == 0 and (rel == 0.0).all() and (X == 0.0).all()


def test_cg_multi_refusals():
    m = laplacian_2d(12)
    n = m.n_rows
    op = _np_operator(m, 0, 1)
    good = torch.ones(n, 2, dtype=torch.float64)
    for bad in (torch.ones(n, dtype=torch.float64),  # 1-D
                torch.ones(n, 2, dtype=torch.float32),  # dtype
                torch.ones(n + 1, 2, dtype=torch.float64),  # rows
                torch.ones(n, 0, dtype=torch.float64),  # k = 0
                torch.ones(2, n, dtype=torch.float64).t(),  # not contiguous
                np.ones((n, 2))):  # not a tensor
        with pytest.raises(sa.SpmvError):
            it.cg_multi(op, bad)
    with pytest.raises(sa.SpmvError):  # a split operator
        it.cg_multi(_np_operator(m, 0, 1, split=True), good)
    with pytest.raises(sa.SpmvError):  # kernels without a multi-vector run
        it.cg_multi(_np_operator(m, 0, 1, kernels=NumpyKernels), good)


@pytest.mark.parametrize("kw", [dict(symmetric="fused", fmt="sell"), dict(symmetric="expand", expand_symmetric=True),
                                dict(symmetric="expand", world=2), dict(symmetric="fused", split=True),
                                dict(symmetric="fused", overlap=True), dict(symmetric="both")])
def test_build_operator_symmetric_refusals(kw, monkeypatch):
    """Refused before anything is uploaded: to_device is never reached."""
    def no_upload(*a, **k):
        raise AssertionError("build_operator uploaded before refusing")

    monkeypatch.setattr(sa, "to_device", no_upload)
    m = laplacian_2d(6)
    low = m.row >= m.col
    half = sa.Coo(m.n_rows, m.n_cols, m.row[low], m.col[low], m.val[low], True, "lower")
    with pytest.raises(sa.SpmvError):
        it.build_operator(half, **kw)
