"""The chunk and tail boundaries of the row-block entry stream (csrc/rowblock.h)
that the transposed scatter kernels and the fused symmetric kernel share.

A workgroup streams its block's entries 256 per pass with 4 loads in flight
per thread: chunks of 1,024 entries, then single passes of 256, the last one
partial.  edge_matrix(E) is a 160-row square lower-triangular matrix of two
blocks: block 0 (rows 0..127) holds exactly E entries over ragged rows, rows 0
and 64 empty; block 1 (the partial block of 32 rows) holds 5.  E runs one
entry short of, at and past one wave-pass (256), one chunk (1,024) and two
chunks (2,048), and a single entry.

Integer data (tests/exact.py): every product and partial sum is an integer
below 2^52 in any order, so every result must EQUAL its int64 reference.  The
host test checks the generator and those references against the library's CPU
loops; the GPU test runs run_t and run_t_multi (k = 2: one lane per entry;
k = 8: four) in scatter mode and run_sym in fused mode, outputs pre-filled
with NaN and guarded by sentinels.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import exact
import spmv_amd as sa
import test_symmetric_gpu as tsg
import test_transpose_gpu as tg
import test_transpose_multi_gpu as tmg
from test_symmetric import integer_half

N = 160
BLOCK = 128
EMPTY = (0, 64)
TAIL_ENTRIES = ((130, 3), (131, 131), (140, 129), (159, 0), (159, 158))
ES = (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)
KS = (2, 8)


@functools.lru_cache(maxsize=None)
def edge_matrix(E: int) -> sa.Coo:
    """Row-sorted, so the CSR keeps this entry order.  Block 0: the E entries
    are dealt one at a time to rows 127, 126, ..., 1 (not 64), a row of r + 1
    distinct columns at the most; each row's columns are drawn from [0, r]."""
    rng = np.random.default_rng(1000 + E)
    count = np.zeros(N, np.int64)
    rows = [r for r in range(BLOCK - 1, 0, -1) if r not in EMPTY]
    left = E
    while left:
        for r in rows:
            if left and count[r] < r + 1:
                count[r] += 1
                left -= 1
    row, col = [], []
    for r in range(BLOCK):
        row += [r] * int(count[r])
        col += sorted(rng.choice(r + 1, int(count[r]), replace=False).tolist())
    row += [r for r, _ in TAIL_ENTRIES]
    col += [c for _, c in TAIL_ENTRIES]
    val = rng.uniform(-1.0, 1.0, len(row))
    return sa.Coo(N, N, np.asarray(row, np.int32), np.asarray(col, np.int32), val, True, f"stream edge E={E}")


@functools.lru_cache(maxsize=None)
def case(E: int):
    """-> (Exact of the matrix: values, xt, ref_t; Xt[160, 8] and the int64
    A^T Xt; the half with the symmetric product's values, its x and int64
    reference)."""
    m = edge_matrix(E)
    e, Xt, ref_multi = tmg.integer_of(m, 2000 + E, max(KS))
    return e, Xt, ref_multi, integer_half(m, seed=3000 + E)


@pytest.mark.parametrize("E", ES)
def test_stream_edges_reference(E):
    """The generator's shape and the int64 references against the CPU loops."""
    m = edge_matrix(E)
    assert (m.n_rows, m.n_cols, m.nnz) == (N, N, E + len(TAIL_ENTRIES))
    assert (m.col <= m.row).all() and (np.diff(m.row) >= 0).all()
    per_row = np.bincount(m.row, minlength=N)
    assert per_row[:BLOCK].sum() == E and per_row[BLOCK:].sum() == len(TAIL_ENTRIES)
    assert all(per_row[r] == 0 for r in EMPTY)
    assert np.count_nonzero(per_row[:BLOCK]) == min(E, BLOCK - len(EMPTY))  # dealt over every other row
    assert len(set(zip(m.row.tolist(), m.col.tolist()))) == m.nnz

    e, Xt, ref_multi, (half, xs, ref_sym) = case(E)
    ptr, col, val = sa.csr_from_coo(e.m)
    assert ptr[BLOCK] == E and ptr[N] - ptr[BLOCK] == len(TAIL_ENTRIES)
    assert np.array_equal(col, m.col)
    y = np.full(N, np.nan)
    sa.cpu_csr_t(N, N, ptr, col, val, np.array(e.xt), y)
    exact.assert_exact(y, e.ref_t, f"E={E} cpu_csr_t")
    Y = np.full((N, max(KS)), np.nan)
    sa.cpu_csr_t_multi(N, N, ptr, col, val, np.array(Xt), Y)
    exact.assert_exact(Y, ref_multi, f"E={E} cpu_csr_t_multi")
    ptr, col, val = sa.csr_from_coo(half)
    y = np.full(N, np.nan)
    sa.cpu_csr_sym(N, ptr, col, val, np.array(xs), y)
    exact.assert_exact(y, ref_sym, f"E={E} cpu_csr_sym")


@pytest.mark.gpu
@pytest.mark.parametrize("E", ES)
def test_stream_edges(E):
    import torch

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    e, Xt, ref_multi, (half, xs, ref_sym) = case(E)

    dm = sa.to_device(e.m, "csr", dev)
    dm.prepare_transpose("scatter")
    info = dm.transpose_info
    assert (info["blocks"], info["lds_blocks"]) == (2, 2)
    assert dm.transpose_multi_info["lds_blocks"] == [2, 2, 2, 2]
    y = tg.run_t(torch, dev, dm, e.m, e.xt)
    exact.assert_exact(y[:N], e.ref_t, f"E={E} run_t")
    assert np.array_equal(y[N:].view(np.int64), np.full(tg.TAIL, tg.SENTINEL).view(np.int64)), "tail of y written"
    for k in KS:
        Y = tmg.run_t_multi(torch, dev, dm, e.m, Xt, k, "plain")  # asserts Y's guards
        exact.assert_exact(Y, ref_multi[:, :k], f"E={E} run_t_multi k={k}")

    ds = sa.to_device(half, "csr", dev)
    ds.prepare_symmetric("fused")
    info = ds.symmetric_info
    assert (info["blocks"], info["window_blocks"]) == (2, 2)
    exact.assert_exact(tsg.run_sym(torch, dev, ds, xs), ref_sym, f"E={E} run_sym")  # asserts y's tail
