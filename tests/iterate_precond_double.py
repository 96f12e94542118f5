"""Numpy stand-in for the preconditioner methods of iterate.HipKernels: TEST
INFRASTRUCTURE ONLY (as tests/iterate_multi_double.py, which it extends).

The preconditioner itself is the host statement (sa.bjacobi_build_host,
sa.cpu_bjacobi_apply_multi), built from a rank's shard exactly as
iterate.build_operator builds the device one.
"""
from __future__ import annotations

import numpy as np
import torch

import iterate as it
import spmv_amd as sa
from iterate_multi_double import NumpyMultiKernels


class HostBlockJacobi:
    """sa.BlockJacobi's stand-in: the inverse blocks of a shard, on the host."""

    def __init__(self, shard: sa.Coo, bs: int, col_base: int = 0, symmetric_half: bool = False):
        ptr, col, val = sa.csr_from_coo(shard)
        self.n, self.bs = shard.n_rows, bs
        self.inv, self.singular = sa.bjacobi_build_host(shard.n_rows, ptr, col, val, bs, col_base, symmetric_half)


class NumpyPrecondKernels(NumpyMultiKernels):
    def precond_apply_dot(self, M, n, R, Z, out, ws):
        assert n == M.n
        k = R.shape[1]
        r = np.ascontiguousarray(R[:n].numpy())
        z = np.empty_like(r)
        sa.cpu_bjacobi_apply_multi(n, M.bs, M.inv, r, z)
        Z[:n] = torch.from_numpy(z)
        out[:k] = torch.from_numpy((r * z).sum(axis=0))
        out[k:2 * k] = torch.from_numpy((r * r).sum(axis=0))

    def precond_ws(self, M, n, k):
        return torch.empty(8, dtype=torch.uint8)


def np_precond_operator(m: sa.Coo, rank: int, world: int, bs: int | None, align: int = 64, split: bool = False):
    """iterate.build_operator on the numpy double: the shard, and its
    preconditioner built with the shard's col_base (rank * pad; a split
    shard: from the local part, col_base 0)."""
    counts = np.bincount(m.row, minlength=m.n_rows).astype(np.int64)
    layout = it.layout_for(m.n_rows, counts, world, align)
    loc = it.local_shard(m, layout, rank)
    if not split:
        M = HostBlockJacobi(loc, bs, rank * layout.pad) if bs else None
        return it.DistOperator(layout, rank, m.n_rows, NumpyPrecondKernels(loc), "cpu", precond=M)
    local, remote = it.split_local_remote(loc, layout, rank)
    M = HostBlockJacobi(local, bs) if bs else None
    return it.DistOperator(layout, rank, m.n_rows, NumpyPrecondKernels(local), "cpu", NumpyPrecondKernels(remote),
                           False, M)
