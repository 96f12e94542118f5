"""Numpy stand-in for the block methods of iterate.HipKernels: TEST
INFRASTRUCTURE ONLY (as tests/iterate_double.py, which it extends).

The ratio methods restate the rule of the device kernels: a zero denominator
gives the ratio 0.
"""
from __future__ import annotations

import numpy as np
import torch

from iterate_double import NumpyKernels


def _ratio(num, den):
    num, den = num.numpy(), den.numpy()
    c = np.zeros_like(num)
    nz = den != 0.0
    c[nz] = num[nz] / den[nz]
    return torch.from_numpy(c)


class NumpyMultiKernels(NumpyKernels):
    multi_supported = True

    def spmm(self, X_full, Y):
        r = self.A.shape[0]
        Y[:r] = torch.from_numpy(self.A @ X_full.numpy())

    def dot_multi(self, n, A, B, out, ws):
        out[:] = (A[:n] * B[:n]).sum(dim=0)

    def axpy_ratio_multi(self, n, num, den, sign, X, Y):
        Y[:n] += sign * _ratio(num, den) * X[:n]

    def xpay_ratio_multi(self, n, num, den, X, Y):
        Y[:n] = X[:n] + _ratio(num, den) * Y[:n]

    def dot_multi_ws(self, n, k):
        return torch.empty(8, dtype=torch.uint8)
