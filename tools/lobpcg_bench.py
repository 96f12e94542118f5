#!/usr/bin/env python3
"""LOBPCG on its two fused block kernels against the same iteration composed
from the kernels that existed before them (a tool, not a test; it needs a GPU
and fails without one).

    timeout -k 10 900 python tools/lobpcg_bench.py [--matrices cantlike_sym,cantlike_sym_bj3,laplacian512]
                                                   [--iters 30] [--tol 1e-6] [--maxit 300] [--window 0.3]

Matrices: the cant-like pattern made symmetric and diagonally dominant (62,451
rows, ~64 entries per row; tools/cg_multi_bench.py's cantlike_sym), without a
preconditioner and with bjacobi = 3, and the 5-point Laplacian on a 512 x 512
grid (262,144 rows).  k in {1, 2, 4, 8}, smallest eigenpairs, format csr.

Both sides run iterate.lobpcg itself, so the iteration is the same by
construction; they differ in the kernels object:
    fused     iterate.HipKernels: spmv_gram_multi (up to four stage-1 launches
              and a final one per Gram matrix) and spmv_block_combine_multi
              (one launch, C in the kernel arguments);
    composed  Gram from ka * kb spmv_dot_multi(n, 1, ...) calls on column
              slices (two launches each), the combine by torch.matmul: C
              uploaded, one mm / addmm per operand block and a copy into Y's
              columns.
Per iteration: tol = 0 and maxit = --iters, so every solve runs exactly
--iters iterations (start, closing product and allocation included on both
sides); device events bracket windows of enough solves to last --window
seconds after a warm-up, the two alternate, five windows each; median and
spread (max - min) in ms per iteration.  To tolerance: one solve each at --tol
with --maxit, wall clock with a final synchronisation; iterations, converged
columns and ms.

Shares: one more solve of each form with a synchronisation after every kernels
call, wall clock per category (product, gram, combine, other kernels); what is
left of the solve's wall clock is the host step (Cholesky, eigh, the reads of
the small matrices).  Launches are counted, not measured: per call, from the
widths.  One JSON line.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "opencl-spmv-algorithms_amd"), str(REPO)]
import iterate as it  # noqa: E402
import spmv_amd as sa  # noqa: E402
from cg_multi_bench import cantlike_sym, laplacian_2d  # noqa: E402

KS = (1, 2, 4, 8)
WINDOWS = 5
GRAM_TILE = 4  # csrc/block.hip


class ComposedKernels(it.HipKernels):
    """gram and block_combine from what the library had before them."""

    def gram(self, n, A, B, out, ws) -> None:
        ka, kb = A.shape[1], B.shape[1]
        for a in range(ka):
            for b in range(kb):
                self.dot_multi(n, A[:, a:a + 1], B[:, b:b + 1], out[a * kb + b:a * kb + b + 1], ws)

    def gram_ws(self, n, ka, kb):
        return self.dot_multi_ws(n, 1)

    def block_combine(self, n, C, blocks, Y) -> None:
        torch = sa._torch()
        Cd = torch.from_numpy(np.ascontiguousarray(C, np.float64)).to(self.dev)
        acc, r0 = None, 0
        for t in blocks:
            w = t.shape[1]
            acc = t[:n] @ Cd[r0:r0 + w] if acc is None else acc.addmm_(t[:n], Cd[r0:r0 + w])
            r0 += w
        Y[:n].copy_(acc)


def gram_launches(fused: bool, ka: int, kb: int) -> int:
    if not fused:
        return 2 * ka * kb
    parts = lambda k: (k // GRAM_TILE > 0) + (k % GRAM_TILE > 0)  # noqa: E731
    return parts(ka) * parts(kb) + 1


class Profiled:
    """Wraps a kernels object: counts launches per category; sync=True also
    times every call with a synchronisation behind it."""

    CATEGORY = {"spmm": "product", "gram": "gram", "block_combine": "combine"}

    def __init__(self, inner, fused: bool, sync: bool):
        self._k, self._fused, self._sync = inner, fused, sync
        self.ms = {c: 0.0 for c in ("product", "gram", "combine", "other")}
        self.launches = dict(self.ms)
        self.multi_supported = inner.multi_supported
        self.stream = inner.stream
        self.dm = inner.dm

    def __getattr__(self, name):
        fn = getattr(self._k, name)
        if name.endswith("_ws") or not callable(fn):
            return fn
        cat = self.CATEGORY.get(name, "other")

        def call(*a, **kw):
            if name == "gram":
                self.launches[cat] += gram_launches(self._fused, a[1].shape[1], a[2].shape[1])
            elif name == "block_combine":
                self.launches[cat] += 1 if self._fused else len(a[2]) + 1
            elif name in ("dot_multi", "dot2_multi"):
                self.launches[cat] += 2
            else:
                self.launches[cat] += 1
            if not self._sync:
                return fn(*a, **kw)
            torch = sa._torch()
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            self.ms[cat] += (time.perf_counter() - t) * 1e3
            return out

        return call


def window_ms(torch, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def calls_for(torch, fn, seconds):
    n = 1
    while True:
        ms = window_ms(torch, fn, n)
        if ms >= seconds * 1e3:
            return n
        n = max(n + 1, int(n * seconds * 1e3 / max(ms, 1e-3) * 1.1) + 1)


def with_kernels(op, kernels):
    return it.DistOperator(op.layout, op.rank, op.n, kernels, op.device, precond=op.precond)


def build(name, dev):
    if name == "cantlike_sym":
        return it.build_operator(cantlike_sym(), 0, 1, "csr", dev)
    if name == "cantlike_sym_bj3":
        return it.build_operator(cantlike_sym(), 0, 1, "csr", dev, bjacobi=3)
    if name.startswith("laplacian"):
        return it.build_operator(laplacian_2d(int(name[len("laplacian"):])), 0, 1, "csr", dev)
    sys.exit(f"lobpcg_bench: unknown matrix {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="cantlike_sym,cantlike_sym_bj3,laplacian512")
    ap.add_argument("--iters", type=int, default=30, help="iterations per timed solve (tol = 0)")
    ap.add_argument("--tol", type=float, default=1e-6, help="tolerance of the solve to tolerance")
    ap.add_argument("--maxit", type=int, default=300, help="cap of the solve to tolerance")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of solves per timing window")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("lobpcg_bench: no GPU")
    dev = torch.device("cuda:0")
    out = {"tool": "lobpcg_bench", "device": sa.device_name(0), "window_s": a.window, "windows": WINDOWS,
           "iters": a.iters, "tol": a.tol, "maxit": a.maxit, "unit": "ms per iteration, all k columns", "results": {}}
    for name in a.matrices.split(","):
        op = build(name, dev)
        forms = {"fused": op.kernels, "composed": ComposedKernels(op.kernels.dm)}
        res = out["results"].setdefault(name, {"rows": op.n})
        for k in KS:
            ops = {f: with_kernels(op, kn) for f, kn in forms.items()}
            fns = {f: (lambda o=o: it.lobpcg(o, k=k, tol=0.0, maxit=a.iters)) for f, o in ops.items()}
            got = {f: fn() for f, fn in fns.items()}  # warm-up
            assert all(r[2] == a.iters for r in got.values()), {f: r[2] for f, r in got.items()}
            torch.cuda.synchronize()
            calls = {f: calls_for(torch, fn, a.window) for f, fn in fns.items()}
            w = {f: [] for f in fns}
            for _ in range(WINDOWS):  # the two alternate
                for f, fn in fns.items():
                    w[f].append(window_ms(torch, fn, calls[f]) / (calls[f] * a.iters))
            med = {f: statistics.median(v) for f, v in w.items()}
            row = {**{f"{f}_ms": round(med[f], 5) for f in fns},
                   **{f"{f}_spread_ms": round(max(v) - min(v), 5) for f, v in w.items()},
                   "composed_over_fused": round(med["composed"] / med["fused"], 3),
                   "fused_faster": max(w["fused"]) < min(w["composed"]),
                   "fused_slower": min(w["fused"]) > max(w["composed"]),
                   "lam_rel_diff": float(np.abs(got["fused"][0] - got["composed"][0]).max() / np.abs(got["fused"][0]).max())}
            for f, kn in forms.items():
                # shares and launch counts: one solve with a synchronisation behind every call
                prof = Profiled(kn, f == "fused", True)
                torch.cuda.synchronize()
                t = time.perf_counter()
                it.lobpcg(with_kernels(op, prof), k=k, tol=0.0, maxit=a.iters)
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t) * 1e3
                host = max(wall - sum(prof.ms.values()), 0.0)
                row[f"{f}_share"] = {**{c: round(v / wall, 3) for c, v in prof.ms.items()}, "host": round(host / wall, 3)}
                row[f"{f}_launches_per_iteration"] = {c: round(v / a.iters, 1) for c, v in prof.launches.items()}
                # to tolerance
                torch.cuda.synchronize()
                t = time.perf_counter()
                lam, _, its, r = it.lobpcg(ops[f], k=k, tol=a.tol, maxit=a.maxit)
                torch.cuda.synchronize()
                row[f"{f}_to_tol"] = {"iterations": its, "ms": round((time.perf_counter() - t) * 1e3, 2),
                                      "converged_columns": int((r <= a.tol * np.abs(lam)).sum())}
            res[str(k)] = row
        del op, forms
    print(json.dumps(out))


if __name__ == "__main__":
    main()
