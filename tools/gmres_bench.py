#!/usr/bin/env python3
"""GMRES's Arnoldi step on its fused basis kernels against the same step
composed from the older kernels, and GMRES(20) against BiCGSTAB in time to a
tolerance (a tool, not a test; it needs a GPU and fails without one).

    timeout -k 10 900 python tools/gmres_bench.py [--grids 2048,250] [--window 0.5] [--maxit 2000]

Matrices: tools/bicgstab_bench.py's upwind convection-diffusion on a g x g grid
(px, py = 1.5, 0.5), ~5 entries per row.  g = 2048 (4.2 M rows) is
bandwidth-bound, g = 250 (62,500 rows) is launch-bound.

Step.  One Arnoldi step at a FIXED basis of c in {5, 20, 31} columns (the
product, the two Gram-Schmidt passes, the closing sums, the normalisation of
column c and the host's one read), on random data:
    fused     what iterate._gmres runs: the product, three
              spmv_krylov_project_dot, one spmv_krylov_normalize: 8 launches;
    unfused   the product, V^T w by spmv_gram_multi (two calls beyond its 24
              columns), w -= V h by torch.matmul and a subtraction, twice, then
              V^T w and w . w again and spmv_scale_rsqrt: the composition
              available before the fused kernels existed.
Solve.  iterate.gmres(restart=20) and iterate.bicgstab, no preconditioner, to
tol = 1e-10 or --maxit Arnoldi steps / iterations (a BiCGSTAB iteration has
two products, a GMRES step one); iterations and the true relative residual of
both are reported, converged or not.

By tools/bicgstab_bench.py's estimator: device events bracket windows of enough
calls to last at least --window seconds, after a warm-up; the sides alternate,
five windows each (--solve-windows for the solves); median and spread
(max - min), in ms per step or per solve.  One JSON line.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "opencl-spmv-algorithms_amd"), str(REPO), str(REPO / "tools")]
import iterate as it  # noqa: E402
import spmv_amd as sa  # noqa: E402
from bicgstab_bench import calls_for, upwind, window_ms  # noqa: E402

BASES = (5, 20, 31)
WINDOWS = 5
GRAM_MAX = 24  # spmv_gram_multi's widest block


class Step:
    """The buffers of one Arnoldi step at a basis of c columns on `op`."""

    def __init__(self, torch, op, c, rng):
        self.torch, self.op, self.c, self.k, self.rows = torch, op, c, op.kernels, op.rows
        dev, n = op.device, op.rows
        self.V = torch.from_numpy(rng.uniform(-1, 1, (n, 32)) / np.sqrt(n)).to(dev)
        self.send = torch.from_numpy(rng.uniform(-1, 1, op.pad)).to(dev)
        self.w = torch.zeros(n, dtype=torch.float64, device=dev)
        self.W = self.w.unsqueeze(1)
        self.d = torch.zeros(3, 34, dtype=torch.float64, device=dev)
        self.ws = self.k.krylov_project_ws(n)
        self.gws = self.k.gram_ws(n, GRAM_MAX, 1)
        self.dws = self.k.dot_multi_ws(n, 1)

    def fused(self):
        k, c, V, W, d, n = self.k, self.c, self.V, self.W, self.d, self.rows
        Vc, v_new = V[:, :c], V[:, c:c + 1]
        k.spmv(self.send, self.w)
        k.krylov_project_dot(n, Vc, None, W, None, d[0, :c + 1], self.ws)
        k.krylov_project_dot(n, Vc, d[0, :c], W, W, d[1, :c + 1], self.ws)
        k.krylov_project_dot(n, Vc, d[1, :c], W, v_new, d[2, :c + 1], self.ws)
        k.krylov_normalize(n, d[2, c:c + 1], v_new, v_new, self.send[:n])
        return d.cpu()

    def _vtw(self, out):
        for lo in range(0, self.c, GRAM_MAX):
            hi = min(self.c, lo + GRAM_MAX)
            self.k.gram(self.rows, self.V[:, lo:hi], self.W, out[lo:hi], self.gws)

    def unfused(self):
        k, c, V, W, d, n = self.k, self.c, self.V, self.W, self.d, self.rows
        k.spmv(self.send, self.w)
        for p in (0, 1):
            self._vtw(d[p])
            self.w.sub_(self.torch.matmul(V[:, :c], d[p, :c]))
        self._vtw(d[2])
        k.dot_multi(n, W, W, d[2, c:c + 1], self.dws)
        k.scale_rsqrt(n, d[2, c:c + 1], self.w, self.send[:n])
        V[:, c].copy_(self.send[:n])
        return d.cpu()


def alternate(torch, fns, window, windows):
    """{name: (median ms per call, spread, calls per window)} with the sides alternating."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    calls = {name: calls_for(torch, fn, window) for name, fn in fns.items()}
    w = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            w[name].append(window_ms(torch, fn, calls[name]) / calls[name])
    return {name: (statistics.median(v), max(v) - min(v), calls[name], min(v), max(v)) for name, v in w.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="2048,250", help="grid sides (rows = side^2)")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per timing window")
    ap.add_argument("--maxit", type=int, default=2000, help="cap of the solves, in GMRES steps / BiCGSTAB iterations")
    ap.add_argument("--solve-windows", type=int, default=3)
    ap.add_argument("--no-solve", action="store_true", help="time the steps only")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("gmres_bench: no GPU")
    dev = torch.device("cuda:0")
    out = {"tool": "gmres_bench", "device": sa.device_name(0), "window_s": a.window, "windows": WINDOWS,
           "solve_windows": a.solve_windows, "maxit": a.maxit, "tol": 1e-10, "results": {}}
    rng = np.random.default_rng(7)
    for g in (int(s) for s in a.grids.split(",")):
        m = upwind(g, 1.5, 0.5)
        op = it.build_operator(m, 0, 1, "csr", dev)
        res = out["results"].setdefault(str(g), {"rows": m.n_rows, "stored_entries": m.nnz, "step_ms": {}})
        for c in BASES:
            st = Step(torch, op, c, rng)
            t = alternate(torch, {"fused": st.fused, "unfused": st.unfused}, a.window, WINDOWS)
            res["step_ms"][str(c)] = {
                **{name: round(v[0], 5) for name, v in t.items()},
                **{f"{name}_spread": round(v[1], 5) for name, v in t.items()},
                "calls": {name: v[2] for name, v in t.items()},
                "unfused_over_fused": round(t["unfused"][0] / t["fused"][0], 3),
                "fused_faster": t["fused"][4] < t["unfused"][3]}
            del st
        if not a.no_solve:
            b = torch.from_numpy(rng.uniform(-0.5, 0.5, m.n_rows)).to(dev)
            fns = {"gmres20": lambda: it.gmres(op, b, tol=1e-10, maxit=a.maxit, restart=20),
                   "bicgstab": lambda: it.bicgstab(op, b, tol=1e-10, maxit=a.maxit, check_every=10)}
            got = {name: fn() for name, fn in fns.items()}
            t = alternate(torch, fns, a.window, a.solve_windows)
            res["solve"] = {name: {"ms": round(t[name][0], 3), "spread_ms": round(t[name][1], 3),
                                   "solves_per_window": t[name][2], "iterations": int(got[name][1]),
                                   "rel": float(got[name][2]), "converged": bool(got[name][2] <= 1e-10)}
                            for name in fns}
            res["solve"]["gmres_over_bicgstab"] = round(t["gmres20"][0] / t["bicgstab"][0], 3)
        del op
    print(json.dumps(out))


if __name__ == "__main__":
    main()
