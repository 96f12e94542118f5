#!/usr/bin/env python3
"""BiCGSTAB on its fused vector kernels against the same recurrence composed
from the older block kernels, and against CG for scale (a tool, not a test; it
needs a GPU and fails without one).

    timeout -k 10 900 python tools/bicgstab_bench.py [--grids 2048,250] [--iters 50] [--window 0.5]

Matrices: 5-point diffusion plus first-order upwind convection on a g x g grid
(diagonal 4 + px + py, west -1 - px, south -1 - py, east and north -1;
px, py = 1.5, 0.5), ~5 entries per row.  g = 2048 (4.2 M rows) is
bandwidth-bound, g = 250 (62,500 rows, the size of the cant-like matrix) is
launch-bound.

For k in {1, 2, 4, 8} right-hand sides it times, with tol = 0 and
maxit = --iters so that every side runs exactly --iters iterations (allocation
of the work vectors, the host's look at rr every --check-every iterations and
the closing residual included, on every side):
    fused     iterate.bicgstab_multi: 10 launches per iteration;
    unfused   the same recurrence in this file from spmv_dot_multi (four per
              iteration, a fifth for rr when the host looks), axpy_ratio_multi
              (five), xpay_ratio_multi (one) and torch arithmetic on the
              k-vectors for beta: the composition available before the fused
              kernels existed;
    cg        iterate.cg_multi on the same grid's symmetric matrix
              (px = py = 0): 8 launches and one product per iteration.
Device events bracket windows of enough solves to last at least --window
seconds, after a warm-up of every shape; the three alternate, five windows
each; the figures are the median and the spread (max - min) of the five, in ms
PER ITERATION (of all k columns).  One JSON line.

--trace N runs nothing but 200 calls each of the three fused kernels on N rows
for k in {1, 2, 4, 8} (the update with Sh == R and apart, dot2 with C == A and
apart): the workload of a kernel-trace run against the byte models per row,
update-dot 64k (56k when Sh == R), dir 32k, dot2 24k (16k when C == A).
Hardware counters, if wanted, go in a run of their own.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "opencl-spmv-algorithms_amd"), str(REPO)]
import iterate as it  # noqa: E402
import spmv_amd as sa  # noqa: E402

KS = (1, 2, 4, 8)
WINDOWS = 5


def upwind(g: int, px: float, py: float) -> sa.Coo:
    n = g * g
    idx = np.arange(n, dtype=np.int64).reshape(g, g)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(n, 4.0 + px + py)]
    for me, nb, v in ((idx[:, 1:], idx[:, :-1], -1.0 - px), (idx[1:, :], idx[:-1, :], -1.0 - py),
                      (idx[:, :-1], idx[:, 1:], -1.0), (idx[:-1, :], idx[1:, :], -1.0)):
        rows.append(me.ravel())
        cols.append(nb.ravel())
        vals.append(np.full(me.size, v))
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    o = np.argsort(r * n + c, kind="stable")
    return sa.Coo(n, n, r[o].astype(np.int32), c[o].astype(np.int32), v[o], False, f"upwind {g}x{g} p=({px},{py})")


def unfused_bicgstab(torch, op, B, maxit, check_every):
    """iterate._bicgstab without a preconditioner on one rank, composed from
    the block kernels that existed before the fused ones; tol = 0."""
    k, rows, nv = op.kernels, op.rows, B.shape[1]

    def zeros(*shape):
        return torch.zeros(shape, dtype=torch.float64, device=B.device)

    p_send, r_send = zeros(op.pad, nv), zeros(op.pad, nv)
    P, R = p_send[:rows], r_send[:rows]
    V, T, X, R0 = zeros(rows, nv), zeros(rows, nv), zeros(rows, nv), B.clone()
    R.copy_(B)
    P.copy_(B)
    ws = k.dot_multi_ws(rows, nv)
    rho, rho_new, rv, ts, tt, rr = (zeros(nv) for _ in range(6))
    k.dot_multi(rows, R0, R0, rho, ws)
    bb = rho.cpu().numpy().copy()
    for i in range(1, maxit + 1):
        k.spmm(p_send, V)
        k.dot_multi(rows, R0, V, rv, ws)
        k.axpy_ratio_multi(rows, rho, rv, -1.0, V, R)  # r -= alpha v
        k.spmm(r_send, T)
        k.dot_multi(rows, T, R, ts, ws)
        k.dot_multi(rows, T, T, tt, ws)
        k.axpy_ratio_multi(rows, rho, rv, 1.0, P, X)  # x += alpha p
        k.axpy_ratio_multi(rows, ts, tt, 1.0, R, X)  # x += omega s
        k.axpy_ratio_multi(rows, ts, tt, -1.0, T, R)  # r -= omega t
        k.dot_multi(rows, R0, R, rho_new, ws)
        k.axpy_ratio_multi(rows, ts, tt, -1.0, V, P)  # p -= omega v
        k.xpay_ratio_multi(rows, rho_new * tt, rv * ts, R, P)  # p = r + beta p
        rho, rho_new = rho_new, rho
        if i % check_every == 0 or i == maxit:
            k.dot_multi(rows, R, R, rr, ws)
            if (rr.cpu().numpy() <= 0.0 * bb).all():
                break
    P.copy_(X)  # the closing residual, as the solver computes it
    k.spmm(p_send, V)
    T.copy_(B)
    one = zeros(nv) + 1.0
    k.axpy_ratio_multi(rows, one, one, -1.0, V, T)
    k.dot_multi(rows, T, T, rv, ws)
    return X, i, np.sqrt(rv.cpu().numpy() / bb)


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


def trace_main(a, torch, dev):
    n = a.trace
    lib = sa.hip_lib()
    rng = np.random.default_rng(7)
    p = sa._ptr
    s = torch.cuda.current_stream(dev).cuda_stream
    for k in KS:
        Ph, Sh, T, R0, X, R, P = (torch.from_numpy(rng.uniform(-1, 1, (n, k))).to(dev) for _ in range(7))
        num = torch.ones(k, dtype=torch.float64, device=dev) * 1e-3  # small ratios: 200 updates stay finite
        den = torch.from_numpy(rng.uniform(1.0, 2.0, k) * 1e3).to(dev)
        out = torch.zeros(2 * k, dtype=torch.float64, device=dev)
        ws = torch.empty(lib.spmv_dot_multi_ws_bytes(n, 2 * k), dtype=torch.uint8, device=dev)
        for sh in (Sh, R):
            for _ in range(200):
                sa._check(lib.spmv_bicgstab_update_dot_multi(n, k, p(num), p(den), p(num), p(den), p(Ph), k, p(sh), k,
                                                             p(T), k, p(R0), k, p(X), k, p(R), k, p(out), p(ws),
                                                             ws.numel(), 0, s), "update_dot")
        for _ in range(200):
            sa._check(lib.spmv_bicgstab_dir_multi(n, k, p(num), p(den), p(num), p(den), p(T), k, p(R), k, p(P), k, 0, s),
                      "dir")
        for c in (X, T):
            for _ in range(200):
                sa._check(lib.spmv_dot2_multi(n, k, p(T), k, p(R), k, p(c), k, p(out), p(ws), ws.numel(), 0, s), "dot2")
    torch.cuda.synchronize()
    print(json.dumps({"tool": "bicgstab_bench", "trace_rows": n, "calls": 200, "ks": KS}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="2048,250", help="grid sides (rows = side^2)")
    ap.add_argument("--iters", type=int, default=50, help="iterations per solve (tol = 0)")
    ap.add_argument("--check-every", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of solves per timing window")
    ap.add_argument("--trace", type=int, default=0, help="rows of the kernel-trace workload (nothing else runs)")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bicgstab_bench: no GPU")
    dev = torch.device("cuda:0")
    if a.trace:
        return trace_main(a, torch, dev)
    out = {"tool": "bicgstab_bench", "device": sa.device_name(0), "window_s": a.window, "windows": WINDOWS,
           "iters": a.iters, "check_every": a.check_every, "unit": "ms per iteration, all k columns", "results": {}}
    rng = np.random.default_rng(7)
    kw = dict(tol=0.0, maxit=a.iters, check_every=a.check_every)
    for g in (int(s) for s in a.grids.split(",")):
        m = upwind(g, 1.5, 0.5)
        op = it.build_operator(m, 0, 1, "csr", dev)
        sym = it.build_operator(upwind(g, 0.0, 0.0), 0, 1, "csr", dev)
        n = m.n_rows
        res = out["results"].setdefault(str(g), {"rows": n, "stored_entries": m.nnz})
        for k in KS:
            B = torch.from_numpy(rng.uniform(-1, 1, (n, k))).to(dev)
            fns = {"fused": lambda: it.bicgstab_multi(op, B, **kw),
                   "unfused": lambda: unfused_bicgstab(torch, op, B, a.iters, a.check_every),
                   "cg": lambda: it.cg_multi(sym, B, **kw)}
            got = {name: fn() for name, fn in fns.items()}  # warm-up; every side runs all the iterations
            assert all(r[1] == a.iters for r in got.values())
            torch.cuda.synchronize()
            xf, xu = got["fused"][0], got["unfused"][0]
            diff = float((xf - xu).abs().max() / xf.abs().max())  # the same recurrence: rounding apart
            calls = {name: calls_for(torch, fn, a.window) for name, fn in fns.items()}
            w = {name: [] for name in fns}
            for _ in range(WINDOWS):  # the three alternate
                for name, fn in fns.items():
                    w[name].append(window_ms(torch, fn, calls[name]) / (calls[name] * a.iters))
            med = {name: statistics.median(v) for name, v in w.items()}
            res[str(k)] = {**{f"{name}_ms": round(med[name], 5) for name in fns},
                           **{f"{name}_spread_ms": round(max(v) - min(v), 5) for name, v in w.items()},
                           "solves": calls, "unfused_over_fused": round(med["unfused"] / med["fused"], 3),
                           "fused_faster": max(w["fused"]) < min(w["unfused"]),
                           "fused_over_cg": round(med["fused"] / med["cg"], 3), "x_rel_diff_fused_unfused": diff,
                           "rel_fused_max": float(got["fused"][2].max())}
        del op, sym
    print(json.dumps(out))


if __name__ == "__main__":
    main()
