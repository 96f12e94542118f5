#!/usr/bin/env python3
"""Multi-right-hand-side CG against a loop of single-vector CG solves (a
tool, not a test; it needs a GPU and fails without one).

    timeout -k 10 900 python tools/cg_multi_bench.py [--grid 2048] [--iters 50] [--window 0.5]

For k in {2, 4, 8} it times
    (a) one iterate.cg_multi solve of k right-hand sides;
    (b) k back-to-back iterate.cg solves, one per column, on the same operator;
both with tol = 0 and maxit = --iters, so both run exactly --iters iterations
per column (allocation of the work vectors and the host's look at rr every
--check-every iterations included, on both sides).  Device events bracket
windows of enough solves to last at least --window seconds, after a warm-up of
every shape; (a) and (b) alternate, five windows each; the figures are the
median and the spread (max - min) of the five, in ms PER ITERATION (of all k
columns).

Matrices:
    laplacian      the 5-point Laplacian on a --grid x --grid grid (~5 entries
                   per row): vector traffic dominates;
    cantlike_sym   the cant-like pattern made symmetric (pattern + its
                   transpose, off-diagonal entries -1) and strictly diagonally
                   dominant (diagonal = row count + 1), ~64 entries per row, as
                   a forward operator on the full matrix ("forward") and as
                   symmetric="expand" / "fused" operators on its lower triangle.

One JSON line: per matrix, mode and k the ms per iteration of (a) and (b) with
their spreads, the ratio (b)/(a), and `faster`: every window of (a) beat every
window of (b), i.e. the margin exceeds the spread.
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

KS = (2, 4, 8)
WINDOWS = 5


def laplacian_2d(g: int) -> sa.Coo:
    n = g * g
    idx = np.arange(n, dtype=np.int64).reshape(g, g)
    rows, cols, vals = [idx.ravel()], [idx.ravel()], [np.full(n, 4.0)]
    for a, b in ((idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])):
        rows += [a.ravel(), b.ravel()]
        cols += [b.ravel(), a.ravel()]
        vals += [np.full(a.size, -1.0), np.full(a.size, -1.0)]
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    o = np.argsort(r * n + c, kind="stable")
    return sa.Coo(n, n, r[o].astype(np.int32), c[o].astype(np.int32), v[o], False, f"2-D Laplacian {g}x{g}")


def cantlike_sym() -> sa.Coo:
    """Pattern of gen_cantlike(0) united with its transpose; off-diagonal
    entries -1, diagonal = off-diagonal count of the row + 1 (strictly
    diagonally dominant, so SPD); sorted by row, then column."""
    m = sa.gen_cantlike(0, 1)
    n = m.n_rows
    r = np.concatenate([m.row, m.col]).astype(np.int64)
    c = np.concatenate([m.col, m.row]).astype(np.int64)
    key = np.unique((r * n + c)[r != c])
    r, c = key // n, key % n
    d = np.arange(n, dtype=np.int64)
    diag = np.bincount(r, minlength=n) + 1.0
    key = np.concatenate([key, d * n + d])
    val = np.concatenate([np.full(r.size, -1.0), diag])
    o = np.argsort(key, kind="stable")
    key, val = key[o], val[o]
    return sa.Coo(n, n, (key // n).astype(np.int32), (key % n).astype(np.int32), val, False, "cant-like, symmetric SPD")


def lower(m: sa.Coo) -> sa.Coo:
    keep = m.row >= m.col
    return sa.Coo(m.n_rows, m.n_cols, m.row[keep], m.col[keep], m.val[keep], True, m.label + " (lower)")


def window_ms(torch, fn, n):
    """n calls of fn between two events on the current stream -> ms in all."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def calls_for(torch, fn, seconds):
    """Solves per window: at least `seconds` of device time."""
    n = 1
    while True:
        ms = window_ms(torch, fn, n)
        if ms >= seconds * 1e3:
            return n
        n = max(n + 1, int(n * seconds * 1e3 / max(ms, 1e-3) * 1.1) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=2048, help="Laplacian grid side (rows = grid^2)")
    ap.add_argument("--iters", type=int, default=50, help="CG iterations per solve (tol = 0)")
    ap.add_argument("--check-every", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of solves per timing window")
    ap.add_argument("--matrices", default="laplacian,cantlike_sym")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("cg_multi_bench: no GPU")
    dev = torch.device("cuda:0")
    out = {"tool": "cg_multi_bench", "device": sa.device_name(0), "window_s": a.window, "windows": WINDOWS,
           "iters": a.iters, "check_every": a.check_every, "unit": "ms per iteration, all k columns", "results": {}}
    rng = np.random.default_rng(7)
    cases = []
    for name in a.matrices.split(","):
        if name == "laplacian":
            cases.append((name, "forward", laplacian_2d(a.grid), None))
        elif name == "cantlike_sym":
            m = cantlike_sym()
            cases.append((name, "forward", m, None))
            cases += [(name, mode, lower(m), mode) for mode in ("expand", "fused")]
        else:
            sys.exit(f"cg_multi_bench: unknown matrix {name}")
    for name, mode, m, sym in cases:
        op = it.build_operator(m, 0, 1, "csr", dev, symmetric=sym)
        n = m.n_rows
        Bs = {k: torch.from_numpy(rng.uniform(-1, 1, (n, k))).to(dev) for k in KS}
        bs = torch.from_numpy(rng.uniform(-1, 1, (max(KS), n))).to(dev)  # k contiguous right-hand sides
        kw = dict(tol=0.0, maxit=a.iters, check_every=a.check_every)
        fns = {k: ((lambda k=k: it.cg_multi(op, Bs[k], **kw)),
                   (lambda k=k: [it.cg(op, bs[j], **kw) for j in range(k)])) for k in KS}
        for k in KS:  # warm-up of every shape; both sides must run all the iterations
            assert fns[k][0]()[1] == a.iters and all(r[1] == a.iters for r in fns[k][1]())
        torch.cuda.synchronize()
        res = out["results"].setdefault(name, {}).setdefault(mode, {"rows": n, "stored_entries": m.nnz})
        for k in KS:
            fa, fb = fns[k]
            na, nb = calls_for(torch, fa, a.window), calls_for(torch, fb, a.window)
            wa, wb = [], []
            for _ in range(WINDOWS):  # (a) and (b) alternate
                wa.append(window_ms(torch, fa, na) / (na * a.iters))
                wb.append(window_ms(torch, fb, nb) / (nb * a.iters))
            ma, mb = statistics.median(wa), statistics.median(wb)
            res[str(k)] = {"multi_ms": round(ma, 5), "multi_spread_ms": round(max(wa) - min(wa), 5),
                           "loop_ms": round(mb, 5), "loop_spread_ms": round(max(wb) - min(wb), 5),
                           "solves": [na, nb], "ratio": round(mb / ma, 3), "faster": max(wa) < min(wb)}
        del op, Bs, bs, fns
    print(json.dumps(out))


if __name__ == "__main__":
    main()
