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

--bjacobi BS measures block-Jacobi preconditioned CG instead (one JSON line):
on the Laplacian, on cantlike_sym (forward) and on the block-congruence matrix
(--congruence-grid g: the g x g Laplacian with BS unknowns per node under a
random congruence per node, condition 1e4 each; tests/precond_cases.py has the
reasoning) it builds ONE operator with build_operator(bjacobi=BS) and reports
    per iteration: cg_multi(precond=False), which is cg_multi as it was before
        the preconditioner existed (same launches, same bits), against
        cg_multi with the preconditioner, same windows as above, tol = 0;
    to --tol: the iterations both need for 2 right-hand sides (at most
        --maxit), and the wall time of each solve.
--trace N (with --bjacobi) runs nothing but 200 calls each of
dot_multi(R, R) and of the fused apply_dot on N rows for k in {1, 2, 4, 8}: the
workload of a kernel-trace run that compares the two kernels.

--chebyshev DEG (with --bjacobi BS) measures the Chebyshev polynomial
preconditioner of degree DEG over block Jacobi against block-Jacobi PCG (one
JSON line).  On the same three matrices it builds ONE operator with
build_operator(bjacobi=BS, chebyshev=DEG) (bounds: 1.1 x the power method's
estimate and that over 30, reported; --cheb-lmax X: X and X / 30 as given) and, for k in {1, 2, 4, 8} right-hand
sides, compares cg_multi(precond=op.precond.M), which is block-Jacobi PCG,
same launches and bits as an operator built with bjacobi alone, with cg_multi
under the polynomial:
    per outer iteration: tol = 0, the windows as above;
    to --tol: the iterations each needs (at most --maxit) and the wall time
        of the solve, warm, median of three.
--trace N with --chebyshev runs nothing but 200 calls each of the general step
(Zout == Zin) and of its dot form on N rows for k in {1, 2, 4, 8}: the workload
of a kernel-trace run against the byte model of (48 k + 8 BS) bytes per row.
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


def block_congruence(g: int, b: int, seed: int = 0) -> sa.Coo:
    """W (L_g (x) I_b) W^T, symmetrised; W = blockdiag(U_q diag(10^u) V_q^T),
    u uniform in [0, 2], U_q and V_q orthogonal (QR of normal samples)."""
    import scipy.sparse as sp

    lap = laplacian_2d(g)
    n = lap.n_rows
    L = sp.csr_matrix((lap.val, (lap.row, lap.col)), shape=(n, n))
    rng = np.random.default_rng(seed)
    U = np.linalg.qr(rng.standard_normal((n, b, b)))[0]
    V = np.linalg.qr(rng.standard_normal((n, b, b)))[0]
    Wq = np.einsum("qij,qj,qkj->qik", U, 10.0 ** rng.uniform(0.0, 2.0, (n, b)), V)
    W = sp.bsr_matrix((Wq, np.arange(n), np.arange(n + 1)), shape=(n * b, n * b)).tocsr()
    A = W @ sp.kron(L, sp.identity(b), format="csr") @ W.T
    A = ((A + A.T) * 0.5).tocoo()
    o = np.lexsort((A.col, A.row))
    return sa.Coo(n * b, n * b, A.row[o].astype(np.int32), A.col[o].astype(np.int32), A.data[o].astype(np.float64),
                  False, f"block congruence {g}x{g} nodes, {b} unknowns each")


def block_diagonal(n: int, b: int, seed: int = 0) -> sa.Coo:
    """n rows of diagonally dominant b x b blocks (the --trace workload)."""
    i = np.arange(n, dtype=np.int64)
    col = (i // b * b)[:, None] + np.arange(b)[None, :]
    val = np.random.default_rng(seed).uniform(-1, 1, (n, b))
    val[col == i[:, None]] += b + 1.0
    keep = (col < n).ravel()
    return sa.Coo(n, n, np.repeat(i, b)[keep].astype(np.int32), col.ravel()[keep].astype(np.int32), val.ravel()[keep],
                  False, f"block diagonal {n} rows")


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
    ap.add_argument("--bjacobi", type=int, default=0, help="block size: measure preconditioned CG instead")
    ap.add_argument("--congruence-grid", type=int, default=128, help="--bjacobi: nodes per side of the congruence matrix")
    ap.add_argument("--tol", type=float, default=1e-10, help="--bjacobi: tolerance of the solves that count iterations")
    ap.add_argument("--maxit", type=int, default=20000)
    ap.add_argument("--trace", type=int, default=0, help="--bjacobi: rows of the kernel-trace workload (nothing else runs)")
    ap.add_argument("--chebyshev", type=int, default=0,
                    help="--bjacobi: degree of the Chebyshev polynomial measured against block-Jacobi PCG")
    ap.add_argument("--cheb-lmax", type=float, default=0.0,
                    help="--chebyshev: take this upper bound (and it over 30) instead of the power method's estimate")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("cg_multi_bench: no GPU")
    dev = torch.device("cuda:0")
    if a.chebyshev and not a.bjacobi:
        sys.exit("cg_multi_bench: --chebyshev needs --bjacobi BS")
    if a.chebyshev:
        return chebyshev_main(a, torch, dev)
    if a.bjacobi:
        return precond_main(a, torch, dev)
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


def precond_main(a, torch, dev):
    bs = a.bjacobi
    rng = np.random.default_rng(7)
    if a.trace:
        n = a.trace
        M = sa.BlockJacobi.from_coo(block_diagonal(n, bs), bs, dev)
        lib = sa.hip_lib()
        for k in (1, 2, 4, 8):
            R = torch.from_numpy(rng.uniform(-1, 1, (n, k))).to(dev)
            Z = torch.zeros_like(R)
            out = torch.zeros(2 * k, dtype=torch.float64, device=dev)
            ws = M.ws(n, k)
            s = torch.cuda.current_stream(dev).cuda_stream
            for _ in range(200):
                sa._check(lib.spmv_dot_multi(n, k, sa._ptr(R), k, sa._ptr(R), k, sa._ptr(out), sa._ptr(ws), ws.numel(), 0,
                                             s), "spmv_dot_multi")
            for _ in range(200):
                M.apply_dot(R, Z, out, ws)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "cg_multi_bench", "trace_rows": n, "bjacobi": bs, "calls": 200}))
        return
    out = {"tool": "cg_multi_bench", "device": sa.device_name(0), "bjacobi": bs, "window_s": a.window,
           "windows": WINDOWS, "iters": a.iters, "check_every": a.check_every, "tol": a.tol, "maxit": a.maxit,
           "unit": "ms per iteration, all k columns", "results": {}}
    cases = []
    for name in a.matrices.split(",") + ["congruence"]:
        if name == "laplacian":
            cases.append((name, laplacian_2d(a.grid)))
        elif name == "cantlike_sym":
            cases.append((name, cantlike_sym()))
        elif name == "congruence":
            cases.append((name, block_congruence(a.congruence_grid, bs)))
        else:
            sys.exit(f"cg_multi_bench: unknown matrix {name}")
    for name, m in cases:
        op = it.build_operator(m, 0, 1, "csr", dev, bjacobi=bs)
        n = m.n_rows
        res = out["results"].setdefault(name, {"rows": n, "stored_entries": m.nnz,
                                               "singular_blocks": op.precond.info()["singular_blocks"]})
        kw = dict(tol=0.0, maxit=a.iters, check_every=a.check_every)
        for k in KS:
            B = torch.from_numpy(rng.uniform(-1, 1, (n, k))).to(dev)
            fa = lambda: it.cg_multi(op, B, precond=False, **kw)  # noqa: E731  the yardstick
            fb = lambda: it.cg_multi(op, B, **kw)  # noqa: E731
            assert fa()[1] == a.iters and fb()[1] == a.iters
            torch.cuda.synchronize()
            na, nb = calls_for(torch, fa, a.window), calls_for(torch, fb, a.window)
            wa, wb = [], []
            for _ in range(WINDOWS):
                wa.append(window_ms(torch, fa, na) / (na * a.iters))
                wb.append(window_ms(torch, fb, nb) / (nb * a.iters))
            ma, mb = statistics.median(wa), statistics.median(wb)
            res[str(k)] = {"cg_ms": round(ma, 5), "cg_spread_ms": round(max(wa) - min(wa), 5), "pcg_ms": round(mb, 5),
                           "pcg_spread_ms": round(max(wb) - min(wb), 5), "solves": [na, nb],
                           "pcg_over_cg": round(mb / ma, 3)}
        B = torch.from_numpy(rng.uniform(-1, 1, (n, 2))).to(dev)
        to_tol = {}
        for label, pre in (("cg", False), ("pcg", None)):
            it.cg_multi(op, B, tol=0.0, maxit=2, precond=pre)  # warm-up
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            _, its, rel = it.cg_multi(op, B, tol=a.tol, maxit=a.maxit, check_every=a.check_every, precond=pre)
            t1.record()
            t1.synchronize()
            to_tol[label] = {"iterations": its, "reached": bool((rel <= a.tol).all()), "rel_max": float(rel.max()),
                             "solve_ms": round(t0.elapsed_time(t1), 3)}
        res["to_tol"] = to_tol
        del op
    print(json.dumps(out))


def chebyshev_main(a, torch, dev):
    bs, deg = a.bjacobi, a.chebyshev
    rng = np.random.default_rng(7)
    ks = (1,) + KS
    if a.trace:
        n = a.trace
        M = sa.BlockJacobi.from_coo(block_diagonal(n, bs), bs, dev)
        for k in ks:
            R, AZ, D, Z = (torch.from_numpy(rng.uniform(-1, 1, (n, k))).to(dev) for _ in range(4))
            out = torch.zeros(2 * k, dtype=torch.float64, device=dev)
            ws = M.ws(n, k)
            for _ in range(200):
                M.cheb_step(0.25, 1e-3, R, AZ, D, Z, Z)
            for _ in range(200):
                M.cheb_step_dot(0.25, 1e-3, R, AZ, D, Z, Z, out, ws)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "cg_multi_bench", "trace_rows": n, "bjacobi": bs, "chebyshev": deg, "calls": 200}))
        return
    out = {"tool": "cg_multi_bench", "device": sa.device_name(0), "bjacobi": bs, "chebyshev": deg,
           "window_s": a.window, "windows": WINDOWS, "iters": a.iters, "check_every": a.check_every, "tol": a.tol,
           "maxit": a.maxit, "unit": "ms per outer iteration, all k columns", "results": {}}
    cases = []
    for name in a.matrices.split(",") + ["congruence"]:
        if name == "laplacian":
            cases.append((name, laplacian_2d(a.grid)))
        elif name == "cantlike_sym":
            cases.append((name, cantlike_sym()))
        elif name == "congruence":
            cases.append((name, block_congruence(a.congruence_grid, bs)))
        else:
            sys.exit(f"cg_multi_bench: unknown matrix {name}")
    for name, m in cases:
        bounds = (a.cheb_lmax / 30.0, a.cheb_lmax) if a.cheb_lmax > 0.0 else None
        op = it.build_operator(m, 0, 1, "csr", dev, bjacobi=bs, chebyshev=deg, cheb_bounds=bounds)
        cheb = op.precond
        n = m.n_rows
        res = out["results"].setdefault(name, {"rows": n, "stored_entries": m.nnz, "lmin": cheb.lmin,
                                               "lmax": cheb.lmax, "bounds_given": bounds is not None})
        kw = dict(tol=0.0, maxit=a.iters, check_every=a.check_every)
        for k in ks:
            B = torch.from_numpy(rng.uniform(-1, 1, (n, k))).to(dev)
            fa = lambda: it.cg_multi(op, B, precond=cheb.M, **kw)  # noqa: E731  the yardstick: block-Jacobi PCG
            fb = lambda: it.cg_multi(op, B, **kw)  # noqa: E731
            assert fa()[1] == a.iters and fb()[1] == a.iters
            torch.cuda.synchronize()
            na, nb = calls_for(torch, fa, a.window), calls_for(torch, fb, a.window)
            wa, wb = [], []
            for _ in range(WINDOWS):
                wa.append(window_ms(torch, fa, na) / (na * a.iters))
                wb.append(window_ms(torch, fb, nb) / (nb * a.iters))
            ma, mb = statistics.median(wa), statistics.median(wb)
            r = {"bj_ms": round(ma, 5), "bj_spread_ms": round(max(wa) - min(wa), 5), "cheb_ms": round(mb, 5),
                 "cheb_spread_ms": round(max(wb) - min(wb), 5), "solves": [na, nb], "cheb_over_bj": round(mb / ma, 3)}
            for label, pre in (("bj", cheb.M), ("cheb", None)):
                times = []
                for _ in range(3):
                    torch.cuda.synchronize()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    _, its, rel = it.cg_multi(op, B, tol=a.tol, maxit=a.maxit, check_every=a.check_every, precond=pre)
                    t1.record()
                    t1.synchronize()
                    times.append(t0.elapsed_time(t1))
                r[label + "_to_tol"] = {"iterations": its, "reached": bool((rel <= a.tol).all()),
                                        "rel_max": float(rel.max()), "solve_ms": round(statistics.median(times), 3),
                                        "solve_spread_ms": round(max(times) - min(times), 3)}
            r["time_to_tol_cheb_over_bj"] = round(r["cheb_to_tol"]["solve_ms"] / r["bj_to_tol"]["solve_ms"], 3)
            res[str(k)] = r
        del op, cheb
    print(json.dumps(out))


if __name__ == "__main__":
    main()
