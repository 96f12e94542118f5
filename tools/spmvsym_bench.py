#!/usr/bin/env python3
"""The symmetric product y = (S + S^T - diag S) x from the stored half against
a forward run over the expanded matrix (a tool, not a test; it needs a GPU and
fails without one).

    timeout -k 10 600 python tools/spmvsym_bench.py [--matrices cantlike2,cantlike2_x32] [--steps 20] [--reps 5]

On the cant-like lower triangle (gen_cantlike(2): 2,034,917 stored entries of a
4,007,383-entry matrix) and the block-diagonal batch of 32 copies, in one
process:
    forward   run of a default CSR plan over the HOST-expanded matrix (the
              yardstick: what a caller without this feature has to run)
    fused     run_sym after prepare_symmetric("fused") on the half storage
    expand    run_sym after prepare_symmetric("expand") on the half storage
each COLD, by tools/spmvt_bench.py's method: a step is a 512 MiB flush by
reading (spmv_flush_cache_read) followed by one launch; a region is `--steps`
such steps between two events; regions of flushes alone are timed the same way
before and after it (F B F B ... F) and one launch costs
(span B - mean of its two F spans) / steps.  The figure is the median of
`--reps` regions, with their spread (max - min).  spmv_cpu_csr_sym is timed
once by the wall clock.

One JSON line: per matrix the three cold times, each mode's ratio to forward,
the bytes each run has to move by sa.bytes_alg (12 per streamed entry + 4 per
row offset + 8 per x and y entry: the stored entries for fused, the expanded
ones for forward and expand) with the GB/s they imply, each mode's
owned_bytes, fused's blocks / window_blocks / flush_entries, and a markdown
table on stderr.

    timeout -k 10 900 python tools/spmvsym_bench.py --vectors 2,4,8

The multi-vector leg instead: for every k, ONE run_sym_multi against k run_sym
calls on the same plan (the yardstick: run_sym is what a caller without
run_sym_multi has to call k times), both cold (one flush, then the k calls
back to back), in both modes, on the same two matrices; then the lower triangle
of the 100,000-row R-MAT (`rmat_tril`) in expand mode, unprepared and after
prepare_multi("balanced").  Every Y is checked against spmv_cpu_csr_sym_multi.
GB/s by sa.bytes_alg_multi over the entries the mode streams (stored for
fused, expanded for expand).  One JSON line and a markdown table on stderr.
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "opencl-spmv-algorithms_amd"), str(REPO), str(REPO / "tools")]
import spmv_amd as sa  # noqa: E402
from spmvt_bench import cold_ms  # noqa: E402  (the same cold estimator)


def matrix(name):
    if name == "cantlike2":
        return sa.gen_cantlike(2)
    if name.startswith("cantlike2_x"):
        return sa.gen_cantlike(2, int(name[len("cantlike2_x"):]))
    if name == "rmat_tril":
        m = sa.gen_rmat(100_000, 1_000_000, scale=17, seed=1)
        keep = m.row >= m.col
        return sa.Coo(100_000, 100_000, m.row[keep], m.col[keep], m.val[keep], True, name)
    sys.exit(f"spmvsym_bench: unknown matrix {name}")


def vectors_leg(torch, dev, flush, a):
    """--vectors: one run_sym_multi against k run_sym calls, same plan, mode
    and process."""
    ks = [int(k) for k in a.vectors.split(",")]
    kmax = max(ks)
    out = {"tool": "spmvsym_bench --vectors", "device": sa.device_name(0), "steps": a.steps, "reps": a.reps,
           "results": {}}
    rng = np.random.default_rng(7)
    rows = []  # (matrix, leg, k, cell) for the table
    for name in a.matrices.split(",") + ["rmat_tril"]:
        m = matrix(name)
        n = m.n_rows
        ptr, col, val = sa.csr_from_coo(m)
        nnz_a = sa.expand_symmetric(m).nnz
        dm = sa.to_device(m, "csr", dev)
        Xh = rng.uniform(-1, 1, (n, kmax))
        Yr = np.empty((n, kmax))
        sa.cpu_csr_sym_multi(n, ptr, col, val, Xh, Yr)
        r = {"n": n, "nnz_stored": m.nnz, "nnz_expanded": nnz_a}
        legs = [("expand", None), ("expand", "balanced")] if name == "rmat_tril" else [("fused", None), ("expand", None)]
        for mode, multi_mode in legs:
            dm.prepare_symmetric(mode)
            dm.prepare_multi(multi_mode)
            leg = mode + (" balanced" if multi_mode else "")
            r[leg] = {"info": dm.symmetric_multi_info}
            streamed = m.nnz if mode == "fused" else nnz_a
            for k in ks:
                X = torch.from_numpy(np.ascontiguousarray(Xh[:, :k])).to(dev)
                Y = torch.empty((n, k), dtype=torch.float64, device=dev)
                xs = [X[:, j].contiguous() for j in range(k)]
                ys = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(k)]

                def k_calls():
                    for x, y in zip(xs, ys):
                        dm.run_sym(x, y)

                multi, m_spread = cold_ms(torch, flush, lambda: dm.run_sym_multi(X, Y), a.steps, a.reps)
                single, s_spread = cold_ms(torch, flush, k_calls, a.steps, a.reps)
                torch.cuda.synchronize()
                err = float(np.max(np.abs(Y.cpu().numpy() - Yr[:, :k])))  # against spmv_cpu_csr_sym_multi
                scale = float(np.max(np.abs(Yr[:, :k])))
                if not err <= 1e-9 * scale:
                    sys.exit(f"spmvsym_bench: {name} {leg} k={k}: Y differs from cpu_csr_sym_multi by {err:g}")
                r[leg][f"k{k}"] = {
                    "multi_ms": round(multi, 5), "multi_spread_ms": round(m_spread, 5), "k_calls_ms": round(single, 5),
                    "k_calls_spread_ms": round(s_spread, 5), "speedup": round(single / multi, 3),
                    "gbs_alg": round(sa.bytes_alg_multi(n, n, streamed, k) / (multi * 1e-3) / 1e9, 1),
                    "max_abs_diff_vs_cpu": err}
                rows.append((name, leg, k, r[leg][f"k{k}"]))
                del X, Y, xs, ys
        dm.prepare_multi(None)
        dm.prepare_symmetric(None)
        out["results"][name] = r
        del dm
    print(json.dumps(out))
    e = sys.stderr
    print("| matrix | mode | k | one run_sym_multi ms (spread) | k run_sym ms (spread) | k calls / one call | "
          "GB/s (byte model) |", file=e)
    print("|---|---|---|---|---|---|---|", file=e)
    for name, leg, k, c in rows:
        print(f"| {name} | {leg} | {k} | {c['multi_ms']:.4f} ({c['multi_spread_ms']:.4f}) | {c['k_calls_ms']:.4f} "
              f"({c['k_calls_spread_ms']:.4f}) | {c['speedup']:.2f} | {c['gbs_alg']:.0f} |", file=e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="cantlike2,cantlike2_x32")
    ap.add_argument("--steps", type=int, default=20, help="launches per timed region")
    ap.add_argument("--reps", type=int, default=5, help="timed regions per figure (their median is reported)")
    ap.add_argument("--vectors", default=None, metavar="K[,K...]",
                    help="the multi-vector leg instead: one run_sym_multi against k run_sym calls (e.g. 2,4,8)")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("spmvsym_bench: no GPU")
    dev = torch.device("cuda:0")
    lib = sa.hip_lib()
    st = torch.cuda.current_stream(dev)

    def flush():
        assert lib.spmv_flush_cache_read(st.cuda_stream, 0) == 0

    flush()  # allocates the scratch
    torch.cuda.synchronize()
    if a.vectors:
        return vectors_leg(torch, dev, flush, a)
    out = {"tool": "spmvsym_bench", "device": sa.device_name(0), "steps": a.steps, "reps": a.reps, "results": {}}
    rng = np.random.default_rng(7)
    for name in a.matrices.split(","):
        m = matrix(name)
        n = m.n_rows
        e = sa.expand_symmetric(m)
        ptr, col, val = sa.csr_from_coo(m)
        xh, yh = rng.uniform(-1, 1, n), np.empty(n)
        t0 = time.perf_counter()
        sa.cpu_csr_sym(n, ptr, col, val, xh, yh)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        x = torch.from_numpy(xh).to(dev)
        y = torch.empty(n, dtype=torch.float64, device=dev)
        bytes_half, bytes_full = sa.bytes_alg(n, n, m.nnz), sa.bytes_alg(n, n, e.nnz)
        r = {"n": n, "nnz_stored": m.nnz, "nnz_expanded": e.nnz, "bytes_alg_stored": bytes_half,
             "bytes_alg_expanded": bytes_full, "cpu_csr_sym_ms": round(cpu_ms, 3)}
        fwd_dm = sa.to_device(e, "csr", dev)
        fwd, spread = cold_ms(torch, flush, lambda: fwd_dm.run(x, y), a.steps, a.reps)
        torch.cuda.synchronize()
        r["forward"] = {"ms": round(fwd, 5), "spread_ms": round(spread, 5), "kernel": fwd_dm.kernel,
                        "stored_bytes": fwd_dm.stored_bytes, "gbs_alg": round(bytes_full / (fwd * 1e-3) / 1e9, 1),
                        "max_abs_diff_vs_cpu": float(np.max(np.abs(y.cpu().numpy() - yh)))}
        del fwd_dm
        dm = sa.to_device(m, "csr", dev)
        r["stored_bytes"] = dm.stored_bytes
        for mode in ("fused", "expand"):
            dm.prepare_symmetric(mode)
            info = dm.symmetric_info
            ms, spread = cold_ms(torch, flush, lambda: dm.run_sym(x, y), a.steps, a.reps)
            torch.cuda.synchronize()
            moved = bytes_half if mode == "fused" else bytes_full
            r[mode] = {"ms": round(ms, 5), "spread_ms": round(spread, 5), "ratio_to_forward": round(ms / fwd, 3),
                       "owned_bytes": info["owned_bytes"], "kernel": info["kernel"],
                       "gbs_alg": round(moved / (ms * 1e-3) / 1e9, 1),
                       "max_abs_diff_vs_cpu": float(np.max(np.abs(y.cpu().numpy() - yh)))}
            if mode == "fused":
                r[mode].update(blocks=info["blocks"], window_blocks=info["window_blocks"], cap=info["cap"],
                               flush_entries=info["flush_entries"])
        dm.prepare_symmetric(None)
        out["results"][name] = r
        del dm, x, y
    print(json.dumps(out))
    err = sys.stderr
    print("| matrix | stored / expanded entries | forward ms (GB/s) | fused ms (x fwd, GB/s) | expand ms (x fwd) | "
          "cpu ms | bytes_alg stored / expanded MB | fused bytes | expand bytes | window / blocks |", file=err)
    print("|---|---|---|---|---|---|---|---|---|---|", file=err)
    for name, r in out["results"].items():
        f, s, x = r["forward"], r["fused"], r["expand"]
        print(f"| {name} | {r['nnz_stored']:,} / {r['nnz_expanded']:,} | {f['ms']:.4f} ({f['gbs_alg']:.0f}) | "
              f"{s['ms']:.4f} ({s['ratio_to_forward']:.2f}, {s['gbs_alg']:.0f}) | {x['ms']:.4f} "
              f"({x['ratio_to_forward']:.2f}) | {r['cpu_csr_sym_ms']:.1f} | {r['bytes_alg_stored'] / 1e6:.1f} / "
              f"{r['bytes_alg_expanded'] / 1e6:.1f} | {s['owned_bytes']:,} | {x['owned_bytes']:,} | "
              f"{s['window_blocks']:,} / {s['blocks']:,} |", file=err)


if __name__ == "__main__":
    main()
