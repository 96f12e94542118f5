#!/usr/bin/env python3
"""The transposed product y = A^T x against the same plan's forward run (a
tool, not a test; it needs a GPU and fails without one).

    timeout -k 10 600 python tools/spmvt_bench.py [--matrices cantlike,cantlike_x32,rmat] [--steps 20] [--reps 5]

On one cant-like matrix, the block-diagonal batch of 32 copies and the
100k-row / 1M-entry R-MAT of the tests, one CSR plan (library defaults) runs
    forward   run                      (the yardstick, same plan, same process)
    scatter   run_t after prepare_transpose("scatter")
    copy      run_t after prepare_transpose("copy")
each COLD: a step is a 512 MiB flush by reading (spmv_flush_cache_read, the
caches then hold clean lines) followed by one launch.  A region is `--steps`
such steps between two events; regions of flushes alone are timed the same way
before and after it (F B F B ... F) and one launch costs
(span B - mean of its two F spans) / steps.  The figure is the median of
`--reps` regions, with their spread (max - min).  spmv_cpu_csr_t is timed once
by the wall clock.

One JSON line: per matrix the three cold times, each mode's ratio to forward,
each mode's owned_bytes, scatter's blocks / lds_blocks / flush_entries and
`flush_gbs` = flush_entries x 8 bytes / scatter time (the atomic bytes per
second of the window flushes, a lower bound of their rate: the time also holds
the matrix stream and the memset of y), and a markdown table on stderr.

    timeout -k 10 900 python tools/spmvt_bench.py --vectors 2,4,8

is the multi-vector leg instead: on the same matrices and in both modes, one
run_t_multi of k vectors against k run_t calls on the same plan, measured by
the same cold estimator.  A step of the yardstick is one flush followed by
the k calls back to back, as a caller would issue them (on a matrix that
fits the Infinity Cache the second to k-th call find it there).  One JSON
line (per matrix, mode and k: both times with their spreads, `speedup` =
k calls / one call, the byte-model GB/s of the one call) and a table on stderr.
With --balanced the copy mode is also timed after prepare_multi("balanced",
--long-len, --seg-len), which extends to the inner plan over A^T:
`balanced_ms`, `balanced_vs_multi` = unprepared / balanced and
`balanced_vs_k_calls` = k calls / balanced, in one more table.
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
import spmv_amd as sa  # noqa: E402


def matrix(name):
    if name == "cantlike":
        return sa.gen_cantlike(0)
    if name.startswith("cantlike_x"):
        return sa.gen_cantlike(0, int(name[len("cantlike_x"):]))
    if name == "rmat":
        return sa.gen_rmat(100_000, 1_000_000, scale=17, seed=1)
    sys.exit(f"spmvt_bench: unknown matrix {name}")


def span_ms(torch, fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def cold_ms(torch, flush, run, steps, reps):
    """Median and spread of `reps` cold figures (ms per launch)."""
    def both():
        flush()
        run()

    for _ in range(3):
        both()
    f = [span_ms(torch, flush, steps)]
    diffs = []
    for _ in range(reps):
        b = span_ms(torch, both, steps)
        f.append(span_ms(torch, flush, steps))
        diffs.append((b - (f[-2] + f[-1]) / 2) / steps)
    return statistics.median(diffs), max(diffs) - min(diffs)


def vectors_leg(torch, dev, flush, a):
    """--vectors: one run_t_multi against k run_t calls, same plan, mode and
    process, both cold (one flush, then the k calls back to back)."""
    ks = [int(k) for k in a.vectors.split(",")]
    out = {"tool": "spmvt_bench --vectors", "device": sa.device_name(0), "steps": a.steps, "reps": a.reps,
           "results": {}}
    rng = np.random.default_rng(7)
    for name in a.matrices.split(","):
        m = matrix(name)
        ptr, col, val = sa.csr_from_coo(m)
        dm = sa.to_device(m, "csr", dev)
        kmax = max(ks)
        Xh = rng.uniform(-1, 1, (m.n_rows, kmax))
        r = {"n_rows": m.n_rows, "n_cols": m.n_cols, "nnz": m.nnz}
        for mode in ("scatter", "copy"):
            dm.prepare_transpose(mode)
            r[mode] = {"info": dm.transpose_multi_info}
            for k in ks:
                X = torch.from_numpy(np.ascontiguousarray(Xh[:, :k])).to(dev)
                Y = torch.empty((m.n_cols, k), dtype=torch.float64, device=dev)
                xs = [X[:, j].contiguous() for j in range(k)]
                ys = [torch.empty(m.n_cols, dtype=torch.float64, device=dev) for _ in range(k)]

                def k_calls():
                    for x, y in zip(xs, ys):
                        dm.run_t(x, y)

                multi, m_spread = cold_ms(torch, flush, lambda: dm.run_t_multi(X, Y), a.steps, a.reps)
                single, s_spread = cold_ms(torch, flush, k_calls, a.steps, a.reps)
                torch.cuda.synchronize()
                Yr = np.empty((m.n_cols, k))
                sa.cpu_csr_t_multi(m.n_rows, m.n_cols, ptr, col, val, np.ascontiguousarray(Xh[:, :k]), Yr)
                err = float(np.max(np.abs(Y.cpu().numpy() - Yr)))  # against spmv_cpu_csr_t_multi
                r[mode][f"k{k}"] = {
                    "multi_ms": round(multi, 5), "multi_spread_ms": round(m_spread, 5), "k_calls_ms": round(single, 5),
                    "k_calls_spread_ms": round(s_spread, 5), "speedup": round(single / multi, 3),
                    "gbs_alg": round(sa.bytes_alg_multi(m.n_cols, m.n_rows, m.nnz, k) / (multi * 1e-3) / 1e9, 1),
                    "max_abs_diff_vs_cpu": err}
                if a.balanced and mode == "copy":
                    dm.prepare_multi("balanced", a.long_len, a.seg_len)
                    r[mode]["balanced_info"] = dm.multi_info
                    bal, b_spread = cold_ms(torch, flush, lambda: dm.run_t_multi(X, Y), a.steps, a.reps)
                    torch.cuda.synchronize()
                    r[mode][f"k{k}"].update({
                        "balanced_ms": round(bal, 5), "balanced_spread_ms": round(b_spread, 5),
                        "balanced_vs_multi": round(multi / bal, 3), "balanced_vs_k_calls": round(single / bal, 3),
                        "balanced_max_abs_diff_vs_cpu": float(np.max(np.abs(Y.cpu().numpy() - Yr)))})
                    dm.prepare_multi(None)
                del X, Y, xs, ys
        dm.prepare_transpose(None)
        out["results"][name] = r
        del dm
    print(json.dumps(out))
    e = sys.stderr
    print("| matrix | mode | k | one run_t_multi ms (spread) | k run_t ms (spread) | k calls / one call | GB/s (byte model) |",
          file=e)
    print("|---|---|---|---|---|---|---|", file=e)
    for name, r in out["results"].items():
        for mode in ("scatter", "copy"):
            for k in ks:
                c = r[mode][f"k{k}"]
                print(f"| {name} | {mode} | {k} | {c['multi_ms']:.4f} ({c['multi_spread_ms']:.4f}) | "
                      f"{c['k_calls_ms']:.4f} ({c['k_calls_spread_ms']:.4f}) | {c['speedup']:.2f} | {c['gbs_alg']:.0f} |",
                      file=e)
    if a.balanced:
        print("\n| matrix | k | balanced run_t_multi ms (spread) | unprepared / balanced | k run_t / balanced |", file=e)
        print("|---|---|---|---|---|", file=e)
        for name, r in out["results"].items():
            for k in ks:
                c = r["copy"][f"k{k}"]
                print(f"| {name} | {k} | {c['balanced_ms']:.4f} ({c['balanced_spread_ms']:.4f}) | "
                      f"{c['balanced_vs_multi']:.2f} | {c['balanced_vs_k_calls']:.2f} |", file=e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="cantlike,cantlike_x32,rmat")
    ap.add_argument("--steps", type=int, default=20, help="launches per timed region")
    ap.add_argument("--reps", type=int, default=5, help="timed regions per figure (their median is reported)")
    ap.add_argument("--vectors", default=None, metavar="K[,K...]",
                    help="the multi-vector leg instead: one run_t_multi against k run_t calls (e.g. 2,4,8)")
    ap.add_argument("--balanced", action="store_true",
                    help="--vectors: also time copy mode after prepare_multi(\"balanced\")")
    ap.add_argument("--long-len", type=int, default=None, help="--balanced: long_len (default: the library's rule)")
    ap.add_argument("--seg-len", type=int, default=None, help="--balanced: seg_len (default: the library's rule)")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("spmvt_bench: no GPU")
    dev = torch.device("cuda:0")
    lib = sa.hip_lib()
    st = torch.cuda.current_stream(dev)

    def flush():
        assert lib.spmv_flush_cache_read(st.cuda_stream, 0) == 0

    flush()  # allocates the scratch
    torch.cuda.synchronize()
    if a.vectors:
        return vectors_leg(torch, dev, flush, a)
    out = {"tool": "spmvt_bench", "device": sa.device_name(0), "steps": a.steps, "reps": a.reps, "results": {}}
    rng = np.random.default_rng(7)
    for name in a.matrices.split(","):
        m = matrix(name)
        ptr, col, val = sa.csr_from_coo(m)
        xh, yh = rng.uniform(-1, 1, m.n_rows), np.empty(m.n_cols)
        t0 = time.perf_counter()
        sa.cpu_csr_t(m.n_rows, m.n_cols, ptr, col, val, xh, yh)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        dm = sa.to_device(m, "csr", dev)
        x_f = torch.from_numpy(rng.uniform(-1, 1, m.n_cols)).to(dev)
        y_f = torch.empty(m.n_rows, dtype=torch.float64, device=dev)
        x_t = torch.from_numpy(xh).to(dev)
        y_t = torch.empty(m.n_cols, dtype=torch.float64, device=dev)
        r = {"n_rows": m.n_rows, "n_cols": m.n_cols, "nnz": m.nnz, "forward_kernel": dm.kernel,
             "cpu_csr_t_ms": round(cpu_ms, 3)}
        fwd, spread = cold_ms(torch, flush, lambda: dm.run(x_f, y_f), a.steps, a.reps)
        r["forward_ms"], r["forward_spread_ms"] = round(fwd, 5), round(spread, 5)
        for mode in ("scatter", "copy"):
            dm.prepare_transpose(mode)
            info = dm.transpose_info
            ms, spread = cold_ms(torch, flush, lambda: dm.run_t(x_t, y_t), a.steps, a.reps)
            torch.cuda.synchronize()
            err = float(np.max(np.abs(y_t.cpu().numpy() - yh)))  # against spmv_cpu_csr_t
            r[mode] = {"ms": round(ms, 5), "spread_ms": round(spread, 5), "ratio_to_forward": round(ms / fwd, 3),
                       "owned_bytes": info["owned_bytes"], "kernel": info["kernel"], "max_abs_diff_vs_cpu": err}
            if mode == "scatter":
                r[mode].update(blocks=info["blocks"], lds_blocks=info["lds_blocks"], cap=info["cap"],
                               flush_entries=info["flush_entries"],
                               flush_gbs=round(info["flush_entries"] * 8 / (ms * 1e-3) / 1e9, 2))
        dm.prepare_transpose(None)
        out["results"][name] = r
        del dm, x_f, y_f, x_t, y_t
    print(json.dumps(out))
    e = sys.stderr
    print("| matrix | forward ms | scatter ms (x fwd) | copy ms (x fwd) | cpu ms | scatter bytes | copy bytes | "
          "lds / blocks | flush MB | flush GB/s |", file=e)
    print("|---|---|---|---|---|---|---|---|---|---|", file=e)
    for name, r in out["results"].items():
        s, c = r["scatter"], r["copy"]
        print(f"| {name} | {r['forward_ms']:.4f} | {s['ms']:.4f} ({s['ratio_to_forward']:.2f}) | {c['ms']:.4f} "
              f"({c['ratio_to_forward']:.2f}) | {r['cpu_csr_t_ms']:.1f} | {s['owned_bytes']:,} | {c['owned_bytes']:,} | "
              f"{s['lds_blocks']:,} / {s['blocks']:,} | {s['flush_entries'] * 8 / 1e6:.2f} | {s['flush_gbs']:.1f} |",
              file=e)


if __name__ == "__main__":
    main()
