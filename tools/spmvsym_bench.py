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
    sys.exit(f"spmvsym_bench: unknown matrix {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="cantlike2,cantlike2_x32")
    ap.add_argument("--steps", type=int, default=20, help="launches per timed region")
    ap.add_argument("--reps", type=int, default=5, help="timed regions per figure (their median is reported)")
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
