#!/usr/bin/env python3
"""Block CSR (BSR, 3x3 blocks) against the default CSR plan and SELL16 (a tool,
not a test; it needs a GPU and fails without one).

    timeout -k 10 900 python tools/bsr_bench.py [--matrices cantlike,cantlike_x32,congruence128] [--block 3]
                                                [--steps 20] [--reps 3] [--rounds 3]

Per matrix, in one process, the three device matrices are built once and then
timed ALTERNATING: every round times bsr, csr, sell16 one after the other,
each COLD by tools/spmvt_bench.py's method (a step is a 512 MiB flush by
reading followed by one launch; a region is `--steps` such steps between two
events, bracketed by regions of flushes alone; `--reps` regions give one
median).  A side's figure is the median of its `--rounds` round medians, its
spread their max - min.

The matrices: one cant-like matrix (fill 1.079 at b = 3), the block-diagonal
batch of 32 copies, and block_congruence(128, 3) of tools/cg_multi_bench.py, a
truly blocked matrix (fill 1.0).

One JSON line: per matrix and side the ms, the spread, the side's stored_bytes
and the GB/s by those bytes; for bsr the time ratio to csr and to sell16 beside
the ratio of the stored bytes.  A markdown table on stderr.  There is no
pass/fail threshold: the byte model says 0.755 (cant-like) and 0.70 (fill 1.0)
of CSR's int32 stream, and the run says what the kernel makes of it.  Every y
is checked against spmv_cpu_csr first.

    timeout -k 10 600 rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bsr_bench.py --trace

The --trace leg, in a run of its own: `--steps` cold launches of each side on
each matrix and nothing else, for the kernel durations of the trace.
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
import spmv_amd as sa  # noqa: E402
from spmvt_bench import cold_ms  # noqa: E402  (the same cold estimator)

SIDES = ("bsr", "csr", "sell16")


def matrix(name):
    if name == "cantlike":
        return sa.gen_cantlike(0)
    if name.startswith("cantlike_x"):
        return sa.gen_cantlike(0, int(name[len("cantlike_x"):]))
    if name.startswith("congruence"):
        from cg_multi_bench import block_congruence

        return block_congruence(int(name[len("congruence"):]), 3)
    sys.exit(f"bsr_bench: unknown matrix {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matrices", default="cantlike,cantlike_x32,congruence128")
    ap.add_argument("--block", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=0, help="BSR lanes per block row (0: the rule)")
    ap.add_argument("--steps", type=int, default=20, help="launches per timed region")
    ap.add_argument("--reps", type=int, default=3, help="timed regions per round median")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds (their median is reported)")
    ap.add_argument("--trace", action="store_true", help="only launch (for rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("bsr_bench: no GPU")
    dev = torch.device("cuda:0")
    lib = sa.hip_lib()
    st = torch.cuda.current_stream(dev)

    def flush():
        assert lib.spmv_flush_cache_read(st.cuda_stream, 0) == 0

    flush()  # allocates the scratch
    torch.cuda.synchronize()
    out = {"tool": "bsr_bench" + (" --trace" if a.trace else ""), "device": sa.device_name(0), "block": a.block,
           "steps": a.steps, "reps": a.reps, "rounds": a.rounds, "results": {}}
    rng = np.random.default_rng(7)
    for name in a.matrices.split(","):
        m = matrix(name)
        ptr, col, val = sa.csr_from_coo(m)
        xh, yh = rng.uniform(-1, 1, m.n_cols), np.empty(max(m.n_rows, 1))
        assert sa.host_lib().spmv_cpu_csr(m.n_rows, sa._ptr(ptr), sa._ptr(col), sa._ptr(val), sa._ptr(xh), sa._ptr(yh),
                                          0) == sa.SUCCESS
        scale = float(np.max(np.abs(yh))) if m.n_rows else 0.0
        x = torch.from_numpy(xh).to(dev)
        y = torch.empty(m.n_rows, dtype=torch.float64, device=dev)
        dms, r = {}, {"n_rows": m.n_rows, "nnz": m.nnz}
        for side in SIDES:
            try:
                dms[side] = (sa.to_device(m, "bsr", dev, block=a.block, lanes=a.lanes, bsr_max_fill=float("inf"))
                             if side == "bsr" else sa.to_device(m, side, dev))
            except sa.SpmvError as e:
                r[side] = {"refused": str(e)}
                continue
            dm = dms[side]
            y.fill_(float("nan"))
            dm.run(x, y)
            torch.cuda.synchronize()
            err = float(np.max(np.abs(y.cpu().numpy() - yh[: m.n_rows]))) if m.n_rows else 0.0
            if not err <= 1e-9 * scale:
                sys.exit(f"bsr_bench: {name} {side}: y differs from spmv_cpu_csr by {err:g}")
            r[side] = {"kernel": dm.kernel, "plan": dm.params.get("plan", ""), "stored_bytes": dm.stored_bytes,
                       "max_abs_diff_vs_cpu": err, "round_ms": []}
        r["bsr"].update(fill=round(dms["bsr"].params["fill"], 4), n_blocks=dms["bsr"].params["n_blocks"],
                        lanes=dms["bsr"].params["lanes"])
        if a.trace:
            for side, dm in dms.items():
                for _ in range(a.steps):
                    flush()
                    dm.run(x, y)
            torch.cuda.synchronize()
            out["results"][name] = r
            continue
        for _ in range(a.rounds):
            for side, dm in dms.items():
                r[side]["round_ms"].append(cold_ms(torch, flush, lambda: dm.run(x, y), a.steps, a.reps)[0])
        torch.cuda.synchronize()
        for side in dms:
            c = r[side]
            ms = statistics.median(c["round_ms"])
            c.update(ms=round(ms, 5), spread_ms=round(max(c["round_ms"]) - min(c["round_ms"]), 5),
                     gbs_stored=round(c["stored_bytes"] / (ms * 1e-3) / 1e9, 1),
                     round_ms=[round(v, 5) for v in c["round_ms"]])
        for other in ("csr", "sell16"):
            if other in dms:
                r["bsr"][f"time_ratio_to_{other}"] = round(r["bsr"]["ms"] / r[other]["ms"], 3)
                r["bsr"][f"byte_ratio_to_{other}"] = round(r["bsr"]["stored_bytes"] / r[other]["stored_bytes"], 3)
        out["results"][name] = r
        del dms, x, y
    print(json.dumps(out))
    if a.trace:
        return
    e = sys.stderr
    print("| matrix | fill | bsr ms (spread, GB/s) | csr ms (spread, GB/s) | sell16 ms (spread, GB/s) | bsr / csr time "
          "(bytes) | bsr / sell16 time (bytes) |", file=e)
    print("|---|---|---|---|---|---|---|", file=e)
    for name, r in out["results"].items():
        def cell(side):
            c = r[side]
            return "refused" if "refused" in c else f"{c['ms']:.4f} ({c['spread_ms']:.4f}, {c['gbs_stored']:.0f})"

        def ratio(other):
            b = r["bsr"]
            k = f"time_ratio_to_{other}"
            return f"{b[k]:.3f} ({b[f'byte_ratio_to_{other}']:.3f})" if k in b else "-"

        print(f"| {name} | {r['bsr']['fill']:.3f} | {cell('bsr')} | {cell('csr')} | {cell('sell16')} | {ratio('csr')} | "
              f"{ratio('sell16')} |", file=e)


if __name__ == "__main__":
    main()
