#!/usr/bin/env python3
"""The timed paths of profiles/csr_mode4/README.md (a tool, not a test; it
needs a GPU and fails without one).

    SPMV_HIP_LIB=<parent's libspmv_hip.so> timeout -k 10 300 python tools/ab_csr_mode4.py > p1.json
    timeout -k 10 300 python tools/ab_csr_mode4.py > t1.json       (alternating, parent first, 3+ runs each)
    python tools/ab_csr_mode4.py --table p1.json p2.json p3.json --tree t1.json t2.json t3.json

One process times every path with the library it loaded, COLD by the estimator
of tools/spmvt_bench.py (512 MiB read before every launch, --steps launches
per region between flush-only regions, median of --reps regions) and prints
one JSON line {path: ms}.  The paths: one cant-like matrix and the 32-copy
batch as a CSR plan (default: ColWin16; csr_col16 = 0: Col32), csr16 and
csrf32 on the one matrix, rows [0, 12,500,000) of the 10^8-row banded matrix
as a CSR plan (default windows: MODE 3; xwin_rows = 128, one chunk per
window: MODE 0, a control) and SELL on the one matrix (a control).
--table prints the markdown table: per path the median and spread (max - min)
of each side's runs and the verdict by the rule of
profiles/round7/ab_csr_col16.md (level when the medians differ by at most
three times the larger spread).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO / "opencl-spmv-algorithms_amd"), str(REPO / "tools")]

BANDED_N, SHARD_ROWS = 100_000_000, 12_500_000


def table(parent, tree):
    sides = [[json.loads(Path(f).read_text()) for f in fs] for fs in (parent, tree)]
    print("| path | parent median ms | parent spread | tree median ms | tree spread | tree - parent | "
          "3 x larger spread | verdict |")
    print("|---|---|---|---|---|---|---|---|")
    for path in sides[0][0]:
        (pm, ps), (tm, ts) = [(statistics.median(v), max(v) - min(v)) for v in ([r[path] for r in s] for s in sides)]
        lim = 3 * max(ps, ts)
        print(f"| {path} | {pm:.5f} | {ps:.5f} | {tm:.5f} | {ts:.5f} | {tm - pm:+.5f} | {lim:.5f} | "
              f"{'level' if abs(tm - pm) <= lim else 'NOT level'} |")
    for side, runs in zip(("parent", "tree"), sides):
        for path in runs[0]:
            print(f"{side} | {path} | " + " ".join(f"{r[path]:.5f}" for r in runs), file=sys.stderr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="launches per timed region")
    ap.add_argument("--reps", type=int, default=5, help="timed regions per figure (their median is reported)")
    ap.add_argument("--table", nargs="+", metavar="JSON", help="the parent's runs: print the table instead")
    ap.add_argument("--tree", nargs="+", metavar="JSON", help="--table: the tree's runs")
    a = ap.parse_args()
    if a.table:
        return table(a.table, a.tree)
    import torch

    import spmv_amd as sa
    from spmvt_bench import cold_ms

    if not torch.cuda.is_available():
        sys.exit("ab_csr_mode4: no GPU")
    dev = torch.device("cuda:0")
    lib = sa.hip_lib()
    st = torch.cuda.current_stream(dev)

    def flush():
        assert lib.spmv_flush_cache_read(st.cuda_stream, 0) == 0

    flush()  # allocates the scratch
    torch.cuda.synchronize()
    out = {}

    def timed(path, dm):
        x = torch.rand(dm.n_cols, dtype=torch.float64, device=dev)
        y = torch.empty(dm.n_rows, dtype=torch.float64, device=dev)
        out[path] = round(cold_ms(torch, flush, lambda: dm.run(x, y), a.steps, a.reps)[0], 5)
        torch.cuda.synchronize()

    for name, m in (("cant", sa.gen_cantlike(0)), ("batch32", sa.gen_cantlike(0, 32))):
        timed(f"{name}, CSR plan default", sa.to_device(m, "csr", dev))
        sa.set_option("csr_col16", 0)
        timed(f"{name}, CSR plan, csr_col16 = 0", sa.to_device(m, "csr", dev))
        sa.set_option("csr_col16", None)
        if name == "cant":
            timed("cant, csr16", sa.to_device(m, "csr16", dev))
            timed("cant, csrf32", sa.to_device(m, "csrf32", dev))
            timed("cant, SELL (control)", sa.to_device(m, "sell", dev))
    timed("banded shard, CSR plan default", sa.banded_to_device(BANDED_N, "csr", dev, 0, SHARD_ROWS))
    timed("banded shard, CSR plan, xwin_rows = 128 (control)",
          sa.banded_to_device(BANDED_N, "csr", dev, 0, SHARD_ROWS, xwin_rows=128))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
