#!/usr/bin/env python3
"""Multi-vector SpMV against a loop of single-vector runs (a tool, not a
test; it needs a GPU and fails without one).

    timeout -k 10 600 python tools/spmm_bench.py [--formats csr,sell] [--copies 1,32] [--window 0.5]
    timeout -k 10 600 python tools/spmm_bench.py --matrix rmat --formats csr --balanced

For formats csr and sell, on the cant-like matrix alone (copies = 1) and on
the block-diagonal batch of 32 copies (1.58 GB of matrix, larger than the
256 MiB Infinity Cache: it streams from HBM on every launch), and for
k in {1, 2, 4, 8}, it times
    (a) one run_multi with k vectors (X and Y row-major, ldx = ldy = k);
    (b) k back-to-back run calls on the same plan, on k contiguous vectors.
Device events bracket windows of enough launches to last at least `--window`
seconds, after a warm-up of every shape; (a) and (b) alternate, five windows
each; the figures are the median and the spread (max - min) of the five.

--matrix rmat replaces the cant-like matrices by the power-law R-MAT of the
transposed bench, gen_rmat(100_000, 1_000_000, scale=17, seed=1) (--rmat-large:
the 10,000,000-row / 100,000,000-entry one of bench.py).  --balanced (CSR only)
also times (c) one run_multi on a second plan prepared with
prepare_multi("balanced", --long-len, --seg-len), alternating with (a) and (b),
and reports it against both: `balanced_vs_multi` = (a)/(c), `balanced_vs_loop`
= (b)/(c), each with its own every-window-beat-every-window flag.

One JSON line: per format, matrix and k the ms per call of (a) and of (b)
(all k runs), GB/s of (a) by bytes_alg_multi and its share of the 8 TB/s HBM
peak, the ratio (b)/(a), and `faster`: every window of (a) beat every window
of (b), i.e. the margin exceeds the spread.
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
import spmv_amd as sa  # noqa: E402

KS = (1, 2, 4, 8)
WINDOWS = 5


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
    """Launches per window: at least `seconds` of device time."""
    n = 10
    while True:
        ms = window_ms(torch, fn, n)
        if ms >= seconds * 1e3:
            return n
        n = max(n + 1, int(n * seconds * 1e3 / max(ms, 1e-3) * 1.1) + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--formats", default="csr,sell")
    ap.add_argument("--copies", default="1,32", help="cant-like copies per matrix (1 = the matrix alone)")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of launches per timing window")
    ap.add_argument("--matrix", default="cantlike", choices=("cantlike", "rmat"))
    ap.add_argument("--rmat-large", action="store_true", help="--matrix rmat: 1e7 rows / 1e8 entries (scale 24)")
    ap.add_argument("--balanced", action="store_true", help="csr: also time a plan prepared with prepare_multi")
    ap.add_argument("--long-len", type=int, default=None, help="--balanced: long_len (default: the library's rule)")
    ap.add_argument("--seg-len", type=int, default=None, help="--balanced: seg_len (default: the library's rule)")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("spmm_bench: no GPU")
    dev = torch.device("cuda:0")
    out = {"tool": "spmm_bench", "device": sa.device_name(0), "window_s": a.window, "windows": WINDOWS,
           "hbm_peak_gbs": sa.HBM_PEAK_GBS, "results": {}}
    rng = np.random.default_rng(7)
    if a.matrix == "rmat":
        mats = [("rmat_1e7" if a.rmat_large else "rmat_1e5",
                 sa.gen_rmat() if a.rmat_large else sa.gen_rmat(100_000, 1_000_000, scale=17, seed=1))]
    else:
        mats = (("cantlike" if c == 1 else f"cantlike_x{c}", sa.gen_cantlike(0, c))
                for c in (int(c) for c in a.copies.split(",")))
    for label, m in mats:
        Xs = {k: torch.from_numpy(rng.uniform(-1, 1, (m.n_cols, k))).to(dev) for k in KS}
        Ys = {k: torch.empty((m.n_rows, k), dtype=torch.float64, device=dev) for k in KS}
        xs = torch.from_numpy(rng.uniform(-1, 1, (max(KS), m.n_cols))).to(dev)  # k contiguous vectors
        ys = torch.empty((max(KS), m.n_rows), dtype=torch.float64, device=dev)
        for fmt in a.formats.split(","):
            dm = sa.to_device(m, fmt, dev)
            bal = None
            if a.balanced and fmt == "csr":
                bal = sa.to_device(m, fmt, dev)
                bal.prepare_multi("balanced", a.long_len, a.seg_len)
            fns = {}
            for k in KS:
                fns[k] = ((lambda k=k: dm.run_multi(Xs[k], Ys[k])),
                          (lambda k=k: [dm.run(xs[j], ys[j]) for j in range(k)]))
                if bal is not None:
                    fns[k] += ((lambda k=k: bal.run_multi(Xs[k], Ys[k])),)
            for k in KS:  # warm-up of every shape
                for fn in fns[k]:
                    for _ in range(3):
                        fn()
            torch.cuda.synchronize()
            res = out["results"].setdefault(fmt, {}).setdefault(label, {})
            for k in KS:
                fa, fb = fns[k][:2]
                na, nb = calls_for(torch, fa, a.window), calls_for(torch, fb, a.window)
                nc = calls_for(torch, fns[k][2], a.window) if bal is not None else 0
                wa, wb, wc = [], [], []
                for _ in range(WINDOWS):  # (a), (b) and (c) alternate
                    wa.append(window_ms(torch, fa, na) / na)
                    wb.append(window_ms(torch, fb, nb) / nb)
                    if bal is not None:
                        wc.append(window_ms(torch, fns[k][2], nc) / nc)
                ma, mb = statistics.median(wa), statistics.median(wb)
                gbs = sa.bytes_alg_multi(m.n_rows, m.n_cols, m.nnz, k) / (ma * 1e-3) / 1e9
                res[str(k)] = {"multi_ms": round(ma, 5), "multi_spread_ms": round(max(wa) - min(wa), 5),
                               "loop_ms": round(mb, 5), "loop_spread_ms": round(max(wb) - min(wb), 5),
                               "calls": [na, nb], "gbs": round(gbs, 1), "hbm_share": round(gbs / sa.HBM_PEAK_GBS, 4),
                               "ratio": round(mb / ma, 3), "faster": max(wa) < min(wb)}
                if bal is not None:
                    mc = statistics.median(wc)
                    res[str(k)].update({"balanced_ms": round(mc, 5), "balanced_spread_ms": round(max(wc) - min(wc), 5),
                                        "balanced_vs_multi": round(ma / mc, 3), "balanced_vs_loop": round(mb / mc, 3),
                                        "balanced_faster_than_multi": max(wc) < min(wa),
                                        "balanced_faster_than_loop": max(wc) < min(wb)})
            res["kernel"] = dm.kernel
            if bal is not None:
                res["balanced"] = bal.multi_info
            del dm, bal
        del Xs, Ys, xs, ys
    print(json.dumps(out))


if __name__ == "__main__":
    main()
