"""What the property calls cost: the wall time of gs_histogram (ALPHA and X at 256 bins), gs_prop_range and gs_select_range on the
synthetic scenes of two bench configurations (1 M splats: C2, 20 M: C5), beside gs_select_sphere on the same context -- the same
streaming read of the records, and the yardstick -- and the pile-up case: the ALPHA histogram of the same rows with every alpha byte 255,
where all 64 lanes of every wave want one bin.  Wall time of the call as a host sees it: launch, kernel, read-back, synchronisation.

  python tools/prop_cost.py [--config C2,C5] [--reps 10]

One JSON line per configuration: per call the minimum and the median over --reps calls (after one warm-up call), in milliseconds.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "aframe-gaussian-splatting_amd"


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return r, {"min": round(min(ms), 3), "median": round(float(np.median(ms)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2,C5")
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    capi = importlib.import_module(PKG + ".capi")
    synth = importlib.import_module(PKG + ".synth")
    BC = importlib.import_module(PKG + ".bench_configs")
    for name in args.config.split(","):
        cfg = BC.ALL[name]
        rows = np.array(BC.make_rows(cfg, synth)).reshape(-1, 32)     # (a copy: the pile-up case writes into it)
        n = int(rows.shape[0])
        line = {"tool": "prop_cost", "config": name, "n_splats": n, "reps": args.reps, "record_mb": round(n * 32 / 1e6, 1)}
        with capi.Context(0) as ctx:
            ctx.push_splat(rows)
            (counts, tally), line["hist_alpha_ms"] = timed(lambda: ctx.histogram(capi.PROP_ALPHA, 0.0, 255.0, 256), args.reps)
            line["hist_alpha_max_bin_share"] = round(float(counts.max()) / n, 3)
            (counts, tally), line["hist_x_ms"] = timed(lambda: ctx.histogram(capi.PROP_X, -8.0, 8.0, 256), args.reps)
            line["hist_x_max_bin_share"] = round(float(counts.max()) / n, 3)
            _, line["hist_size2_4096_ms"] = timed(lambda: ctx.histogram(capi.PROP_SIZE2, 0.0, 0.05, 4096), args.reps)
            _, line["prop_range_x_ms"] = timed(lambda: ctx.prop_range(capi.PROP_X), args.reps)
            hit, line["select_range_x_ms"] = timed(lambda: ctx.select_range(capi.PROP_X, -1.0, 1.0, set_bits=capi.STATE_SELECTED), args.reps)
            line["select_range_hit"] = int(hit)
            hit, line["select_sphere_ms"] = timed(lambda: ctx.select_sphere((0.0, 0.0, 0.0), 2.0, set_bits=capi.STATE_SELECTED), args.reps)
            line["select_sphere_hit"] = int(hit)
            # the same histograms with the state byte in the read (a filter with a mask, the store present)
            _, line["hist_alpha_visible_ms"] = timed(lambda: ctx.histogram(capi.PROP_ALPHA, 0.0, 255.0, 256, capi.STATE_HIDDEN, 0), args.reps)
        rows[:, 27] = 255
        with capi.Context(0) as ctx:
            ctx.push_splat(rows)
            (counts, tally), line["hist_alpha_pileup_ms"] = timed(lambda: ctx.histogram(capi.PROP_ALPHA, 0.0, 255.0, 256), args.reps)
            assert int(counts[255]) == n and int(tally[0]) == n
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
