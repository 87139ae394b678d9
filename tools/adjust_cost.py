"""What an in-place change costs: the wall time of gs_adjust_colour at 1 048 576 splats -- without an SH store and with a degree-3 one, for
every splat and for 10 % selected -- and of gs_replace_splat of 1 % and of all rows, beside two yardsticks measured in the same run:
gs_select_range over the same cloud (one streaming pass with a count, like the adjustment) and gs_clear + gs_push_splat of all rows (what
a host had to do before these calls existed).  Wall time of the call as a host sees it: drain, launches, kernels, synchronisation.

  python tools/adjust_cost.py [--n 1048576] [--reps 7]

One JSON line: per call the minimum and the median over --reps calls (after one warm-up call), in milliseconds.
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
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"min": round(min(ms), 3), "median": round(float(np.median(ms)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    capi = importlib.import_module(PKG + ".capi")
    synth = importlib.import_module(PKG + ".synth")
    n = args.n
    rows = synth.make_splat_rows_fast(n, seed=20261021).reshape(n, 32)
    # close to the identity, so that repeated calls neither saturate nor fade the cloud
    adj = capi.colour_adjust([[1.0, 0.015625, 0.0], [0.0, 1.0, 0.015625], [0.015625, 0.0, 1.0]], (0.25, -0.25, 0.0), 1.0, 0.0)
    line = {"tool": "adjust_cost", "n_splats": n, "reps": args.reps}
    with capi.Context(0) as ctx:
        ctx.push_splat(rows)
        store = np.zeros(n, np.uint8)
        store[::10] = capi.STATE_SELECTED
        ctx.set_state(0, store)
        sel = (capi.STATE_SELECTED, capi.STATE_SELECTED)
        line["selected"] = int(ctx.adjust_colour(capi.colour_adjust(), sel))
        line["select_range_ms"] = timed(lambda: ctx.select_range(capi.PROP_ALPHA, 0, 255, set_bits=0x40), args.reps)
        line["adjust_all_ms"] = timed(lambda: ctx.adjust_colour(adj, "all"), args.reps)
        line["adjust_10pct_ms"] = timed(lambda: ctx.adjust_colour(adj, sel), args.reps)
        g = np.random.Generator(np.random.PCG64(5))
        sh = g.standard_normal((n, 48), dtype=np.float32) * np.float32(0.2)
        ctx.push_sh(sh, 3)
        line["sh_mb"] = round(sh.nbytes / 1e6, 1)
        line["adjust_all_sh3_ms"] = timed(lambda: ctx.adjust_colour(adj, "all"), args.reps)
        line["adjust_10pct_sh3_ms"] = timed(lambda: ctx.adjust_colour(adj, sel), args.reps)
        k = n // 100
        line["replace_1pct_ms"] = timed(lambda: ctx.replace_splat(n // 2, rows[:k]), args.reps)
        line["replace_all_ms"] = timed(lambda: ctx.replace_splat(0, rows), args.reps)
        line["replace_sh_1pct_ms"] = timed(lambda: ctx.replace_sh(n // 2, sh[:k], 3), args.reps)

        def again():
            ctx.clear()
            ctx.push_splat(rows)

        line["clear_push_all_ms"] = timed(again, args.reps)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
