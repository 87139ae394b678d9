"""What moving resident splats costs: the wall time of gs_transform at 1 048 576 splats -- a pure translation (no covariance work, no SH
kernel) and a general similarity (rotation, scale, translation), for every splat and for 10 % selected, without an SH store and with a
degree-3 one -- beside the workaround it replaces, measured in the same run: gs_export_splat of all rows + gs_replace_splat of all rows
(the two transfers and the pack; the host's own arithmetic on the rows is left out, so the yardstick is a lower bound), and
gs_select_range over the same cloud (one streaming pass with a count).  Wall time of the call as a host sees it: drain, launches,
kernels, synchronisation.

  python tools/transform_cost.py [--n 1048576] [--reps 7]

One JSON line: per call the minimum and the median over --reps calls (after one warm-up call), in milliseconds.
"""
import argparse
import importlib
import json
import math
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
    # small steps, so that repeated calls keep the cloud where the numbers are ordinary: 2 degrees about a skew axis, 1 % larger
    h = math.radians(2.0) / 2
    axis = np.array([0.3, -0.8, 0.52]) / np.linalg.norm([0.3, -0.8, 0.52])
    general = capi.similarity((math.cos(h), *(math.sin(h) * axis)), 1.01, (0.01, -0.02, 0.015))
    move = capi.similarity(translation=(0.01, -0.02, 0.015))
    line = {"tool": "transform_cost", "n_splats": n, "reps": args.reps}
    with capi.Context(0) as ctx:
        ctx.push_splat(rows)
        store = np.zeros(n, np.uint8)
        store[::10] = capi.STATE_SELECTED
        ctx.set_state(0, store)
        sel = (capi.STATE_SELECTED, capi.STATE_SELECTED)
        line["selected"] = int(ctx.transform(capi.similarity(), sel))
        line["select_range_ms"] = timed(lambda: ctx.select_range(capi.PROP_ALPHA, 0, 255, set_bits=0x40), args.reps)
        line["translate_all_ms"] = timed(lambda: ctx.transform(move, "all"), args.reps)
        line["general_all_ms"] = timed(lambda: ctx.transform(general, "all"), args.reps)
        line["general_10pct_ms"] = timed(lambda: ctx.transform(general, sel), args.reps)
        g = np.random.Generator(np.random.PCG64(5))
        sh = g.standard_normal((n, 48), dtype=np.float32) * np.float32(0.2)
        ctx.push_sh(sh, 3)
        line["sh_mb"] = round(sh.nbytes / 1e6, 1)
        line["translate_all_sh3_ms"] = timed(lambda: ctx.transform(move, "all"), args.reps)
        line["general_all_sh3_ms"] = timed(lambda: ctx.transform(general, "all"), args.reps)
        line["general_10pct_sh3_ms"] = timed(lambda: ctx.transform(general, sel), args.reps)

        def workaround():
            ctx.replace_splat(0, ctx.export_splat())

        line["export_replace_all_ms"] = timed(workaround, args.reps)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
