"""What a contribution frame costs: a synchronous gs_render_contrib_device (colour on the device, every applied fragment's weight added
to the contribution store) and the same frame as a plain synchronous gs_render_device on the forced lists path -- the fair parent: a
contribution frame always takes tile lists -- at one pose of a bench configuration, on a fresh context each.  Outside bench.py's
timed region.

  python tools/contrib_cost.py [--config C2,R_outside] [--frames 200] [--warmup 20]

Median wall time of --frames calls after --warmup calls, one sort before them (the order is reused: what is timed is the frame).
The contribution frame's time includes the copy of the store queued in front of its kernels (8 bytes per splat, device to device, no
host wait); store_copy_us is that copy alone as a synchronous hipMemcpy -- an upper bound: it includes a host wait the frame does not pay.
One JSON line per configuration.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "aframe-gaussian-splatting_amd"


def median_us(call, frames, warmup):
    for _ in range(warmup):
        call()
    t = []
    for _ in range(frames):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return round(1e6 * float(np.median(t)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2,R_outside")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    capi = importlib.import_module(PKG + ".capi")
    synth = importlib.import_module(PKG + ".synth")
    BC = importlib.import_module(PKG + ".bench_configs")
    for name in args.config.split(","):
        cfg = BC.ALL[name]
        rows = np.asarray(BC.make_rows(cfg, synth)).reshape(-1, 32)
        cams, views, W, H = BC.poses(cfg, synth, capi)
        p = views[0][0]
        p.flags = 0
        out = {}
        for kind in ("plain", "contrib"):
            with capi.Context(0) as ctx:
                BC.apply_options(ctx, capi, BC.options_for(cfg, env={}))
                for k, v in ((capi.OPT_BINNING, 0), (capi.OPT_ROW_WALK, 0), (capi.OPT_SUBTILE, 0), (capi.OPT_BLEND_SPLIT, 0)):
                    ctx.set_option(k, v)                              # the lists path, for both kinds of frame
                ctx.push_splat(rows)
                ctx.sort(cams[0]["view"], cams[0]["cutout"], want_indices=False)
                call = (lambda: ctx.render_device(p, None)) if kind == "plain" else (lambda: ctx.render_contrib_device(p, None))
                out[kind] = median_us(call, args.frames, args.warmup)
                st = ctx.stats()
                out[kind + "_stats"] = {k: st[k] for k in ("row_walk", "subtile", "binning", "near_permille", "n_visible", "n_pairs")}
                if kind == "contrib":
                    rows_n, frames_n = ctx.contrib_info()
                    store = ctx.download_contrib()
                    out["seen"] = {"rows": rows_n, "frames": frames_n, "splats_with_weight": int((store > 0).sum()),
                                   "pixels_per_frame": round(float(store.sum()) / 65536.0 / max(frames_n, 1), 1)}
        hip = capi.hip_runtime()
        buf, nbytes = C.c_void_p(), 8 * int(rows.shape[0])
        assert hip.hipMalloc(C.byref(buf), 2 * nbytes) == 0
        copy_us = median_us(lambda: hip.hipMemcpy(buf, C.c_void_p(buf.value + nbytes), nbytes, 3), args.frames, args.warmup)
        hip.hipFree(buf)
        out["contrib_stats"]["store_copy_us"] = copy_us
        print(json.dumps({"tool": "contrib_cost", "config": name, "size": [W, H], "n_splats": int(rows.shape[0]), "frames": args.frames,
                          "plain_lists_us": out["plain"], "contrib_us": out["contrib"], "contrib_over_plain": round(out["contrib"] / out["plain"], 3),
                          "plain_stats": out["plain_stats"], "contrib_stats": out["contrib_stats"], "seen": out["seen"]}), flush=True)


if __name__ == "__main__":
    main()
