"""What the surface output costs: a synchronous surface frame (gs_render_surface_device: colour + id, depth and alpha planes, all on
the device), the same frame as a plain synchronous gs_render_device on the forced lists path -- the fair parent: a surface frame
always takes tile lists -- and a one-point gs_pick, at one pose of a bench configuration.  Outside bench.py's timed region.

  python tools/surface_cost.py [--config C2,R_outside] [--frames 200] [--warmup 20]

Median wall time of --frames calls after --warmup calls, one sort before them (the order is reused: what is timed is the frame).
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
    hip = capi.hip_runtime()
    for name in args.config.split(","):
        cfg = BC.ALL[name]
        rows = np.asarray(BC.make_rows(cfg, synth)).reshape(-1, 32)
        cams, views, W, H = BC.poses(cfg, synth, capi)
        p = views[0][0]
        p.flags = 0
        planes = C.c_void_p()
        n = W * H
        stride = (4 * n + 255) & ~255
        assert hip.hipMalloc(C.byref(planes), 3 * stride) == 0
        with capi.Context(0) as ctx:
            BC.apply_options(ctx, capi, BC.options_for(cfg, env={}))
            for k, v in ((capi.OPT_BINNING, 0), (capi.OPT_ROW_WALK, 0), (capi.OPT_SUBTILE, 0), (capi.OPT_BLEND_SPLIT, 0)):
                ctx.set_option(k, v)                                  # the lists path, for both kinds of frame
            ctx.push_splat(rows)
            ctx.sort(cams[0]["view"], cams[0]["cutout"], want_indices=False)
            plain = median_us(lambda: ctx.render_device(p, None), args.frames, args.warmup)
            st0 = ctx.stats()
            surf = median_us(lambda: ctx.render_surface_device(p, None, planes.value, planes.value + stride, planes.value + 2 * stride),
                             args.frames, args.warmup)
            st1 = ctx.stats()
            pt = [(W // 2, H // 2)]
            pick = median_us(lambda: ctx.pick(p, pt), args.frames, args.warmup)
            hit = ctx.pick(p, pt)[0]
        hip.hipFree(planes)
        print(json.dumps({"tool": "surface_cost", "config": name, "size": [W, H], "n_splats": int(rows.shape[0]), "frames": args.frames,
                          "plain_lists_us": plain, "surface_us": surf, "surface_over_plain": round(surf / plain, 3), "pick1_us": pick,
                          "plain_stats": {k: st0[k] for k in ("row_walk", "subtile", "binning", "surface")},
                          "surface_stats": {k: st1[k] for k in ("row_walk", "subtile", "binning", "surface")},
                          "centre_hit": {"id": int(hit["id"]), "depth": float(hit["depth"]), "alpha": float(hit["alpha"])}}), flush=True)


if __name__ == "__main__":
    main()
