"""What view-dependent colour costs: frames/s of a bench configuration with GS_OPT_SH_DEGREE at 0 and at --degree, same build, same
loop shape as bench.py's steady state (queued frames over the orbit's poses, one gs_sync per window).  Outside bench.py's timed region.

  python tools/sh_cost.py [--config C2,R_outside] [--degree 3] [--frames 240] [--only D]

The scene is the configuration's, written as an INRIA .ply (synth.rows_to_inria_ply) with random f_rest and loaded through
gs_load_ply.  One JSON line per (configuration, degree).  --only D runs a single degree, for a profiler run of its own:
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/sh_cost.py --config R_outside --only 3
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2,R_outside")
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--only", type=int, default=None)
    args = ap.parse_args()
    capi = importlib.import_module(PKG + ".capi")
    synth = importlib.import_module(PKG + ".synth")
    BC = importlib.import_module(PKG + ".bench_configs")
    for name in args.config.split(","):
        cfg = BC.ALL[name]
        rows = np.asarray(BC.make_rows(cfg, synth)).reshape(-1, 32)
        rest = (np.random.default_rng(7).standard_normal((rows.shape[0], 45)) * 0.3).astype(np.float32)
        ply = synth.rows_to_inria_ply(rows, rest)
        del rest
        cams, views, W, H = BC.poses(cfg, synth, capi)
        for degree in ([args.only] if args.only is not None else [0, args.degree, 0, args.degree]):
            with capi.Context(0) as ctx:
                BC.apply_options(ctx, capi, BC.options_for(cfg, env={}))
                ctx.set_option(capi.OPT_SH_DEGREE, degree)
                ctx.load_ply(ply)

                def frame(k, flags):
                    k %= BC.ORBIT_FRAMES
                    ctx.sort(cams[k]["view"], cams[k]["cutout"], want_indices=False)
                    p = views[k][0]
                    p.flags = flags
                    ctx.render_device(p, None)

                for k in range(24):                                   # settle the binning share synchronously, then warm the lanes
                    frame(k, 0)
                for k in range(48):
                    frame(k, capi.RENDER_ASYNC)
                ctx.sync()
                t0 = time.perf_counter()
                for k in range(args.frames):
                    frame(k, capi.RENDER_ASYNC)
                    if k % 24 == 23:
                        ctx.sync()
                ctx.sync()
                dt = time.perf_counter() - t0
                st = ctx.stats()
                print(json.dumps({"tool": "sh_cost", "config": name, "sh_degree_option": degree, "sh_degree_ran": st["sh_degree"],
                                  "sh_rows": ctx.sh_count()[0], "frames": args.frames, "fps": round(args.frames / dt, 1),
                                  "us_per_frame": round(1e6 * dt / args.frames, 1), "n_visible": st["n_visible"], "n_sorted": st["n_sorted"],
                                  "retried_frames": st["retried_frames"]}), flush=True)


if __name__ == "__main__":
    main()
