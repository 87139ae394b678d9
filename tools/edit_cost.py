"""What the state store costs a frame, and what the editing calls cost: frames/s of a bench configuration with the store empty, present
with nothing hidden, and with 10 % of the splats hidden -- same build, same run, same loop shape as bench.py's steady state (queued
frames over the orbit's poses, one gs_sync per window) -- and the wall time of select_box, select_rect and compact on that scene
(1 M splats for the headline configuration).  Outside bench.py's timed region.

  python tools/edit_cost.py [--config C2] [--frames 240] [--only empty|present|hidden] [--no-calls]

One JSON line per (configuration, setting); the settings alternate empty, present, hidden, empty, present, hidden so that a drift of
the machine shows.  --only S runs a single setting: `--only empty` is what runs unchanged on a build without the editing calls (a
parent commit loaded through GS_SPLAT_LIB, or checked out), for the comparison "an empty store launches the kernels it launched
before": the two must agree within the spread the alternating settings of one run show.  Through GS_SPLAT_LIB only the fps of such a
build is meaningful -- gs_stats gained a field, so the counters of an older library read through this binding are not.
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
SETTINGS = ("empty", "present", "hidden")


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--only", choices=SETTINGS, default=None)
    ap.add_argument("--no-calls", action="store_true", help="skip the timing of select_box / select_rect / compact")
    args = ap.parse_args()
    capi = importlib.import_module(PKG + ".capi")
    synth = importlib.import_module(PKG + ".synth")
    BC = importlib.import_module(PKG + ".bench_configs")
    has_edit = hasattr(capi.load(), "gs_set_state")
    for name in args.config.split(","):
        cfg = BC.ALL[name]
        rows = np.asarray(BC.make_rows(cfg, synth)).reshape(-1, 32)
        n = int(rows.shape[0])
        cams, views, W, H = BC.poses(cfg, synth, capi)
        hid = (np.random.Generator(np.random.PCG64(11)).random(n) < 0.1).astype(np.uint8)
        for setting in ([args.only] if args.only else SETTINGS + SETTINGS):
            if setting != "empty" and not has_edit:
                print(json.dumps({"tool": "edit_cost", "config": name, "setting": setting, "skipped": "this library has no gs_set_state"}), flush=True)
                continue
            with capi.Context(0) as ctx:
                BC.apply_options(ctx, capi, BC.options_for(cfg, env={}))
                ctx.push_splat(rows)
                if setting == "present":
                    ctx.set_state(0, np.zeros(n, np.uint8))
                elif setting == "hidden":
                    ctx.set_state(0, hid)

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
                line = {"tool": "edit_cost", "config": name, "size": [W, H], "n_splats": n, "setting": setting, "frames": args.frames,
                        "fps": round(args.frames / dt, 1), "us_per_frame": round(1e6 * dt / args.frames, 1)}
                if has_edit:
                    st = ctx.stats()
                    line.update({"state_rows": ctx.state_count()[0], "n_hidden": st["n_hidden"], "n_sorted": st["n_sorted"],
                                 "near_permille": st["near_permille"], "retried_frames": st["retried_frames"]})
                print(json.dumps(line), flush=True)
        if args.no_calls or not has_edit:
            continue
        # the editing calls themselves, each on a freshly loaded context (wall time of the call: drain, kernel, count, read-back)
        with capi.Context(0) as ctx:
            ctx.push_splat(rows)
            p = views[0][0]
            p.flags = 0
            box = cams[0]["cutout"]
            if box is None:                                           # a box of half the cloud's extent around its centre
                box = np.zeros(16, np.float32); box[0] = box[5] = box[10] = 0.25; box[15] = 1.0
            ctx.sort(cams[0]["view"], None, want_indices=False)
            ctx.render_device(p, None)
            calls = {}
            for rep in range(3):
                hit, ms = timed(lambda: ctx.select_box(box, set_bits=capi.STATE_SELECTED))
                calls.setdefault("select_box_ms", []).append(round(ms, 3)); calls["select_box_hit"] = hit
                ctx.sort(cams[0]["view"], None, want_indices=False)
                hit, ms = timed(lambda: ctx.select_rect(p, (W // 4, H // 4, 3 * W // 4, 3 * H // 4), set_bits=capi.STATE_SELECTED))
                calls.setdefault("select_rect_ms", []).append(round(ms, 3)); calls["select_rect_hit"] = hit
            ctx.set_state(0, hid)
            old, ms = timed(ctx.compact)
            calls["compact_ms"] = round(ms, 3); calls["compact_kept"] = int(old.size)
            print(json.dumps(dict({"tool": "edit_cost", "config": name, "n_splats": n, "setting": "calls"}, **calls)), flush=True)


if __name__ == "__main__":
    main()
