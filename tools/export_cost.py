"""What an export costs: the wall time of gs_export_splat (rows alone; rows, wide parts and indices; with a filter that reads the state
store), of its size query and of gs_export_ply on the synthetic scene of a bench configuration (C2: the headline's 1 M splats; C5: 20 M),
beside gs_download of the two packed records of the same splats -- the same number of bytes over the same link, with no arithmetic:
the yardstick.  Wall time of the call as a host sees it: launches, kernels, the copy to pageable host memory, synchronisation.

  python tools/export_cost.py [--config C2] [--reps 5]

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
    ap.add_argument("--config", default="C2")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    capi = importlib.import_module(PKG + ".capi")
    synth = importlib.import_module(PKG + ".synth")
    BC = importlib.import_module(PKG + ".bench_configs")
    for name in args.config.split(","):
        cfg = BC.ALL[name]
        rows = np.asarray(BC.make_rows(cfg, synth)).reshape(-1, 32)
        n = int(rows.shape[0])
        line = {"tool": "export_cost", "config": name, "n_splats": n, "reps": args.reps, "row_mb": round(n * 32 / 1e6, 1)}
        with capi.Context(0) as ctx:
            ctx.push_splat(rows)

            def download():
                return ctx.download(capi.BUF_CENTER_SCALE, n, np.float32, 4), ctx.download(capi.BUF_COV_COLOR, n, np.uint32, 4)

            _, line["download_records_ms"] = timed(download, args.reps)
            out, line["export_rows_ms"] = timed(lambda: ctx.export_splat("all"), args.reps)
            assert out.shape == (n, 32)
            _, line["export_rows_wide_index_ms"] = timed(lambda: ctx.export_splat("all", want_wide=True, want_index=True), args.reps)
            store = np.zeros(n, np.uint8)
            store[::10] = capi.STATE_HIDDEN
            ctx.set_state(0, store)
            out, line["export_visible_ms"] = timed(lambda: ctx.export_splat("visible"), args.reps)
            line["visible_rows"] = int(len(out))
            import ctypes as C
            k = C.c_size_t(0)
            _, line["size_query_ms"] = timed(lambda: ctx._ck(ctx._L.gs_export_splat(ctx._h, capi.STATE_HIDDEN, 0, None, None, None, C.byref(k))), args.reps)
            ply, line["export_ply_ms"] = timed(lambda: ctx.export_ply("visible", 0), args.reps)
            line["ply_mb"] = round(len(ply) / 1e6, 1)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
