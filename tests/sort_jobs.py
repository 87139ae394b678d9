"""The job runner of tests/test_sort_paths_gpu.py: a JOB is one fresh context and a list of steps on it; every sorting step yields an
index list.  The test module runs jobs in its own process (default environment: the MSD sort where run_sort allows it) and, as
`python sort_jobs.py DIR`, in a child process started with GS_SORT_MSD=0 in the environment (the library reads the switch once per
process): the child reads DIR/jobs.json, whose steps name arrays stored as DIR/<name>.npy, and writes every list to DIR/<out>.npy.

Steps (lists, JSON-able; an array argument is a numpy array in process and the name of a .npy in the child):
    ["push", rows4]                      rows (x, y, z, size) f32, pushed as worker matrices (tests/test_gpu_parity._expand's layout)
    ["clear"]
    ["wide", 0 | 1]                      GS_OPT_WIDE_PAIRS
    ["sort", view, cutout | None, out]   gs_sort -> the list `out`
    ["posted", view, cutout | None, out] gs_sort_begin + gs_sort_poll(wait) -> the list `out`
"""
import json
import os
import sys

import numpy as np

PUSH_ROWS = 1 << 20                 # rows per push_matrices call (64 bytes each as pushed: 64 MB of host memory at a time)


def expand(rows4):
    m = np.zeros((rows4.shape[0], 16), np.float32)
    m[:, 12:16] = rows4
    m[:, :12] = 3.25                # must be ignored (index.js:520-548 read only 12..15)
    return m


def run_job(capi, steps, load=lambda a: a):
    """-> {out name: uint32 list} of the job's sorting steps, in one fresh context"""
    got = {}
    with capi.Context(0) as c:
        for st in steps:
            op = st[0]
            if op == "push":
                rows4 = np.ascontiguousarray(load(st[1]), np.float32).reshape(-1, 4)
                for o in range(0, rows4.shape[0], PUSH_ROWS):
                    c.push_matrices(expand(rows4[o:o + PUSH_ROWS]))
            elif op == "clear":
                c.clear()
            elif op == "wide":
                c.set_option(capi.OPT_WIDE_PAIRS, int(st[1]))
            elif op in ("sort", "posted"):
                view, cut = load(st[1]), None if st[2] is None else load(st[2])
                assert st[3] not in got, st[3]
                if op == "sort":
                    got[st[3]] = c.sort(view, cut)
                else:
                    c.sort_begin(view, cut)
                    got[st[3]] = c.sort_poll(wait=True)
            else:
                raise ValueError("unknown step %r" % (op,))
    return got


def child_main(d):
    here = os.path.dirname(os.path.abspath(__file__))
    if here not in sys.path:
        sys.path.insert(0, here)
    from conftest import pkg
    capi = pkg("capi")
    with open(os.path.join(d, "jobs.json")) as f:
        jobs = json.load(f)
    cache = {}

    def load(name):
        if name not in cache:
            cache.clear()                                          # (one array at a time: the long ones are tens of MB)
            cache[name] = np.load(os.path.join(d, name + ".npy"))
        return cache[name]

    for k, steps in enumerate(jobs):
        for name, idx in run_job(capi, steps, load).items():
            np.save(os.path.join(d, name + ".npy"), idx)
        print("job %d of %d done" % (k + 1, len(jobs)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(child_main(sys.argv[1]))
