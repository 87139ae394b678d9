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
and for tests/test_near_sort_gpu.py (renderable rows; the lane's order as it lies):
    ["splat", rows4]                     the same rows as 32-byte .splat records (scale = size three times, alpha 255): a renderable context
    ["state", first, states]             gs_set_state
    ["opt", option, value]               gs_set_option
    ["rows", out]                        the resident sort rows, as uint32 words -> `out`
    ["near", view, cutout | None, out]   gs_sort without a list + gs_sort_inspect -> `out`: the INFO_FIELDS words, then the lane's records
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


INFO_FIELDS = ("form", "near_req", "n_kept", "n_valid", "n_records", "order_incomplete", "near_overflow", "spec_fail", "threshold_bin")


def splat_rows(rows4):
    """rows (x, y, z, size) -> .splat records whose sort row is exactly that row (index.js:396-401: position, max scale * alpha / 255)"""
    rows4 = np.ascontiguousarray(rows4, np.float32).reshape(-1, 4)
    rec = np.zeros(rows4.shape[0], dtype=[("p", "<f4", 3), ("s", "<f4", 3), ("c", "u1", 4), ("q", "u1", 4)])
    rec["p"] = rows4[:, :3]
    rec["p"][:, 2] = -rows4[:, 2]                                   # (index.js:350-354: the row holds -z)
    rec["s"] = rows4[:, 3:4]
    rec["c"] = (200, 180, 160, 255)
    rec["q"] = (255, 128, 128, 128)
    return rec.view(np.uint8).reshape(-1, 32)


def near_sort(c, view, cut=None):
    """gs_sort without a list, then the lane's order as it lies -> INFO_FIELDS words + records"""
    c.sort(view, cut, want_indices=False)
    info, rec = c.sort_inspect()
    return np.concatenate([np.array([info[k] for k in INFO_FIELDS], np.uint32), rec])


def decode(words):
    k = len(INFO_FIELDS)
    return {f: int(w) for f, w in zip(INFO_FIELDS, words[:k])}, words[k:]


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
            elif op == "splat":
                rows4 = np.ascontiguousarray(load(st[1]), np.float32).reshape(-1, 4)
                for o in range(0, rows4.shape[0], PUSH_ROWS):
                    c.push_splat(splat_rows(rows4[o:o + PUSH_ROWS]))
            elif op == "state":
                c.set_state(int(st[1]), load(st[2]))
            elif op == "opt":
                c.set_option(int(st[1]), int(st[2]))
            elif op == "rows":
                got[st[1]] = c.download(capi.BUF_SORT_ROWS, c.count(), np.float32, 4).view(np.uint32).reshape(-1)
            elif op == "near":
                assert st[3] not in got, st[3]
                got[st[3]] = near_sort(c, load(st[1]), None if st[2] is None else load(st[2]))
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
