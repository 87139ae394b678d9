"""CPU tier: the round-0 share policy (csrc/gs_share.h -- host-only arithmetic on the integers a collection reads from the lanes'
control blocks) replayed over scripted collections by tests/host_check/share_replay.cpp and compared, byte for byte, with
tests/golden/share_policy.trace.  The trace was recorded from the functions the header replaced (share_raise, share_from_need,
share_missed, round1_skippable, the policy part of collect_status and the four hand-written resets), and it carries its script: the
lines that start with "> ".  After every step every field of the policy state and every output go into one line, floats as bit
patterns; the trace holds that line for the resets and at each script's end and its 32-bit hash for every collection (in full it
is 680 KB).  A change to a margin, a hold, a threshold or a reset shows here without a GPU."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

HC_DIR = os.path.join(ROOT, "tests", "host_check")
CSRC = os.path.join(ROOT, "aframe-gaussian-splatting_amd", "csrc")


@pytest.fixture(scope="module")
def replay():
    so = os.path.join(HC_DIR, "libshare_replay.so")
    srcs = [os.path.join(HC_DIR, "share_replay.cpp"), os.path.join(HC_DIR, "share_replay.h"), os.path.join(CSRC, "gs_share.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fvisibility=hidden", "-Wall", "-Werror",
                               "-I", CSRC, "-o", so, srcs[0]])
    L = C.CDLL(so)
    L.share_replay.restype = C.c_size_t
    L.share_replay.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]

    def run(script, full=False):
        n = L.share_replay(script.encode(), int(full), None, 0)
        buf = C.create_string_buffer(n)
        assert L.share_replay(script.encode(), int(full), buf, n) == n
        return buf.raw.decode()
    return run


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "share_policy.trace")) as f:
        return f.read()


def script_of(trace):
    return "".join(l[2:] + "\n" for l in trace.split("\n") if l.startswith("> "))


def steps_of(trace):
    """one item per step: its line, or -- a collection in the short form -- its hash"""
    items = []
    for l in trace.split("\n"):
        if l.startswith("= "):
            items += l[2:].split()
        elif l and not l.startswith("> "):
            items.append(l)
    return items


def test_policy_replays_the_recorded_trace_exactly(replay, golden):
    script = script_of(golden)
    got = replay(script)
    if got != golden:
        g, w, full = steps_of(got), steps_of(golden), steps_of(replay(script, full=True))
        assert len(full) == len(g)
        k = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        name = next((l for l in reversed(w[:k + 1]) if l.startswith("# ")), "?")
        pytest.fail("first difference at step %d (%s): recorded %s, now %s\n now in full: %s\n the step before: %s" % (
            k, name, w[k] if k < len(w) else "<end>", g[k] if k < len(g) else "<end>", full[k] if k < len(full) else "<end>", full[k - 1] if k else ""))


def test_the_scripts_reach_what_they_are_there_for(replay, golden):
    """The trace is only a regression check where its scripts take the paths: each script collects 50-400 times, and the states that
    the scripts are named after occur in the trace printed in full."""
    steps, body, name = {}, {}, None
    for l in replay(script_of(golden), full=True).split("\n"):
        if l.startswith("# "):
            name = l[2:]
        elif l.startswith(("sync ", "frame ")):
            steps[name] = steps.get(name, 0) + 1
            body.setdefault(name, []).append(l)
    assert len(steps) == 15 and all(50 <= v <= 400 for v in steps.values()), steps
    assert sum(len(h) == 8 for h in steps_of(golden)) == sum(steps.values())                                            # one hash per collection
    assert any("frac=3f000000 " in l and "meas=0" in l for l in body["reprobe_after_64_single_round_frames"])        # back to 0.5
    assert any("margin=3f851eb8 " in l for l in body["miss_under_measured_share"])                                     # the margin at 1.04 ...
    assert any("margin=3fa66666 " in l for l in body["miss_under_measured_share"])                                     # ... after 1.3
    assert any("frac=3a83126f " in l and "skip=1" in l for l in body["walked_share_never_fails"])                      # the minimum share
    assert sum("failed=1" in l for l in body["six_lanes_one_failure"]) == 5
    assert any("frac=3f800000 " in l for l in body["sky"]) and any("skip=1" in l and "nc=4294967295" not in l for l in body["sky"])
    assert any(" pos=15 " in l for l in body["window_rollover"]) and any(" pos=0 " in l and " 15=" in l for l in body["window_rollover"])
