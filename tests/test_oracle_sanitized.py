"""CPU tier: the C restatement (oracle/gs_oracle.c) under AddressSanitizer + UndefinedBehaviorSanitizer.
The oracle is what most parity claims are trusted through -- the golden vectors pin its RESULTS, this pins that it gets them
without reading or writing out of bounds, without signed overflow, misaligned access or an invalid shift.  The sanitized build
is loaded by a child interpreter (libasan has to come first in the process), which runs the reference-generated sort / pack /
PLY / camera vectors, a GL golden and seeded renders with strips, scene inputs and ragged sizes through it."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(os.environ["GS_ROOT"], "tests")); sys.path.insert(0, os.environ["GS_ROOT"])
from conftest import cases_of, load_case, pkg
from oracle import oracle
assert oracle._SO.endswith("libgs_oracle_san.so")
synth = pkg("synth")
n = 0
for name in cases_of("sort"):
    c = load_case(name)
    if "rows4" not in c:
        continue
    m = np.zeros((c["rows4"].size // 4, 16), np.float32); m[:, 12:16] = c["rows4"].reshape(-1, 4)
    got = oracle.sort(m, c["view"], c.get("cutout"))
    assert np.array_equal(got, c["sorted"]), name
    n += 1
for name in cases_of("pack"):
    c = load_case(name)
    cs, cc, mats = oracle.pack(c["rows"])
    assert np.array_equal(cs.view(np.uint32).reshape(-1), c["center_scale"].view(np.uint32).reshape(-1)), name
    assert np.array_equal(cc.reshape(-1), c["cov_color"].reshape(-1)), name
    n += 1
for name in cases_of("ply"):
    c = load_case(name)
    assert np.array_equal(oracle.ply_to_splat(c["ply"].tobytes()).reshape(-1), c["rows"].reshape(-1)), name
    n += 1
# seeded renders: ragged sizes (partial tiles), strips, flipped... whatever the wrapper offers, plus a scene depth / colour image
rows = synth.make_splat_rows(6000, seed=31)
cs, cc, mats = oracle.pack(rows)
for (w, h, yaw, x0, x1) in ((333, 190, 75.0, 0, 333), (320, 180, 10.0, 17, 203), (64, 48, 200.0, 0, 64)):
    cam = synth.index_html_camera(w, h, yaw)
    idx = oracle.sort(mats, cam["view"])
    img, _, frags = oracle.render(cs, cc, idx, cam["gs_mv"].astype(np.float32), cam["gs_proj"].astype(np.float32), np.float32(cam["focal"]),
                                  w, h, x0=x0, x1=x1, want_f32=False)
    assert np.asarray(img).size == (x1 - x0) * h * 4 and frags > 0
    n += 1
cam = synth.index_html_camera(256, 144, 130.0)
idx = oracle.sort(mats, cam["view"])
depth = np.full((144, 256), 0.9995, np.float32); rgba = np.full((144, 256, 4), 200, np.uint8)
oracle.render(cs, cc, idx, cam["gs_mv"].astype(np.float32), cam["gs_proj"].astype(np.float32), np.float32(cam["focal"]), 256, 144,
              want_f32=False, scene_depth=depth, scene_rgba=rgba)
# degenerate inputs the reference has defined answers for: nothing kept, one splat, equal depths
z = np.zeros((3, 16), np.float32); z[:, 14] = -5.0; z[:, 15] = 1.0
assert oracle.sort(z, np.array([0, 0, 1, 0], np.float32)).tolist() == [0, 1, 2]
assert oracle.sort(z, np.array([0, 0, -1, 0], np.float32)).size == 0
print("sanitized oracle ok:", n + 3, "cases")
'''


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_oracle_under_asan_and_ubsan():
    from oracle import oracle
    try:
        so = oracle.build_sanitized()
    except subprocess.CalledProcessError:
        pytest.skip("this gcc cannot build with -fsanitize=address,undefined")
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(asan) or not os.path.exists(asan):
        pytest.skip("libasan.so not found")
    # (the runtime goes first in the preload list; whatever the environment already preloads stays behind it)
    env = dict(os.environ, GS_ORACLE_LIB=so, GS_ROOT=ROOT, LD_PRELOAD=":".join(p for p in (asan, os.environ.get("LD_PRELOAD")) if p),
               ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "sanitized oracle ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
