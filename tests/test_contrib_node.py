"""The per-splat contribution through the reference-language host side: the addon's renderContrib / contribClear / contribInfo and the
component shim's accumulateSeen / clearSeen and the property name 'seen', driven by node (tests/js/test_contrib.js) on one 64x48
scene, and compared with capi: the range and the 64-bin histogram of GS_PROP_SEEN after one contribution frame of the same view, the
number of splats the view never shows, and the histogram after they are deleted."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

JS = os.path.join(ROOT, "tests", "js")
NODE = shutil.which("node")


def _addon():
    b = pkg("build")
    b.build_lib()
    return b.build_addon()


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_and_shim_contrib_cpu():
    assert _addon() is not None
    r = subprocess.run([NODE, os.path.join(JS, "test_contrib.js"), "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "contrib cpu checks ok" in r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_accumulate_seen_against_capi_gpu(tmp_path):
    synth, capi = pkg("synth"), pkg("capi")
    assert _addon() is not None
    n, W, H = 2000, 64, 48
    rows = synth.make_splat_rows(n, seed=77)
    scene = tmp_path / "scene.splat"
    scene.write_bytes(rows.tobytes())
    proj, cam_w, obj_w = synth.perspective(80.0, W / H), synth.compose((0.0, 1.6, 0.0)), synth.compose((0.0, 1.5, -2.0), 15.0)
    pose = tmp_path / "pose.json"
    pose.write_text(json.dumps({"width": W, "height": H, "proj": [float(v) for v in proj], "camera": [float(v) for v in cam_w],
                                "object": [float(v) for v in obj_w]}))
    r = subprocess.run([NODE, os.path.join(JS, "test_contrib.js"), "gpu", str(scene), str(pose)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "contrib gpu checks ok" in r.stdout
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    u = synth.uniforms(cam_w, obj_w, proj, W, H, capi=capi)
    with capi.Context(0) as c:
        c.push_splat(rows)
        c.sort(u["view"])
        c.render_contrib(capi.make_params(u["gs_mv"], u["gs_proj"], W, H, focal_=u["focal"]), want_rgba=False)
        mn, mx, cnt = c.prop_range(capi.PROP_SEEN)
        counts, _ = c.histogram(capi.PROP_SEEN, mn, mx, 64)
        unseen = c.select_range(capi.PROP_SEEN, 0, 0, set_bits=capi.STATE_HIDDEN)
        c.compact()
        after, _ = c.histogram(capi.PROP_SEEN, mn, mx, 64)
    assert got["count"] == cnt == n and (got["min"], got["max"]) == (mn, mx)
    assert got["counts"] == [int(v) for v in counts] and got["unseen"] == unseen and got["after"] == [int(v) for v in after]
