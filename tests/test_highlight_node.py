"""The highlighted selection and lasso / mask selection through the reference-language host side: the addon's selectMask, maskPolygon and
highlightInfo and the component shim's highlightSelected, selectMask and selectLasso, driven by node (tests/js/test_highlight.js) on the
4096-splat scene of test_edit_gpu at 256 x 144, against the ctypes path: the frames are equal, the counts are the ctypes calls' counts."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pkg

JS = os.path.join(ROOT, "tests", "js")
NODE = shutil.which("node")
LASSO = [(30.5, 20.0), (220.0, 12.5), (236.0, 120.0), (128.0, 60.0), (44.0, 131.0)]
COLOR, WEIGHT = (255, 32, 200), 160


def _addon():
    b = pkg("build")
    b.build_lib()
    return b.build_addon()


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_and_shim_highlight_cpu():
    assert _addon() is not None
    r = subprocess.run([NODE, os.path.join(JS, "test_highlight.js"), "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "highlight cpu checks ok" in r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_highlight_selected_and_select_lasso_equal_the_ctypes_path_gpu(tmp_path):
    capi, synth = pkg("capi"), pkg("synth")
    assert _addon() is not None
    n, W, H = 4096, 256, 144
    rows = synth.make_splat_rows(n, seed=77)
    (tmp_path / "scene.splat").write_bytes(rows.tobytes())
    (tmp_path / "pose.json").write_text(json.dumps({
        "width": W, "height": H, "proj": [float(v) for v in synth.perspective(80.0, W / H)],
        "camera": [float(v) for v in synth.compose((0.0, 1.6, 0.0))], "object": [float(v) for v in synth.compose((0.0, 1.5, -2.0), 15.0)],
        "lasso": [list(p) for p in LASSO], "color": list(COLOR), "weight": WEIGHT}))
    r = subprocess.run([NODE, os.path.join(JS, "test_highlight.js"), "gpu", str(tmp_path / "scene.splat"), str(tmp_path / "out"),
                        str(tmp_path / "pose.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "highlight gpu checks ok" in r.stdout
    counts = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    cam = synth.index_html_camera(W, H, yaw_deg=15.0, capi=capi)                  # the pose above
    p = capi.make_params(cam["gs_mv"], cam["gs_proj"], W, H, focal_=cam["focal"])
    mask = capi.mask_polygon(LASSO, W, H)
    with capi.Context(0) as c:
        c.push_splat(rows)
        c.sort(cam["view"], want_indices=False)
        plain = c.render(p)
        depth = c.render_surface(p)[2]
        visible = c.select_mask(p, mask, depth, set_bits=0)
        c.sort(cam["view"], want_indices=False)
        assert c.select_mask(p, np.ones((H, W), np.uint8), set_bits=0) == counts["all"]
        c.sort(cam["view"], want_indices=False)
        assert c.select_mask(p, mask, set_bits=0, flags=capi.SELECT_INVERT) == counts["inverted"]
        c.sort(cam["view"], want_indices=False)
        hit = c.select_mask(p, mask, set_bits=capi.STATE_SELECTED)
        c.set_option(capi.OPT_HIGHLIGHT, capi.highlight_option(COLOR, WEIGHT))
        c.sort(cam["view"], want_indices=False)
        lit = c.render(p)
        assert c.highlight_info()[1] == 1
    assert (counts["hit"], counts["visible"]) == (hit, visible) and 0 < visible < hit
    got = {tag: np.frombuffer((tmp_path / ("out.%s.rgba" % tag)).read_bytes(), np.uint8).reshape(H, W, 4) for tag in ("plain", "lit")}
    assert np.array_equal(got["plain"], plain) and np.array_equal(got["lit"], lit) and not np.array_equal(lit, plain)
