"""The anti-aliased splats through the reference-language host side: the component shim's `antialias` property and the addon's stats
field, driven by node (tests/js/test_antialias.js) on the 96x64 scene of test_antialias_gpu, against the ctypes path."""
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
def test_shim_schema_cpu():
    assert _addon() is not None
    r = subprocess.run([NODE, os.path.join(JS, "test_antialias.js"), "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "antialias cpu checks ok" in r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_shim_antialias_frames_equal_the_ctypes_path_gpu(tmp_path):
    from test_antialias_cpu import scene
    capi, synth = pkg("capi"), pkg("synth")
    assert _addon() is not None
    sc = scene()
    W, H = sc.W, sc.H
    # the frustum of test_blend_paths_gpu.camera (off = 0.5), as three.js matrices for the shim; identity camera and entity poses
    f, n = float(max(W, H, 64)), 0.005
    proj = synth.frustum(0.5 * f / f * n, (W + 0.5 * f) / f * n, (H + 0.5 * f) / f * n, 0.5 * f / f * n, n, 10000.0)
    eye = synth.compose((0.0, 0.0, 0.0))
    assert np.array_equal(capi.model_view_matrix(eye, eye), sc.cam["gs_mv"]) and np.array_equal(capi.projection_matrix(proj), sc.cam["gs_proj"])
    (tmp_path / "scene.splat").write_bytes(sc.rows.tobytes())
    (tmp_path / "pose.json").write_text(json.dumps({"width": W, "height": H, "proj": [float(v) for v in proj]}))
    r = subprocess.run([NODE, os.path.join(JS, "test_antialias.js"), "gpu", str(tmp_path / "scene.splat"), str(tmp_path / "out"),
                        str(tmp_path / "pose.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "antialias gpu checks ok" in r.stdout
    want = {}
    for aa in (0, 1):
        with capi.Context(0) as c:
            c.set_option(capi.OPT_ANTIALIAS, aa)
            c.push_splat(sc.rows)
            c.sort(sc.cam["view"])
            want[aa] = c.render(sc.params())
    assert not np.array_equal(want[0], want[1])
    for tag, aa in (("init_on", 1), ("live_off", 0), ("live_on", 1), ("live_off_again", 0)):
        got = np.frombuffer((tmp_path / ("out.%s.rgba" % tag)).read_bytes(), np.uint8).reshape(H, W, 4)
        assert np.array_equal(got, want[aa]), tag
