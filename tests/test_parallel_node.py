"""The parallel-projection cameras through the reference-language host side: the constant RENDER_PARALLEL of the addon and the component
shim, and frames drawn through the shim with it, driven by node (tests/js/test_parallel.js) on the 96x64 scene of test_parallel_gpu,
against the ctypes path."""
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
def test_constants_cpu():
    assert _addon() is not None
    r = subprocess.run([NODE, os.path.join(JS, "test_parallel.js"), "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "parallel cpu checks ok" in r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_shim_parallel_frames_equal_the_ctypes_path_gpu(tmp_path):
    from test_parallel_cpu import FAR, NEAR, PAR, VOLUMES, scene
    capi, synth = pkg("capi"), pkg("synth")
    assert _addon() is not None
    sc = scene()
    W, H = sc.W, sc.H
    a, b = VOLUMES[(W, H)]
    proj = capi.ortho_matrix(-a, a, b, -b, NEAR, FAR)                 # the OrthographicCamera's projectionMatrix, as three.js holds it
    obj = synth.compose((0.3, -0.2, -6.0), 25.0)
    eye = synth.compose((0.0, 0.0, 0.0))
    assert np.array_equal(capi.model_view_matrix(eye, obj), sc.cam["gs_mv"]) and np.array_equal(capi.projection_matrix(proj), sc.cam["gs_proj"])
    (tmp_path / "scene.splat").write_bytes(sc.rows.tobytes())
    (tmp_path / "pose.json").write_text(json.dumps({"width": W, "height": H, "proj": [float(v) for v in proj], "obj": [float(v) for v in obj],
                                                    "persp": [float(v) for v in synth.perspective(80.0, W / H)]}))
    r = subprocess.run([NODE, os.path.join(JS, "test_parallel.js"), "gpu", str(tmp_path / "scene.splat"), str(tmp_path / "out"),
                        str(tmp_path / "pose.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "parallel gpu checks ok" in r.stdout
    want = {}
    with capi.Context(0) as c:
        c.push_splat(sc.rows)
        c.sort(sc.cam["view"])
        for parallel in (True, False):
            want[parallel] = c.render(sc.params(parallel=parallel))
    assert not np.array_equal(want[True], want[False])
    for tag, parallel in (("parallel", True), ("plain", False), ("parallel_again", True)):
        got = np.frombuffer((tmp_path / ("out.%s.rgba" % tag)).read_bytes(), np.uint8).reshape(H, W, 4)
        assert np.array_equal(got, want[parallel]), tag
