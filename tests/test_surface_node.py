"""The surface output through the reference-language host side: the addon's renderSurface / pick and the component shim's pick(x, y),
driven by node (tests/js/test_surface.js) on the batch-edge scene of test_surface_gpu (k = 65), against the ctypes path."""
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
def test_addon_and_shim_surface_cpu():
    assert _addon() is not None
    r = subprocess.run([NODE, os.path.join(JS, "test_surface.js"), "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "surface cpu checks ok" in r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_render_surface_and_pick_equal_the_ctypes_path_gpu(tmp_path):
    from test_surface_cpu import NONE, batch_scene
    capi, synth = pkg("capi"), pkg("synth")
    assert _addon() is not None
    k = 65
    sc = batch_scene(k)
    W, H = sc.W, sc.H
    # the frustum of test_blend_paths_gpu.camera (off = 0.5), as three.js matrices for the shim; identity camera and entity poses
    f, n = float(max(W, H, 64)), 0.005
    proj = synth.frustum(0.5 * f / f * n, (W + 0.5 * f) / f * n, (H + 0.5 * f) / f * n, 0.5 * f / f * n, n, 10000.0)
    eye = synth.compose((0.0, 0.0, 0.0))
    assert np.array_equal(capi.model_view_matrix(eye, eye), sc.cam["gs_mv"]) and np.array_equal(capi.projection_matrix(proj), sc.cam["gs_proj"])
    points = [[24, 24], [20, 27], [16, 16], [0, 0], [63, 47], [31, 31], [60, 5], [27, 20]]
    scene = tmp_path / "scene.splat"
    scene.write_bytes(sc.rows.tobytes())
    pose = tmp_path / "pose.json"
    pose.write_text(json.dumps({"width": W, "height": H, "proj": [float(v) for v in proj], "points": points, "centre": [24, 24],
                                "splat_centre": [24.0, 24.0], "translate": [3.0, -1.5, 2.0]}))
    r = subprocess.run([NODE, os.path.join(JS, "test_surface.js"), "gpu", str(scene), str(tmp_path / "out"), str(pose)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "surface gpu checks ok" in r.stdout
    with capi.Context(0) as c:
        c.push_splat(sc.rows)
        c.sort(sc.cam["view"])
        rgba, sid, dep, alp = c.render_surface(sc.params())
        hits = c.pick(sc.params(), points)
    for tag, want in (("rgba", rgba), ("id", sid), ("depth", dep), ("alpha", alp)):
        got = np.frombuffer((tmp_path / ("out." + tag)).read_bytes(), want.dtype).reshape(want.shape)
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), tag
    assert (sid[20:28, 20:28] == k - 1).all()
    js = json.loads((tmp_path / "out.hits.json").read_text())
    pos = sc.rows.reshape(-1, 32)[:, 0:12].copy().view("<f4").reshape(-1, 3)
    for (x, y), h, j in zip(points, hits, js["hits"]):
        if h["id"] == NONE:
            assert j["index"] == -1 and j["position"] is None
        else:
            assert j["index"] == int(h["id"]) and [np.float32(v) for v in j["position"].values()] == list(pos[h["id"]])
        assert np.float32(j["depth"]) == h["depth"] and np.float32(j["alpha"]) == h["alpha"]
    assert js["base"]["index"] == k - 1 and js["moved"]["index"] == k - 1
    p = pos[k - 1]
    assert np.allclose(js["base"]["worldPosition"], [p[0], -p[1], -p[2]], atol=0, rtol=0)
    assert np.allclose(js["moved"]["worldPosition"], [p[0] + 3.0, -p[1] - 1.5, -p[2] + 2.0], atol=1e-5)
