"""The export through the reference-language host side: the addon's exportSplat / exportPly and the component shim's exportSplat({of}) /
exportPly({of, shDegree}), driven by node (tests/js/test_export.js): byte lengths and the first and last rows agree with the ctypes binding
for the same cloud, and the shim's of: 'visible' is the filter (HIDDEN, 0)."""
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
def test_addon_and_shim_export_cpu():
    assert _addon() is not None
    r = subprocess.run([NODE, os.path.join(JS, "test_export.js"), "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "export cpu checks ok" in r.stdout


def _expect(rows, ply):
    rows = np.asarray(rows, np.uint8).reshape(-1, 32)
    n = len(rows)
    body = np.asarray(ply, np.uint8)[len(ply) - 68 * n:].reshape(n, 68)                  # 17 f32 per vertex without f_rest
    return {"rows": n, "first": rows[0].tobytes().hex(), "last": rows[-1].tobytes().hex(), "plyBytes": int(len(ply)),
            "plyFirst": body[0].tobytes().hex(), "plyLast": body[-1].tobytes().hex()}


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_export_splat_and_ply_agree_with_the_binding_gpu(tmp_path):
    synth, capi = pkg("synth"), pkg("capi")
    assert _addon() is not None
    n, W, H = 4096, 256, 144
    rows = synth.make_splat_rows(n, seed=78)
    hide = [int(i) for i in range(3, n, 11)]
    with capi.Context(0) as c:
        c.push_splat(rows)
        expect = {"hide": hide, "all": _expect(c.export_splat("all"), c.export_ply("all", 0))}
        c.set_state_ids(hide, capi.STATE_HIDDEN, 0)
        expect["visible"] = _expect(c.export_splat((capi.STATE_HIDDEN, 0)), c.export_ply((capi.STATE_HIDDEN, 0), 3))
    assert expect["visible"]["rows"] == n - len(hide)
    scene = tmp_path / "scene.splat"
    scene.write_bytes(rows.tobytes())
    pose = tmp_path / "pose.json"
    pose.write_text(json.dumps({
        "width": W, "height": H, "proj": [float(v) for v in synth.perspective(80.0, W / H)],
        "camera": [float(v) for v in synth.compose((0.0, 1.6, 0.0))], "object": [float(v) for v in synth.compose((0.0, 1.5, -2.0), 15.0)]}))
    want = tmp_path / "expect.json"
    want.write_text(json.dumps(expect))
    r = subprocess.run([NODE, os.path.join(JS, "test_export.js"), "gpu", str(scene), str(pose), str(want)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "export gpu checks ok" in r.stdout
