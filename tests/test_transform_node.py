"""gs_transform through the reference-language host side: the addon's transform and the component shim's method of the same name, driven
by node (tests/js/test_transform.js): the hit count is the ctypes binding's, and after each step the exported rows and .ply (which carries
the SH rows) hash to what the binding exports after the same step on the same cloud."""
import hashlib
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
def test_addon_and_shim_transform_cpu():
    assert _addon() is not None
    r = subprocess.run([NODE, os.path.join(JS, "test_transform.js"), "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "transform cpu checks ok" in r.stdout


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_transform_agrees_with_the_binding_gpu(tmp_path):
    synth, capi = pkg("synth"), pkg("capi")
    assert _addon() is not None
    n, sh_n, W, H = 4096, 3000, 256, 144
    rows = synth.make_splat_rows(n, seed=188).reshape(n, 32)
    g = np.random.Generator(np.random.PCG64(190))
    sh = (g.normal(size=(sh_n, 12)) * 0.3).astype(np.float32)
    select = [int(i) for i in range(2, n, 5)]
    rotation, scale, translation = [0.5, -0.25, 0.75, 0.125], 1.5, [0.25, -1.0, 2.5]      # (exact in f32: both sides hand over the same bits)
    with capi.Context(0) as c:
        c.push_splat(rows); c.push_sh(sh, 1)
        c.set_state_ids(select, capi.STATE_SELECTED, 0)
        hit = c.transform(capi.similarity(rotation, scale, translation), "selected")
        steps = {"moved": {"rows": _sha(c.export_splat()), "ply": _sha(c.export_ply("all", 1))}}
        assert c.transform(capi.similarity(translation=translation)) == n
        steps["shifted"] = {"rows": _sha(c.export_splat())}
    assert hit == len(select) and len({steps["moved"]["rows"], steps["shifted"]["rows"], _sha(rows)}) == 3
    scene = tmp_path / "scene.splat"
    scene.write_bytes(rows.tobytes())
    pose = tmp_path / "pose.json"
    pose.write_text(json.dumps({
        "width": W, "height": H, "proj": [float(v) for v in synth.perspective(80.0, W / H)],
        "camera": [float(v) for v in synth.compose((0.0, 1.6, 0.0))], "object": [float(v) for v in synth.compose((0.0, 1.5, -2.0), 15.0)]}))
    want = tmp_path / "expect.json"
    want.write_text(json.dumps({
        "select": select, "rotation": rotation, "scale": scale, "translation": translation, "hit": hit,
        "sh": [float(v) for v in sh.reshape(-1)], "steps": steps}))
    r = subprocess.run([NODE, os.path.join(JS, "test_transform.js"), "gpu", str(scene), str(pose), str(want)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "transform gpu checks ok" in r.stdout
