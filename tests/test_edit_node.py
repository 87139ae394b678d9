"""The editing calls through the reference-language host side: the addon's setState ... compact and the component shim's hideSplats,
showAll, selectBox, selectRect and deleteHidden, driven by node (tests/js/test_edit.js): hide by the pick(x, y) id and the picked pixel
changes; selectBox {invert, hide} draws the frame of the same box as cutoutEntity; deleteHidden lowers count."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT, pkg

JS = os.path.join(ROOT, "tests", "js")
NODE = shutil.which("node")


def _addon():
    b = pkg("build")
    b.build_lib()
    return b.build_addon()


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_and_shim_edit_cpu():
    assert _addon() is not None
    r = subprocess.run([NODE, os.path.join(JS, "test_edit.js"), "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "edit cpu checks ok" in r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_hide_by_pick_select_box_and_delete_hidden_gpu(tmp_path):
    synth = pkg("synth")
    assert _addon() is not None
    n, W, H = 4096, 256, 144
    rows = synth.make_splat_rows(n, seed=77)
    scene = tmp_path / "scene.splat"
    scene.write_bytes(rows.tobytes())
    pose = tmp_path / "pose.json"
    pose.write_text(json.dumps({
        "width": W, "height": H, "proj": [float(v) for v in synth.perspective(80.0, W / H)],
        "camera": [float(v) for v in synth.compose((0.0, 1.6, 0.0))], "object": [float(v) for v in synth.compose((0.0, 1.5, -2.0), 15.0)],
        "box": [float(v) for v in synth.compose((0.0, 1.5, -2.0), 0.0, (4.0, 3.0, 4.0))]}))
    r = subprocess.run([NODE, os.path.join(JS, "test_edit.js"), "gpu", str(scene), str(pose)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "edit gpu checks ok" in r.stdout
