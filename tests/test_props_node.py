"""The per-splat properties through the reference-language host side: the addon's propRange / histogram / selectRange and the component
shim's histogram(prop, {bins, lo, hi, of}) and selectRange(prop, lo, hi, {hide, invert}), driven by node (tests/js/test_props.js): the
alpha histogram sums to count and has one bin per byte value; selectRange {hide} followed by deleteHidden lowers count by the
histogram's first 17 bins."""
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
def test_addon_and_shim_props_cpu():
    assert _addon() is not None
    r = subprocess.run([NODE, os.path.join(JS, "test_props.js"), "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "props cpu checks ok" in r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_histogram_select_range_and_delete_hidden_gpu(tmp_path):
    synth = pkg("synth")
    assert _addon() is not None
    n, W, H = 4096, 256, 144
    rows = synth.make_splat_rows(n, seed=77)
    scene = tmp_path / "scene.splat"
    scene.write_bytes(rows.tobytes())
    pose = tmp_path / "pose.json"
    pose.write_text(json.dumps({
        "width": W, "height": H, "proj": [float(v) for v in synth.perspective(80.0, W / H)],
        "camera": [float(v) for v in synth.compose((0.0, 1.6, 0.0))], "object": [float(v) for v in synth.compose((0.0, 1.5, -2.0), 15.0)]}))
    r = subprocess.run([NODE, os.path.join(JS, "test_props.js"), "gpu", str(scene), str(pose)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "props gpu checks ok" in r.stdout
