"""The in-place changes through the reference-language host side: the addon's adjustColour / replaceSplat / replaceSh and the component shim's
methods of the same names, driven by node (tests/js/test_adjust.js): after each step the exported rows and .ply (which carries the SH rows)
hash to what the ctypes binding exports after the same step on the same cloud."""
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
def test_addon_and_shim_adjust_cpu():
    assert _addon() is not None
    r = subprocess.run([NODE, os.path.join(JS, "test_adjust.js"), "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "adjust cpu checks ok" in r.stdout


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_adjust_and_replace_agree_with_the_binding_gpu(tmp_path):
    synth, capi = pkg("synth"), pkg("capi")
    assert _addon() is not None
    n, sh_n, W, H = 4096, 3000, 256, 144
    rows = synth.make_splat_rows(n, seed=88).reshape(n, 32)
    other = synth.make_splat_rows(40, seed=89).reshape(40, 32)
    g = np.random.Generator(np.random.PCG64(90))
    sh = (g.normal(size=(sh_n, 12)) * 0.3).astype(np.float32)
    sh2 = (g.normal(size=(25, 12)) * 0.3).astype(np.float32)
    select = [int(i) for i in range(2, n, 5)]
    matrix, offset, a_s, a_o = [0.5, 0.25, 0.0, 0.0, 1.5, -0.25, 0.125, 0.0, 0.75], [8.0, -4.5, 30.0], 0.5, 12.0
    adj = capi.colour_adjust(matrix, offset, a_s, a_o)
    first, sh_first = 2040, 2990
    with capi.Context(0) as c:
        c.push_splat(rows); c.push_sh(sh, 1)
        c.set_state_ids(select, capi.STATE_SELECTED, 0)
        hit = c.adjust_colour(adj, "selected")
        steps = {"adjusted": {"rows": _sha(c.export_splat()), "ply": _sha(c.export_ply("all", 1))}}
        c.replace_splat(first, other)
        steps["replaced"] = {"rows": _sha(c.export_splat())}
        c.replace_sh(sh_first, sh2[:10], 1)
        steps["shReplaced"] = {"ply": _sha(c.export_ply("all", 1))}
    assert hit == len(select) and len({steps["adjusted"]["rows"], steps["replaced"]["rows"], _sha(rows)}) == 3
    assert steps["adjusted"]["ply"] != steps["shReplaced"]["ply"]
    scene = tmp_path / "scene.splat"
    scene.write_bytes(rows.tobytes())
    pose = tmp_path / "pose.json"
    pose.write_text(json.dumps({
        "width": W, "height": H, "proj": [float(v) for v in synth.perspective(80.0, W / H)],
        "camera": [float(v) for v in synth.compose((0.0, 1.6, 0.0))], "object": [float(v) for v in synth.compose((0.0, 1.5, -2.0), 15.0)]}))
    want = tmp_path / "expect.json"
    want.write_text(json.dumps({
        "select": select, "matrix": matrix, "offset": offset, "alphaScale": a_s, "alphaOffset": a_o, "hit": hit, "first": first,
        "other": other.tobytes().hex(), "shFirst": sh_first, "sh": [float(v) for v in sh.reshape(-1)], "sh2": [float(v) for v in sh2[:10].reshape(-1)],
        "steps": steps}))
    r = subprocess.run([NODE, os.path.join(JS, "test_adjust.js"), "gpu", str(scene), str(pose), str(want)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "adjust gpu checks ok" in r.stdout
