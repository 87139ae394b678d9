"""The compressed .ply through the reference-language host side: the addon's cplyInfo / loadCply / exportCply and the component shim, driven
by node (tests/js/test_cply.js).  The shim sends a .ply whose header cplyInfo accepts to loadCply (an INRIA file keeps its path), and
exportCply returns the host writer's bytes for the same cloud."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_case, pkg
from test_cply_cpu import make_rows

JS = os.path.join(ROOT, "tests", "js")
NODE = shutil.which("node")


def _addon():
    b = pkg("build")
    b.build_lib()
    return b.build_addon()


def _file(capi, n, degree, seed):
    rows, wide = make_rows(n, seed)
    sh = (np.random.Generator(np.random.PCG64(seed)).normal(size=(n, 3 * (degree + 1) ** 2)) * 0.4).astype(np.float32)
    return bytes(capi.splat_to_cply(rows, wide, sh, degree, morton=True))


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_sniffs_compressed_files_cpu(tmp_path):
    capi = pkg("capi")
    assert _addon() is not None
    inria, comp = tmp_path / "inria.ply", tmp_path / "compressed.ply"
    inria.write_bytes(bytes(load_case("ply_inria64")["ply"]))
    comp.write_bytes(_file(capi, 300, 1, seed=8))
    r = subprocess.run([NODE, os.path.join(JS, "test_cply.js"), "cpu", str(inria), str(comp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cply cpu checks ok" in r.stdout


def _host(capi, c, of, sh_degree, morton):
    """the host writer fed with the export of the same filter"""
    rows, wide = c.export_splat(of, want_wide=True)
    sh, stored = c.export_sh(of)
    D = min(sh_degree, stored)
    cut = np.ascontiguousarray(sh.reshape(-1, 3, (stored + 1) ** 2)[:, :, :(D + 1) ** 2]).reshape(len(sh), -1) if len(sh) else None
    return bytes(capi.splat_to_cply(rows, wide, cut, D, morton=morton)).hex()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_shim_loads_and_exports_compressed_files_gpu(tmp_path):
    synth, capi = pkg("synth"), pkg("capi")
    assert _addon() is not None
    n, W, H = 700, 256, 144
    data = _file(capi, n, 1, seed=21)
    hide = [int(i) for i in range(3, n, 11)]
    with capi.Context(0) as c:
        c.set_option(capi.OPT_SH_DEGREE, 1)
        c.load_cply(data)
        assert c.count() == n and c.sh_count() == (n, 1)
        expect = {"splats": n, "shDegree": 1, "hide": hide, "all": _host(capi, c, "all", 3, True), "plain": _host(capi, c, "all", 0, False)}
        c.set_state_ids(hide, capi.STATE_HIDDEN, 0)
        expect["visible"] = _host(capi, c, "visible", 1, True)
    scene = tmp_path / "scene.ply"
    scene.write_bytes(data)
    pose = tmp_path / "pose.json"
    pose.write_text(json.dumps({
        "width": W, "height": H, "proj": [float(v) for v in synth.perspective(80.0, W / H)],
        "camera": [float(v) for v in synth.compose((0.0, 1.6, 0.0))], "object": [float(v) for v in synth.compose((0.0, 1.5, -2.0), 15.0)]}))
    want = tmp_path / "expect.json"
    want.write_text(json.dumps(expect))
    r = subprocess.run([NODE, os.path.join(JS, "test_cply.js"), "gpu", str(scene), str(pose), str(want)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cply gpu checks ok" in r.stdout
