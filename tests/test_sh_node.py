"""View-dependent colour through the reference-language host side: the component shim's `shDegree` property and the addon's
plySh / pushSh, driven by node (tests/js/test_sh.js), against the ctypes path of test_sh_gpu."""
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
def test_shim_schema_and_addon_surface_cpu():
    assert _addon() is not None
    r = subprocess.run([NODE, os.path.join(JS, "test_sh.js"), "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sh cpu checks ok" in r.stdout


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_shim_sh_degree_frame_equals_the_ctypes_path_gpu(tmp_path):
    from test_sh_gpu import Scene, draw, plain_context, sh_context
    capi, synth = pkg("capi"), pkg("synth")
    assert _addon() is not None
    sc = Scene(20000, 4600)
    ply = tmp_path / "scene.ply"
    ply.write_bytes(sc.ply)
    w, h, yaw = 320, 180, 35.0
    r = subprocess.run([NODE, os.path.join(JS, "test_sh.js"), "gpu", str(ply), str(tmp_path / "frame"), str(w), str(h), str(yaw)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sh gpu checks ok" in r.stdout
    got_sh = np.frombuffer((tmp_path / "frame.sh3.rgba").read_bytes(), np.uint8).reshape(h, w, 4)
    got_plain = np.frombuffer((tmp_path / "frame.plain.rgba").read_bytes(), np.uint8).reshape(h, w, 4)
    cam = synth.index_html_camera(w, h, yaw, capi=capi)
    with sh_context(sc, 3, "load_ply") as c:                                  # shDegree: 3 == the ctypes path of the substitution test
        assert np.array_equal(got_sh, draw(c, cam))
    with plain_context(sc.substituted(3, cam["gs_mv"])) as p:
        assert np.array_equal(got_sh, draw(p, cam))
    with plain_context(sc.rows) as p:                                          # shDegree absent == today's frame
        assert np.array_equal(got_plain, draw(p, cam))
    assert not np.array_equal(got_sh, got_plain)
