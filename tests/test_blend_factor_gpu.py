"""GPU tier: the blend's coverage factor (csrc/gs_render.hip, GS_BLEND_FACTOR) changes no pixel.

Plain frames take the coverage test as a factor, since GS_BLEND_FACTOR 2 one packed fma per pixel pair, w = clamp(q * -1e30 + c).  Here
every frame of the library as built is compared, bit for bit, with the same frame from a variant of the library compiled with
-DGS_BLEND_FACTOR=0: the compare / select step that counting renders, scene depth and surface frames keep.  The module's fixture builds
the variant with build.py's flags into a temporary directory (all sources, in parallel: about a minute, once per run of this file); each
library then draws the frames in a fresh child process of its own -- this file run as a script, the variant named by GS_SPLAT_LIB -- and
writes them to an .npz the tests compare.

Frames: the 320x180 synthetic cloud of tests/test_blend_paths_gpu.py at its four poses; paths walk, lists and subtile; the default
share (GS_OPT_NEAR_PERMILLE 0) and 400 (two rounds); GS_OPT_FRAME_BATCH 1 (synchronous) and 2 (the four frames queued, then one sync).
Strips, synchronous, every path and both shares: tiles are anchored at a strip's left edge, so the 64-pixel strip (200, 264) is four whole
tiles; (100, 150) ends 2 pixels into a group of four and 6 pixels into its last tile (lanes whose four pixels are all outside, qm = -1);
(257, 320) ends on the frame's edge 3 pixels into a group of four (lanes with pixels of both kinds).  The frame's last tile row holds
rows 176..191 of 180: lanes outside in every frame.  A counting render (compare form in both libraries) reports its fragment count."""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATHS = ("walk", "lists", "subtile")
SHARES = (0, 400)
STRIPS = ((200, 264), (100, 150), (257, 320))
W, H = 320, 180

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- the child: draw everything with the library the environment names

def _draw_all(out_path):
    from conftest import pkg
    from test_gpu_parity import assert_path, force_path
    capi, synth = pkg("capi"), pkg("synth")
    rows = synth.make_splat_rows(20000, seed=4242)
    cams = [synth.index_html_camera(W, H, 50.0 * k, capi=capi) for k in range(4)]

    def params(cam, x0=0, x1=None, flags=0):
        return capi.make_params(cam["gs_mv"], cam["gs_proj"], W, H, x0=x0, x1=x1, focal_=cam["focal"], flags=flags)

    res = {}
    for path in PATHS:
        for share in SHARES:
            tag = "%s_%d" % (path, share)
            with capi.Context(0) as c:
                force_path(c, path, share)
                c.push_splat(rows)
                for k, cam in enumerate(cams):
                    c.sort(cam["view"])
                    res["%s_b1_pose%d" % (tag, k)] = c.render(params(cam))
                    assert_path(c, path, tag)
                    if k == 0:
                        for x0, x1 in STRIPS:
                            res["%s_strip_%d_%d" % (tag, x0, x1)] = c.render(params(cam, x0, x1))
                            assert_path(c, path, (tag, x0, x1))
                c.set_option(capi.OPT_FRAME_BATCH, 2)
                bufs = [capi.host_frame(H, W) for _ in cams]
                for (b, _), cam in zip(bufs, cams):
                    c.sort(cam["view"], want_indices=False)
                    c.render_into(params(cam, flags=capi.RENDER_ASYNC), b)
                c.sync()
                assert_path(c, path, tag + "_paired")
                for k, (b, o) in enumerate(bufs):
                    res["%s_b2_pose%d" % (tag, k)] = b.copy()
                    o.free()
    for path in ("lists", "subtile"):
        with capi.Context(0) as c:
            force_path(c, path)
            c.push_splat(rows)
            c.sort(cams[0]["view"])
            c.render(params(cams[0], flags=capi.RENDER_COUNT_FRAGS))
            res["count_%s" % path] = np.array([c.stats()["n_frags"]], np.uint64)
    np.savez(out_path, **res)
    print("drew %d results with %s" % (len(res), os.environ.get("GS_SPLAT_LIB") or "the library as built"))


if __name__ == "__main__":
    _draw_all(sys.argv[1])
    sys.exit(0)


# ---------------------------------------------------------------- the parent: build the variant, run both children, compare

def _build_variant(out_dir):
    from conftest import pkg
    build = pkg("build")
    flags = build.HIP_FLAGS + ["-DGS_BLEND_FACTOR=0"]

    def compile_one(src):
        obj = os.path.join(out_dir, os.path.splitext(os.path.basename(src))[0] + ".o")
        subprocess.run([build.HIPCC] + flags + ["-x", "hip", "-c", src, "-o", obj], check=True, capture_output=True, timeout=900)
        return obj

    # (the longest source first: it bounds the build)
    srcs = sorted(build.sources(), key=os.path.getsize, reverse=True)
    with ThreadPoolExecutor(max_workers=min(16, len(srcs))) as pool:
        objs = list(pool.map(compile_one, srcs))
    lib = os.path.join(out_dir, "libgs_variant_compare.so")
    subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs, check=True, capture_output=True, timeout=300)
    return lib


def _child(lib, out_path):
    e = dict(os.environ)
    e.pop("GS_SPLAT_LIB", None)
    if lib:
        e["GS_SPLAT_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), out_path], capture_output=True, text=True, timeout=300, env=e, cwd=ROOT)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    print(p.stdout.strip().splitlines()[-1])
    with np.load(out_path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    from conftest import pkg
    build = pkg("build")
    if not (os.path.exists(build.HIPCC) or shutil.which(build.HIPCC)):
        pytest.skip("no hipcc: the compare / select variant cannot be built")
    d = str(tmp_path_factory.mktemp("blend_factor"))
    lib = _build_variant(d)
    assert open(lib, "rb").read() != open(build.LIB, "rb").read(), "the variant is the library as built"
    return _child(None, os.path.join(d, "factor.npz")), _child(lib, os.path.join(d, "compare.npz"))


def _frames(both, pick):
    got, want = both
    keys = sorted(k for k in want if pick(k))
    assert keys and sorted(k for k in got if pick(k)) == keys
    return [(k, got[k], want[k]) for k in keys]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("share", SHARES)
@pytest.mark.parametrize("batch", (1, 2))
def test_frames_equal_the_compare_form_bit_for_bit(both, path, share, batch):
    fr = _frames(both, lambda k: k.startswith("%s_%d_b%d_" % (path, share, batch)))
    assert len(fr) == 4
    for k, a, b in fr:
        assert a.shape == (H, W, 4) and a.any(), k
        d = int(np.abs(a.astype(int) - b.astype(int)).max())
        print(k, "max |dRGBA8| =", d)
        assert np.array_equal(a, b), (k, d)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("share", SHARES)
def test_strips_with_lanes_outside_equal_the_compare_form(both, path, share):
    fr = _frames(both, lambda k: k.startswith("%s_%d_strip_" % (path, share)))
    assert len(fr) == len(STRIPS)
    for k, a, b in fr:
        x0, x1 = (int(v) for v in k.split("_")[-2:])
        assert a.shape == (H, x1 - x0, 4) and a.any(), k
        assert np.array_equal(a, b), (k, int(np.abs(a.astype(int) - b.astype(int)).max()))


def test_counting_render_reports_the_same_fragments(both):
    fr = _frames(both, lambda k: k.startswith("count_"))
    assert len(fr) == 2
    for k, a, b in fr:
        print(k, int(a[0]), int(b[0]))
        assert int(a[0]) == int(b[0]) and int(a[0]) > 0, (k, a, b)
