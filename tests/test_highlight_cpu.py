"""CPU tier of the highlighted selection (GS_OPT_HIGHLIGHT) and of mask-image selection: gs_highlight_word -- the kernel's own function,
compiled for the host -- against a numpy mirror of the integer rule the header states, gs_mask_polygon against a numpy mirror of its f64
rule, the refusals of the new entry points that need no GPU, and the constants of the ctypes binding against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg

capi = pkg("capi")

NEW = ["gs_select_mask", "gs_multi_select_mask", "gs_mask_polygon", "gs_highlight_info", "gs_highlight_word"]


def _header():
    with open(os.path.join(ROOT, "include", "gs_splat.h")) as f:
        return f.read()


def _define(name):
    m = re.search(r"^#define\s+%s\s+(\d+)u?\b" % name, _header(), re.M)
    assert m, name
    return int(m.group(1))


def highlight_mirror(word, value):
    """c' = (c * (255 - W) + h * W + 127) / 255 per colour byte, unsigned, truncating; the alpha byte stays; W = 0: unchanged"""
    word = np.asarray(word, np.uint32)
    w = np.uint32(value >> 24)
    if w == 0:
        return word.copy()
    out = word & np.uint32(0xFF000000)
    for s in (0, 8, 16):
        c = (word >> np.uint32(s)) & np.uint32(255)
        h = np.uint32((value >> s) & 255)
        out = out | (((c * (np.uint32(255) - w) + h * w + np.uint32(127)) // np.uint32(255)) << np.uint32(s))
    return out.astype(np.uint32)


def polygon_mirror(points, W, H):
    """the header's rule, vectorised over the pixel centres, every operation in f64 and in the stated order"""
    pts = np.asarray(points, np.float32).reshape(-1, 2).astype(np.float64)
    mask = np.zeros((H, W), np.uint8)
    if len(pts) < 3:
        return mask
    px = (np.arange(W, dtype=np.float64) + 0.5)[None, :]
    py = (np.arange(H, dtype=np.float64) + 0.5)[:, None]
    count = np.zeros((H, W), np.int64)
    with np.errstate(all="ignore"):
        for k in range(len(pts)):
            (xa, ya), (xb, yb) = pts[k], pts[(k + 1) % len(pts)]
            cross = (ya <= py) != (yb <= py)
            xc = xa + (py - ya) * (xb - xa) / (yb - ya)
            count += cross & (px < xc)
    return (count & 1).astype(np.uint8)


# ---------------------------------------------------------------- binding and header

def test_symbols_are_declared_exported_and_bound():
    hdr = _header()
    L = capi.load()
    for name in NEW:
        assert re.search(r"GS_API\s+int\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in capi.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name
    for name in ("select_mask", "highlight_info"):
        assert hasattr(capi.Context, name), name
    assert hasattr(capi.Multi, "select_mask")


def test_constants_agree_with_the_header():
    assert capi.OPT_HIGHLIGHT == _define("GS_OPT_HIGHLIGHT") == 23
    assert capi.STATE_SELECTED == _define("GS_STATE_SELECTED") == 2
    assert capi.SELECT_INVERT == _define("GS_SELECT_INVERT") == 1
    assert capi.highlight_option((1, 2, 3), 4) == 0x04030201
    out = re.search(r"Out of scope:([^*]*?in-place edits.*?)\*/", _header(), re.S).group(1)
    assert "highlight" not in out and "lasso" not in out and "undo" in out


def test_stats_keep_their_last_fields():
    """the feature reports through gs_highlight_info: gs_stats is what it was"""
    names = [n for n, _ in capi.Stats._fields_]
    assert names[-5:] == ["n_hidden", "surface", "antialias", "seg_count", "n_runs"]
    assert not any("highlight" in n for n in names)


def test_null_and_bad_arguments_are_refused_without_a_gpu():
    L = capi.load()
    assert L.gs_select_mask(None, None, None, 0, None, 0, 0, 0, None) == capi.E_BADARG
    assert L.gs_multi_select_mask(None, None, None, 0, None, 0, 0, 0, None) == capi.E_BADARG
    assert L.gs_highlight_info(None, None, None) == capi.E_BADARG
    assert L.gs_highlight_word(0, 0, None) == capi.E_BADARG
    xy = np.array([0, 0, 4, 0, 0, 4], np.float32)
    m = np.zeros(64, np.uint8)
    ok = lambda *a: L.gs_mask_polygon(*a)
    assert ok(xy.ctypes.data, 3, 8, 8, m.ctypes.data, 0) == capi.GS_OK
    assert ok(None, 3, 8, 8, m.ctypes.data, 0) == capi.E_BADARG
    assert ok(xy.ctypes.data, 3, 8, 8, None, 0) == capi.E_BADARG
    assert ok(xy.ctypes.data, 3, 0, 8, m.ctypes.data, 0) == capi.E_BADARG
    assert ok(xy.ctypes.data, 3, 8, -1, m.ctypes.data, 0) == capi.E_BADARG
    assert ok(xy.ctypes.data, 3, 8, 8, m.ctypes.data, 7) == capi.E_BADARG
    assert ok(xy.ctypes.data, 3, 8, 8, m.ctypes.data, 8) == capi.GS_OK


# ---------------------------------------------------------------- gs_highlight_word

@pytest.mark.parametrize("w", [1, 127, 128, 254, 255])
def test_highlight_word_equals_the_integer_rule(w):
    """all 256 x 256 (c, h) pairs, once per byte lane: word = c in the lane (other lanes and alpha carry a pattern that must survive or
    follow the rule by itself), highlight = h in the lane"""
    c, h = np.meshgrid(np.arange(256, dtype=np.uint32), np.arange(256, dtype=np.uint32), indexing="ij")
    c, h = c.reshape(-1), h.reshape(-1)
    lane = 8 * (int(w) % 3)                                              # (each weight exercises one lane in full: 65536 calls per case)
    others = np.uint32(0xA55A3CC3) & ~np.uint32(0xFF << lane)
    word = (c << np.uint32(lane)) | others
    got = np.empty(c.size, np.uint32)
    f, out = capi.load().gs_highlight_word, C.c_uint32(0)
    for hv in range(256):
        value = (w << 24) | (hv << lane) | (0x00112233 & ~(0xFF << lane))
        sel = np.flatnonzero(h == hv)
        for i in sel:
            assert f(int(word[i]), value, C.byref(out)) == capi.GS_OK
            got[i] = out.value
        want = highlight_mirror(word[sel], value)
        assert np.array_equal(got[sel], want), (w, hv)
        assert np.array_equal(got[sel] >> 24, word[sel] >> 24)           # the alpha byte
        if w == 255:
            assert np.array_equal(got[sel] & 0xFFFFFF, np.full(sel.size, value & 0xFFFFFF, np.uint32))


def test_highlight_word_weight_zero_and_full():
    words = np.array([0, 0xFFFFFFFF, 0x80402010, 0x01FE7F80], np.uint32)
    for colour in (0, 0x00FFFFFF, 0x00123456):
        assert np.array_equal(capi.highlight_word(words, colour), words)                               # W = 0: off, whatever the colour
        full = capi.highlight_word(words, colour | 0xFF000000)
        assert np.array_equal(full, (words & 0xFF000000) | np.uint32(colour))                          # W = 255: exactly h, alpha kept
    assert capi.highlight_word(np.uint32(0x80402010), 0x80FF00FF) == highlight_mirror(np.uint32(0x80402010), 0x80FF00FF)


# ---------------------------------------------------------------- gs_mask_polygon

POLYGONS = {
    "triangle": [(3.2, 2.1), (30.7, 9.4), (11.0, 20.9)],
    "concave": [(2, 2), (34, 3), (33, 21), (18, 8), (4, 20)],
    "self_intersecting": [(5, 4), (30, 19), (30, 4), (5, 19)],                                      # a bow tie, and ...
    "star": [(18, 1), (25, 22), (3, 8), (34, 8), (11, 22)],                                         # ... a pentagram: its centre is even
    "on_centres": [(4.5, 3.5), (20.5, 3.5), (20.5, 15.5), (12.5, 9.5), (4.5, 15.5)],
    "partly_outside": [(-20.0, -7.5), (50.3, 5.0), (18.0, 40.0)],
    "degenerate_edges": [(6, 6), (6, 6), (20, 6), (20, 6.0), (20, 18), (6, 18)],
}


@pytest.mark.parametrize("size", [(37, 23), (320, 180)])
@pytest.mark.parametrize("name", sorted(POLYGONS))
def test_mask_polygon_equals_the_f64_rule(name, size):
    W, H = size
    pts = np.array(POLYGONS[name], np.float32) * np.float32(W / 37.0 if W != 37 else 1.0)
    if name == "on_centres":
        pts = np.floor(pts) + np.float32(0.5)
        assert ((pts - 0.5) == np.floor(pts - 0.5)).all()
    got = capi.mask_polygon(pts, W, H)
    want = polygon_mirror(pts, W, H)
    assert got.shape == (H, W) and set(np.unique(got)) <= {0, 1}
    assert 0 < want.sum() < W * H, "the case proves nothing"
    assert np.array_equal(got, want), (name, size, int((got != want).sum()))


def test_mask_polygon_even_odd_centre_of_the_star_is_outside():
    pts = np.array(POLYGONS["star"], np.float32)
    got = capi.mask_polygon(pts, 37, 23)
    assert got[11, 18] == 0 and got[4, 18] == 1                          # the pentagon in the middle is covered twice; a tip once


@pytest.mark.parametrize("npoints", [0, 2])
def test_mask_polygon_fewer_than_three_points_clears(npoints):
    out = np.full((23, 37), 9, np.uint8)
    pts = np.array([(1, 1), (30, 20)], np.float32)[:npoints]
    assert capi.mask_polygon(pts, 37, 23, out=out) is out and not out.any()


@pytest.mark.parametrize("size", [(37, 23), (320, 180)])
def test_mask_polygon_stride_leaves_the_padding(size):
    W, H = size
    pts = np.array(POLYGONS["concave"], np.float32) * np.float32(W / 37.0)
    out = np.full((H, W + 5), 0xEE, np.uint8)
    capi.mask_polygon(pts, W, H, out=out)
    assert (out[:, W:] == 0xEE).all()
    assert np.array_equal(out[:, :W], polygon_mirror(pts, W, H))
