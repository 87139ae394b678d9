"""CPU tier of the surface output (include/gs_splat.h: gs_render_surface, gs_pick): the numpy MIRROR of the definition, the scenes the
GPU tier (test_surface_gpu.py) draws, and the condition under which those scenes may be relied on.

The mirror takes a pixel's fragments nearest first -- the splats in reversed gs_sort order, projected by oracle.project, kept where
q <= 4 and, with a scene depth, where the window depth passes LEQUAL -- and runs T_k = T_{k-1} - alpha * (e^-q * T_{k-1}) in f64.  The
surface is the first k with T_{k-1} >= 0.5 > T_k.  The kernel runs the same recurrence in f32 with v_exp_f32, so a pixel is UNDECIDED,
and left out of the id / depth comparison, where rounding could move the answer: some |T_k - 0.5| < 1e-3, or a fragment with
|q - 4| < 1e-3 or a window depth within 1e-6 of the scene's at or before the crossing.  At most 3 % of a strip's pixels may be
undecided in any scene a test uses: asserted here, on the CPU, for every scene the GPU tier draws (those it compares with the mirror,
and the 64x48 / 100x70 clouds of its colour and strip tests).  The strict rule at T == 0.5 exactly is not pinned by a scene: byte alphas
give none whose f32 transmittance lands on it, and the rule above would call such a pixel undecided."""
import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_blend_paths_gpu import Scene, camera, splat

capi = pkg("capi")
synth = pkg("synth")

NONE = 0xFFFFFFFF
UNDECIDED_CAP = 0.03
BATCH_EDGES = (1, 2, 63, 64, 65, 128, 129)             # k: the crossing is the k-th entry of its tile's list
TILE = (1, 1)                                           # the tile under test (tile column, tile row) of a 64x48 frame
INNER = (slice(20, 28), slice(20, 28))                  # its inner 8x8 pixels (rows, columns)
N_BEHIND = 5


def window_depth(scene, i):
    """float32(zndc * 0.5 + 0.5) of row i: what k_project writes to zwin"""
    c = scene.cam
    p = oracle.project(scene.cs, scene.cc, int(i), c["gs_mv"].astype(np.float32), c["gs_proj"].astype(np.float32), c["focal"], scene.W, scene.H)
    return np.float32(np.float32(p.zndc) * np.float32(0.5) + np.float32(0.5))


def mirror(scene, idx, x0=0, x1=None, scene_depth=None):
    """-> id u32 [H, sw], depth f32, alpha f64, undecided bool, T after every fragment's minimum over the pixels that have not crossed
    (per pixel: the smallest T seen while no surface was found; 1 where nothing covered it)."""
    W, H, c = scene.W, scene.H, scene.cam
    x1 = W if x1 is None else x1
    sw = x1 - x0
    mv, pr = c["gs_mv"].astype(np.float32), c["gs_proj"].astype(np.float32)
    fx = (np.arange(x0, x1, dtype=np.float32) + np.float32(0.5))[None, :]
    fy = (np.float32(H - 1) - np.arange(H, dtype=np.float32) + np.float32(0.5))[:, None]      # GL window y of image row r
    T = np.ones((H, sw))
    sid = np.full((H, sw), NONE, np.uint32)
    dep = np.ones((H, sw), np.float32)
    found = np.zeros((H, sw), bool)
    und = np.zeros((H, sw), bool)
    sd = None if scene_depth is None else np.asarray(scene_depth, np.float32)[:, x0:x1]
    for i in np.asarray(idx)[::-1]:
        p = oracle.project(scene.cs, scene.cc, int(i), mv, pr, c["focal"], W, H)
        if not p.visible:
            continue
        zw = np.float32(np.float32(p.zndc) * np.float32(0.5) + np.float32(0.5))
        dx = (fx - np.float32(p.cx)).astype(np.float64)
        dy = (fy - np.float32(p.cy)).astype(np.float64)
        ppx, ppy = dx * p.ax + dy * p.ay, dx * p.bx + dy * p.by
        q = ppx * ppx + ppy * ppy
        keep = q <= 4.0
        edge = np.abs(q - 4.0) < 1e-3
        if sd is not None:
            keep &= zw <= sd
            edge |= (q <= 4.0 + 1e-3) & (np.abs(zw.astype(np.float64) - sd.astype(np.float64)) <= 1e-6)
        if not (keep.any() or edge.any()):
            continue
        Tn = np.where(keep, T - p.alpha * (np.exp(-q) * T), T)
        und |= edge & ~found
        und |= np.abs(Tn - 0.5) < 1e-3
        cross = ~found & (T >= 0.5) & (Tn < 0.5)
        sid[cross] = i
        dep[cross] = zw
        found |= cross
        T = Tn
    return sid, dep, 1.0 - T, und


def batch_scene(k, n_behind=N_BEHIND, opaque=True):
    """64x48: k-1 faint flat splats over the tile TILE (alpha byte 1: the least the sort keeps at that size), then one wide opaque
    splat whose e^-q is >= 0.9 over the tile's inner 8x8 pixels (row k-1), then n_behind more behind it."""
    W, H = 64, 48
    cam = camera(W, H)
    cx, cy = TILE[0] * 16 + 8.0, TILE[1] * 16 + 8.0
    rows, d = [], 1.0
    for i in range(k - 1):
        d += 0.002
        rows.append(splat(cam, cx, cy, 12.0, 11.0, d, (40 + i % 200, 200, 30, 1)))
        assert rows[-1][27] == 1
    if opaque:
        d += 0.002
        rows.append(splat(cam, cx, cy, 40.0, 39.0, d, (255, 30, 0, 255)))
    for i in range(n_behind):
        d += 0.002
        rows.append(splat(cam, cx + 2 * i, cy, 14.0, 13.0, d, (0, 50 * i, 255, 200)))
    return Scene(W, H, rows)


def half_depth(scene, k):
    """a scene depth that lies in front of row k-1 (the opaque splat) on the left half of the tile's inner pixels, far elsewhere"""
    z = np.ones((scene.H, scene.W), np.float32)
    zo, zf = window_depth(scene, k - 1), (window_depth(scene, k - 2) if k > 1 else np.float32(0.0))
    z[:, :24] = np.float32(0.5 * (float(zo) + float(zf)))
    assert zf < z[0, 0] < zo
    return z


def synth_scene(seed, W=96, H=64, n=300):
    """a random cloud whose splats are large enough on a small frame for surfaces to exist"""
    rows = synth.make_splat_rows(n, seed=seed).reshape(-1, 32).copy()
    sc = rows[:, 12:24].copy().view("<f4")
    rows[:, 12:24] = (sc * np.float32(6.0)).view(np.uint8)
    s = Scene.__new__(Scene)
    s.W, s.H, s.cam = W, H, synth.index_html_camera(W, H, 20.0 * seed, capi=capi)
    s.rows = rows.reshape(-1)
    s.cs, s.cc, s.mats = oracle.pack(s.rows)
    return s


SYNTH_SEEDS = (11, 12, 13)


def every_scene():
    """(name, scene, scene depth or None, strips) of everything test_surface_gpu.py compares with the mirror"""
    out = []
    for k in BATCH_EDGES:
        sc = batch_scene(k)
        out.append(("batch%d" % k, sc, None, [(0, None)]))
    sc = batch_scene(65)
    out.append(("depth65", sc, half_depth(sc, 65), [(0, None)]))
    out.append(("faint", batch_scene(100, 0, opaque=False), None, [(0, None)]))
    for seed in SYNTH_SEEDS:
        out.append(("synth%d" % seed, synth_scene(seed), None, [(0, None)]))
    out.append(("synth21_100x70", synth_scene(21, 100, 70), None, [(0, None)]))       # the strip / pick / option tests' scene
    for w, h in ((64, 48), (100, 70)):
        out.append(("synth31_%dx%d" % (w, h), synth_scene(31, w, h), None, [(0, None)]))   # the colour tests' scenes
    return out


def order(scene):
    return oracle.sort(scene.mats, scene.cam["view"])


@pytest.mark.parametrize("case", every_scene(), ids=lambda c: c[0])
def test_undecided_share_of_every_scene(case):
    name, sc, sdepth, strips = case
    idx = order(sc)
    for x0, x1 in strips:
        sid, dep, alpha, und = mirror(sc, idx, x0, x1, sdepth)
        share = und.mean()
        print("%s [%s,%s): undecided %.4f, surfaces %.3f" % (name, x0, x1, share, (sid != NONE).mean()))
        assert share <= UNDECIDED_CAP, (name, share)
        if name.startswith("synth"):
            assert (sid != NONE).mean() > 0.1 and (sid == NONE).mean() > 0.02, "the scene should hold surfaces and pixels without one"


@pytest.mark.parametrize("k", BATCH_EDGES)
def test_batch_scene_is_what_it_claims(k):
    """the faint stack keeps T above 0.55; the opaque splat's e^-q is >= 0.9 on the inner pixels; the mirror finds row k-1 there"""
    sc = batch_scene(k)
    idx = order(sc)
    assert list(idx[::-1][:k]) == list(range(k)), "rows come nearest first"
    faint = batch_scene(k, 0, opaque=False)
    if k > 1:
        _, _, a, _ = mirror(faint, order(faint))
        assert (1.0 - a).min() > 0.55
    only = Scene(sc.W, sc.H, [sc.rows.reshape(-1, 32)[k - 1]])
    _, _, a1, _ = mirror(only, order(only))
    assert a1[INNER].min() >= 0.9 * (255.0 / 255.0) - 1e-12
    sid, dep, _, und = mirror(sc, idx)
    assert not und[INNER].any()
    assert (sid[INNER] == k - 1).all() and (dep[INNER] == window_depth(sc, k - 1)).all()


def test_mirror_on_one_splat_by_hand():
    """one splat, alpha byte 204 (0.8), centred on pixel centre (24.5, 24.5) with half extents 16 x 15 (splat() needs hx > hy: an exactly
    round ellipse has no eigenvector in the reference's projection; the tilt it adds is 1e-3 rad): q = 4 (d / 16)^2 along the row,
    4 (d / 15)^2 along the column.  At the centre e^-q = 1, T = 0.2: a surface.  T crosses one half where 0.8 e^-q = 0.5, q = ln 1.6:
    d = 16 sqrt(ln 1.6 / 4) = 5.48 pixels along the row, 5.14 along the column."""
    W, H = 64, 48
    cam = camera(W, H)
    sc = Scene(W, H, [splat(cam, 24.5, 24.5, 16.0, 15.0, 1.0, (9, 9, 9, 204))])
    sid, dep, alpha, und = mirror(sc, order(sc))
    zw = window_depth(sc, 0)
    assert 0.0 < zw < 1.0
    assert sid[24, 24] == 0 and dep[24, 24] == zw and abs(alpha[24, 24] - 0.8) < 1e-3
    for d, inside in ((5, True), (6, False)):                       # along the row: 5 pixels off crosses, 6 does not
        q = 4.0 * (d / 16.0) ** 2
        assert abs(alpha[24, 24 + d] - 0.8 * np.exp(-q)) < 2e-3
        assert (sid[24, 24 + d] == 0) == inside and (dep[24, 24 + d] == (zw if inside else np.float32(1.0)))
        assert (sid[24 + d, 24] == 0) == inside
    assert sid[24, 24 + 17] == NONE and alpha[24, 24 + 17] == 0.0 and dep[24, 24 + 17] == np.float32(1.0)   # q > 4: no fragment
    assert 0.0 < alpha[24, 24 + 15] < 0.05 and sid[24, 24 + 15] == NONE                                      # covered, no surface
    # a scene depth in front of the splat removes its fragments; equal depth passes (LEQUAL)
    z = np.full((H, W), zw, np.float32)
    z[:, :24] = np.nextafter(zw, np.float32(0.0))
    sid2, _, a2, und2 = mirror(sc, order(sc), scene_depth=z)
    assert sid2[24, 23] == NONE and a2[24, 23] == 0.0 and sid2[24, 24] == 0
    assert und2[24, 20] and und2[24, 24]                            # within 1e-6 of the scene's depth: undecided by rule
