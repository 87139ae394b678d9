"""GPU tier: every blend path, forced by name on a fresh context and proven by the frame's statistics, against the CPU oracle at the
edges where a blend goes wrong -- and against each other (include/gs_splat.h: lists, pair records, the row walk, sub-tile lists and
paired frames draw the same pixels bit for bit; the split blend within 1 LSB).

Paths (test_gpu_parity.PATH_OPTIONS / PATH_PROOF): lists (span lists), walk (GS_OPT_ROW_WALK 2: no tile lists, the blend collects a
tile's entries from its row's runs), subtile (GS_OPT_SUBTILE 2), pairs (GS_OPT_BINNING 1: pair records; gs_stats.binning == 1),
split (GS_OPT_BLEND_SPLIT 1); two binning rounds (GS_OPT_NEAR_PERMILLE 3 / 400) and paired queued frames (GS_OPT_FRAME_BATCH 2).

Scenes are built here from 32-byte .splat rows: flat, axis-aligned splats at distinct depths in front of a camera whose principal
point lies to the left of and below the frame (so that a wide splat's screen ellipse has a small, well-defined tilt), each placed
to make a chosen run of tile columns in a chosen tile row.  Before a layout is relied on it is checked on the lists path
(GS_OPT_RECORD_STAGED + GS_BUF_TILE_STATS list lengths): "column 4 of tile row 5 holds exactly 65 entries".  The oracle draws only the
strip under test.

Budget: about 3 s of wall time on one MI355X (1.5 s of test time as last measured, 0.15 s of it the nine contexts of the paired-frames
test: ~180 fresh contexts, the oracle drawing only the strips under test)."""
import math

import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_gpu_parity import PIXEL_TOL_LSB, assert_path, force_path, pix_check

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

EXACT = ("lists", "walk", "subtile", "pairs")          # bit-identical to each other; "split" within 1 LSB


# ---------------------------------------------------------------- constructed scenes

def camera(W, H, off=0.5):
    """Identity pose; a frustum whose principal point lies `off` focal lengths left of and below the frame, focal = the longer side.
    A splat centred off the axis in x and y gets a screen covariance term j02 * j12 * sz^2: splat() uses it to give wide ellipses a
    tilt of ~1e-3 rad -- an exactly axis-aligned ellipse whose long axis is horizontal has no defined eigenvector in the reference's
    projection (index.js:131-140) and is culled or flipped by rounding."""
    f = float(max(W, H, 64))
    px0, py0, n = -off * f, -(0.05 if off > 1 else off) * f, 0.005
    proj = synth.frustum((0 - px0) / f * n, (W - px0) / f * n, (H - py0) / f * n, (0 - py0) / f * n, n, 10000.0)
    return synth.uniforms(synth.compose((0.0, 0.0, 0.0)), synth.compose((0.0, 0.0, 0.0)), proj, W, H, capi=capi)


def splat(cam, cx, cy, hx, hy, depth, rgba):
    """One .splat row whose quad is centred at image pixel (cx, cy) (top-down rows) with half extents hx, hy pixels, depth units away."""
    W, H, gp, f = cam["vw"], cam["vh"], cam["gs_proj"], cam["focal"]
    X = (2.0 * cx / W - 1.0 + gp[8]) * depth / gp[0]
    Y = (2.0 * (H - cy) / H - 1.0 + gp[9]) * depth / gp[5]
    camx, camy, camz = X, Y, -depth                      # (the model-view matrix is the identity; a row's z is the camera's -z)
    j00, j02, j11, j12 = f / camz, -(f * camx) / (camz * camz), -f / camz, (f * camy) / (camz * camz)
    d1, d2 = hx * hx / 8.0 - 0.3, hy * hy / 8.0 - 0.3    # half extent = 2 sqrt(2 (cov + 0.3))
    sz2 = 0.001 * (d1 - d2) / abs(j02 * j12) if hx > hy else 0.0
    sx, sy = math.sqrt((d1 - j02 * j02 * sz2) / (j00 * j00)), math.sqrt((d2 - j12 * j12 * sz2) / (j11 * j11))
    # the depth sort keeps a splat only if max(scale) * alpha > 1e-4 * depth (index.js:397, 548): alpha is raised to what keeps it
    a = max(int(rgba[3]), int(math.ceil(255.0 * 1.5e-4 * depth / max(sx, sy, math.sqrt(sz2)))))
    assert a <= 255, "splat too small to survive the sort"
    rgba = (rgba[0], rgba[1], rgba[2], a)
    r = np.zeros(32, np.uint8)
    r[0:12] = np.array([X, Y, depth], "<f4").view(np.uint8)
    r[12:24] = np.array([sx, sy, math.sqrt(sz2) + 1e-4 * min(sx, sy)], "<f4").view(np.uint8)
    r[24:28] = rgba
    r[28:32] = (255, 128, 128, 128)                      # identity rotation
    return r


def run(cam, ty, a, b, depth, rgba):
    """A splat whose quad covers tile columns a..b of tile row ty (edges 3.5 px inside the end tiles, rows 3..13 of the tile row)."""
    return splat(cam, (a + b) * 8.0 + 8.0, ty * 16.0 + 8.0, (b - a) * 8.0 + 4.5, 5.0, depth, rgba)


class Scene:
    def __init__(self, W, H, rows, off=0.5):
        self.W, self.H, self.cam = W, H, camera(W, H, off)
        self.rows = np.concatenate(rows) if len(rows) else np.zeros(0, np.uint8)
        self.cs, self.cc, self.mats = oracle.pack(self.rows) if len(rows) else (None, None, None)

    def params(self, x0=0, x1=None, **kw):
        return capi.make_params(self.cam["gs_mv"], self.cam["gs_proj"], self.W, self.H, x0=x0, x1=x1, focal_=self.cam["focal"], **kw)

    def oracle(self, idx, x0=0, x1=None, **kw):
        if not len(self.rows):
            bg = np.asarray(kw.get("bg", (0, 0, 0, 1)), np.float32)
            return np.broadcast_to(np.floor(np.clip(bg, 0, 1) * 255 + 0.5).astype(np.uint8), (self.H, (x1 or self.W) - x0, 4)).copy(), 0
        c = self.cam
        u8, _, fr = oracle.render(self.cs, self.cc, idx, c["gs_mv"].astype(np.float32), c["gs_proj"].astype(np.float32), c["focal"],
                                  self.W, self.H, x0=x0, x1=x1, want_f32=False, **kw)
        return u8, fr


def draw(scene, path, views=((0, None),), flags=0, opts=(), bg=(0.0, 0.0, 0.0, 1.0)):
    """Render the strips `views` of a scene on a fresh context with `path` forced; every frame's statistics prove the path."""
    out = []
    with capi.Context(0) as c:
        force_path(c, path)
        for k, v in opts:
            c.set_option(k, v)
        if len(scene.rows):
            c.push_splat(scene.rows)
        idx = c.sort(scene.cam["view"])
        for x0, x1 in views:
            out.append(c.render(scene.params(x0, x1, flags=flags, background=bg)))
            st = assert_path(c, path, (x0, x1))
    return out, idx, st


def tile_lengths(c, scene, x0=0, x1=None):
    """(tiles_y, tiles_x) list length per tile of the strip [x0, x1) that context c drew last with GS_OPT_RECORD_STAGED set (GS_BUF_TILE_STATS)."""
    tx, ty = ((x1 or scene.W) - x0 + 15) // 16, (scene.H + 15) // 16
    return c.download(capi.BUF_TILE_STATS, tx * ty, np.uint32, 2)[:, 1].reshape(ty, tx)


def list_lengths(scene, path="lists", x0=0, x1=None):
    """(tiles_y, tiles_x) list length per tile, from the lists path (GS_OPT_RECORD_STAGED, GS_BUF_TILE_STATS) or another one that builds lists."""
    with capi.Context(0) as c:
        force_path(c, path)
        c.set_option(capi.OPT_RECORD_STAGED, 1)
        c.push_splat(scene.rows)
        c.sort(scene.cam["view"])
        c.render(scene.params(x0, x1))
        assert_path(c, path)
        return tile_lengths(c, scene, x0, x1)


def compare_paths(scene, views, paths=EXACT + ("split",), tag="", oracle_views=None, **kw):
    """Every path equal to the first one bit for bit (split: within 1 LSB), and the first within the oracle's bar on each strip."""
    imgs, idx = {}, None
    for p in paths:
        imgs[p], i, _ = draw(scene, p, views, **kw)
        if idx is None:
            idx = i
            if len(scene.rows):
                assert np.array_equal(idx, oracle.sort(scene.mats, scene.cam["view"]))
        assert np.array_equal(i, idx)
    ref = imgs[paths[0]]
    for p in paths[1:]:
        for (x0, x1), a, b in zip(views, ref, imgs[p]):
            if p == "split":
                assert np.abs(a.astype(int) - b.astype(int)).max() <= 1, (tag, p, x0, x1)
            else:
                assert np.array_equal(a, b), (tag, p, x0, x1, int(np.abs(a.astype(int) - b.astype(int)).max()))
    for k, (x0, x1) in enumerate(views):
        if oracle_views is None or (x0, x1) in oracle_views:
            want, _ = scene.oracle(idx, x0, x1, bg=kw.get("bg", (0.0, 0.0, 0.0, 1.0)))
            pix_check("%s_%s_%d_%s" % (tag, paths[0], x0, x1), ref[k], want)
    return imgs, idx


# ---------------------------------------------------------------- the row walk's batches

TARGET = 4                          # the column every case row is about (10 tile columns)
CASES = [(c, m) for c in (1, 3, 63, 64, 65, 127, 128, 129) for m in (0, 1, 37, 64, 200)]
STRONG = {1, 3, 63, 65, 67}         # hit ranks (0 = nearest) drawn strong: an odd batch's unpadded slot would re-blend one of them


def _covering_scene(seed=5):
    """Tile row r holds case r: c runs that cover column 4 interleaved (by depth) with m that miss it -- half of them ending at
    column 3, the column the coverage test must not stretch to.  Rows beyond the cases: the nearest 64 / 128 / 300 runs miss,
    then 5 hits; a column no run covers between covered neighbours; faint runs (alpha 1-3, or the least the sort keeps); and an
    empty tile row at the end.  (Saturation: test_saturation_inside_and_at_the_edges_of_batches.)"""
    g = np.random.Generator(np.random.PCG64(seed))
    W, rows, want, depth = 160, [], {}, [1.0]
    H = 16 * (len(CASES) + 3 + 1 + 1 + 1)
    cam = camera(W, H)
    hit_shapes, miss_shapes = [(4, 4), (2, 6), (4, 9), (0, 4), (3, 5)], [(3, 3), (0, 3), (5, 5), (5, 9), (1, 3), (6, 8)]

    def put(ty, a, b, alpha, rgb=None):
        depth[0] += 0.002
        rgb = g.integers(0, 256, 3) if rgb is None else rgb
        rows.append(run(cam, ty, a, b, depth[0], (int(rgb[0]), int(rgb[1]), int(rgb[2]), int(alpha))))

    ty = 0
    for c, m in CASES:
        order = sorted([((i + 0.5) / c, 0, i) for i in range(c)] + [((k + 0.5) / m, 1, k) for k in range(m)])
        for _, miss, k in order:
            if miss:
                put(ty, *miss_shapes[k % len(miss_shapes)], alpha=6)
            else:
                put(ty, *hit_shapes[k % len(hit_shapes)], alpha=60 if k in STRONG else 3,
                    rgb=(255, 30, 0) if k in STRONG else None)
        want[ty] = c
        ty += 1
    for m in (64, 128, 300):                                       # misses first, hits at the far end
        for k in range(m):
            put(ty, *miss_shapes[k % len(miss_shapes)], alpha=4)
        for k in range(5):
            put(ty, *hit_shapes[k % len(hit_shapes)], alpha=40)
        want[ty] = 5
        ty += 1
    for k in range(70):                                            # column 4 covered by nothing, both neighbours by 70 runs
        put(ty, *((0, 3) if k % 2 else (5, 9)), alpha=5)
    want[ty] = 0
    ty += 1
    for k in range(150):                                           # faint
        put(ty, *hit_shapes[k % len(hit_shapes)], alpha=1 + k % 3)
    want[ty] = 150
    ty += 1
    assert ty + 1 == H // 16                                       # (and the last tile row is empty)
    return Scene(W, H, rows), want


@pytest.fixture(scope="module")
def covering():
    return _covering_scene()


def test_constructed_layout_is_what_it_claims(covering):
    scene, want = covering
    lens = list_lengths(scene)
    assert lens.shape == (scene.H // 16, 10)
    for ty, c in want.items():
        assert lens[ty, TARGET] == c, "column %d of tile row %d holds %d entries, not %d" % (TARGET, ty, lens[ty, TARGET], c)
    nothing = [ty for ty, c in want.items() if c == 0]
    for ty in nothing:
        assert lens[ty, TARGET - 1] == 70 // 2 and lens[ty, TARGET + 1] == 70 // 2
    assert lens[-1].sum() == 0                                      # the empty tile row
    print("column %d list lengths per tile row:" % TARGET, lens[:, TARGET].tolist())


def test_covering_runs_every_path_and_the_oracle(covering):
    scene, _ = covering
    views = [(0, None), (64, 80), (48, 96)]                        # the frame, the target column alone, and with its neighbours
    compare_paths(scene, views, tag="covering")


def test_covering_runs_modes_walk_and_lists(covering):
    scene, _ = covering
    idx = None
    for flags in (capi.RENDER_NO_EARLY_OUT, capi.RENDER_FLIP_Y):
        imgs = {p: draw(scene, p, flags=flags)[0][0] for p in ("walk", "lists")}
        assert np.array_equal(imgs["walk"], imgs["lists"]), flags
        if idx is None:
            idx = draw(scene, "lists")[1]
        want, _ = scene.oracle(idx)
        pix_check("covering_flags%d" % flags, imgs["lists"][::-1] if flags == capi.RENDER_FLIP_Y else imgs["lists"], want)
    for term in (256, 65536):
        imgs = {p: draw(scene, p, opts=((capi.OPT_TERMINATION, term),))[0][0] for p in ("walk", "lists")}
        assert np.array_equal(imgs["walk"], imgs["lists"]), term
        want, _ = scene.oracle(idx)
        pix_check("covering_term%d" % term, imgs["lists"], want)
    bg = (0.2, 0.4, 0.6, 0.5)
    imgs = {p: draw(scene, p, bg=bg)[0][0] for p in ("walk", "lists")}
    assert np.array_equal(imgs["walk"], imgs["lists"])
    pix_check("covering_bg", imgs["lists"], scene.oracle(idx, bg=bg)[0])


def test_count_frags_on_the_list_paths_and_never_walked(covering):
    scene, _ = covering
    _, idx, _ = draw(scene, "lists")
    _, frags = scene.oracle(idx)
    for p in ("lists", "pairs", "subtile", "walk"):
        with capi.Context(0) as c:
            force_path(c, p)
            c.push_splat(scene.rows)
            c.sort(scene.cam["view"])
            c.render(scene.params(flags=capi.RENDER_COUNT_FRAGS))
            st = c.stats()
            assert st["row_walk"] == 0, p                            # counting renders keep the lists by design
            if p != "walk":
                assert_path(c, p)
            assert st["n_frags"] == frags, (p, st["n_frags"], frags)


def test_walk_need_record_equals_the_lists():
    """Every tile saturates (tall opaque bars), so the frame's need record (gs_stats.need_splats: the sorted position at which a tile's
    last lane left its list, at step granularity) is the largest over both tile columns -- column 1, which saturates deeper.  Its list
    holds bars of column 1 only; 301 bars of column 0 (runs that END at column 0) lie in front of them, so a walk that took them for
    column 1 would shift every later entry by an odd number of slots and record another position."""
    W, H = 32, 16
    cam = camera(W, H)
    rows, d = [], 1.0
    for k in range(301):
        d += 0.002
        rows.append(splat(cam, 8.0, 8.0, 7.9, 200.0, d, (200, 40, 40, 255)))
        if k % 10 == 0:
            d += 0.002
            rows.append(splat(cam, 24.0, 8.0, 7.9, 200.0, d, (40, 40, 200, 4)))
    for k in range(500):
        d += 0.002
        rows.append(splat(cam, 24.0, 8.0, 7.9, 200.0, d, (40, 200, 40, 255)))
    scene = Scene(W, H, rows)
    lens = list_lengths(scene)
    assert lens.tolist() == [[301, 31 + 500]], lens
    got = {}
    for p in ("lists", "walk", "pairs"):
        imgs, idx, st = draw(scene, p)
        got[p] = (imgs[0], st["need_splats"])
    want, _ = scene.oracle(idx)
    pix_check("need_probe", got["lists"][0], want)
    assert got["lists"][1] not in (0, 0xFFFFFFFF), got["lists"][1]
    for p in ("walk", "pairs"):
        assert np.array_equal(got[p][0], got["lists"][0]), p
        assert got[p][1] == got["lists"][1], (p, got[p][1], got["lists"][1])


@pytest.mark.parametrize("wall", [20, 63, 64, 95])
def test_saturation_inside_and_at_the_edges_of_batches(wall):
    """Column 4 holds 128 faint runs (interleaved with runs that end at column 3) and two opaque splats far wider and taller than the
    frame, hit number `wall` (0 = nearest) and the one behind it: the first saturates every pixel of column 4 at once, the second the
    rest of the frame.  The tile then stops inside the first
    batch (20), on the first batch's last entry (63: the walk must not start a second batch), on the second batch's first entry (64)
    and mid-batch (95).  Where it stopped is checked on the lists path (GS_OPT_RECORD_STAGED 2: entries the tile evaluated, counted by
    steps of two entries); every tile saturates, so the need records of walk, pairs and lists are compared too."""
    W, H = 160, 16
    cam = camera(W, H)
    g = np.random.Generator(np.random.PCG64(wall))
    rows, d = [], 1.0
    shapes = [(4, 4), (2, 6), (4, 9), (0, 4), (3, 5)]
    for k in range(129):
        d += 0.002
        if k == wall:                                                  # (and a second one behind it: every other tile saturates too)
            rows.append(splat(cam, 72.0, 8.0, 2000.0, 2040.0, d, (250, 250, 20, 255)))
            d += 0.002
            rows.append(splat(cam, 72.0, 8.0, 2000.0, 2040.0, d, (20, 250, 250, 255)))
        else:
            rows.append(run(cam, 0, *shapes[k % len(shapes)], d, (int(g.integers(0, 256)), 60, 200, 3)))
        if k % 2:
            d += 0.002
            rows.append(run(cam, 0, *((3, 3) if k % 4 == 1 else (0, 3)), d, (30, 200, 30, 40)))
    scene = Scene(W, H, rows)
    assert list_lengths(scene)[0, TARGET] == 130
    with capi.Context(0) as c:
        force_path(c, "lists")
        c.set_option(capi.OPT_RECORD_STAGED, 2)
        c.push_splat(scene.rows)
        c.sort(scene.cam["view"])
        c.render(scene.params())
        evaluated = int(c.download(capi.BUF_TILE_STATS, W // 16, np.uint32, 2)[TARGET, 0])
    want = 64 * (wall // 64) + 2 * ((wall % 64) // 2) + 2
    assert evaluated == want, "column %d stopped after %d entries, not %d (the opaque splat is entry %d)" % (TARGET, evaluated, want, wall)
    imgs, _ = compare_paths(scene, [(0, None), (64, 80)], tag="wall%d" % wall)
    need = {}
    for p in ("lists", "walk", "pairs"):
        _, _, st = draw(scene, p)
        need[p] = st["need_splats"]
    assert need["lists"] not in (0, 0xFFFFFFFF) and need["walk"] == need["lists"] and need["pairs"] == need["lists"], need


def test_very_long_tile_row_walked():
    """More than 8192 runs in one tile row (the automatic choice declines such rows; forced on the walk must still be right)."""
    g = np.random.Generator(np.random.PCG64(17))
    W, H = 1280, 32
    cam = camera(W, H)
    n = 9000
    cols = g.integers(0, W // 16, n)
    rows = [run(cam, 0, int(a), int(a), 1.0 + 0.001 * k, (int(g.integers(0, 256)), 90, int(g.integers(0, 256)), int(g.integers(1, 12))))
            for k, a in enumerate(cols)]
    scene = Scene(W, H, rows)
    lens = list_lengths(scene)
    assert lens[0].sum() == n and lens[1].sum() == 0
    compare_paths(scene, [(0, None), (1264, 1280)], paths=("walk", "lists", "pairs"), tag="long_row", oracle_views=[(1264, 1280)])


# ---------------------------------------------------------------- shapes

@pytest.fixture(scope="module")
def cloud():
    rows = synth.make_splat_rows(20000, seed=4242)
    cs, cc, mats = oracle.pack(rows)
    return rows, cs, cc, mats


def _cloud_paths(cloud, w, h, views, oracle_views, paths=EXACT + ("split",), flags=0, yaw=30.0):
    rows, cs, cc, mats = cloud
    cam = synth.index_html_camera(w, h, yaw, capi=capi)
    mv, P = cam["gs_mv"].astype(np.float32), cam["gs_proj"].astype(np.float32)
    imgs = {}
    idx = None
    for p in paths:
        with capi.Context(0) as c:
            force_path(c, p)
            c.push_splat(rows)
            i = c.sort(cam["view"])
            idx = i if idx is None else idx
            assert np.array_equal(i, idx)
            imgs[p] = []
            for x0, x1 in views:
                imgs[p].append(c.render(capi.make_params(cam["gs_mv"], cam["gs_proj"], w, h, x0=x0, x1=x1, focal_=cam["focal"], flags=flags)))
                assert_path(c, p, (w, h, x0, x1))
    assert np.array_equal(idx, oracle.sort(mats, cam["view"]))
    for p in paths[1:]:
        for a, b in zip(imgs[paths[0]], imgs[p]):
            d = int(np.abs(a.astype(int) - b.astype(int)).max()) if a.size else 0
            assert d <= (1 if p == "split" else 0), (w, h, p, d)
    for k, (x0, x1) in enumerate(views):
        if (x0, x1) in oracle_views:
            want, _, _ = oracle.render(cs, cc, idx, mv, P, cam["focal"], w, h, x0=x0, x1=x1, want_f32=False)
            pix_check("cloud_%dx%d_%d_%d" % (w, h, x0, x1), imgs[paths[0]][k], want)
    return imgs


@pytest.mark.parametrize("w,h", [(1, 1), (3, 5), (17, 17), (31, 47), (333, 211), (1283, 721)])
def test_frame_shapes_every_path(cloud, w, h):
    last = max(0, (w - 1) // 16 * 16)                              # the last (partial) tile column
    views = [(0, w)] + ([(last, w)] if last else [])
    oracle_views = [(0, w)] if w * h < 100000 else [(last, w)]
    _cloud_paths(cloud, w, h, views, oracle_views)


def test_strips_every_offset_and_width_walk_and_lists(cloud):
    w, h = 640, 360
    views = [(x0, x0 + sw) for x0 in (0, 4, 12, 20) for sw in (1, 4, 15, 16, 17, 611)]
    _cloud_paths(cloud, w, h, views, oracle_views=[v for v in views if v[1] - v[0] <= 17] + [(20, 631)], paths=("walk", "lists", "pairs"))


def _wide_scene(W, H):
    """A one-tile-row splat whose run spans every tile column (4096 wide: the packed run word's first column 0 and length - 1 = 255), a
    two-tile-row splat whose two runs span at least 240 columns each (both halves of the packed word near that limit: the ends of a
    slightly tilted ellipse lie in one of its rows), small splats in the last column and row, and faint bars over the rest.  (The principal point lies 40
    focal lengths to the left: the tilt that defines a 4096-pixel ellipse's long axis then adds next to nothing to its height.)"""
    cam = camera(W, H, 40.0)
    rows = [splat(cam, W / 2.0, 8.0, 2300.0, 5.0, 2.0, (255, 60, 20, 120)),
            splat(cam, W / 2.0, 31.5, 2300.0, 10.0, 2.5, (20, 200, 60, 120))]
    g = np.random.Generator(np.random.PCG64(W + H))
    for k in range(400):
        x, y = float(g.uniform(0, W)), float(g.uniform(0, H))
        rows.append(splat(cam, x, y, 6.0, 7.0, 3.0 + 0.003 * k, (int(g.integers(0, 256)), 128, int(g.integers(0, 256)), 40)))
    rows.append(splat(cam, W - 8.0, H - 8.0, 4.0, 5.0, 1.5, (0, 0, 255, 200)))
    return Scene(W, H, rows, 40.0)


def test_256_tile_columns_packed_runs_at_their_limit():
    scene = _wide_scene(4096, 64)
    lens = list_lengths(scene)
    assert lens.shape == (4, 256)
    assert (lens[0] >= 1).all(), "the one-tile-row splat does not span every column"                  # first 0, length - 1 = 255
    assert (lens[1] >= 1).sum() >= 240 and (lens[2] >= 1).sum() >= 240, "the two-tile-row splat is not as wide as made"
    views = [(0, 4096), (0, 64), (2032, 2064), (4032, 4096)]
    compare_paths(scene, views, paths=("walk", "lists", "pairs", "subtile"), tag="w4096", oracle_views=views[1:])


def test_256_tile_rows():
    W, H = 64, 4096
    cam = camera(W, H)
    g = np.random.Generator(np.random.PCG64(64))
    rows = [splat(cam, 32.0, float(y), 20.0 + (k % 5), 30.0, 2.0 + 0.004 * k, (200, int(g.integers(0, 256)), 40, 90))
            for k, y in enumerate(range(8, H, 24))]
    rows.append(splat(cam, 56.0, H - 8.0, 4.0, 5.0, 1.5, (0, 0, 255, 200)))
    scene = Scene(W, H, rows)
    compare_paths(scene, [(0, W), (48, W)], paths=("walk", "lists", "pairs", "subtile"), tag="h4096")


@pytest.mark.parametrize("W,H", [(4112, 64), (64, 4112)])
def test_beyond_256_tiles_falls_back_to_pair_records(W, H):
    """More than 256 tile columns or rows: span lists do not apply, every path bins pair records (gs_stats.binning) and none walks."""
    scene = _wide_scene(W, H) if W > H else Scene(W, H, [splat(camera(W, H), 32.0, float(y), 20.0, 30.0, 2.0 + 0.01 * k, (200, 40, 90, 90))
                                                        for k, y in enumerate(range(8, H, 40))])
    views = [(0, W), (0, 64)] + ([(W - 32, W)] if W > 64 else [(48, 64)])
    imgs = {}
    for p in ("lists", "walk", "pairs"):
        with capi.Context(0) as c:
            force_path(c, p)
            c.push_splat(scene.rows)
            idx = c.sort(scene.cam["view"])
            imgs[p] = []
            for x0, x1 in views:
                imgs[p].append(c.render(scene.params(x0, x1)))
                st = c.stats()
                wide = (x1 - x0 + 15) // 16 > 256 or (H + 15) // 16 > 256
                assert st["binning"] == (1 if wide or p == "pairs" else 0), (p, x0, x1, st["binning"])
                assert st["row_walk"] == (1 if p == "walk" and not wide else 0), (p, x0, x1)
    for p in ("walk", "pairs"):
        for a, b in zip(imgs["lists"], imgs[p]):
            assert np.array_equal(a, b), p
    for k, (x0, x1) in enumerate(views[1:], 1):
        pix_check("fallback_%dx%d_%d" % (W, H, x0), imgs["lists"][k], scene.oracle(idx, x0, x1)[0])


def test_empty_frame_every_path():
    """Nothing resident: the background, whatever the path, and the statistics still name the path (gs_stats.binning of a frame
    without a binning round: the binning its round would take)."""
    scene = Scene(48, 40, [])
    for p in EXACT + ("split",):
        imgs, _, _ = draw(scene, p, views=[(0, None), (4, 21)], bg=(1.0, 0.0, 0.5, 1.0))
        for img in imgs:
            assert np.all(img == np.array([255, 0, 128, 255], np.uint8)), p


# ---------------------------------------------------------------- modes on the cloud: stereo, scene inputs, two rounds, paired frames

def test_stereo_walk_and_lists(cloud):
    rows, cs, cc, mats = cloud
    l, r, head = synth.xr_eye_cameras(60.0, 0.25, capi=capi)
    out = {}
    for p in ("walk", "lists"):
        with capi.Context(0) as c:
            force_path(c, p)
            c.push_splat(rows)
            idx = c.sort(head["view"])
            pl = capi.make_params(l["gs_mv"], l["gs_proj"], l["vw"], l["vh"], focal_=l["focal"])
            pr = capi.make_params(r["gs_mv"], r["gs_proj"], r["vw"], r["vh"], focal_=r["focal"])
            out[p] = c.render_stereo(pl, pr)
            assert_path(c, p)
    for a, b in zip(out["walk"], out["lists"]):
        assert np.array_equal(a, b)
    for eye, img in zip((l, r), out["lists"]):
        x0 = (eye["vw"] // 2) & ~15
        want, _, _ = oracle.render(cs, cc, idx, eye["gs_mv"].astype(np.float32), eye["gs_proj"].astype(np.float32), eye["focal"],
                                   eye["vw"], eye["vh"], x0=x0, x1=x0 + 48, want_f32=False)
        pix_check("stereo_%d" % eye["vw"], img[:, x0:x0 + 48], want)


def test_scene_depth_and_colour_walk_and_lists(cloud):
    rows, cs, cc, mats = cloud
    w, h = 320, 180
    cam = synth.index_html_camera(w, h, 75.0, capi=capi)
    g = np.random.Generator(np.random.PCG64(9))
    depth = g.uniform(0.995, 1.0, (h, w)).astype(np.float32)
    depth[:, : w // 3] = 1.0
    rgba = g.integers(0, 256, (h, w, 4)).astype(np.uint8)
    out = {}
    for p in ("walk", "lists"):
        with capi.Context(0) as c:
            force_path(c, p)
            c.push_splat(rows)
            idx = c.sort(cam["view"])
            c.set_scene(depth, rgba)
            out[p] = c.render(capi.make_params(cam["gs_mv"], cam["gs_proj"], w, h, focal_=cam["focal"]))
            assert_path(c, p)
    assert np.array_equal(out["walk"], out["lists"])
    want, _, _ = oracle.render(cs, cc, idx, cam["gs_mv"].astype(np.float32), cam["gs_proj"].astype(np.float32), cam["focal"], w, h,
                               want_f32=False, scene_depth=depth, scene_rgba=rgba)
    pix_check("scene_inputs", out["lists"], want)


def test_two_rounds_walk_and_lists(cloud):
    rows, cs, cc, mats = cloud
    w, h = 640, 360
    cam = synth.index_html_camera(w, h, 200.0, capi=capi)
    tx, ty = (w + 15) // 16, (h + 15) // 16
    res, unsat = {}, 0
    for p in ("walk", "lists"):
        res[p] = []
        with capi.Context(0) as c:
            force_path(c, p)
            c.push_splat(rows)
            idx = c.sort(cam["view"])
            for permille in (3, 400):
                c.set_option(capi.OPT_NEAR_PERMILLE, permille)
                img = c.render(capi.make_params(cam["gs_mv"], cam["gs_proj"], w, h, focal_=cam["focal"]))
                assert_path(c, p, permille)
                mask = c.download(capi.BUF_UNSAT_MASK, ty, np.uint32, (tx + 31) // 32)
                res[p].append((img, mask, c.frame_status()))
    for (ia, ma, sa), (ib, mb, sb) in zip(res["walk"], res["lists"]):
        assert np.array_equal(ia, ib) and np.array_equal(ma, mb) and sa == sb
        unsat += int(mb.any())
    assert unsat > 0, "no frame left a tile to the second round"
    want, _, _ = oracle.render(cs, cc, idx, cam["gs_mv"].astype(np.float32), cam["gs_proj"].astype(np.float32), cam["focal"], w, h, want_f32=False)
    for img, _, _ in res["lists"]:
        pix_check("two_rounds", img, want)


def _paired_equal_synchronous(rows, path, near_permille=1000, scene=None):
    """Four poses of the 320x180 cloud drawn synchronously, then queued -- all four before the first sync() -- with GS_OPT_FRAME_BATCH 2."""
    w, h = 320, 180
    cams = [synth.index_html_camera(w, h, 50.0 * k, capi=capi) for k in range(4)]
    tag = (path, near_permille, scene is not None)
    with capi.Context(0) as c:
        force_path(c, path, near_permille)
        c.push_splat(rows)
        if scene is not None:
            c.set_scene(*scene)
        want = []
        for cam in cams:
            c.sort(cam["view"])
            want.append(c.render(capi.make_params(cam["gs_mv"], cam["gs_proj"], w, h, focal_=cam["focal"])))
            assert_path(c, path, tag)
        c.set_option(capi.OPT_FRAME_BATCH, 2)
        bufs = [capi.host_frame(h, w) for _ in cams]
        for (b, _), cam in zip(bufs, cams):
            c.sort(cam["view"], want_indices=False)
            c.render_into(capi.make_params(cam["gs_mv"], cam["gs_proj"], w, h, focal_=cam["focal"], flags=capi.RENDER_ASYNC), b)
        c.sync()
        assert_path(c, path, tag + ("paired",))
        for k, ((b, o), wnt) in enumerate(zip(bufs, want)):
            d = int(np.abs(b.astype(int) - wnt.astype(int)).max())
            print("paired vs synchronous:", tag, "pose", k, "max |dRGBA8| =", d)
            assert d == 0, (tag, k, d)
            o.free()


def test_paired_frames_equal_synchronous_ones(cloud):
    """GS_OPT_FRAME_BATCH 2: queued frames drawn two per launch equal the same frames drawn synchronously, bit for bit, on every path --
    walked, listed, sub-tile lists, pair records (the paired radix passes and k_tile_ranges) and the split blend (the paired k_blend_px)
    -- each against its own synchronous frames; walked and listed also over two binning rounds (GS_OPT_NEAR_PERMILLE 400: the share
    test_two_rounds_walk_and_lists shows leaves tiles to round 1) and with scene depth + colour set.  (Pairing
    is opportunistic -- an enqueue thread that does not see the twin frame in time draws the frame alone -- and no statistic counts
    it, so this proves the frames right whichever way they were drawn, not that they were paired.  The two-view form is no surer a way
    in: its enqueue thread gives the second view 200 us and then draws the first alone too, and it takes device outputs only, which
    render_stereo does not use.)"""
    rows = cloud[0]
    for p in ("walk", "lists", "subtile", "pairs", "split"):
        _paired_equal_synchronous(rows, p)
    g = np.random.Generator(np.random.PCG64(9))
    depth = g.uniform(0.995, 1.0, (180, 320)).astype(np.float32)
    depth[:, : 320 // 3] = 1.0
    rgba = g.integers(0, 256, (180, 320, 4)).astype(np.uint8)
    for p in ("walk", "lists"):
        _paired_equal_synchronous(rows, p, near_permille=400)
        _paired_equal_synchronous(rows, p, scene=(depth, rgba))
