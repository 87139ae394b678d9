"""GPU tier: tile and sub-tile coverage on tilted, thin, clamped and grazing splats, through every form that consumes it.  The CPU
tier (test_coverage_cpu.py) sweeps the coverage arithmetic with an emulated 1-ulp reciprocal and square root; here the same shapes
run on the hardware's own v_rcp_f32 / v_sqrt_f32, and a tile or 4x4 block the binning leaves out shows as a fragment count below the
oracle's -- the forms of the binning share the code, so agreement among them proves nothing about it.

Scenes are built from 32-byte .splat rows by tilted(): an identity pose and a symmetric frustum, scales (long, short, 1e-4 short) and
a rotation about the view axis in the quantised, un-normalised quaternion bytes, so the drawn ellipse differs a little from the one
asked for: the oracle is the truth, not the construction.
  fan         160 x 128 and 333 x 211: splats 150-400 px long, about 3 px wide (the 0.3 px^2 dilation's floor), at 1, 10, 30, 45, 60,
              89, 90, 135 and 179 degrees, centred on tile corners, on pixel centres and up to a tenth of the frame outside it; one
              at exactly 0 degrees, which has no eigenvector in the reference's projection and is invisible.
  clamps      256 x 256: splats whose long axis sits on the 1024 clamp near 45 and 135 degrees (their runs are wider than the frame
              in every row; the 16-bit covariances of such a splat carry an error of several px^2, which puts the short axis of some of
              them on the 0.1 clamp: both are asserted), thin mid-sized ones, and the smallest splats there are -- half extents of about
              1.8 by 1.55 px, the dilation's floor; a round one has no eigenvector and is invisible -- on tile corners, block corners
              and pixel centres.
  dense thin  64 x 64: 48 short thin tilted splats through each of three tiles, each reaching a few 4x4 blocks, so that every staged
              batch is split into block lists (proven: fewer entries walked with GS_OPT_SUBTILE 2 than with 0 on those tiles).

Measured on one MI355X: 17 tests in 1.3 s of wall time, the slowest (six paths of the clamps scene) 0.3 s; ~130 fresh contexts, the
oracle drawing only the strips under test, once each.  What these tests found: a counting frame of a strip whose width is no multiple
of 4 counted the up to three pixels the blend works on beyond x1 (docs/LAB_NOTES.md 9i); fixed in k_blend_body."""
import math

import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_blend_paths_gpu import Scene, compare_paths, draw, list_lengths, tile_lengths
from test_gpu_parity import PATH_OPTIONS, assert_path, force_path, pix_check

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

PATHS = ("lists", "segc", "pairs", "walk", "subtile", "split")      # the first five bit-identical, split within 1 LSB
COUNTING = ("segc", "lists", "pairs", "subtile")                     # (walk and split cannot count fragments)
PALETTE = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255), (255, 128, 0), (255, 255, 255)]
assert set(PATHS) <= set(PATH_OPTIONS)


# ---------------------------------------------------------------- constructed scenes

def sym_camera(W, H):
    """Identity pose, symmetric frustum, focal = the longer side (at least 64)."""
    f, n = float(max(W, H, 64)), 0.005
    proj = synth.frustum(-0.5 * W / f * n, 0.5 * W / f * n, 0.5 * H / f * n, -0.5 * H / f * n, n, 10000.0)
    return synth.uniforms(synth.compose((0.0, 0.0, 0.0)), synth.compose((0.0, 0.0, 0.0)), proj, W, H, capi=capi)


def tilted(cam, cx, cy, long_px, short_px, deg, depth, rgba):
    """One .splat row centred at image pixel (cx, cy) (top-down rows) whose |p| <= 2 ellipse is asked to be long_px by short_px pixels
    with its long axis at deg degrees (no less than the 0.3 px^2 dilation leaves of it: 3.1 px)."""
    W, H, gp, f = cam["vw"], cam["vh"], cam["gs_proj"], cam["focal"]
    X = (2.0 * cx / W - 1.0 + gp[8]) * depth / gp[0]
    Y = (2.0 * (H - cy) / H - 1.0 + gp[9]) * depth / gp[5]
    # full extent = 2 * 2 sqrt(2 (cov + 0.3)); a screen variance below 0.0025 px^2 would not survive the sort at any alpha
    sl, ss = (math.sqrt(max((e / 4.0) ** 2 / 2.0 - 0.3, 0.0025)) * depth / f for e in (long_px, short_px))
    # the depth sort keeps a splat only if max(scale) * alpha > 1e-4 * depth (index.js:397, 548): alpha is raised to what keeps it
    a = max(int(rgba[3]), int(math.ceil(255.0 * 1.5e-4 * depth / max(sl, ss))))
    assert a <= 255, "splat too small to survive the sort"
    h = math.radians(deg) / 2.0
    r = np.zeros(32, np.uint8)
    r[0:12] = np.array([X, Y, depth], "<f4").view(np.uint8)
    r[12:24] = np.array([sl, ss, 1e-4 * ss], "<f4").view(np.uint8)
    r[24:28] = (rgba[0], rgba[1], rgba[2], a)
    r[28:32] = (128 + int(round(127 * math.cos(h))), 128, 128, 128 + int(round(127 * math.sin(h))))
    return r


class TiltScene(Scene):
    """test_blend_paths_gpu.Scene with the symmetric camera; oracle frames are drawn once per strip."""

    def __init__(self, W, H, rows):
        Scene.__init__(self, W, H, rows)
        self.cam = sym_camera(W, H)
        self._drawn = {}

    def oracle(self, idx, x0=0, x1=None, **kw):
        key = (x0, x1 or self.W, tuple(kw.get("bg", ())), idx.tobytes())
        if key not in self._drawn:
            self._drawn[key] = Scene.oracle(self, idx, x0, x1, **kw)
        return self._drawn[key]


def _centres(W, H, g, n):
    """tile corners, pixel centres and points up to a tenth of the frame outside it, on every side"""
    out = []
    for k in range(n):
        kind = k % 4
        if kind == 0:
            out.append((16.0 * int(g.integers(0, W // 16 + 1)), 16.0 * int(g.integers(0, H // 16 + 1))))
        elif kind == 1:
            out.append((int(g.integers(0, W)) + 0.5, int(g.integers(0, H)) + 0.5))
        elif kind == 2:
            side = (k // 4) % 4
            ux, uy = float(g.uniform(0.0, 0.1 * W)), float(g.uniform(0.0, 0.1 * H))
            out.append([(-ux, float(g.uniform(0, H))), (W + ux, float(g.uniform(0, H))), (float(g.uniform(0, W)), -uy), (float(g.uniform(0, W)), H + uy)][side])
        else:
            out.append((float(g.uniform(0, W)), float(g.uniform(0, H))))
    return out


def fan_scene(W, H):
    g = np.random.Generator(np.random.PCG64(W * 1000 + H))
    cam = sym_camera(W, H)
    angles = [1.0, 10.0, 30.0, 45.0, 60.0, 89.0, 90.0, 135.0, 179.0]
    rows = []
    for k, (cx, cy) in enumerate(_centres(W, H, g, 12 * len(angles))):
        rows.append(tilted(cam, cx, cy, 150.0 + (k * 37) % 251, 1.0 + k % 3, angles[k % len(angles)], 2.0 + 0.004 * k,
                           PALETTE[k % len(PALETTE)] + (150 + (k * 7) % 71,)))
    rows.append(tilted(cam, W / 2.0, H / 2.0 + 0.5, 200.0, 2.0, 0.0, 1.9, (255, 255, 255, 220)))     # exactly 0 degrees: the last row
    return TiltScene(W, H, rows)


def clamps_scene():
    W = H = 256
    g = np.random.Generator(np.random.PCG64(256))
    cam = sym_camera(W, H)
    rows, k = [], 0

    def put(cx, cy, lp, sp, deg):
        nonlocal k
        rows.append(tilted(cam, cx, cy, lp, sp, deg, 2.0 + 0.004 * k, PALETTE[k % len(PALETTE)] + (150 + (k * 7) % 71,)))
        k += 1

    for i, (cx, cy) in enumerate(_centres(W, H, g, 24)):                      # the 1024 clamp: 4096 px long
        put(cx, cy, 6000.0 + 500.0 * (i % 5), 1.0, [45.0, 44.0, 135.0, 46.0, 134.0, 45.5][i % 6])
    for i, (cx, cy) in enumerate(_centres(W, H, g, 24)):                      # thin, a few tiles long
        put(cx, cy, 40.0 + 9.0 * (i % 7), 1.0, [45.0, 30.0, 135.0, 60.0, 10.0, 89.0][i % 6])
    for ty in range(0, 17, 4):                                                # the smallest splats: on tile corners ...
        for tx in range(0, 17, 4):
            put(16.0 * tx, 16.0 * ty, 4.0, 1.0, 45.0)                        # (a round one has no eigenvector: invisible)
    for i in range(60):                                                       # ... block corners, pixel centres and just off them
        bx, by = int(g.integers(1, 64)), int(g.integers(1, 64))
        off = [(0.0, 0.0), (0.5, 0.5), (1e-3, -1e-3), (0.5 + 1e-3, 0.5), (0.0, 0.5)][i % 5]
        put(4.0 * bx + off[0], 4.0 * by + off[1], 3.6 + 0.4 * (i % 3), 1.0, [45.0, 135.0, 20.0, 90.0][i % 4])
    return TiltScene(W, H, rows)


DENSE_TILES = [(1, 1), (2, 3), (0, 3)]                                        # (tile column, tile row) of the 64 x 64 frame


def dense_scene():
    W = H = 64
    g = np.random.Generator(np.random.PCG64(64))
    cam = sym_camera(W, H)
    rows, k = [], 0
    for tx, ty in DENSE_TILES:
        for i in range(48):
            cx, cy = 16.0 * tx + float(g.uniform(1.0, 15.0)), 16.0 * ty + float(g.uniform(1.0, 15.0))
            rows.append(tilted(cam, cx, cy, 6.0 + i % 4, 1.0, [20.0, 45.0, 70.0, 110.0, 135.0, 160.0][i % 6], 2.0 + 0.004 * k,
                               PALETTE[k % len(PALETTE)] + (150 + (k * 7) % 71,)))
            k += 1
    return TiltScene(W, H, rows)


@pytest.fixture(scope="module")
def scenes():
    return {"fan160": fan_scene(160, 128), "fan333": fan_scene(333, 211), "clamps": clamps_scene(), "dense": dense_scene()}


VIEWS = {"fan160": [(0, None), (37, 118), (64, 80)], "fan333": [(0, None), (21, 300), (320, 333)],
         "clamps": [(0, None), (37, 240), (149, 165)], "dense": [(0, None), (5, 43), (19, 35)]}
NAMES = sorted(VIEWS)


# ---------------------------------------------------------------- what is checked

def surely_touched(o, W, H, x0, x1):
    """Tiles of the strip that hold a pixel centre which passes q <= 4 whatever the rounding: q in f64 from the oracle's f32 record,
    less a margin above the f32 evaluation's error.  (Each of the four products carries one rounding and dx, dy one more, each sum
    another: under 4 u (|dx ax| + |dy ay|) on ppx with u = 2^-24, likewise ppy; q = ppx^2 + ppy^2 with |pp| <= 2 then moves by less
    than 2 * 2 * 4 u (Tx + Ty) + 3 u q < 1e-6 (Tx + Ty + 4).)  A lower bound of the truth, which is what a '>=' needs."""
    xs = (np.arange(x0, x1, dtype=np.float64) + 0.5) - float(o.cx)
    ys = (np.arange(0, H, dtype=np.float64) + 0.5) - float(o.cy)                 # GL rows, bottom-up
    dx, dy = np.meshgrid(xs, ys)
    ax, ay, bx, by = float(o.ax), float(o.ay), float(o.bx), float(o.by)
    ppx, ppy = dx * ax + dy * ay, dx * bx + dy * by
    margin = 1e-6 * (np.abs(dx * ax) + np.abs(dy * ay) + np.abs(dx * bx) + np.abs(dy * by) + 4.0)
    jj, ii = np.nonzero(ppx * ppx + ppy * ppy <= 4.0 - margin)
    return len(set(zip(((H - 1 - jj) // 16).tolist(), (ii // 16).tolist())))


def project_all(scene, idx):
    c = scene.cam
    mv, P, focal = c["gs_mv"].astype(np.float32), c["gs_proj"].astype(np.float32), np.float32(c["focal"])
    return [oracle.project(scene.cs, scene.cc, int(i), mv, P, focal, scene.W, scene.H) for i in idx]


@pytest.mark.parametrize("name", NAMES)
def test_every_path_draws_the_oracles_frame(scenes, name):
    """lists, segc, pairs, walk and subtile bit-identical, split within 1 LSB, the first within the oracle's bar: the whole frame, a
    strip at an odd offset and width, and a 16-pixel strip."""
    compare_paths(scenes[name], VIEWS[name], paths=PATHS, tag="coverage_" + name)


@pytest.mark.parametrize("name", NAMES)
def test_fragment_counts_equal_the_oracles(scenes, name):
    """The superset proof on the hardware's reciprocal and square root: a counting frame counts exactly the oracle's fragments."""
    scene = scenes[name]
    idx = oracle.sort(scene.mats, scene.cam["view"])
    for p in COUNTING:
        with capi.Context(0) as c:
            force_path(c, p)
            c.push_splat(scene.rows)
            assert np.array_equal(c.sort(scene.cam["view"]), idx)
            for x0, x1 in VIEWS[name]:
                c.render(scene.params(x0, x1, flags=capi.RENDER_COUNT_FRAGS))
                st = assert_path(c, p, (name, x0, x1))
                want = scene.oracle(idx, x0, x1)[1]
                print("fragments", name, p, x0, x1, st["n_frags"], want)
                assert st["n_frags"] == want, (name, p, x0, x1, st["n_frags"], want)
                assert want > 0


@pytest.mark.parametrize("name", NAMES)
def test_records_counts_and_tile_lists_against_the_oracle(scenes, name):
    """n_sorted and n_visible against oracle.sort / oracle.project; the projected records of the visible positions bit-equal; per sorted
    position GS_BUF_TILE_COUNT no less than the tiles that surely hold a passing pixel; span lists and pair records of equal lengths."""
    scene = scenes[name]
    W, H = scene.W, scene.H
    idx = oracle.sort(scene.mats, scene.cam["view"])
    proj = project_all(scene, idx)
    n_clamp_long = n_clamp_short = 0
    with capi.Context(0) as c:
        force_path(c, "lists")
        c.push_splat(scene.rows)
        assert np.array_equal(c.sort(scene.cam["view"]), idx)
        for x0, x1 in VIEWS[name]:
            x1 = x1 or W
            c.render(scene.params(x0, x1))
            st = assert_path(c, "lists", (name, x0, x1))
            V = idx.size
            assert st["n_sorted"] == V
            rec = c.download(capi.BUF_PROJECTED, V, np.float32, 8)
            cnt = c.download(capi.BUF_TILE_COUNT, V, np.uint32, 1).reshape(-1)
            touched_any = 0
            for j, o in enumerate(proj):
                if not o.visible:
                    assert cnt[j] == 0, (name, j)
                    continue
                need = surely_touched(o, W, H, x0, x1)
                touched_any += need > 0
                assert cnt[j] >= need, (name, x0, x1, j, int(cnt[j]), need)
                if cnt[j]:
                    want = np.array([o.cx, o.cy, o.ax, o.ay, o.bx, o.by], np.float32)
                    assert np.array_equal(rec[j, :6].view(np.uint32), want.view(np.uint32)), (name, j)
                    assert rec[j, 7] == np.float32(o.alpha)
            assert st["n_visible"] == int((cnt > 0).sum())
            assert touched_any <= st["n_visible"] <= sum(1 for o in proj if o.visible)
            assert touched_any > 0
    for x0, x1 in VIEWS[name]:
        assert np.array_equal(list_lengths(scene, "lists", x0, x1), list_lengths(scene, "pairs", x0, x1)), (name, x0, x1)
    if name.startswith("fan"):
        # the splat at exactly 0 degrees (the last row) is invisible in the oracle -- and, above, in the library
        last = int(np.nonzero(idx == len(scene.rows) // 32 - 1)[0][0])
        assert not proj[last].visible
        assert sum(1 for o in proj if o.visible) == idx.size - 1
    if name == "clamps":
        for o in proj:
            if o.visible:
                n_clamp_long += math.hypot(o.v1x, o.v1y) >= 1023.99
                n_clamp_short += abs(math.hypot(o.v2x, o.v2y) - math.sqrt(0.2)) < 1e-4
        assert n_clamp_long >= 12 and n_clamp_short >= 3, (n_clamp_long, n_clamp_short)


@pytest.mark.parametrize("name", NAMES)
def test_two_binning_rounds_draw_the_same_frame(scenes, name):
    """GS_OPT_NEAR_PERMILLE 400 and 3 against 1000, span lists and sub-tile lists: round 1's run emit sees the same runs against the mask."""
    scene = scenes[name]
    for p in ("lists", "subtile"):
        ref, idx, _ = draw(scene, p, VIEWS[name])
        for permille in (400, 3):
            got, i2, _ = draw(scene, p, VIEWS[name], opts=((capi.OPT_NEAR_PERMILLE, permille),))
            assert np.array_equal(i2, idx)
            for v, a, b in zip(VIEWS[name], ref, got):
                assert np.array_equal(a, b), (name, p, permille, v)


def test_dense_thin_batches_are_split_and_nothing_changes(scenes):
    """The sub-tile split really happens on the chosen tiles (fewer entries walked: GS_OPT_RECORD_STAGED 2, GS_BUF_TILE_STATS column 0),
    counting frames with evaluated fragments and frames without early termination agree between GS_OPT_SUBTILE 0 and 2, and one pair
    of queued frames (GS_OPT_FRAME_BATCH 2) equals the synchronous frames."""
    scene = scenes["dense"]
    W, H = scene.W, scene.H
    res = {}
    for mode in (0, 2):
        with capi.Context(0) as c:
            force_path(c, "subtile" if mode else "lists")
            c.push_splat(scene.rows)
            idx = c.sort(scene.cam["view"])
            c.set_option(capi.OPT_RECORD_STAGED, 2)
            c.render(scene.params())
            stats = c.download(capi.BUF_TILE_STATS, (W // 16) * (H // 16), np.uint32, 2).reshape(H // 16, W // 16, 2)
            assert np.array_equal(stats[..., 1], tile_lengths(c, scene))
            c.set_option(capi.OPT_RECORD_STAGED, 0)
            c.render(scene.params(flags=capi.RENDER_COUNT_FRAGS | capi.RENDER_COUNT_EVALUATED))
            evaluated = c.stats()["n_frags"]
            plain = c.render(scene.params())
            full = c.render(scene.params(flags=capi.RENDER_NO_EARLY_OUT))
            c.set_option(capi.OPT_FRAME_BATCH, 2)
            bufs = [capi.host_frame(H, W) for _ in range(2)]
            for b, _ in bufs:
                c.sort(scene.cam["view"], want_indices=False)
                c.render_into(scene.params(flags=capi.RENDER_ASYNC), b)
            c.sync()
            for b, o in bufs:
                assert np.array_equal(b, plain), mode
                o.free()
            res[mode] = (stats, evaluated, plain, full)
    for tx, ty in DENSE_TILES:
        assert res[0][0][ty, tx, 1] >= 40 and res[2][0][ty, tx, 1] == res[0][0][ty, tx, 1]
        print("dense thin tile", (tx, ty), "list", int(res[0][0][ty, tx, 1]), "walked", int(res[0][0][ty, tx, 0]), "->", int(res[2][0][ty, tx, 0]))
        assert res[2][0][ty, tx, 0] < res[0][0][ty, tx, 0], (tx, ty)
    assert res[0][1] == res[2][1] and res[0][1] > 0
    assert np.array_equal(res[0][2], res[2][2]) and np.array_equal(res[0][3], res[2][3])
    pix_check("coverage_dense_no_early_out", res[2][3], scene.oracle(idx)[0])
