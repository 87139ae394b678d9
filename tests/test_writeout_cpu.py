"""CPU tier of the write-out tests (test_writeout_gpu.py): the scene every write-out is drawn from, the frame sizes and strips, and the
proof -- on the oracle alone -- that its frames can show a misplaced write.

test_writeout_gpu.py renders into destinations that lie inside allocations pre-filled with the guard word G = 0xA5A5A5A5 and asserts that
every byte outside the documented rectangle is still G and that the rectangle holds the frame.  That says something only if
  1. no pixel of a frame IS the guard word (a pixel that was never written would pass for one that was),
  2. the frame is not constant (a row or column shifted by one would otherwise be the same image), and
  3. every tile row and every tile column holds a pixel that differs from its destination -- the background, or the scene's colour where a
     scene is set -- (a 16 x 16 tile that is never written would otherwise equal a frame that is all background there).
A fourth condition serves the two-round frames (GS_OPT_NEAR_PERMILLE 300): in every frame some pixel keeps more than 1 % transmittance behind
ALL splats, so its tile cannot saturate in the first round and the second round's write-out has to run.

The scene: 400 splats of synth.make_splat_rows, scales times 8 (large on a frame of at most 64 x 33 pixels), index.html's pose, and a
camera of FIXED focal length whose principal point is the frame's centre: every frame size sees the same cloud at the same scale."""
import functools

import numpy as np
import pytest

from conftest import pkg
from oracle import oracle

capi = pkg("capi")
synth = pkg("synth")

G = 0xA5A5A5A5
G_BYTE = 0xA5
SEED, N_SPLATS, SCALE, FOCAL = 4725, 400, 8.0, 48.0      # (the seed: the first from 4711 on whose frames meet all four conditions)
BG = (0.125, 0.25, 0.5, 1.0)
TILE = 16

HEIGHTS = (1, 15, 16, 17, 33)
WIDTHS = (1, 3, 4, 5, 15, 16, 17, 20, 33, 64)
# every width and every height at least once; both tile-ragged and tile-exact in each direction; several tiles each way
SIZES = ((1, 1), (3, 15), (4, 16), (5, 17), (15, 33), (16, 1), (17, 15), (20, 16), (33, 17), (64, 33), (16, 16), (64, 17), (33, 33), (4, 1))
SCENE_SIZES = ((1, 1), (5, 17), (16, 16), (20, 16), (33, 17), (64, 33))          # the sizes also drawn over a scene (gs_set_scene)
STRIP_FRAME = (64, 33)
# strips [x0, x1) of the 64-wide frame: x0 on and off the 4-pixel and the tile grid, widths 1, 4, 5, 16, 17 and up to the frame's edge
STRIPS = tuple((x0, x0 + d) for x0 in (0, 4, 16, 20, 3) for d in (1, 4, 5, 16, 17)) + tuple((x0, 64) for x0 in (4, 16, 20, 3)) + ((20, 63), (3, 62))
EYE_YAWS = (12.0, -9.0)                                                             # the two views of the stereo / XR cases
POSE_YAWS = (0.0, 40.0, 80.0, 120.0, 160.0, 200.0)                                  # the six poses of the frames in flight

assert {w for w, _ in SIZES} == set(WIDTHS) and {h for _, h in SIZES} == set(HEIGHTS)
assert set(SCENE_SIZES) <= set(SIZES) and STRIP_FRAME in SCENE_SIZES
assert {x1 - x0 for x0, x1 in STRIPS} >= {1, 4, 5, 16, 17} and {x0 for x0, _ in STRIPS} == {0, 4, 16, 20, 3}


class Cloud:
    def __init__(self):
        rows = synth.make_splat_rows(N_SPLATS, seed=SEED).reshape(-1, 32).copy()
        rows[:, 12:24] = (rows[:, 12:24].copy().view("<f4") * np.float32(SCALE)).view(np.uint8)
        self.rows = rows.reshape(-1)
        self.cs, self.cc, self.mats = oracle.pack(self.rows)


@functools.lru_cache(maxsize=None)
def cloud():
    return Cloud()


@functools.lru_cache(maxsize=None)
def camera(W, H, yaw=0.0):
    """index.html's pose (the camera inside the cloud) with the entity turned by `yaw`; focal length FOCAL pixels whatever the frame size,
    principal point at the frame's centre"""
    n = 0.005
    proj = synth.frustum(-0.5 * W / FOCAL * n, 0.5 * W / FOCAL * n, 0.5 * H / FOCAL * n, -0.5 * H / FOCAL * n, n, 10000.0)
    return synth.uniforms(synth.compose((0.0, 1.6, 0.0)), synth.compose((0.0, 1.5, -2.0), yaw), proj, W, H, capi=capi)


def params(W, H, x0=0, x1=None, flags=0, yaw=0.0):
    cam = camera(W, H, yaw)
    return capi.make_params(cam["gs_mv"], cam["gs_proj"], W, H, x0=x0, x1=x1, focal_=cam["focal"], background=BG, flags=flags)


@functools.lru_cache(maxsize=None)
def scene_planes(W, H):
    """the opaque scene of the frames drawn over one: window depths around the cloud's (0 on every seventh pixel of a row: nothing survives there) and a
    random colour image whose alpha byte is never the guard's"""
    g = np.random.Generator(np.random.PCG64(1000 * W + H))
    depth = g.uniform(0.997, 1.0, (H, W)).astype(np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    depth[(xx + yy) % 7 == 3] = 0.0
    rgba = g.integers(0, 256, (H, W, 4)).astype(np.uint8)
    rgba[..., 3][rgba[..., 3] == G_BYTE] = G_BYTE + 1
    depth.setflags(write=False); rgba.setflags(write=False)
    return depth, rgba


@functools.lru_cache(maxsize=None)
def order(yaw=0.0):
    o = oracle.sort(cloud().mats, camera(*STRIP_FRAME, yaw)["view"])               # (the view row does not depend on the frame size)
    o.setflags(write=False)
    return o


@functools.lru_cache(maxsize=None)
def _reference(W, H, with_scene, yaw, bg, want_f32):
    c, cam = cloud(), camera(W, H, yaw)
    depth, rgba = scene_planes(W, H) if with_scene else (None, None)
    # (the two eyes are drawn from the head camera's order, yaw 0, as gs_render_stereo and the XR frames draw them: index.js:441)
    u8, f32, _ = oracle.render(c.cs, c.cc, order(0.0 if yaw in EYE_YAWS else yaw), cam["gs_mv"].astype(np.float32), cam["gs_proj"].astype(np.float32), cam["focal"], W, H,
                               bg=bg, want_f32=want_f32, scene_depth=depth, scene_rgba=rgba)
    out = f32 if want_f32 else u8
    out.setflags(write=False)
    return out


def reference(W, H, with_scene=False, yaw=0.0):
    """oracle.render of the full W x H frame (RGBA8, row 0 = top); computed once per frame, shared and read-only"""
    return _reference(W, H, bool(with_scene), float(yaw), BG, False)


def every_frame():
    """(W, H, with_scene, yaw) of every full frame test_writeout_gpu.py draws"""
    out = [(w, h, False, 0.0) for w, h in SIZES] + [(w, h, True, 0.0) for w, h in SCENE_SIZES]
    out += [(w, h, False, y) for w, h in ((33, 17), (64, 33), (20, 16), (17, 15)) for y in EYE_YAWS + POSE_YAWS]
    return sorted(set(out))


FRAMES = every_frame()


def _words(img):
    return np.ascontiguousarray(img).view(np.uint32)[..., 0]


@pytest.mark.parametrize("W,H,with_scene,yaw", FRAMES)
def test_no_pixel_is_the_guard_word(W, H, with_scene, yaw):
    ref = reference(W, H, with_scene, yaw)
    assert ref.shape == (H, W, 4)
    assert not (_words(ref) == G).any()


@pytest.mark.parametrize("W,H,with_scene,yaw", [f for f in FRAMES if f[0] * f[1] > 1])
def test_frame_is_not_constant(W, H, with_scene, yaw):
    w = _words(reference(W, H, with_scene, yaw))
    assert len(np.unique(w)) > 1
    # a shift by one row or one column changes the image, and so does turning it upside down
    if H > 1:
        assert not np.array_equal(w[1:], w[:-1]) and not np.array_equal(w, w[::-1])
    if W > 1:
        assert not np.array_equal(w[:, 1:], w[:, :-1])


@pytest.mark.parametrize("W,H,with_scene,yaw", FRAMES)
def test_every_tile_row_and_column_is_drawn_into(W, H, with_scene, yaw):
    ref = reference(W, H, with_scene, yaw)
    if with_scene:
        dest = _words(scene_planes(W, H)[1])
    else:
        dest = np.full((H, W), _words(np.floor(np.asarray(BG, np.float32) * 255 + 0.5).astype(np.uint8).reshape(1, 1, 4))[0, 0], np.uint32)
    drawn = _words(ref) != dest
    for ty in range(0, H, TILE):
        assert drawn[ty:ty + TILE].any(), ("tile row", ty // TILE)
    for tx in range(0, W, TILE):
        assert drawn[:, tx:tx + TILE].any(), ("tile column", tx // TILE)


@pytest.mark.parametrize("W,H,with_scene,yaw", FRAMES)
def test_some_pixel_never_saturates(W, H, with_scene, yaw):
    """over a transparent black background the f32 alpha is 1 - T behind all splats: T > 1 % somewhere, ten times the blend's termination
    threshold (1/1024), so that pixel's tile is handed to the second binning round whatever the first one holds.  (A scene's depth plane
    only removes fragments: T is no smaller with one.)"""
    a = _reference(W, H, False, float(yaw), (0.0, 0.0, 0.0, 0.0), True)[..., 3]
    assert a.min() < 0.99, float(a.min())


def test_strips_are_what_the_issue_lists():
    W = STRIP_FRAME[0]
    assert all(0 <= x0 < x1 <= W for x0, x1 in STRIPS)
    assert any(x1 == W and x0 % 4 for x0, x1 in STRIPS) and any(x1 % 4 and x0 % 16 == 0 for x0, x1 in STRIPS)
    assert len(order()) > N_SPLATS // 2 and len(cloud().rows) == 32 * N_SPLATS
