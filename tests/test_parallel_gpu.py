"""GPU tier of the parallel-projection cameras (GS_RENDER_PARALLEL): the projection kernel's records against the numpy mirror of
test_parallel_cpu.py (word for word), frames against its f64 blend (1 LSB; pixels with a fragment within 1e-4 of the q = 4 discard
boundary left out -- at most 2 % of a frame, asserted on the CPU tier), and the flag against every way a frame is drawn or a
projection is consumed: blend paths, strips, two binning rounds, stereo, scene inputs, FLIP_Y, surface planes, gs_pick, contribution
frames, screen-space selections, strip sorts, queued and paired frames, SH + anti-aliasing + highlight, gs_multi.  ~300 splats, frames
of 96x64 and 100x70 pixels, fresh contexts."""
import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_antialias_cpu import bits, blend_mirror, project_mirror, record_words
from test_gpu_parity import assert_path, force_path
from test_parallel_cpu import PAR, project_mirror_parallel, scene, scene_inputs
from test_sh_cpu import sh_mirror

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")
f32 = np.float32
SELECTED = capi.STATE_SELECTED


def context(sc, path="lists", permille=1000, opts=()):
    c = capi.Context(0)
    force_path(c, path, permille)
    for k, v in opts:
        c.set_option(k, v)
    c.push_splat(sc.rows)
    return c


def frame(sc, path="lists", permille=1000, parallel=True, x0=0, x1=None, flags=0, depth=None, rgba=None, bg=(0.0, 0.0, 0.0, 1.0)):
    with context(sc, path, permille) as c:
        idx = c.sort(sc.cam["view"])
        assert np.array_equal(idx, sc.idx)
        if depth is not None or rgba is not None:
            c.set_scene(depth, rgba)
        img = c.render(sc.params(x0, x1, flags=flags, parallel=parallel, background=bg))
        st = assert_path(c, path)
        assert c.projection_info() == (1 if parallel else 0)
    return img, st


def close_to(tag, got, want, excl):
    d = np.abs(got.astype(int) - want.astype(int)).max(axis=2)
    print("%s: max |dRGBA8| %d outside the %d excluded pixels (%d inside), pixels off by one %.4f" % (
        tag, d[~excl].max(), excl.sum(), d[excl].max() if excl.any() else 0, (d[~excl] == 1).mean()))
    assert d[~excl].max() <= 1, tag


@pytest.fixture(scope="module")
def par_frame():
    """the 96x64 parallel frame on the lists path in one round: what every other way of drawing it is compared with"""
    return frame(scene())[0]


def coverage_of(pm, W, H):
    """(must, may) per row.  must: a pixel centre of the frame lies inside the drawn ellipse with room to spare (q <= 3.99 in f64); may:
    the ellipse's bounding box plus one pixel meets the frame.  The tile ranges are a padded superset of the true coverage by contract
    (gs_device_math.h: ellipse_rows_setup), so a splat between the two may or may not be counted; outside `may` it never is."""
    fx = (np.arange(W) + 0.5)[None, :]
    fy = (H - 1 - np.arange(H) + 0.5)[:, None]
    n = len(pm["cx"])
    must, may = np.zeros(n, bool), np.zeros(n, bool)
    v1x, v1y, v2x, v2y = (np.asarray(a, np.float64) for a in pm["v"])
    for i in np.nonzero(pm["visible"])[0]:
        cx, cy = float(pm["cx"][i]), float(pm["cy"][i])
        hw, hh = 2.0 * np.hypot(v1x[i], v2x[i]) + 1.0, 2.0 * np.hypot(v1y[i], v2y[i]) + 1.0
        may[i] = cx + hw >= 0 and cx - hw <= W and cy + hh >= 0 and cy - hh <= H
        if may[i]:
            dx, dy = fx - cx, fy - cy
            q = (dx * float(pm["ax"][i]) + dy * float(pm["ay"][i])) ** 2 + (dx * float(pm["bx"][i]) + dy * float(pm["by"][i])) ** 2
            must[i] = (q <= 3.99).any()
    return must, may


# ---------------------------------------------------------------- records

@pytest.mark.parametrize("size", [(96, 64), (100, 70)])
def test_records_equal_the_mirror_and_coverage_follows_it(size):
    sc = scene(*size)
    must, may = coverage_of(sc.pm, sc.W, sc.H)
    with context(sc) as c:
        assert np.array_equal(c.sort(sc.cam["view"]), sc.idx)
        assert c.projection_info() == 0
        c.render(sc.params())
        assert c.projection_info() == 1
        v = c.stats()["n_sorted"]
        tc = c.download(capi.BUF_TILE_COUNT, v, np.uint32, 1)[:, 0]
        proj = c.download(capi.BUF_PROJECTED, v, np.uint32, 8)
        live = tc > 0
        want = record_words(sc.pm, False)[sc.idx]
        print("%dx%d: live %d, must %d, may %d" % (sc.W, sc.H, live.sum(), must[sc.idx].sum(), may[sc.idx].sum()))
        assert live.sum() >= 190 and c.stats()["n_visible"] == live.sum()
        assert np.array_equal(proj[live], want[live]), int((proj[live] != want[live]).any(axis=1).sum())
        assert (live >= must[sc.idx]).all() and (live <= may[sc.idx]).all()
        assert (may[sc.idx] & ~must[sc.idx]).sum() <= 0.05 * live.sum()       # (the band in between is thin: the test decides nearly every splat)
        # the same scene without the flag: the perspective mirror, as before
        c.render(sc.params(parallel=False))
        assert c.projection_info() == 0
        tc0 = c.download(capi.BUF_TILE_COUNT, v, np.uint32, 1)[:, 0]
        proj0 = c.download(capi.BUF_PROJECTED, v, np.uint32, 8)
        want0 = record_words(sc.pm_persp, False)[sc.idx]
        assert (tc0 > 0).sum() >= 150 and np.array_equal(proj0[tc0 > 0], want0[tc0 > 0])
        both = live & (tc0 > 0)
        assert (proj[both][:, 2:6] != proj0[both][:, 2:6]).any(axis=1).mean() > 0.95


def test_perspective_matrix_with_the_flag_is_refused():
    sc = scene()
    persp = synth.perspective(80.0, sc.W / sc.H)
    bad = capi.make_params(sc.cam["gs_mv"], capi.projection_matrix(persp), sc.W, sc.H, flags=PAR)
    with context(sc) as c:
        c.sort(sc.cam["view"])
        calls = [lambda: c.render(bad), lambda: c.render_surface(bad), lambda: c.render_contrib(bad), lambda: c.render_stereo(sc.params(), bad),
                 lambda: c.pick(bad, [(1, 1)]), lambda: c.select_rect(bad, (0, 0, 8, 8), set_bits=SELECTED),
                 lambda: c.select_mask(bad, np.ones((sc.H, sc.W), np.uint8), set_bits=SELECTED),
                 lambda: c.sort_for(sc.cam["view"], None, bad), lambda: c.sort_gathered(sc.cam["view"], None, bad)]
        for k, call in enumerate(calls):
            with pytest.raises(capi.GsError) as e:
                call()
            assert e.value.code == capi.E_BADARG, k
        assert "bottom row" in str(e.value) or "PARALLEL" in str(e.value)
        bad.flags = 0
        c.sort(sc.cam["view"])
        c.render(bad)                                                # without the flag the matrix is a camera like any other
        assert c.projection_info() == 0
    with capi.Multi([0, 0]) as m:
        m.push_splat(sc.rows)
        bad.flags = PAR
        with pytest.raises(capi.GsError) as e:
            m.sort(sc.cam["view"], None, bad)
        assert e.value.code == capi.E_BADARG


# ---------------------------------------------------------------- pixels

@pytest.mark.parametrize("size", [(96, 64), (100, 70)])
def test_frames_against_the_f64_blend(size):
    sc = scene(*size)
    imgs = {}
    for parallel in (True, False):
        want, excl = sc.blend(parallel)
        for flags in (capi.RENDER_NO_EARLY_OUT, 0):
            img, _ = frame(sc, parallel=parallel, flags=flags)
            close_to("%dx%d parallel %d flags %d" % (sc.W, sc.H, parallel, flags), img, want, excl)
            imgs[(parallel, flags)] = img
    assert (imgs[(True, 0)] != imgs[(False, 0)]).any(axis=2).mean() > 0.2


@pytest.mark.parametrize("path", ["walk", "subtile", "pairs", "split"])
def test_blend_paths(par_frame, path):
    img, _ = frame(scene(), path)
    print(path, "max |dRGBA8| against the lists frame:", np.abs(img.astype(int) - par_frame.astype(int)).max())
    assert np.array_equal(img, par_frame)


def test_ragged_frame_paths_agree():
    sc = scene(100, 70)
    ref, _ = frame(sc)
    for path in ("walk", "subtile", "pairs"):
        assert np.array_equal(frame(sc, path)[0], ref), path


def test_strips_two_rounds_flip_and_stereo(par_frame):
    sc = scene()
    for x0, x1 in ((16, 64), (4, 37), (32, 96), (0, 50)):
        assert np.array_equal(frame(sc, x0=x0, x1=x1)[0], par_frame[:, x0:x1]), (x0, x1)
    for path in ("lists", "walk"):                                            # the second binning round runs and changes nothing
        img, st = frame(sc, path, permille=300)
        assert st["unsat_tiles"] > 0 and np.array_equal(img, par_frame), path
    assert np.array_equal(frame(sc, flags=capi.RENDER_FLIP_Y)[0], par_frame[::-1])
    # stereo: one sort, one eye parallel and one perspective; each equals that eye drawn alone
    with context(sc) as c:
        c.sort(sc.cam["view"])
        left, right = c.render_stereo(sc.params(), sc.params(parallel=False))
        assert c.projection_info() == 0                                       # (the last eye drawn)
        alone = c.render(sc.params(parallel=False))
        right2, left2 = c.render_stereo(sc.params(parallel=False), sc.params())
        assert c.projection_info() == 1
    assert np.array_equal(left, par_frame) and np.array_equal(right, alone) and not np.array_equal(left, right)
    assert np.array_equal(left2, par_frame) and np.array_equal(right2, alone)


def test_scene_depth_and_colour():
    sc = scene()
    depth, rgba = scene_inputs(sc)
    want, excl = sc.blend(scene_depth=depth, scene_rgba=rgba)
    img, _ = frame(sc, depth=depth, rgba=rgba)
    close_to("scene", img, want, excl)
    assert np.array_equal(frame(sc, "walk", depth=depth, rgba=rgba)[0], img)
    plain, _ = sc.blend()
    assert (want != plain).any(axis=2).mean() > 0.2


# ---------------------------------------------------------------- surface, pick, contribution

def test_surface_pick_and_contribution(par_frame):
    sc = scene()
    with context(sc) as c:
        c.sort(sc.cam["view"])
        p = sc.params()
        img, sid, dep, alpha = c.render_surface(p)
        assert c.stats()["surface"] == 1 and c.projection_info() == 1
        assert np.array_equal(img, par_frame)
        hit = np.argwhere(sid != capi.SURFACE_NONE)
        none = np.argwhere(sid == capi.SURFACE_NONE)
        assert len(hit) > 50
        # the planes hold the mirror's numbers: the surface splat's window depth
        zwin = (sc.pm["zndc"] * f32(0.5) + f32(0.5))
        ys, xs = hit[:, 0], hit[:, 1]
        assert np.array_equal(bits(dep[ys, xs]), bits(zwin[sid[ys, xs]]))
        pts = [(int(x), int(y)) for y, x in list(hit[:: max(1, len(hit) // 6)][:6]) + list(none[:1])] + [(0, 0), (sc.W - 1, sc.H - 1)]
        for (x, y), h in zip(pts, c.pick(sc.params(), pts)):
            assert h["id"] == sid[y, x], (x, y)
            assert bits(h["depth"]) == bits(dep[y, x]) and bits(h["alpha"]) == bits(alpha[y, x])
        assert np.array_equal(c.render_contrib(p), par_frame) and c.projection_info() == 1
        seen = c.download_contrib()
        assert (seen[sc.idx[sc.pm["visible"][sc.idx]]] > 0).sum() > 100
        # ... and the perspective planes of the same params differ
        _, sid0, _, _ = c.render_surface(sc.params(parallel=False))
        assert (sid0 != sid).mean() > 0.05


# ---------------------------------------------------------------- selection

def rect_rule(pm, idx, W, H, rect):
    x0, y0, x1, y1 = rect
    px, py = np.floor(pm["cx"][idx]), f32(H - 1) - np.floor(pm["cy"][idx])
    return pm["visible"][idx] & (px >= x0) & (px < x1) & (py >= y0) & (py < y1)


def test_select_rect_and_mask_follow_the_parallel_centres():
    sc = scene()
    rect = (20, 10, 70, 50)
    want = rect_rule(sc.pm, sc.idx, sc.W, sc.H, rect)
    persp = capi.projection_matrix(synth.perspective(80.0, sc.W / sc.H))
    pmp = project_mirror(sc.cs, sc.cc, sc.mv, persp.astype(f32), (sc.H / 2.0) * abs(float(f32(persp[5]))), sc.W, sc.H)
    want_persp = rect_rule(pmp, sc.idx, sc.W, sc.H, rect)
    assert want.sum() > 40 and want_persp.sum() > 5 and (want != want_persp).sum() > 20
    with context(sc) as c:
        c.sort(sc.cam["view"])
        assert c.select_rect(sc.params(), rect, set_bits=SELECTED) == want.sum()
        st = c.download_state()
        exp = np.zeros(sc.n, np.uint8)
        exp[sc.idx[want]] = SELECTED
        assert np.array_equal(st, exp)
        # a perspective camera selects a frustum: another set for the same rectangle
        c.set_state(0, np.zeros(sc.n, np.uint8))
        c.sort(sc.cam["view"])
        assert c.select_rect(capi.make_params(sc.cam["gs_mv"], persp, sc.W, sc.H), rect, set_bits=SELECTED) == want_persp.sum()
        exp = np.zeros(sc.n, np.uint8)
        exp[sc.idx[want_persp]] = SELECTED
        assert np.array_equal(c.download_state(), exp)
        # a mask with the surface's depth plane: what is visible under a disc
        c.set_state(0, np.zeros(sc.n, np.uint8))
        c.sort(sc.cam["view"])
        _, sid, dep, _ = c.render_surface(sc.params())
        yy, xx = np.mgrid[0:sc.H, 0:sc.W]
        mask = (((xx - 50) ** 2 + (yy - 30) ** 2) < 27 ** 2).astype(np.uint8)
        fx, fy = np.floor(sc.pm["cx"][sc.idx]), np.floor(sc.pm["cy"][sc.idx])
        inside = sc.pm["visible"][sc.idx] & (fx >= 0) & (fx < sc.W) & (fy >= 0) & (fy < sc.H)
        col, row = np.where(inside, fx, 0).astype(int), np.where(inside, sc.H - 1 - fy, 0).astype(int)
        zwin = (sc.pm["zndc"] * f32(0.5) + f32(0.5))[sc.idx]
        in_mask = inside & (mask[row, col] != 0)
        want_m = in_mask & (zwin <= dep[row, col])
        assert 10 < want_m.sum() < in_mask.sum()
        c.sort(sc.cam["view"])
        assert c.select_mask(sc.params(), mask, dep, set_bits=SELECTED) == want_m.sum()
        exp = np.zeros(sc.n, np.uint8)
        exp[sc.idx[want_m]] = SELECTED
        assert np.array_equal(c.download_state(), exp)


# ---------------------------------------------------------------- sorts

def test_strip_sorts_keep_every_splat(par_frame):
    sc = scene()
    with context(sc) as c:
        strip = sc.params(32, 80)
        assert np.array_equal(c.sort_for(sc.cam["view"], None, strip), sc.idx)
        assert np.array_equal(c.render(strip), par_frame[:, 32:80])
        whole = sc.params()
        assert np.array_equal(c.sort_for(sc.cam["view"], None, whole), sc.idx)
        assert np.array_equal(c.render(whole), par_frame)
        c.sort_gathered(sc.cam["view"], None, whole)
        c.render_gathered(whole)
        assert np.array_equal(c.read_gathered(0, sc.W, sc.H), par_frame)


# ---------------------------------------------------------------- queued, paired frames

def test_flag_switched_between_queued_paired_frames():
    sc = scene()
    kinds = [True, True, False, True]                                         # parallel, parallel, perspective, parallel
    poses = []
    for k in range(4):
        mv = sc.cam["gs_mv"].copy()
        mv[12] += 0.04 * k                                                    # (the view row, and so the order, stays)
        poses.append(capi.make_params(mv, sc.cam["gs_proj"], sc.W, sc.H, focal_=sc.cam["focal"], flags=PAR if kinds[k] else 0))
    want = []
    with context(sc, "lists", permille=0) as c:
        c.sort(sc.cam["view"])
        for p in poses:
            want.append(c.render(p))
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[3])
    frames = [capi.host_frame(sc.H, sc.W) for _ in range(12)]
    with capi.Context(0) as c:
        c.set_option(capi.OPT_PIPELINE_DEPTH, 3)
        c.set_option(capi.OPT_FRAME_BATCH, 2)
        c.push_splat(sc.rows)
        for f in range(12):
            p = poses[f % 4]
            p.flags |= capi.RENDER_ASYNC
            c.sort(sc.cam["view"], want_indices=False)
            c.render_into(p, frames[f][0])
        c.sync()
        print("retried frames:", c.stats()["retried_frames"])
    for f in range(12):
        assert np.array_equal(frames[f][0], want[f % 4]), f
    for _, owner in frames:
        owner.free()


# ---------------------------------------------------------------- with SH, anti-aliasing and highlight

def test_with_view_dependent_colour_antialiasing_and_highlight():
    sc = scene()
    rows = sc.rows.reshape(-1, 32)
    n = len(rows)
    rest = np.random.default_rng(5).standard_normal((n, 45)).astype(np.float32) * np.float32(0.35)
    ply = synth.rows_to_inria_ply(rows.copy(), rest)
    conv = capi.ply_to_splat(ply).reshape(-1, 32)
    sh3, d = capi.ply_sh(ply, 3)
    assert d == 3 and len(conv) == n
    cs, cc, mats = oracle.pack(conv.reshape(-1))
    pm = project_mirror_parallel(cs, cc, sc.mv, sc.pr, sc.W, sc.H)
    idx = oracle.sort(mats, sc.cam["view"])
    pos = conv[:, 0:12].copy().view("<f4").reshape(n, 3)
    cam_obj = capi.camera_in_object(sc.mv) * np.array([1.0, 1.0, -1.0])
    rgb = sh_mirror(sh3.reshape(n, 3, 16), 3, cam_obj, pos).astype(np.uint32)
    hl = capi.highlight_option((255, 32, 200), 160)
    states = np.where(np.arange(n) % 3 == 0, SELECTED, 0).astype(np.uint8)
    word = (cc[:, 3] & np.uint32(0xFF000000)) | rgb[:, 0] | (rgb[:, 1] << 8) | (rgb[:, 2] << 16)
    word = np.where(states == SELECTED, capi.highlight_word(word, hl), word).astype(np.uint32)
    want = record_words(pm, True)
    want[:, 6] = word
    with capi.Context(0) as c:
        force_path(c, "lists")
        c.set_option(capi.OPT_SH_DEGREE, 3)
        c.set_option(capi.OPT_ANTIALIAS, 1)
        c.load_ply(ply)
        c.set_state(0, states)
        c.set_option(capi.OPT_HIGHLIGHT, hl)
        assert np.array_equal(c.sort(sc.cam["view"]), idx)
        img = c.render(sc.params())
        st = c.stats()
        assert (st["sh_degree"], st["antialias"]) == (3, 1) and c.highlight_info() == (hl, 1) and c.projection_info() == 1
        live = c.download(capi.BUF_TILE_COUNT, st["n_sorted"], np.uint32, 1)[:, 0] > 0
        rec = c.download(capi.BUF_PROJECTED, st["n_sorted"], np.uint32, 8)[live]
    assert live.sum() >= 190
    w = want[idx][live]
    assert np.array_equal(rec[:, :6], w[:, :6]) and np.array_equal(rec[:, 7], w[:, 7])
    assert np.array_equal(rec[:, 6], w[:, 6]), int((rec[:, 6] != w[:, 6]).sum())
    plain = record_words(pm, False)[idx][live]
    assert (rec[:, 6] != plain[:, 6]).mean() > 0.9 and (rec[:, 7] != plain[:, 7]).mean() > 0.5
    wimg, excl = blend_mirror(pm, idx, sc.W, sc.H, True, rgb=np.stack([word & 0xFF, (word >> 8) & 0xFF, (word >> 16) & 0xFF], 1))
    assert excl.mean() <= 0.02
    close_to("sh3 + aa + hl", img, wimg, excl)


# ---------------------------------------------------------------- gs_multi

def test_two_contexts_of_one_process(par_frame):
    sc = scene()
    fr, owner = capi.host_frame(sc.H, sc.W)
    with capi.Multi([0, 0]) as m:
        for opt, v in ((capi.OPT_NEAR_PERMILLE, 1000), (capi.OPT_BINNING, 0), (capi.OPT_ROW_WALK, 0), (capi.OPT_SUBTILE, 0)):
            m.set_option(opt, v)
        m.push_splat(sc.rows)
        m.sort(sc.cam["view"], None, sc.params())
        m.render(sc.params(), fr)
        assert [m.ctx_projection_info(i) for i in range(2)] == [1, 1]
        assert np.array_equal(fr, par_frame)
        # the flag may also come with the call, for all views
        m.sort(sc.cam["view"], None, sc.params(parallel=False))
        m.render(sc.params(parallel=False), fr, flags=PAR)
        assert np.array_equal(fr, par_frame)
        m.sort(sc.cam["view"], None, sc.params(parallel=False))
        m.render(sc.params(parallel=False), fr)
        assert [m.ctx_projection_info(i) for i in range(2)] == [0, 0] and not np.array_equal(fr, par_frame)
    owner.free()
