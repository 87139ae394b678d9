"""GPU tier of the anti-aliased splats (GS_OPT_ANTIALIAS): the projection's compensated records against the numpy mirror of
test_antialias_cpu.py (word for word), frames against its f64 blend (1 LSB; pixels with a fragment within 1e-4 of
the q = 4 discard boundary left out -- at most 2 % of a scene, asserted on the CPU tier), and the option against every way a frame is
drawn: blend paths, strips, stereo, two binning rounds, scene inputs, strip sorts, queued and paired frames, SH, surface planes,
gs_multi.  Frames of 96x64 and 100x70 pixels, ~300 splats, fresh contexts."""
import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_antialias_cpu import bits, blend_mirror, project_mirror, record_words, scene, scene_inputs
from test_gpu_parity import assert_path, force_path
from test_sh_cpu import sh_mirror

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")
AA = capi.OPT_ANTIALIAS


def context(sc, aa, path="lists", permille=1000, opts=()):
    c = capi.Context(0)
    force_path(c, path, permille)
    for k, v in opts:
        c.set_option(k, v)
    c.set_option(AA, aa)
    c.push_splat(sc.rows)
    return c


def frame(sc, aa, path="lists", permille=1000, opts=(), x0=0, x1=None, flags=0, depth=None, rgba=None, bg=(0.0, 0.0, 0.0, 1.0)):
    with context(sc, aa, path, permille, opts) as c:
        idx = c.sort(sc.cam["view"])
        assert np.array_equal(idx, sc.idx)
        if depth is not None or rgba is not None:
            c.set_scene(depth, rgba)
        img = c.render(sc.params(x0, x1, flags=flags, background=bg))
        st = assert_path(c, path)
        assert st["antialias"] == aa
    return img, st


def close_to(tag, got, want, excl):
    d = np.abs(got.astype(int) - want.astype(int)).max(axis=2)
    print("%s: max |dRGBA8| %d outside the %d excluded pixels (%d inside), pixels off by one %.4f" % (
        tag, d[~excl].max(), excl.sum(), d[excl].max() if excl.any() else 0, (d[~excl] == 1).mean()))
    assert d[~excl].max() <= 1, tag


@pytest.fixture(scope="module")
def on_frame():
    """the 96x64 frame with the option on, on the lists path in one round: what every other way of drawing it is compared with"""
    return frame(scene(), 1)[0]


# ---------------------------------------------------------------- option and stats

def test_option_values_and_stats():
    sc = scene()
    with capi.Context(0) as c:
        for bad in (2, -1, 255):
            with pytest.raises(capi.GsError) as ei:
                c.set_option(AA, bad)
            assert ei.value.code == capi.E_BADARG
        c.push_splat(sc.rows)
        c.sort(sc.cam["view"])
        c.render(sc.params())
        assert c.stats()["antialias"] == 0                         # the default
        c.set_option(AA, 1)
        on = c.render(sc.params())
        assert c.stats()["antialias"] == 1
        c.set_option(AA, 0)
        off = c.render(sc.params())
        assert c.stats()["antialias"] == 0
        assert not np.array_equal(on, off)


# ---------------------------------------------------------------- records

@pytest.mark.parametrize("size", [(96, 64), (100, 70)])
def test_records_differ_in_the_alpha_word_only_and_equal_the_mirror(size):
    sc = scene(*size)
    got = {}
    for aa in (0, 1):
        with context(sc, aa) as c:
            idx = c.sort(sc.cam["view"])
            assert np.array_equal(idx, sc.idx)
            c.render(sc.params())
            st = c.stats()
            v = st["n_sorted"]
            tc = c.download(capi.BUF_TILE_COUNT, v, np.uint32, 1)[:, 0]
            proj = c.download(capi.BUF_PROJECTED, v, np.uint32, 8)
            c.render(sc.params(flags=capi.RENDER_COUNT_FRAGS))
            got[aa] = (tc, proj, st["n_visible"], st["n_pairs"], c.stats()["n_frags"])
    (tc0, p0, vis0, pairs0, fr0), (tc1, p1, vis1, pairs1, fr1) = got[0], got[1]
    assert np.array_equal(tc0, tc1) and (vis0, pairs0, fr0) == (vis1, pairs1, fr1)
    live = tc0 > 0
    assert live.sum() > 200 and vis0 == live.sum() and fr0 > 0
    assert np.array_equal(p0[live][:, :7], p1[live][:, :7])                   # every word but the alpha float
    assert (p0[live][:, 7] != p1[live][:, 7]).mean() > 0.9
    for aa, p in ((0, p0), (1, p1)):
        want = record_words(sc.pm, aa)[sc.idx][live]
        assert np.array_equal(p[live], want), (aa, int((p[live] != want).any(axis=1).sum()))
    zero = p1[live][:, 7] == 0
    assert zero.sum() >= 3 and (tc1[live][zero] > 0).all()                    # c = 0: written, counted and binned all the same


# ---------------------------------------------------------------- pixels

@pytest.mark.parametrize("size", [(96, 64), (100, 70)])
def test_frames_against_the_f64_blend_on_and_off(size):
    sc = scene(*size)
    imgs = {}
    for aa in (1, 0):
        want, excl = sc.blend(bool(aa))
        for flags in (capi.RENDER_NO_EARLY_OUT, 0):
            img, _ = frame(sc, aa, flags=flags)
            close_to("%dx%d aa %d flags %d" % (sc.W, sc.H, aa, flags), img, want, excl)
            imgs[(aa, flags)] = img
    assert (imgs[(1, 0)] != imgs[(0, 0)]).any(axis=2).mean() > 0.2            # a test that can tell on from off


# ---------------------------------------------------------------- every path

@pytest.mark.parametrize("path", ["walk", "subtile", "pairs", "split"])
def test_blend_paths(on_frame, path):
    img, _ = frame(scene(), 1, path)
    if path == "split":
        assert np.abs(img.astype(int) - on_frame.astype(int)).max() <= 1
    else:
        assert np.array_equal(img, on_frame)


def test_ragged_frame_paths_agree():
    sc = scene(100, 70)
    ref, _ = frame(sc, 1)
    for path in ("walk", "subtile", "pairs"):
        assert np.array_equal(frame(sc, 1, path)[0], ref), path


def test_strip_stereo_two_rounds_and_strip_sort(on_frame):
    sc = scene()
    assert np.array_equal(frame(sc, 1, x0=16, x1=64)[0], on_frame[:, 16:64])
    for path in ("lists", "walk"):                                            # the second binning round runs and changes nothing
        img, st = frame(sc, 1, path, permille=300)
        assert st["unsat_tiles"] > 0 and np.array_equal(img, on_frame), path
    # stereo: one sort, two eyes (the second eye half a unit to the right); each eye equals that eye drawn alone
    mv2 = sc.cam["gs_mv"].copy()
    mv2[12] += 0.01
    eye2 = capi.make_params(mv2, sc.cam["gs_proj"], sc.W, sc.H, focal_=sc.cam["focal"])
    with context(sc, 1) as c:
        c.sort(sc.cam["view"])
        left, right = c.render_stereo(sc.params(), eye2)
        assert c.stats()["antialias"] == 1
        alone = c.render(eye2)
    assert np.array_equal(left, on_frame) and np.array_equal(right, alone) and not np.array_equal(left, right)
    # a strip's own sort (gs_sort_for) draws the pixels of the full order
    with context(sc, 1) as c:
        strip = sc.params(32, 80)
        sub = c.sort_for(sc.cam["view"], None, strip)
        assert len(sub) <= len(sc.idx)
        assert np.array_equal(c.render(strip), on_frame[:, 32:80])


def test_scene_depth_and_colour():
    sc = scene()
    depth, rgba = scene_inputs(sc)
    want, excl = sc.blend(True, scene_depth=depth, scene_rgba=rgba)
    img, _ = frame(sc, 1, depth=depth, rgba=rgba)
    close_to("scene", img, want, excl)
    assert np.array_equal(frame(sc, 1, "walk", depth=depth, rgba=rgba)[0], img)
    plain, _ = sc.blend(True)
    assert (want != plain).any(axis=2).mean() > 0.2                           # the scene inputs matter


# ---------------------------------------------------------------- asynchronous frames

def test_option_switched_between_queued_paired_frames():
    sc = scene()
    poses = []
    for k in range(4):
        mv = sc.cam["gs_mv"].copy()
        mv[12] += 0.004 * k                                                   # (the view row, and so the order, stays)
        poses.append(capi.make_params(mv, sc.cam["gs_proj"], sc.W, sc.H, focal_=sc.cam["focal"]))
    want = {}
    for aa in (0, 1):
        with context(sc, aa, "lists", permille=0) as c:
            c.sort(sc.cam["view"])
            for k, p in enumerate(poses):
                want[(aa, k)] = c.render(p)
    assert not np.array_equal(want[(0, 1)], want[(1, 1)]) and not np.array_equal(want[(1, 0)], want[(1, 1)])
    frames = [capi.host_frame(sc.H, sc.W) for _ in range(12)]
    with capi.Context(0) as c:
        c.set_option(capi.OPT_PIPELINE_DEPTH, 3)
        c.set_option(capi.OPT_FRAME_BATCH, 2)
        c.push_splat(sc.rows)
        setting = []
        for f in range(12):
            if f == 4:
                c.set_option(AA, 1)
            if f == 8:
                c.set_option(AA, 0)
            setting.append(1 if 4 <= f < 8 else 0)
            p = poses[f % 4]
            p.flags = capi.RENDER_ASYNC
            c.sort(sc.cam["view"], want_indices=False)
            c.render_into(p, frames[f][0])
        c.sync()
        st = c.stats()
        print("retried frames:", st["retried_frames"])
    for f in range(12):
        assert np.array_equal(frames[f][0], want[(setting[f], f % 4)]), (f, setting[f])
    for p in poses:
        p.flags = 0
    for _, owner in frames:
        owner.free()


# ---------------------------------------------------------------- with SH

def test_with_view_dependent_colour():
    sc = scene()
    rows = sc.rows.reshape(-1, 32)
    scales = rows[:, 12:24].copy().view("<f4")
    rows = rows[(scales > 0).all(axis=1)]                                     # (a .ply stores log scales)
    n = len(rows)
    rest = np.random.default_rng(5).standard_normal((n, 45)).astype(np.float32) * np.float32(0.35)
    ply = synth.rows_to_inria_ply(rows.copy(), rest)
    conv = capi.ply_to_splat(ply).reshape(-1, 32)
    sh3, d = capi.ply_sh(ply, 3)
    assert d == 3 and len(conv) == n
    cs, cc, mats = oracle.pack(conv.reshape(-1))
    pm = project_mirror(cs, cc, sc.mv, sc.pr, sc.cam["focal"], sc.W, sc.H)
    idx = oracle.sort(mats, sc.cam["view"])
    pos = conv[:, 0:12].copy().view("<f4").reshape(n, 3)
    cam_obj = capi.camera_in_object(sc.mv) * np.array([1.0, 1.0, -1.0])
    rgb = sh_mirror(sh3.reshape(n, 3, 16), 2, cam_obj, pos)
    rec = {}
    for key, deg, aa in (("both", 2, 1), ("sh", 2, 0), ("aa", 0, 1)):
        with capi.Context(0) as c:
            force_path(c, "lists")
            c.set_option(capi.OPT_SH_DEGREE, deg)
            c.set_option(AA, aa)
            c.load_ply(ply)
            assert np.array_equal(c.sort(sc.cam["view"]), idx)
            img = c.render(sc.params())
            st = c.stats()
            assert (st["sh_degree"], st["antialias"]) == (deg, aa)
            live = c.download(capi.BUF_TILE_COUNT, st["n_sorted"], np.uint32, 1)[:, 0] > 0
            rec[key] = (c.download(capi.BUF_PROJECTED, st["n_sorted"], np.uint32, 8)[live], live, img)
    both, sh, aa = rec["both"], rec["sh"], rec["aa"]
    assert np.array_equal(both[1], sh[1]) and np.array_equal(both[1], aa[1])
    assert np.array_equal(both[0][:, 6], sh[0][:, 6]) and (both[0][:, 6] != aa[0][:, 6]).any()      # SH colour bytes
    assert np.array_equal(both[0][:, 7], aa[0][:, 7]) and (both[0][:, 7] != sh[0][:, 7]).any()      # compensated alpha
    assert np.array_equal(both[0][:, 7], record_words(pm, True)[idx][both[1]][:, 7])
    want, excl = blend_mirror(pm, idx, sc.W, sc.H, True, rgb=rgb)
    assert excl.mean() <= 0.02
    close_to("sh2 + aa", both[2], want, excl)


# ---------------------------------------------------------------- surface

def test_surface_planes_and_pick():
    sc = scene()
    clear = (0.0, 0.0, 0.0, 0.0)
    planes = {}
    for aa in (1, 0):
        with context(sc, aa) as c:
            c.sort(sc.cam["view"])
            p = sc.params(background=clear)
            plain = c.render(p)
            img, sid, dep, alpha = c.render_surface(p)
            st = c.stats()
            assert st["surface"] == 1 and st["antialias"] == aa
            assert np.array_equal(img, plain)
            # the colour's alpha byte is the alpha plane, rounded (include/gs_splat.h)
            assert np.array_equal(np.floor(alpha * np.float32(255.0) + np.float32(0.5)).astype(np.uint8), img[:, :, 3])
            hit = np.argwhere(sid != capi.SURFACE_NONE)
            assert len(hit) > 50
            # (this scene is dense: with the option off every pixel has a surface; "none" pixels are picked too where there are any)
            none = np.argwhere(sid == capi.SURFACE_NONE)
            pts = [(int(x), int(y)) for y, x in list(hit[:: max(1, len(hit) // 6)][:6]) + list(none[:1])] + [(0, 0), (sc.W - 1, sc.H - 1)]
            for (x, y), h in zip(pts, c.pick(sc.params(background=clear), pts)):
                assert h["id"] == sid[y, x], (x, y)
                assert bits(h["depth"]) == bits(dep[y, x]) and bits(h["alpha"]) == bits(alpha[y, x])
            planes[aa] = sid
    assert (planes[1] != planes[0]).any(), "the compensated transmittance crosses one half later somewhere"


# ---------------------------------------------------------------- gs_multi

def test_two_contexts_of_one_process(on_frame):
    sc = scene()
    fr, owner = capi.host_frame(sc.H, sc.W)
    with capi.Multi([0, 0]) as m:
        for opt, v in ((capi.OPT_NEAR_PERMILLE, 1000), (capi.OPT_BINNING, 0), (capi.OPT_ROW_WALK, 0), (capi.OPT_SUBTILE, 0), (AA, 1)):
            m.set_option(opt, v)                                              # through gs_multi_set_option
        m.push_splat(sc.rows)
        m.sort(sc.cam["view"], None, sc.params())
        m.render(sc.params(), fr)
        assert [m.ctx_stats(i)["antialias"] for i in range(2)] == [1, 1]
    assert np.array_equal(fr, on_frame)
    owner.free()
