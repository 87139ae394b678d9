"""GPU tier of the surface output: gs_render_surface / gs_pick against the numpy mirror of the definition (test_surface_cpu.py, which
also proves on the CPU that at most 3 % of the pixels of every scene used here are undecided) and against themselves: colour
untouched, the crossing at batch edges, "none", two binning rounds, pair records, strips and orientation, scene depth, random scenes,
options that must not leak, and gs_pick.  Fresh contexts throughout; frames of 64x48 to 100x70 pixels."""
import numpy as np
import pytest

from conftest import pkg
from test_gpu_parity import force_path
from test_surface_cpu import (BATCH_EDGES, INNER, NONE, SYNTH_SEEDS, batch_scene, half_depth, mirror, synth_scene, window_depth)

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")


def surface(scene, permille=1000, opts=(), x0=0, x1=None, flags=0, depth=None, rgba=None, plain=False):
    """(rgba, id, depth, alpha), order, stats of a surface frame on a fresh context on the lists path (plain: gs_render instead)"""
    with capi.Context(0) as c:
        force_path(c, "lists", permille)
        for k, v in opts:
            c.set_option(k, v)
        if len(scene.rows):
            c.push_splat(scene.rows)
        idx = c.sort(scene.cam["view"])
        if depth is not None or rgba is not None:
            c.set_scene(depth, rgba)
        p = scene.params(x0, x1, flags=flags)
        out = (c.render(p), None, None, None) if plain else c.render_surface(p)
        return out, idx, c.stats()


def same_planes(a, b, tag=""):
    for x, y, n in zip(a[1:], b[1:], ("id", "depth", "alpha")):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (tag, n, int((x.view(np.uint32) != y.view(np.uint32)).sum()))


@pytest.fixture(scope="module")
def s65():
    return batch_scene(65)


@pytest.fixture(scope="module")
def big():
    """the 100x70 scene of the strip tests: a synth cloud (ragged right and bottom edges, several tiles each way)"""
    return synth_scene(21, 100, 70)


# 1 ---------------------------------------------------------------- colour untouched
@pytest.mark.parametrize("size", [(64, 48), (100, 70)])
@pytest.mark.parametrize("with_scene", [False, True])
def test_colour_is_gs_renders(size, with_scene):
    sc = synth_scene(31, *size)
    g = np.random.default_rng(3)
    depth = rgba = None
    if with_scene:
        depth = np.where(g.random((sc.H, sc.W)) < 0.5, np.float32(0.99), np.float32(1.0)).astype(np.float32)
        rgba = g.integers(0, 256, (sc.H, sc.W, 4)).astype(np.uint8)
    for permille in (1000, 400):
        got, _, st = surface(sc, permille, depth=depth, rgba=rgba)
        want, _, st0 = surface(sc, permille, depth=depth, rgba=rgba, plain=True)
        assert st["surface"] == 1 and st0["surface"] == 0
        assert np.array_equal(got[0], want[0]), (size, with_scene, permille)
        assert got[0].any()


def test_colour_is_gs_renders_with_sh():
    rows = synth.make_splat_rows(400, seed=77).reshape(-1, 32).copy()
    rows[:, 12:24] = (rows[:, 12:24].copy().view("<f4") * np.float32(6.0)).view(np.uint8)
    rest = np.random.default_rng(78).standard_normal((400, 45)).astype(np.float32) * np.float32(0.35)
    ply = synth.rows_to_inria_ply(rows, rest)
    cam = synth.index_html_camera(64, 48, 30.0, capi=capi)
    p = capi.make_params(cam["gs_mv"], cam["gs_proj"], 64, 48, focal_=cam["focal"])
    out = []
    for surf in (True, False):
        with capi.Context(0) as c:
            force_path(c, "lists")
            c.set_option(capi.OPT_SH_DEGREE, 3)
            c.load_ply(ply)
            c.sort(cam["view"])
            out.append(c.render_surface(p)[0] if surf else c.render(p))
            assert c.stats()["sh_degree"] == 3
    assert np.array_equal(out[0], out[1]) and out[0].any()


# 2 ---------------------------------------------------------------- where the crossing is found
@pytest.mark.parametrize("k", BATCH_EDGES)
def test_crossing_at_batch_edges(k):
    sc = batch_scene(k)
    (_, sid, dep, alpha), idx, _ = surface(sc)
    assert (sid[INNER] == k - 1).all(), (k, np.unique(sid[INNER]))
    assert (dep[INNER].view(np.uint32) == window_depth(sc, k - 1).view(np.uint32)).all()
    m_id, m_dep, m_alpha, und = mirror(sc, idx)
    assert np.array_equal(sid[~und], m_id[~und]) and np.array_equal(dep[~und], m_dep[~und])
    assert np.abs(alpha - m_alpha).max() <= 1.0 / 1024 + len(idx) * 2.0 ** -21


# 3 ---------------------------------------------------------------- none
def test_none_values():
    sc = batch_scene(100, 0, opaque=False)                          # 99 faint splats: T stays above one half
    (_, sid, dep, alpha), idx, _ = surface(sc)
    assert (sid == NONE).all() and (dep == np.float32(1.0)).all()
    assert alpha[INNER].min() > 0.1 and alpha.max() < 0.45
    assert (alpha[:, 48:] == 0.0).all() and (alpha[40:, :] == 0.0).all()       # uncovered pixels: 0xFFFFFFFF / 1.0 / 0.0
    empty = batch_scene(1, 0, opaque=False)
    assert len(empty.rows) == 0
    (img, sid, dep, alpha), _, st = surface(empty)
    assert st["surface"] == 1
    assert (sid == NONE).all() and (dep == np.float32(1.0)).all() and (alpha == 0.0).all()
    assert (img == np.array([0, 0, 0, 255], np.uint8)).all()


# 4, 5 ------------------------------------------------------------- two rounds; pair records
@pytest.mark.parametrize("k", (65, 129))
def test_two_rounds_equal_one(k):
    sc = batch_scene(k)
    want, _, _ = surface(sc)
    tx, ty = (sc.W + 15) // 16, (sc.H + 15) // 16
    for permille in (3, 400):
        with capi.Context(0) as c:
            force_path(c, "lists", permille)
            c.push_splat(sc.rows)
            c.sort(sc.cam["view"])
            got = c.render_surface(sc.params())
            mask = c.download(capi.BUF_UNSAT_MASK, ty, np.uint32, (tx + 31) // 32)
            st = c.stats()
        assert int(np.ceil(permille / 1000.0 * (k + 5))) < k, "the opaque splat lies beyond the near share"
        assert mask.any() and (mask[1, 0] >> 1) & 1, "round 1 ran for the tile under test"
        print("permille %d: unsat_tiles %d" % (permille, st["unsat_tiles"]))
        assert np.array_equal(got[0], want[0])
        same_planes(got, want, permille)
        assert (got[1][INNER] == k - 1).all()


def test_pair_records_equal_span_lists(s65, big):
    for sc in (s65, big):
        want, _, st0 = surface(sc)
        got, _, st = surface(sc, opts=((capi.OPT_BINNING, 1),))
        assert st0["binning"] == 0 and st["binning"] == 1 and st["surface"] == 1
        same_planes(got, want)
        got, _, st = surface(sc, 400, opts=((capi.OPT_BINNING, 1),))
        same_planes(got, want, "two rounds")


# 6 ---------------------------------------------------------------- strips and orientation
def test_strips_flip_and_null_planes(big):
    full, idx, _ = surface(big)
    assert (full[1] != NONE).any() and (full[1] == NONE).any()
    m_id, m_dep, m_alpha, und = mirror(big, idx)                    # the frame the strips are compared with, against the mirror
    assert und.mean() <= 0.03
    assert np.array_equal(full[1][~und], m_id[~und]) and np.array_equal(full[2][~und].view(np.uint32), m_dep[~und].view(np.uint32))
    assert np.abs(full[3] - m_alpha).max() <= 1.0 / 1024 + len(idx) * 2.0 ** -21
    for x0, x1 in ((0, 52), (52, 100), (36, 37)):
        got, _, _ = surface(big, x0=x0, x1=x1)
        assert got[1].shape == (70, x1 - x0)
        same_planes(got, tuple(None if a is None else a[:, x0:x1] for a in full), (x0, x1))
        assert np.array_equal(got[0], full[0][:, x0:x1])
    flip, _, _ = surface(big, flags=capi.RENDER_FLIP_Y)
    same_planes(flip, tuple(a[::-1] for a in full), "flip")
    # a NULL plane is not written, and its neighbours in one allocation stay what they were (device planes between sentinels)
    hip = capi.hip_runtime()
    import ctypes as C
    n = 100 * 70
    words = 3 * n + 4 * 64
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), words * 4) == 0
    try:
        sentinel = np.full(words, 0xA5A5A5A5, np.uint32)
        offs = [64, 128 + n, 192 + 2 * n]                           # 256-byte aligned planes, 64 sentinel words around each
        for skip in range(3):
            assert hip.hipMemcpy(buf, sentinel.ctypes.data_as(C.c_void_p), words * 4, 1) == 0
            ptrs = [None if k == skip else buf.value + 4 * offs[k] for k in range(3)]
            with capi.Context(0) as c:
                force_path(c, "lists")
                c.push_splat(big.rows)
                c.sort(big.cam["view"])
                c.render_surface_device(big.params(), None, *ptrs)
            back = np.zeros(words, np.uint32)
            assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), buf, words * 4, 2) == 0
            keep = np.ones(words, bool)
            for k in range(3):
                if k != skip:
                    keep[offs[k]:offs[k] + n] = False
                    assert np.array_equal(back[offs[k]:offs[k] + n], full[1 + k].view(np.uint32).ravel()), (skip, k)
            assert (back[keep] == 0xA5A5A5A5).all(), skip
    finally:
        hip.hipFree(buf)
    with capi.Context(0) as c:                                       # host planes: only the ones asked for
        force_path(c, "lists")
        c.push_splat(big.rows)
        c.sort(big.cam["view"])
        img, sid, dep, alp = c.render_surface(big.params(), rgba=False, planes=("depth",))
        assert img is None and sid is None and alp is None and np.array_equal(dep, full[2])


# 7 ---------------------------------------------------------------- scene depth
def test_scene_depth_moves_the_surface(s65):
    k = 65
    z = half_depth(s65, k)
    want, idx, _ = surface(s65)
    got, _, _ = surface(s65, depth=z)
    sid, dep = got[1], got[2]
    right = (slice(20, 28), slice(24, 28))
    left = (slice(20, 28), slice(20, 24))
    assert (sid[right] == k - 1).all() and np.array_equal(dep[right], want[2][right])
    # (what lies behind the opaque splat lies behind the scene's depth too: that half has no surface, only the faint stack's alpha)
    assert (sid[left] == NONE).all() and (dep[left] == np.float32(1.0)).all() and (got[3][left] > 0).all()
    m_id, m_dep, m_alpha, und = mirror(s65, idx, scene_depth=z)
    assert np.array_equal(sid[~und], m_id[~und]) and np.array_equal(dep[~und], m_dep[~und])
    for permille in (3, 400):
        two, _, _ = surface(s65, permille, depth=z)
        same_planes(two, got, permille)


# 8 ---------------------------------------------------------------- random scenes against the mirror
@pytest.mark.parametrize("seed", SYNTH_SEEDS)
def test_random_scenes_against_the_mirror(seed):
    sc = synth_scene(seed)
    for flags, slack in ((0, 1.0 / 1024), (capi.RENDER_NO_EARLY_OUT, 0.0)):
        (_, sid, dep, alpha), idx, _ = surface(sc, flags=flags)
        m_id, m_dep, m_alpha, und = mirror(sc, idx)
        assert und.mean() <= 0.03
        bad = (sid != m_id) & ~und
        assert not bad.any(), (seed, int(bad.sum()))
        assert np.array_equal(dep[~und].view(np.uint32), m_dep[~und].view(np.uint32))
        err = np.abs(alpha - m_alpha).max()
        print("seed %d flags %d: undecided %.4f, max |alpha - mirror| %.3g, surfaces %.3f" % (seed, flags, und.mean(), err, (sid != NONE).mean()))
        assert err <= slack + len(idx) * 2.0 ** -21
    two, _, _ = surface(sc, 400)
    one, _, _ = surface(sc)
    same_planes(two, one, "two rounds")


# 9 ---------------------------------------------------------------- options do not leak
@pytest.mark.parametrize("opt,val,stat", [(capi.OPT_ROW_WALK, 2, "row_walk"), (capi.OPT_SUBTILE, 2, "subtile"),
                                          (capi.OPT_BLEND_SPLIT, 1, None), (capi.OPT_FRAME_BATCH, 2, None)])
def test_options_do_not_leak(big, opt, val, stat):
    """(the row walk's context also switches the adaptive sub-tile lists off, as test_gpu_parity.PATH_OPTIONS does: with small splats
    GS_OPT_SUBTILE 1 takes every frame after the first collected one, and sub-tile lists keep the tile lists by design)"""
    with capi.Context(0) as c:
        c.push_splat(big.rows)
        c.sort(big.cam["view"])
        want = c.render_surface(big.params())
    with capi.Context(0) as c:
        c.set_option(opt, val)
        if opt == capi.OPT_ROW_WALK:
            c.set_option(capi.OPT_SUBTILE, 0)
        c.push_splat(big.rows)
        c.sort(big.cam["view"])
        before = c.render(big.params())
        st_b = c.stats()
        got = c.render_surface(big.params())
        st = c.stats()
        after = c.render(big.params())
        st_a = c.stats()
    same_planes(got, want, opt)
    assert st["surface"] == 1 and st["row_walk"] == 0 and st["subtile"] == 0
    assert st_b["surface"] == 0 and st_a["surface"] == 0
    if stat:
        assert st_b[stat] == 1 and st_a[stat] == 1
    assert np.array_equal(before, after)
    if opt != capi.OPT_BLEND_SPLIT:                                  # (the split blend's colour is within 1 LSB, not bit-identical)
        assert np.array_equal(got[0], before)


# 10 --------------------------------------------------------------- gs_pick
def test_pick(big):
    full, idx, _ = surface(big)
    sid = full[1]
    none = np.argwhere(sid == NONE)
    assert len(none)
    pts = [(0, 0), (15, 15), (16, 16), (99, 0), (99, 69), (0, 69), (96, 64), (int(none[0][1]), int(none[0][0]))]
    hit_any = np.argwhere(sid != NONE)
    pts.append((int(hit_any[len(hit_any) // 2][1]), int(hit_any[len(hit_any) // 2][0])))
    pos = big.rows.reshape(-1, 32)[:, 0:12].copy().view("<f4").reshape(-1, 3)
    with capi.Context(0) as c:
        c.push_splat(big.rows)
        c.sort(big.cam["view"])
        hits = c.pick(big.params(), pts)
        assert c.stats()["surface"] == 1
        assert len(c.pick(big.params(), np.zeros((0, 2), np.int32))) == 0
        for bad in ([(100, 0)], [(0, 70)], [(-1, 3)], [(5, 5), (5, -1)]):
            with pytest.raises(capi.GsError) as ei:
                c.pick(big.params(), bad)
            assert ei.value.code == capi.E_BADARG and "outside" in ei.value.message
        for call in (lambda p: c.pick(p, pts), c.render_surface):
            with pytest.raises(capi.GsError) as ei:
                call(big.params(flags=capi.RENDER_COUNT_FRAGS))
            assert ei.value.code == capi.E_BADARG and "COUNT_FRAGS" in ei.value.message
        c.render_surface(big.params(flags=capi.RENDER_NO_EARLY_OUT))
    assert (hits["id"] != NONE).sum() >= 1 and (hits["id"] == NONE).sum() >= 1
    for (x, y), h in zip(pts, hits):
        assert h["id"] == sid[y, x], (x, y)
        assert h["depth"].view(np.uint32) == full[2][y, x].view(np.uint32) and h["alpha"].view(np.uint32) == full[3][y, x].view(np.uint32)
        if h["id"] == NONE:
            assert np.isnan(h["pos"]).all()
        else:
            assert np.array_equal(h["pos"].view(np.uint32), pos[h["id"]].view(np.uint32)), (x, y)
    with capi.Context(0) as c:                                       # a context fed with worker rows only can sort, not pick
        c.push_matrices(big.mats)
        c.sort(big.cam["view"])
        with pytest.raises(capi.GsError) as ei:
            c.pick(big.params(), pts)
        assert ei.value.code == capi.E_STATE
