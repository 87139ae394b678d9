"""GPU tier of the per-splat contribution: gs_render_contrib and GS_PROP_SEEN against the numpy mirror (test_contrib_cpu.py, which also
asserts on the CPU that the comparison is sharp for the scenes used here), against gs_render / gs_render_surface, and against
themselves: the exact equalities the integer sums promise.  Fresh contexts throughout; frames of 64x48 to 100x70 pixels."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
from test_antialias_cpu import project_mirror
from test_contrib_cpu import CONTRIB_SEEDS, every_scene, mirror, mirror_of, tolerance
from test_gpu_parity import force_path
from test_surface_cpu import batch_scene, synth_scene, window_depth

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

STRIPS = ((0, 16), (16, 52), (52, 100))


def contrib(scene, permille=1000, opts=(), views=((0, None),), flags=0, depth=None, rgba=None, hide=None, plain=False):
    """([rgba per view], store u64[gs_count()], order, (rows, frames), stats) of contribution frames (plain: gs_render) on a fresh context on the lists"""
    with capi.Context(0) as c:
        force_path(c, "lists", permille)
        for k, v in opts:
            c.set_option(k, v)
        if len(scene.rows):
            c.push_splat(scene.rows)
        if hide is not None:
            c.set_state(0, hide)
        idx = c.sort(scene.cam["view"])
        if depth is not None or rgba is not None:
            c.set_scene(depth, rgba)
        imgs = []
        for x0, x1 in views:
            p = scene.params(x0, x1, flags=flags)
            imgs.append(c.render(p) if plain else c.render_contrib(p))
        return imgs, full_store(c), idx, c.contrib_info(), c.stats()


def full_store(c):
    """the store padded with the zeros of the splats beyond it"""
    s = np.zeros(c.count(), np.uint64)
    d = c.download_contrib()
    s[:len(d)] = d
    return s


@pytest.fixture(scope="module")
def big():
    return synth_scene(21, 100, 70)


@pytest.fixture(scope="module")
def big_store(big):
    _, store, _, info, _ = contrib(big)
    assert info == (len(big.rows) // 32, 1) and store.any()
    return store


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
        got, store, _, info, st = contrib(sc, permille, depth=depth, rgba=rgba)
        want, store0, _, info0, _ = contrib(sc, permille, depth=depth, rgba=rgba, plain=True)
        assert np.array_equal(got[0], want[0]), (size, with_scene, permille)
        assert got[0].any() and store.any() and info[1] == 1
        assert info0 == (0, 0) and not store0.any(), "a context that never draws a contribution frame has no store"
        assert st["surface"] == 0 and st["row_walk"] == 0 and st["subtile"] == 0


def test_a_later_plain_frame_is_what_it_is_without_the_call(big):
    """with the path pinned: the later frame and its statistics are those of a context that never made the call.  With the default,
    adaptive options a contribution frame is a collected frame like any other -- the hints the next frame adapts to (sub-tile lists,
    the measured share) are what gs_render of the same frame leaves: compared with a context that drew that instead."""
    keys = ("n_sorted", "n_visible", "n_pairs", "n_tiles", "unsat_tiles", "near_permille", "binning", "row_walk", "subtile", "surface", "seg_count", "n_runs", "sh_degree")
    for pinned in (True, False):
        out = []
        for with_call in (True, False):
            with capi.Context(0) as c:
                if pinned:
                    force_path(c, "lists", 400)
                else:
                    c.set_option(capi.OPT_NEAR_PERMILLE, 400)
                c.push_splat(big.rows)
                c.sort(big.cam["view"])
                if with_call:
                    c.render_contrib(big.params(), want_rgba=False)
                elif not pinned:
                    c.render(big.params())
                img = c.render(big.params())
                st = c.stats()
                out.append((img, {k: st[k] for k in keys}))
        assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1], (pinned, out[0][1], out[1][1])


# 2 ---------------------------------------------------------------- against the mirror
@pytest.mark.parametrize("case", every_scene(), ids=lambda c: c[0])
def test_against_the_mirror(case):
    name, sc, sdepth, kinds = case
    worst = 0.0
    for early in kinds:                                             # (test_contrib_cpu.every_scene: which kind of frame a scene is compared as)
        flags = 0 if early else capi.RENDER_NO_EARLY_OUT
        _, store, idx, info, _ = contrib(sc, flags=flags, depth=sdepth)
        Wt, cover, edge_n, _ = mirror_of(name, sc, sdepth, idx)
        tol = tolerance(len(idx), cover, edge_n, early)
        dev = np.abs(store.astype(np.float64) / 65536.0 - Wt)
        ratio = float((dev / np.maximum(tol, 1e-300))[cover > 0].max()) if (cover > 0).any() else 0.0
        worst = max(worst, ratio)
        print("%s early=%d: worst deviation / tol %.4f, sum store %.2f px, sum W %.2f px, splats with weight %d of %d" % (
            name, early, ratio, store.sum() / 65536.0, Wt.sum(), int((store > 0).sum()), len(store)))
        assert (dev <= tol).all(), (name, early, int(np.argmax(dev - tol)), float(dev.max()))
        assert info == (len(store), 1 if len(store) else 0)
        if name == "empty":
            assert len(store) == 0
    if name.startswith(("batch", "front")) and name[5:].isdigit():
        k = int(name[5:])
        assert store[k - 1] > 100 * 65536, "the opaque splat at slot %d of its tile's list holds most of the weight" % (k - 1)
    if name == "faint":
        assert (store > 0).all() and store.max() < 2 * 65536


# 3 ---------------------------------------------------------------- conservation, GPU against GPU
@pytest.mark.parametrize("seed", CONTRIB_SEEDS)
def test_conservation(seed):
    sc = synth_scene(seed)
    _, store, _, _, _ = contrib(sc)
    with capi.Context(0) as c:
        force_path(c, "lists")
        c.push_splat(sc.rows)
        c.sort(sc.cam["view"])
        alpha = c.render_surface(sc.params(), rgba=False, planes=("alpha",))[3]
    with capi.Context(0) as c:
        force_path(c, "lists")
        c.push_splat(sc.rows)
        c.sort(sc.cam["view"])
        c.render(sc.params(flags=capi.RENDER_COUNT_FRAGS))
        n_frags = c.stats()["n_frags"]
    total, want = store.sum() / 65536.0, float(alpha.astype(np.float64).sum())
    print("seed %d: sum store %.4f px, sum alpha %.4f px, fragments %d, bound %.4f" % (seed, total, want, n_frags, n_frags * (2.0 ** -17 + 2.0 ** -23)))
    assert n_frags > 1000
    assert abs(total - want) <= n_frags * (2.0 ** -17 + 2.0 ** -23)


# 4 ---------------------------------------------------------------- exact equalities
@pytest.mark.parametrize("k", (65, 129))
def test_two_rounds_equal_one(k):
    sc = batch_scene(k)
    _, want, _, _, _ = contrib(sc)
    tx, ty = (sc.W + 15) // 16, (sc.H + 15) // 16
    for permille in (3, 400):
        with capi.Context(0) as c:
            force_path(c, "lists", permille)
            c.push_splat(sc.rows)
            c.sort(sc.cam["view"])
            c.render_contrib(sc.params(), want_rgba=False)
            mask = c.download(capi.BUF_UNSAT_MASK, ty, np.uint32, (tx + 31) // 32)
            got = full_store(c)
        assert int(np.ceil(permille / 1000.0 * (k + 5))) < k, "the opaque splat lies beyond the near share"
        assert mask.any() and (mask[1, 0] >> 1) & 1, "round 1 ran for the tile under test"
        assert np.array_equal(got, want), (k, permille)


def test_pair_records_equal_span_lists(big, big_store):
    for permille in (1000, 400):
        _, got, _, _, st = contrib(big, permille, opts=((capi.OPT_BINNING, 1),))
        assert st["binning"] == 1
        assert np.array_equal(got, big_store), permille


def test_strips_flip_repeat_and_sum(big, big_store):
    imgs, got, _, info, _ = contrib(big, views=STRIPS)
    assert info[1] == 3 and np.array_equal(got, big_store), "a frame = the sum of its strips with x0 % 4 == 0"
    _, flip, _, _, _ = contrib(big, flags=capi.RENDER_FLIP_Y)
    assert np.array_equal(flip, big_store)
    _, twice, _, info, _ = contrib(big, views=((0, None), (0, None)))
    assert info[1] == 2 and np.array_equal(twice, 2 * big_store)
    # frame A then frame B on one context = store(A) + store(B) from two contexts
    other = synth.index_html_camera(100, 70, 75.0, capi=capi)
    pb = capi.make_params(other["gs_mv"], other["gs_proj"], 100, 70, focal_=other["focal"])
    with capi.Context(0) as c:
        force_path(c, "lists")
        c.push_splat(big.rows)
        c.sort(other["view"])
        c.render_contrib(pb, want_rgba=False)
        store_b = full_store(c)
        c.sort(big.cam["view"])
        c.render_contrib(big.params(), want_rgba=False)
        both = full_store(c)
        assert c.contrib_info() == (len(both), 2)
    assert store_b.any() and not np.array_equal(store_b, big_store)
    assert np.array_equal(both, big_store + store_b)


@pytest.mark.parametrize("opt,val,stat", [(capi.OPT_SUBTILE, 2, "subtile"), (capi.OPT_ROW_WALK, 2, "row_walk"),
                                          (capi.OPT_BLEND_SPLIT, 512, None), (capi.OPT_FRAME_BATCH, 2, None)])
def test_options_do_not_leak(big, big_store, opt, val, stat):
    with capi.Context(0) as c:
        c.set_option(capi.OPT_NEAR_PERMILLE, 1000)
        c.set_option(opt, val)
        if opt == capi.OPT_ROW_WALK:
            c.set_option(capi.OPT_SUBTILE, 0)
        c.push_splat(big.rows)
        c.sort(big.cam["view"])
        before = c.render(big.params())
        st_b = c.stats()
        img = c.render_contrib(big.params())
        st = c.stats()
        got = full_store(c)
        after = c.render(big.params())
        st_a = c.stats()
    assert np.array_equal(got, big_store), opt
    assert st["row_walk"] == 0 and st["subtile"] == 0
    if stat:
        assert st_b[stat] == 1 and st_a[stat] == 1
    assert np.array_equal(before, after)
    if opt != capi.OPT_BLEND_SPLIT:                                  # (the split blend's colour is within 1 LSB, not bit-identical)
        assert np.array_equal(img, before)


# 5 ---------------------------------------------------------------- zeros
def test_zeros(big, big_store):
    n = len(big.rows) // 32
    hide = np.zeros(n, np.uint8)
    hide[::3] = capi.STATE_HIDDEN
    _, store, _, _, _ = contrib(big, hide=hide)
    assert (store[::3] == 0).all() and store.any(), "hidden splats are not in the order"
    # splats outside the frustum: the projection culls them
    pm = project_mirror(big.cs, big.cc, big.cam["gs_mv"], big.cam["gs_proj"], big.cam["focal"], big.W, big.H)
    culled = ~pm["visible"]
    assert culled.any() and (big_store[culled] == 0).all()
    # splats whose quad lies wholly in another strip: their mirror weight in the strip is zero, and so is the store
    _, strip, idx, _, _ = contrib(big, views=((0, 16),))
    Wt, cover, _, _ = mirror(big, idx, 0, 16)
    elsewhere = (cover == 0) & (big_store > 0)
    assert elsewhere.sum() >= 5 and (strip[cover == 0] == 0).all()
    # a frame before any sort adds nothing; splats pushed after a frame start at zero and lie beyond the store
    with capi.Context(0) as c:
        force_path(c, "lists")
        c.push_splat(big.rows)
        img = c.render_contrib(big.params())
        assert c.contrib_info() == (n, 0) and not c.download_contrib().any()
        assert (img == np.array([0, 0, 0, 255], np.uint8)).all()
        c.sort(big.cam["view"])
        c.render_contrib(big.params(), want_rgba=False)
        c.push_splat(big.rows[:32 * 7])
        assert c.contrib_info() == (n, 1) and c.count() == n + 7
        assert np.array_equal(c.download_contrib(), big_store)
        mn, mx, cnt = c.prop_range(capi.PROP_SEEN)
        assert cnt == n + 7 and mn == 0.0 and mx == big_store.max() / 65536.0
        assert c.select_range(capi.PROP_SEEN, 0, 0, set_bits=capi.STATE_SELECTED) == int((big_store == 0).sum()) + 7
    # a splat fully behind a scene depth
    sc = batch_scene(65)
    z = np.full((sc.H, sc.W), np.nextafter(window_depth(sc, 64), np.float32(0.0)), np.float32)
    _, store, _, _, _ = contrib(sc, depth=z)
    assert (store[64:] == 0).all() and (store[:64] > 0).all()


# 6 ---------------------------------------------------------------- lifetime
def test_compact_clear_and_contrib_clear(big, big_store):
    n = len(big.rows) // 32
    with capi.Context(0) as c:
        force_path(c, "lists")
        c.push_splat(big.rows)
        c.sort(big.cam["view"])
        c.render_contrib(big.params(), want_rgba=False)
        c.push_splat(big.rows[:32 * 5])                              # five splats beyond the store
        hide = np.zeros(n + 5, np.uint8)
        hide[1::2] = capi.STATE_HIDDEN
        c.set_state(0, hide)
        old = c.compact()
        assert len(old) == c.count() == int((hide == 0).sum())
        rows, frames = c.contrib_info()
        assert rows == int((hide[:n] == 0).sum()) and frames == 1, "the kept splats among those that have a word"
        want = np.zeros(len(old), np.uint64)
        want[old < n] = big_store[old[old < n]]
        assert np.array_equal(full_store(c), want)
        # the store keeps accumulating for the compacted cloud
        c.sort(big.cam["view"])
        c.render_contrib(big.params(), want_rgba=False)
        assert c.contrib_info() == (c.count(), 2) and (full_store(c) >= want).all()
        c.contrib_clear()
        assert c.contrib_info() == (0, 0) and len(c.download_contrib()) == 0
        c.render_contrib(big.params(), want_rgba=False)             # (compact dropped no order since: the frame draws)
        assert c.contrib_info() == (c.count(), 1)
        c.clear()
        assert c.contrib_info() == (0, 0) and c.count() == 0
        c.push_splat(big.rows)
        c.sort(big.cam["view"])
        c.render_contrib(big.params(), want_rgba=False)
        assert np.array_equal(full_store(c), big_store), "a cleared store starts from zero"


def test_sh_highlight_and_antialias():
    rows = synth.make_splat_rows(300, seed=77).reshape(-1, 32).copy()
    rows[:, 12:24] = (rows[:, 12:24].copy().view("<f4") * np.float32(6.0)).view(np.uint8)
    rest = np.random.default_rng(78).standard_normal((300, 45)).astype(np.float32) * np.float32(0.35)
    ply = synth.rows_to_inria_ply(rows, rest)
    cam = synth.index_html_camera(64, 48, 30.0, capi=capi)
    p = capi.make_params(cam["gs_mv"], cam["gs_proj"], 64, 48, focal_=cam["focal"], flags=capi.RENDER_NO_EARLY_OUT)
    out = {}
    for name, opts in (("plain", ()), ("sh", ((capi.OPT_SH_DEGREE, 3),)), ("hl", ((capi.OPT_HIGHLIGHT, 0x80FF00FF),)), ("aa", ((capi.OPT_ANTIALIAS, 1),))):
        with capi.Context(0) as c:
            force_path(c, "lists")
            for k, v in opts:
                c.set_option(k, v)
            c.load_ply(ply)
            if name == "hl":
                c.set_state_ids(np.arange(0, c.count(), 2), set_bits=capi.STATE_SELECTED)
            idx = c.sort(cam["view"])
            img = c.render_contrib(p)
            st = c.stats()
            out[name] = (img, full_store(c), idx, c.download(capi.BUF_CENTER_SCALE, c.count(), np.float32, 4), c.download(capi.BUF_COV_COLOR, c.count(), np.uint32, 4))
            if name == "sh":
                assert st["sh_degree"] == 3
            if name == "aa":
                assert st["antialias"] == 1
            if name == "hl":
                assert c.highlight_info()[1] == 1
    plain = out["plain"][1]
    assert plain.any()
    assert np.array_equal(out["sh"][1], plain) and not np.array_equal(out["sh"][0], out["plain"][0]), "colour is no part of the weight"
    assert np.array_equal(out["hl"][1], plain) and not np.array_equal(out["hl"][0], out["plain"][0])
    # anti-aliased: the record's opacity is alpha * factor, an f32 that no alpha BYTE of a pushed row can hold, so a twin context fed the
    # compensated opacities -- whose store would have to be EQUAL -- cannot be built through the API; the store is compared with the
    # mirror run on that opacity, under the mirror's tolerance
    _, store, idx, cs, cc = out["aa"]
    assert not np.array_equal(store, plain)

    class S:
        pass
    sc = S()
    sc.W, sc.H, sc.cam, sc.cs, sc.cc = 64, 48, cam, cs, cc
    sc.rows = np.zeros(32 * len(cs), np.uint8)
    pm = project_mirror(cs, cc, cam["gs_mv"], cam["gs_proj"], cam["focal"], 64, 48)
    Wt, cover, edge_n, _ = mirror(sc, idx, alpha_scale=pm["c"])
    tol = tolerance(len(idx), cover, edge_n, False)
    dev = np.abs(store.astype(np.float64) / 65536.0 - Wt)
    print("antialias: worst deviation / tol %.4f" % float((dev / np.maximum(tol, 1e-300))[cover > 0].max()))
    assert (dev <= tol).all()


# 7 ---------------------------------------------------------------- the property
def test_seen_property(big, big_store):
    n = len(big.rows) // 32
    v = big_store.astype(np.float64) / 65536.0
    hide = np.zeros(n, np.uint8)
    hide[::4] = capi.STATE_HIDDEN
    with capi.Context(0) as c:
        force_path(c, "lists")
        c.push_splat(big.rows)
        # an empty store: every value is 0
        assert c.prop_range(capi.PROP_SEEN) == (0.0, 0.0, n)
        c.sort(big.cam["view"])
        c.render_contrib(big.params(), want_rgba=False)
        assert np.array_equal(c.download_contrib(), big_store)
        c.set_state(0, hide)                                         # (after the frame: the filter, not the order)
        for mask, value in ((0, 0), (capi.STATE_HIDDEN, 0)):
            sel = (hide & mask) == value
            mn, mx, cnt = c.prop_range(capi.PROP_SEEN, mask, value)
            assert (mn, mx, cnt) == (v[sel].min(), v[sel].max(), int(sel.sum()))
            lo, hi = float(v.min()), float(v.max())
            counts, tally = c.histogram(capi.PROP_SEEN, lo, hi, 64, mask, value)
            bins = np.minimum(np.floor((v[sel] - lo) * (64.0 / (hi - lo))).astype(np.int64), 63)
            assert np.array_equal(counts, np.bincount(bins, minlength=64).astype(np.uint32))
            assert list(tally) == [int(sel.sum()), 0, 0, 0]
        med = float(np.median(v[v > 0]))
        assert c.select_range(capi.PROP_SEEN, med, 1e30, set_bits=capi.STATE_SELECTED) == int((v >= med).sum())
        assert np.array_equal((c.download_state() & capi.STATE_SELECTED) != 0, v >= med)
        assert c.select_range(capi.PROP_SEEN, med, 1e30, clear_bits=capi.STATE_SELECTED, flags=capi.SELECT_INVERT) == int((v < med).sum())
        assert c.select_range(capi.PROP_SEEN, 0, 0, clear_bits=capi.STATE_SELECTED) == int((v == 0).sum())
        assert np.array_equal((c.download_state() & capi.STATE_SELECTED) != 0, v >= med)
        for prop in range(8, 16):
            for call in (lambda: c.prop_range(prop), lambda: c.histogram(prop, 0, 1, 4), lambda: c.select_range(prop, 0, 1)):
                with pytest.raises(capi.GsError) as ei:
                    call()
                assert ei.value.code == capi.E_BADARG
    with capi.Context(0) as c:                                       # nothing resident; then worker rows only
        assert c.prop_range(capi.PROP_SEEN)[2] == 0 and c.select_range(capi.PROP_SEEN, 0, 0) == 0
        c.push_matrices(big.mats)
        c.sort(big.cam["view"])
        for call in (lambda: c.prop_range(capi.PROP_SEEN), lambda: c.histogram(capi.PROP_SEEN, 0, 1, 4), lambda: c.select_range(capi.PROP_SEEN, 0, 1),
                     lambda: c.render_contrib(big.params())):
            with pytest.raises(capi.GsError) as ei:
                call()
            assert ei.value.code == capi.E_STATE


def test_seen_on_every_device(big, big_store):
    """the gs_multi_ forms read each device's own store: after the same frame on each context, the same answers"""
    n = len(big.rows) // 32
    L = capi.load()
    view = np.ascontiguousarray(big.cam["view"], np.float32)
    p = big.params()
    with capi.Multi([0, 0]) as m:
        m.push_splat(big.rows)
        hs = [L.gs_multi_ctx(m._h, i) for i in range(2)]
        for h in hs:
            for k, v in ((capi.OPT_NEAR_PERMILLE, 1000), (capi.OPT_ROW_WALK, 0), (capi.OPT_SUBTILE, 0)):
                assert L.gs_set_option(h, k, v) == capi.GS_OK
            assert L.gs_sort(h, view.ctypes.data_as(C.c_void_p), None, None, None) == capi.GS_OK
            assert L.gs_render_contrib(h, C.byref(p), None, 0) == capi.GS_OK
        mn, mx, cnt = m.prop_range(capi.PROP_SEEN)
        assert (mn, mx, cnt) == (0.0, big_store.max() / 65536.0, n)
        assert m.select_range(capi.PROP_SEEN, 0, 0, set_bits=capi.STATE_HIDDEN) == int((big_store == 0).sum())
        m.sync()
        for h in hs:
            rows, hidden = C.c_size_t(0), C.c_size_t(0)
            assert L.gs_state_count(h, C.byref(rows), C.byref(hidden)) == capi.GS_OK
            assert hidden.value == int((big_store == 0).sum())


# 8 ---------------------------------------------------------------- the workflow
def test_workflow_prune_what_is_never_seen(big):
    other = synth.index_html_camera(100, 70, 75.0, capi=capi)
    views = [(big.cam["view"], big.params()), (other["view"], capi.make_params(other["gs_mv"], other["gs_proj"], 100, 70, focal_=other["focal"]))]
    with capi.Context(0) as c:
        force_path(c, "lists")
        c.push_splat(big.rows)
        n = c.count()
        before = []
        for view, p in views:
            c.sort(view)
            before.append(c.render_contrib(p))
        unseen = c.select_range(capi.PROP_SEEN, 0, 0, set_bits=capi.STATE_HIDDEN)
        assert 0 < unseen < n and c.contrib_info() == (n, 2)
        old = c.compact()
        assert c.count() == n - unseen == len(old) and c.count() < n
        assert (full_store(c) > 0).all()
        for (view, p), want in zip(views, before):
            c.sort(view)
            got = c.render(p)
            assert np.array_equal(got, want), "a splat whose every weight rounds to 0 changed no pixel"


# 9 ---------------------------------------------------------------- arguments
def test_arguments(big):
    L = capi.load()
    with capi.Context(0) as c:
        force_path(c, "lists")
        c.push_splat(big.rows)
        c.sort(big.cam["view"])
        assert L.gs_render_contrib(c._h, None, None, 0) == capi.E_BADARG
        assert L.gs_render_contrib_device(c._h, None, None) == capi.E_BADARG
        with pytest.raises(capi.GsError) as ei:
            c.render_contrib(big.params(flags=capi.RENDER_COUNT_FRAGS))
        assert ei.value.code == capi.E_BADARG and "COUNT_FRAGS" in ei.value.message
        c.set_scene(np.ones((48, 64), np.float32), None)
        with pytest.raises(capi.GsError) as ei:
            c.render_contrib(big.params())
        assert ei.value.code == capi.E_BADARG
        c.set_scene(None, None)
        assert c.contrib_info() == (0, 0), "a refused frame leaves no store behind"
        c.render_contrib_device(big.params())                       # no image asked for, by either entry point
        c.render_contrib(big.params(), want_rgba=False)
        rows, frames = c.contrib_info()
        assert (rows, frames) == (c.count(), 2)
        buf = np.zeros(rows + 1, np.uint64)
        vp = buf.ctypes.data_as(C.c_void_p)
        assert L.gs_download(c._h, capi.BUF_CONTRIB, vp, (rows + 1) * 8) == capi.E_BADARG      # more than the store holds
        assert L.gs_download(c._h, capi.BUF_CONTRIB, vp, rows * 8 - 3) == capi.E_BADARG        # no whole words
        assert L.gs_download(c._h, capi.BUF_CONTRIB, vp, 16) == capi.GS_OK and buf[2] == 0
        assert np.array_equal(buf[:2], c.download_contrib()[:2])
        only_rows, only_frames = C.c_size_t(0), C.c_uint64(0)
        assert L.gs_contrib_info(c._h, C.byref(only_rows), None) == capi.GS_OK and only_rows.value == rows
        assert L.gs_contrib_info(c._h, None, C.byref(only_frames)) == capi.GS_OK and only_frames.value == 2
