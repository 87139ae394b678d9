"""GPU tier: scene compositing (gs_set_scene: the LEQUAL depth test and the per-pixel destination) and early termination
(GS_OPT_TERMINATION) on every blend path, at their edges.  Scenes, planes and the count condition: test_scene_edges_cpu.py.

Paths are forced by name on fresh contexts and proven per frame by the frame's statistics (test_gpu_parity.force_path / assert_path):
lists, walk, subtile and pairs draw the same pixels bit for bit, the split blend within 1 LSB of them; lists is held to the oracle
drawing the same scene (PIXEL_TOL_LSB), and GS_RENDER_COUNT_FRAGS on the list paths to the oracle's fragment count exactly -- a plane
AT an entry's window depth and one ulp below differ by that entry's pixels, so `<` for `<=` is a count, not a 1 LSB question.

Budget: about 1.4 s of wall time on one MI355X as last measured (8 tests, the slowest 0.22 s: ~190 fresh contexts, frames of 1x1 to
320x180 pixels and the 160x368 stacks; test_blend_paths_gpu.py takes about 3 s)."""
import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_blend_paths_gpu import EXACT, list_lengths          # (camera, run, Scene: through the scenes of test_scene_edges_cpu)
from test_gpu_parity import assert_path, force_path, pix_check
from test_scene_edges_cpu import (BACKGROUNDS, CASES, ODD_REJECTS, RAGGED, STRIP_W, STRIP_X0, TARGET, TERMINATIONS, Stacks, count_condition,
                                  destination_scene, odd_plane, odd_values, oracle_frame, order, ragged_scene, strips_scene,
                                  termination_stacks)

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

PATHS = EXACT + ("split",)
COUNTED = ("lists", "subtile", "pairs")                 # GS_RENDER_COUNT_FRAGS keeps these paths (a counting frame is never walked or split)
NONE = capi.SURFACE_NONE


def job(depth=None, rgba=None, bg=(0.0, 0.0, 0.0, 1.0), flags=0, x0=0, x1=None, count=False):
    return dict(depth=depth, rgba=rgba, bg=bg, flags=flags, x0=x0, x1=x1, count=count)


def frames(scene, path, jobs, opts=(), near=1000):
    """Draw the jobs on ONE fresh context with `path` forced, each frame's statistics proving the path -> ([(image, n_frags | None)],
    order, [stats]).  A job with count=True is drawn a second time with GS_RENDER_COUNT_FRAGS for its fragment count."""
    out, stats = [], []
    with capi.Context(0) as c:
        force_path(c, path, near)
        for k, v in opts:
            c.set_option(k, v)
        c.push_splat(scene.rows)
        idx = c.sort(scene.cam["view"])
        have = (None, None)
        for j in jobs:
            if j["depth"] is not have[0] or j["rgba"] is not have[1]:
                c.set_scene(j["depth"], j["rgba"])
                have = (j["depth"], j["rgba"])
            img = c.render(scene.params(j["x0"], j["x1"], flags=j["flags"], background=j["bg"]))
            stats.append(assert_path(c, path, (j["x0"], j["x1"], j["flags"])))
            n = None
            if j["count"] and path in COUNTED:
                c.render(scene.params(j["x0"], j["x1"], flags=j["flags"] | capi.RENDER_COUNT_FRAGS, background=j["bg"]))
                n = assert_path(c, path, "count")["n_frags"]
            out.append((img, n))
    return out, idx, stats


def every_path(scene, jobs, tag, paths=PATHS, opts=(), to_oracle=True):
    """The jobs on every path: the exact paths bit-identical, split within 1 LSB, the first path within the oracle's bar, the counts of
    the list paths the oracle's.  -> {path: [image]}, order, [oracle's fragment count per job]"""
    res, idx = {}, None
    for p in paths:
        res[p], i, _ = frames(scene, p, jobs, opts)
        idx = i if idx is None else idx
        assert np.array_equal(i, idx)
    assert np.array_equal(idx, order(scene))
    want_frags = []
    for k, j in enumerate(jobs):
        ref = res[paths[0]][k][0]
        for p in paths[1:]:
            d = int(np.abs(ref.astype(int) - res[p][k][0].astype(int)).max()) if ref.size else 0
            print("%s job %d: %s vs %s max |dRGBA8| = %d" % (tag, k, p, paths[0], d))
            assert d <= (1 if p == "split" else 0), (tag, k, p, d)
        if to_oracle or j["count"]:
            want, fr = oracle_frame(scene, idx, j["depth"], j["rgba"], j["bg"], j["x0"], j["x1"])
            want = want[::-1] if j["flags"] & capi.RENDER_FLIP_Y else want
            pix_check("%s_%d_%s" % (tag, k, paths[0]), ref, want)
            want_frags.append(fr)
            for p in paths:
                if res[p][k][1] is not None:
                    print("%s job %d: n_frags on %s = %d, the oracle's %d" % (tag, k, p, res[p][k][1], fr))
                    assert res[p][k][1] == fr, (tag, k, p, res[p][k][1], fr)
    return {p: [a for a, _ in r] for p, r in res.items()}, idx, want_frags


@pytest.fixture(scope="module")
def stacks():
    return Stacks(CASES)


@pytest.fixture(scope="module")
def cloud():
    rows = synth.make_splat_rows(20000, seed=4242)
    return rows


# ---------------------------------------------------------------- the cut at an entry, inside a lane, inside a block

def test_stack_lists_hold_what_the_cases_claim(stacks):
    lens = list_lengths(stacks.scene)
    assert lens.shape == (len(CASES), 10)
    for t, (K, m) in enumerate(stacks.cases):
        assert lens[t, TARGET] == K, "column %d of tile row %d holds %d entries, not %d" % (TARGET, t, lens[t, TARGET], K)


def test_depth_cut_at_and_just_below_an_entry(stacks):
    exact, below = stacks.exact(), stacks.below()
    imgs, idx, frags = every_path(stacks.scene, [job(exact, stacks.rgba, count=True), job(below, stacks.rgba, count=True)], "cut")
    covered = count_condition(stacks, idx, exact, below)            # every case: the two counts differ by entry m's pixels, > 0
    assert frags[0] - frags[1] == covered > 0
    for p in PATHS:                                                 # and the entry is in the picture of one and not of the other, in every case
        d = np.abs(imgs[p][0].astype(int) - imgs[p][1].astype(int)).reshape(len(CASES), 16, stacks.W, 4).max(axis=(1, 2, 3))
        assert (d >= 2).all(), (p, d.tolist())                      # (beyond the 1 LSB the comparisons allow)


def test_cuts_that_differ_inside_a_lane_and_a_block(stacks):
    pl = stacks.planes()
    jobs = [job(pl[n], stacks.rgba, count=True) for n in ("alternating", "checker", "one_pixel")]
    every_path(stacks.scene, jobs, "lane_block")


def test_non_finite_and_out_of_range_depths():
    st = Stacks([(65, 32)], seed=4)
    assert list_lengths(st.scene)[0, TARGET] == 65
    plane, v = odd_plane(st), odd_values()
    imgs, _, _ = every_path(st.scene, [job(plane, st.rgba, count=True), job(plane, None, bg=(0.25, 0.5, 0.75, 0.5), count=True)], "odd")
    rej = np.isin(np.arange(st.W) % v.size, ODD_REJECTS)
    for p in PATHS:
        assert np.array_equal(imgs[p][0][:, rej], st.rgba[:, rej]), p      # NaN, -inf (and 0, -0, -1, the denormal): the destination exactly
        assert np.all(imgs[p][1][:, rej] == np.array([64, 128, 191, 128], np.uint8)), p
        assert (imgs[p][0][3:13, ~rej] != st.rgba[3:13, ~rej]).any(), p


# ---------------------------------------------------------------- the destination

def test_destination_colour_and_alpha():
    scene, depth, rgba = destination_scene()
    jobs = [job(d, c, bg) for bg in BACKGROUNDS for d, c in ((depth, rgba), (None, rgba), (depth, None))]
    imgs, _, _ = every_path(scene, jobs, "dest")
    for p in PATHS:
        for k, j in enumerate(jobs):
            got = imgs[p][k][0:16, 0:64]                            # four tiles no run covers
            if j["rgba"] is not None:
                assert np.array_equal(got, rgba[0:16, 0:64]), (p, k)     # all 256 values of each channel come back
            else:
                a = j["bg"][3]
                assert np.all(got == np.array([64, 128, 191, {0.0: 0, 0.5: 128, 1.0: 255}[a]], np.uint8)), (p, k)
    for c in range(4):
        assert sorted(rgba[0:16, 16 * c:16 * c + 16, c].reshape(-1).tolist()) == list(range(256))


# ---------------------------------------------------------------- layout: flip, strips, ragged frames, a scene of another size

def test_flip_strips_and_ragged_frames_with_a_scene(stacks):
    # the scene is read at the image row, the output written at the flipped one
    plane = stacks.alternating()
    for p in PATHS:
        (a, _), (b, _) = frames(stacks.scene, p, [job(plane, stacks.rgba), job(plane, stacks.rgba, flags=capi.RENDER_FLIP_Y)])[0]
        assert np.array_equal(np.flipud(a), b), p
        assert not np.array_equal(a, b)
    # strips: a different cut in every column, read up to x1b
    scene, depth, rgba = strips_scene()
    views = [(x0, x0 + w) for x0 in STRIP_X0 for w in STRIP_W]
    jobs = [job(depth, rgba)] + [job(depth, rgba, x0=a, x1=b) for a, b in views]
    for term in (1024, 256):
        imgs, idx, _ = every_path(scene, jobs, "strips_t%d" % term, opts=((capi.OPT_TERMINATION, term),), to_oracle=False)
        for p in PATHS:
            full = imgs[p][0]
            for (a, b), img in zip(views, imgs[p][1:]):
                d = int(np.abs(img.astype(int) - full[:, a:b].astype(int)).max())
                # (a lane's four pixels are the full frame's when x0 is on the 4-pixel grid; the split blend stops pixel by pixel at
                # steps of its own list, which changes with the tile's columns: within 1 LSB throughout)
                assert d <= (0 if a % 4 == 0 and p in EXACT else 1), (p, term, a, b, d)
        for k in (0, 3, 9, 14, 20):                                  # the frame and some strips against the oracle
            j = jobs[k]
            pix_check("strips_t%d_%d" % (term, k), imgs["lists"][k], oracle_frame(scene, idx, depth, rgba, x0=j["x0"], x1=j["x1"])[0])
    # ragged frames: the last lane group hangs over the right edge, the last tile row over the bottom
    for w, h in RAGGED:
        sc, d, c = ragged_scene(w, h)
        every_path(sc, [job(d, c, count=True), job(d, None, bg=(0.2, 0.4, 0.6, 0.5))], "ragged_%dx%d" % (w, h))
    # a scene of another size
    sc, d, c = ragged_scene(31, 47)
    with capi.Context(0) as ctx:
        force_path(ctx, "lists")
        ctx.push_splat(sc.rows)
        idx = ctx.sort(sc.cam["view"])
        ctx.set_scene(np.ones((47, 32), np.float32), None)
        l, r, head = synth.xr_eye_cameras(45.0, 0.02, capi=capi)
        eyes = [capi.make_params(e["gs_mv"], e["gs_proj"], e["vw"], e["vh"], focal_=e["focal"]) for e in (l, r)]
        for call in (lambda: ctx.render(sc.params()), lambda: ctx.render_surface(sc.params()), lambda: ctx.render_contrib(sc.params()),
                     lambda: ctx.render_stereo(*eyes)):
            with pytest.raises(capi.GsError) as ei:
                call()
            assert ei.value.code == capi.E_BADARG
        ctx.set_scene(None, None)
        pix_check("after_badarg", ctx.render(sc.params()), oracle_frame(sc, idx)[0])
        assert_path(ctx, "lists")


# ---------------------------------------------------------------- modes: two rounds, paired frames, stereo, surface, contribution

def _wall(h, w, seed):
    """depth 1.0 but 0.0 over the left half of tile column 4 (a tile that can never saturate) and on single pixels elsewhere; random colour"""
    g = np.random.Generator(np.random.PCG64(seed))
    depth = np.ones((h, w), np.float32)
    depth[:, 64:72] = 0.0
    depth[g.integers(0, h, 60), g.integers(0, w, 60)] = 0.0
    return depth, g.integers(0, 256, (h, w, 4)).astype(np.uint8)


def test_modes_with_a_scene(cloud, stacks):
    w, h = 320, 180
    depth, rgba = _wall(h, w, 31)
    cam = synth.index_html_camera(w, h, 200.0, capi=capi)
    prm = lambda cm, **kw: capi.make_params(cm["gs_mv"], cm["gs_proj"], cm["vw"], cm["vh"], focal_=cm["focal"], **kw)
    # two rounds: the tile behind the wall keeps its state and is resumed
    one, unsat = None, 0
    for p in ("lists", "pairs"):
        with capi.Context(0) as c:
            force_path(c, p)
            c.push_splat(cloud)
            idx = c.sort(cam["view"])
            c.set_scene(depth, rgba)
            for permille in (1000, 3, 400):
                c.set_option(capi.OPT_NEAR_PERMILLE, permille)
                img = c.render(prm(cam))
                st = assert_path(c, p, permille)
                if permille == 1000:
                    one = img if one is None else one
                else:
                    unsat += st["unsat_tiles"]
                assert np.array_equal(img, one), (p, permille)
    assert unsat > 0, "no frame left a tile to the second round"
    cs, cc, _ = oracle.pack(cloud)
    want, _, _ = oracle.render(cs, cc, idx, cam["gs_mv"].astype(np.float32), cam["gs_proj"].astype(np.float32), cam["focal"], w, h,
                               want_f32=False, scene_depth=depth, scene_rgba=rgba)
    pix_check("wall_two_rounds", one, want)
    assert np.array_equal(one[:, 64:72], rgba[:, 64:72])            # behind the wall: the scene's colour
    # paired queued frames (the k_twin forms), the scene set beforehand: six frames equal their synchronous twins
    cams = [synth.index_html_camera(w, h, 40.0 * k, capi=capi) for k in range(6)]
    for p in PATHS:
        with capi.Context(0) as c:
            force_path(c, p)
            c.push_splat(cloud)
            c.set_scene(depth, rgba)
            want = []
            for cm in cams:
                c.sort(cm["view"])
                want.append(c.render(prm(cm)))
                assert_path(c, p, "sync")
            c.set_option(capi.OPT_FRAME_BATCH, 2)
            bufs = [capi.host_frame(h, w) for _ in cams]
            for (b, _), cm in zip(bufs, cams):
                c.sort(cm["view"], want_indices=False)
                c.render_into(prm(cm, flags=capi.RENDER_ASYNC), b)
            c.sync()
            assert_path(c, p, "paired")
            for k, ((b, o), wnt) in enumerate(zip(bufs, want)):
                d = int(np.abs(b.astype(int) - wnt.astype(int)).max())
                o.free()
                assert d == 0, (p, k, d)
    # stereo: one scene for both eyes, each eye its own gs_render
    l, r, head = synth.xr_eye_cameras(60.0, 0.125, capi=capi)
    sd, sc = _wall(l["vh"], l["vw"], 32)
    for p in ("lists", "walk"):
        with capi.Context(0) as c:
            force_path(c, p)
            c.push_splat(cloud)
            c.sort(head["view"])
            c.set_scene(sd, sc)
            o0, o1 = c.render_stereo(prm(l), prm(r))
            assert_path(c, p, "stereo")
            assert np.array_equal(o0, c.render(prm(l))) and np.array_equal(o1, c.render(prm(r))), p
            assert not np.array_equal(o0, o1) and np.array_equal(o0[:, 64:72], sc[:, 64:72])
    # surface and contribution frames under the cut planes of the first test
    scene = stacks.scene
    for name, plane in (("exact", stacks.exact()), ("below", stacks.below())):
        with capi.Context(0) as c:
            force_path(c, "lists")
            c.push_splat(scene.rows)
            c.sort(scene.cam["view"])
            c.set_scene(plane, stacks.rgba)
            img = c.render(scene.params())
            assert_path(c, "lists")
            simg, pid, dep, alp = c.render_surface(scene.params())
            assert np.array_equal(simg, img), name
            assert (pid != NONE).any() and (dep[pid != NONE] <= plane[pid != NONE]).all(), name
            assert np.all(dep[pid == NONE] == 1.0)
            cimg = c.render_contrib(scene.params())
            assert np.array_equal(cimg, img), name
            store = np.zeros(c.count(), np.uint64)
            got = c.download_contrib()
            store[:len(got)] = got
        for t, (K, m) in enumerate(stacks.cases):
            s = store[stacks.first[t]:stacks.first[t] + K]
            last = m if name == "exact" else m - 1                  # the farthest entry whose window depth is <= the plane
            assert not s[last + 1:].any(), (name, K, m)
            assert (s[:last + 1] > 0).all(), (name, K, m)
        if name == "exact":                                         # the strong entry m crosses one half somewhere: a surface AT the plane
            assert (dep[pid != NONE] == plane[pid != NONE]).any()


# ---------------------------------------------------------------- GS_OPT_TERMINATION: the header's 1 LSB promise

def test_termination_bound():
    """What early termination leaves out of a pixel is sum w_i (c_i - dst) over the entries behind the stop, |.| <= T_stop < eps <= 1/256
    of full scale: under one byte step before rounding, so the rounded frames differ by at most 1 -- for every eps <= 1/256, whatever
    the scene's colour; a lane that blends on for its neighbours only lowers what is left out.  Derived, not measured."""
    st = termination_stacks()
    scene = st.scene
    cut = st.alternating()
    none = capi.RENDER_NO_EARLY_OUT
    jobs = [job(None, st.rgba), job(cut, st.rgba), job(None, None, bg=(0.0, 1.0, 0.0, 0.5))]
    for p in PATHS:
        ref = [a for a, _ in frames(scene, p, [dict(j, flags=none) for j in jobs])[0]]
        if p == "lists":
            idx = order(scene)
            for k, j in enumerate(jobs):
                pix_check("term_all_%d" % k, ref[k], oracle_frame(scene, idx, j["depth"], j["rgba"], j["bg"])[0])
        for term in TERMINATIONS:
            got = frames(scene, p, jobs, opts=((capi.OPT_TERMINATION, term),))[0]
            for k, (a, _) in enumerate(got):
                d = int(np.abs(a.astype(int) - ref[k].astype(int)).max())
                print("termination %d on %s, job %d: max |dRGBA8| against NO_EARLY_OUT = %d" % (term, p, k, d))
                assert d <= 1, (p, term, k, d)
    # the option is not ignored: fewer fragments are evaluated the earlier a pixel stops
    ev = capi.RENDER_COUNT_FRAGS | capi.RENDER_COUNT_EVALUATED
    for p in COUNTED:
        n = {}
        for term, flags in ((2, ev), (1024, ev), (0, ev | none)):
            with capi.Context(0) as c:
                force_path(c, p)
                if term:
                    c.set_option(capi.OPT_TERMINATION, term)
                c.push_splat(scene.rows)
                c.sort(scene.cam["view"])
                c.set_scene(None, st.rgba)
                c.render(scene.params(flags=flags))
                n[term] = assert_path(c, p, term)["n_frags"]
        print("fragments evaluated on %s: eps 1/2 %d, 1/1024 %d, no early out %d" % (p, n[2], n[1024], n[0]))
        assert 0 < n[2] < n[1024] < n[0], (p, n)
