"""GPU tier: the span-list binning (k_row_scan, k_emit_runs, k_seg_count, k_lists in csrc/gs_render.hip) at the edges of its own
tables and segments, each form forced by name, proven by the frame's statistics and compared with the CPU oracle and with the others.

Forms (test_gpu_parity.PATH_OPTIONS / PATH_PROOF): segc (GS_OPT_SEG_COUNT 2: k_seg_count + k_lists<0, true>; gs_stats.seg_count == 1),
lists (GS_OPT_SEG_COUNT 0: every k_lists item counts its row itself; seg_count == 0), pairs (GS_OPT_BINNING 1: pair records through two
radix passes -- kernels that share nothing with the span lists) and, where a plain frame allows it, walk (GS_OPT_ROW_WALK 2: the same runs,
no lists).  The constants the edges are placed from are parsed out of the source.

Every scene is constructed from .splat rows (test_blend_paths_gpu.run / splat) in the order of their sorted positions: position 0 is the
farthest splat, and every scene asserts that the order came out as built.  Before a layout is relied on, three things are asserted about
it: gs_stats.n_runs equals the runs built, the per-tile list lengths (GS_OPT_RECORD_STAGED, GS_BUF_TILE_STATS) of the span lists equal the
lengths the construction gives in plain Python, and so do the lengths of the pair records.  Then: pixels within test_gpu_parity.PIXEL_TOL_LSB (pix_check) of
oracle.render on the strips under test, the fragment count of a GS_RENDER_COUNT_FRAGS frame equal to the oracle's, and the forms equal to
each other bit for bit.  Lists of compared tiles are short (about six entries, strong alphas, saturated colours) so that the ORDER of
a list shows in its pixels; a row's surplus runs sit in a few sacrificial columns.

A two-round frame's statistic speaks of round 0 alone (seg_count == 1 with the form forced); round 1 cannot take the form -- k_seg_count<1>
is not instantiated -- and is pinned by its frames: equal to those of GS_OPT_SEG_COUNT 0 and to the one-round frame.

Budget: 22 tests, 3.05 s of wall time on one MI355X as last measured (3.1 .. 3.8 s over three runs); the slowest are the two chunks of
tall splats with their strips, 0.55 s each, then the 256-splat row word with 0.31 s; every other test stays under 0.25 s."""
import math

import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_blend_paths_gpu import Scene, _paired_equal_synchronous, camera, compare_paths, draw, run, splat, tile_lengths
from test_gpu_parity import PATH_OPTIONS, assert_path, force_path, pix_check
from test_sort_paths_gpu import _constant

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

LIST_SEG = _constant("GS_LIST_SEG", "gs_render.hip")
LIST_SEGS = _constant("GS_LIST_SEGS", "gs_render.hip")
SEGC_RUNS_PER_ROW = _constant("GS_SEGC_RUNS_PER_ROW", "gs_render.hip")
LIST_LOADS = _constant("GS_LIST_LOADS", "gs_render.hip")
BLOCK = _constant("GS_BLOCK", "gs_internal.h")
# what the shapes below rest on: one thread per tile column and per chunk position, 64-run words, a segment of at least one batch
assert BLOCK == 256 and LIST_SEG % 64 == 0 and LIST_SEG >= BLOCK and LIST_SEGS >= 2 and LIST_LOADS >= 1, (BLOCK, LIST_SEG, LIST_SEGS)

FORMS = ("segc", "lists", "pairs")                         # bit-identical frames, identical per-tile lengths
PALETTE = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255), (255, 128, 0), (128, 0, 255)]
STEP = 0.0003                                              # depth between neighbouring sorted positions


def seg_len(nr):
    """list_seg_len of gs_render.hip: the runs a k_lists item walks."""
    s = (nr + LIST_SEGS - 1) // LIST_SEGS
    return LIST_SEG if s <= LIST_SEG else (s + 63) & ~63


def items(nr):
    return max(1, -(-nr // seg_len(nr)))


def depth_of(p, n):
    """Sorted position p of n: the order is far to near (index.js:507-570 sorts the view depth, which is negative, ascending)."""
    return 1.0 + STEP * (n - 1 - p)


def tall(cam, r0, r1, depth, rgba):
    """A splat of tile rows r0..r1 (r1 > r0) of a 64-pixel frame, all four tile columns in every one of them: centred at x = 32, its
    ends 8 px inside the end rows, and as wide as it takes to be 72 px wide at the last pixel centre of its first row (7.5 px from its
    end) -- so every row's run is the four columns, with 4 px to spare, and width / height stays far from what the 16-bit covariance
    of a .splat row resolves (a 15 px x 4080 px splat is drawn 3 px wide)."""
    hy = (r1 - r0) * 8.0
    hx = 36.0 / math.sqrt(1.0 - ((hy - 7.5) / hy) ** 2)
    return splat(cam, 32.0, (r0 + r1) * 8.0 + 8.0, hx, hy, depth, rgba)


class Built(Scene):
    """A Scene from `shapes`, one per sorted position (0 = farthest): ("run", ty, a, b, rgba) or ("tall", r0, r1, rgba) or
    ("raw", cx, cy, hx, hy, rgba, cover) with cover = [(ty, a, b), ...] the tile-row runs the construction gives it.  want: the
    per-tile list lengths of the whole frame, runs: its tile-row runs, tiles[p]: the tiles of position p."""

    def __init__(self, W, H, shapes, off=0.5):
        cam = camera(W, H, off)
        n = len(shapes)
        tx, ty = (W + 15) // 16, (H + 15) // 16
        self.want = np.zeros((ty, tx), np.int64)
        self.tiles = np.zeros(n, np.int64)
        self.runs = 0
        self.cover = []
        rows = []
        for p, s in enumerate(shapes):
            d = depth_of(p, n)
            if s[0] == "run":
                _, r, a, b, rgba = s
                rows.append(run(cam, r, a, b, d, rgba))
                cover = [(r, a, b)]
            elif s[0] == "tall":
                _, r0, r1, rgba = s
                assert W == 64
                rows.append(tall(cam, r0, r1, d, rgba))
                cover = [(r, 0, 3) for r in range(r0, r1 + 1)]
            else:
                _, cx, cy, hx, hy, rgba, cover = s
                rows.append(splat(cam, cx, cy, hx, hy, d, rgba))
            self.cover.append(cover)
            for r, a, b in cover:
                self.want[r, a:b + 1] += 1
                self.tiles[p] += b - a + 1
            self.runs += len(cover)
        super().__init__(W, H, rows, off)
        self.n = n

    def want_of(self, lo, hi):
        """Per-tile list lengths from the sorted positions [lo, hi) alone: what one binning round over them builds."""
        w = np.zeros_like(self.want)
        for cover in self.cover[lo:hi]:
            for r, a, b in cover:
                w[r, a:b + 1] += 1
        return w


def frame(scene, path, x0=0, x1=None, flags=0, opts=(), staged=False, near=1000):
    """One strip of a scene on a fresh context with `path` forced: (image, statistics, per-tile list lengths or None, order, tiles per
    sorted position) -- all of one frame (test_blend_paths_gpu.list_lengths gives the lengths alone)."""
    with capi.Context(0) as c:
        force_path(c, path, near)
        for k, v in opts:
            c.set_option(k, v)
        if staged:
            c.set_option(capi.OPT_RECORD_STAGED, 1)
        c.push_splat(scene.rows)
        idx = c.sort(scene.cam["view"])
        img = c.render(scene.params(x0, x1, flags=flags))
        st = assert_path(c, path, (x0, x1, flags))
        lens = None
        if staged:
            lens = tile_lengths(c, scene, x0, x1).astype(np.int64)
        tc = c.download(capi.BUF_TILE_COUNT, int(st["n_sorted"]), np.uint32, 1)[:, 0].astype(np.int64)
    return img, st, lens, idx, tc


def assert_layout(scene, tag):
    """The scene is what it claims to be: order as built, every splat kept and visible, n_runs, the tiles per splat and the per-tile
    lengths of both span-list forms and of the pair records equal to the construction."""
    for p in FORMS:
        _, st, lens, idx, tc = frame(scene, p, staged=True)
        assert np.array_equal(idx, np.arange(scene.n, dtype=idx.dtype)), (tag, p, "the order is not the one built")
        assert st["n_sorted"] == scene.n and st["n_visible"] == scene.n, (tag, p, st["n_sorted"], st["n_visible"], scene.n)
        if p != "pairs":                                            # (pair records know no runs: the statistic keeps its last value)
            assert st["n_runs"] == scene.runs, (tag, p, st["n_runs"], scene.runs)
        assert st["n_pairs"] == scene.want.sum(), (tag, p, st["n_pairs"], int(scene.want.sum()))
        bad = np.argwhere(lens != scene.want)
        assert not len(bad), "%s %s: %d tiles differ from the construction, first (row, column) %s: %d entries, built %d" % (
            tag, p, len(bad), bad[0].tolist(), lens[tuple(bad[0])], scene.want[tuple(bad[0])])
        bad = np.flatnonzero(tc != scene.tiles)
        assert not len(bad), "%s %s: tiles of %d sorted positions differ, first %d: %d, built %d" % (
            tag, p, len(bad), bad[0], tc[bad[0]], scene.tiles[bad[0]])


def assert_forms(scene, views, oracle_views, tag, paths=FORMS, frags_views=((0, None),), near=1000):
    """Pixels: the forms equal bit for bit on every view, the first within the oracle's bar on oracle_views.  Fragment counts of a
    counting frame == the oracle's, and the per-tile lengths of the forms equal to each other, on frags_views."""
    imgs, idx = compare_paths(scene, views, paths=paths, tag=tag, oracle_views=oracle_views,
                              opts=((capi.OPT_NEAR_PERMILLE, near),) if near != 1000 else ())
    for x0, x1 in frags_views:
        _, want = scene.oracle(idx, x0, x1)
        ref = None
        for p in FORMS:
            _, st, lens, _, tc = frame(scene, p, x0, x1, flags=capi.RENDER_COUNT_FRAGS, staged=True)
            print("fragments", tag, p, (x0, x1), st["n_frags"], "oracle", want)
            assert st["n_frags"] == want, (tag, p, x0, x1, st["n_frags"], want)
            if ref is None:
                ref = (lens, tc, st["n_pairs"])
            assert np.array_equal(lens, ref[0]) and np.array_equal(tc, ref[1]) and st["n_pairs"] == ref[2], (tag, p, x0, x1)
    return imgs, idx


# ---------------------------------------------------------------- segment edges

def _row_plan(n, C):
    """The n runs of one tile row of C columns, in sorted order: runs at the row's ends, at both sides of the first segment boundary, in
    a middle segment and at the start of the last one are `special` -- they cover the compared columns (0..3, the middle one, the last
    four), among them runs over all C columns (a -1 at index C: 256 at C == 256) and runs that end in the last column; every other
    run is one tile in a sacrificial column."""
    S = seg_len(n)
    mid, far = C * 100 // 256, C * 140 // 256
    special = {}
    for pos, ab in ((0, (0, C - 1)), (n - 1, (0, C - 1)), (n // 2, (0, C - 1)), (1, (C - 6, C - 1)), (S - 1, (0, 3)), (S, (C - 56, C - 1)),
                    ((items(n) - 1) * S, (mid, C - 1)), (n - 2, (0, far))):
        if 0 <= pos < n and pos not in special:
            special[pos] = ab
    out = []
    for i in range(n):
        if i in special:
            out.append(special[i] + (PALETTE[len([k for k in special if k < i]) % len(PALETTE)] + (150,),))
        else:
            out.append((16 + i % 4, 16 + i % 4, (40 + 50 * (i % 5), 255 - 60 * (i % 4), 30 + 70 * (i % 3), 60)))
    return out


def _segment_scene(C, counts, seed):
    """Tile row r holds counts[r] runs; the rows' runs are interleaved at random over the sorted positions (a chunk holds runs of
    several rows)."""
    g = np.random.Generator(np.random.PCG64(seed))
    plans = [_row_plan(n, C) for n in counts]
    owner = np.repeat(np.arange(len(counts)), counts)
    g.shuffle(owner)
    nxt = [0] * len(counts)
    shapes = []
    for r in owner:
        a, b, rgba = plans[r][nxt[r]]
        nxt[r] += 1
        if C == BLOCK and (a, b) == (0, C - 1):
            # (index.js:148 clamps a quad's half extent at 2 x 1024 px: asked for wider, the run is exactly the 4096 px of the frame)
            shapes.append(("raw", 8.0 * C, 16.0 * r + 8.0, 2300.0, 5.0, rgba, [(int(r), a, b)]))
        else:
            shapes.append(("run", int(r), a, b, rgba))
    return Built(16 * C, 16 * len(counts), shapes, off=40.0)


EDGE_COUNTS = {
    # G == 1 in k_lists (more than 128 tile columns): 0, 1, one segment less one / exact / plus one, sixteen segments exact / plus one
    # (the segment grows by 64, fewer items), and sixteen of THOSE plus one (it grows again)
    256: [0, 1, LIST_SEG - 1, LIST_SEG, LIST_SEG + 1, LIST_SEGS * LIST_SEG, LIST_SEGS * LIST_SEG + 1, LIST_SEGS * (LIST_SEG + 64) + 1],
    # G == 2 (at most 128 tile columns)
    128: [LIST_SEG + 1, 0, LIST_SEGS * LIST_SEG + 1, 1],
}


@pytest.fixture(scope="module", params=[256, 128])
def segments(request):
    C = request.param
    return C, _segment_scene(C, EDGE_COUNTS[C], seed=C)


def test_segment_length_steps_where_the_rows_are_placed():
    n = LIST_SEGS * LIST_SEG
    assert seg_len(n) == LIST_SEG and items(n) == LIST_SEGS
    assert seg_len(n + 1) == LIST_SEG + 64 and items(n + 1) == -(-(n + 1) // (LIST_SEG + 64)) < LIST_SEGS
    m = LIST_SEGS * (LIST_SEG + 64)
    assert seg_len(m) == LIST_SEG + 64 and seg_len(m + 1) == LIST_SEG + 128 and items(m + 1) <= LIST_SEGS
    assert max(EDGE_COUNTS[256]) > SEGC_RUNS_PER_ROW             # (a row the automatic choice would count in k_seg_count too)
    print("segment lengths:", {c: (seg_len(c), items(c)) for c in EDGE_COUNTS[256]})


def test_segment_edges_layout(segments):
    C, scene = segments
    assert scene.W == 16 * C and scene.want.shape == (len(EDGE_COUNTS[C]), C)
    for r, n in enumerate(EDGE_COUNTS[C]):
        if n >= 3:                                                  # every compared column: the first, a middle and the last segment
            assert scene.want[r, [0, 3, C * 100 // 256, C - 4, C - 1]].min() >= 3, (r, n)
            assert scene.want[r, [0, 3, C * 100 // 256, C - 4, C - 1]].max() <= 8, (r, n)
    assert_layout(scene, "segments%d" % C)


def test_segment_edges_forced_form_oracle_and_each_other(segments):
    C, scene = segments
    strips = [(0, 64), (16 * (C * 100 // 256), 16 * (C * 100 // 256) + 16), (16 * (C - 4), 16 * C)]
    assert_forms(scene, [(0, None)] + strips, strips, "segments%d" % C, paths=FORMS + ("walk",))


# ---------------------------------------------------------------- the automatic choice

def _auto_scene(n):
    """One tile row of 16 columns with n runs: single tiles in columns 0..7, and six strong two-column runs over columns 13..15."""
    shapes = []
    strong = {int(k * (n - 1) / 5) for k in range(6)}
    for p in range(n):
        if p in strong:
            k = len([q for q in strong if q < p])
            shapes.append(("run", 0, 13 + k % 2, 14 + k % 2, PALETTE[k] + (160,)))
        else:
            shapes.append(("run", 0, p % 8, p % 8, (30 + p % 200, 255 - p % 180, 90, 40)))
    return Built(256, 16, shapes)


AUTO = dict(PATH_OPTIONS["lists"])
AUTO[capi.OPT_SEG_COUNT] = 1


@pytest.mark.parametrize("extra", [0, 1])
def test_automatic_choice_at_its_threshold(extra):
    """GS_OPT_SEG_COUNT 1: a collected frame of exactly GS_SEGC_RUNS_PER_ROW x tile rows runs leaves the next frame without k_seg_count,
    one run more with it; a fresh and a cleared context start without; hinted or not, many runs or few, the frames are the lists'."""
    n = SEGC_RUNS_PER_ROW * 1 + extra
    scene = _auto_scene(n)
    few = (192, 256)                                                # columns 12..15: the six strong runs
    (want_all, want_few), idx, _ = draw(scene, "lists", views=[(0, None), few])
    with capi.Context(0) as c:
        c.set_option(capi.OPT_NEAR_PERMILLE, 1000)
        for k, v in AUTO.items():
            c.set_option(k, v)
        seen = []
        for cleared in (False, True):
            c.push_splat(scene.rows)
            assert np.array_equal(c.sort(scene.cam["view"]), idx)
            a = c.render(scene.params())                            # no hint yet, many runs
            sa = c.stats()
            b = c.render(scene.params())                            # hinted by frame a
            sb = c.stats()
            f = c.render(scene.params(*few))                        # hinted by frame b, six runs of its own
            sf = c.stats()
            g = c.render(scene.params())                            # hinted by the six-run frame
            sg = c.stats()
            seen.append([s["seg_count"] for s in (sa, sb, sf, sg)])
            assert sa["n_runs"] == n and sb["n_runs"] == n and sf["n_runs"] == 6 and sg["n_runs"] == n, (sa["n_runs"], sf["n_runs"])
            assert sa["row_walk"] == 0 and sa["binning"] == 0 and sa["subtile"] == 0
            for img in (a, b, g):
                assert np.array_equal(img, want_all), (extra, cleared)
            assert np.array_equal(f, want_few), (extra, cleared)
            c.clear()
        print("seg_count of (first, hinted, strip, after the strip) frames, fresh and cleared:", seen)
        assert seen[0] == seen[1] == [0, extra, extra, 0], (n, seen)
    want, _ = scene.oracle(idx, *few)
    pix_check("auto_%d" % n, want_few, want)


def test_option_values():
    with capi.Context(0) as c:
        for v in (0, 1, 2):
            c.set_option(capi.OPT_SEG_COUNT, v)
        for v in (-1, 3, 1 << 40):
            with pytest.raises(capi.GsError) as e:
                c.set_option(capi.OPT_SEG_COUNT, v)
            assert e.value.code == capi.E_BADARG


# ---------------------------------------------------------------- where the form must not apply; paired frames

@pytest.fixture(scope="module")
def cloud():
    return synth.make_splat_rows(20000, seed=4242)


def _cloud_frame(rows, cam, w, h, opts):
    with capi.Context(0) as c:
        for k, v in opts.items():
            c.set_option(k, v)
        c.push_splat(rows)
        c.sort(cam["view"])
        img = c.render(capi.make_params(cam["gs_mv"], cam["gs_proj"], w, h, focal_=cam["focal"]))
        return img, c.stats()


def test_forced_form_leaves_other_rounds_alone(cloud):
    """GS_OPT_SEG_COUNT 2 against 0 (same frames bit for bit): round 0 of one- and two-round frames takes the form (the statistic is
    round 0's; round 1 has no such kernel: its part of the frame is pinned by the equalities); a walked frame and a pair-record frame
    do not."""
    w, h = 640, 360
    cam = synth.index_html_camera(w, h, 200.0, capi=capi)
    base = dict(PATH_OPTIONS["lists"])
    one = None
    for permille in (1000, 3, 400):
        got = {}
        for v in (0, 2):
            got[v] = _cloud_frame(cloud, cam, w, h, {**base, capi.OPT_SEG_COUNT: v, capi.OPT_NEAR_PERMILLE: permille})
            st = got[v][1]
            assert (st["seg_count"], st["row_walk"], st["binning"]) == (1 if v else 0, 0, 0), (permille, v, st["seg_count"])
        assert np.array_equal(got[0][0], got[2][0]), permille
        assert got[0][1]["n_pairs"] == got[2][1]["n_pairs"] and got[0][1]["n_runs"] == got[2][1]["n_runs"] > 0
        print("forced form, %d permille: unsat_tiles %d, n_runs %d, n_pairs %d" % (permille, got[2][1]["unsat_tiles"], got[2][1]["n_runs"], got[2][1]["n_pairs"]))
        # (at 400 permille nothing here shows that round 1 had work: the equality then only says that a round 1 with little or nothing
        # to finish changed nothing.  That round 1 bins exactly the positions round 0 left is proven in test_chunk_seams, from the
        # per-tile lengths a recording two-round frame leaves.)
        if permille == 3:                                           # 60 splats saturate no frame: round 1 had tiles to finish, and did
            assert got[0][1]["unsat_tiles"] > 0 and got[2][1]["unsat_tiles"] == got[0][1]["unsat_tiles"], got[2][1]["unsat_tiles"]
        if one is None:
            one = got[2][0]
        assert np.array_equal(got[2][0], one), "the two-round frame (%d permille) is not the one-round frame" % permille
    for name, more, proof in (("walk", {capi.OPT_ROW_WALK: 2}, {"row_walk": 1, "binning": 0}), ("pairs", {capi.OPT_BINNING: 1}, {"row_walk": 0, "binning": 1})):
        got = {}
        for v in (0, 2):
            got[v] = _cloud_frame(cloud, cam, w, h, {**base, **more, capi.OPT_SEG_COUNT: v, capi.OPT_NEAR_PERMILLE: 1000})
            st = got[v][1]
            assert st["seg_count"] == 0 and {k: st[k] for k in proof} == proof, (name, v, st["seg_count"])
        assert np.array_equal(got[0][0], got[2][0]) and np.array_equal(got[2][0], one), name
    cs, cc, mats = oracle.pack(cloud)
    idx = oracle.sort(mats, cam["view"])
    want, _, _ = oracle.render(cs, cc, idx, cam["gs_mv"].astype(np.float32), cam["gs_proj"].astype(np.float32), cam["focal"], w, h, x0=304, x1=352,
                               want_f32=False)
    pix_check("forced_form_cloud", one[:, 304:352], want)


def test_forced_form_beyond_256_tile_rows_bins_pair_records():
    W, H = 64, 16 * (BLOCK + 1)
    cam = camera(W, H)
    rows = [splat(cam, 32.0, float(y), 20.0, 30.0, 2.0 + 0.01 * k, (200, 40, 90, 90)) for k, y in enumerate(range(8, H, 40))]
    scene = Scene(W, H, rows)
    got = {}
    for v in (0, 2):
        with capi.Context(0) as c:
            force_path(c, "lists")
            c.set_option(capi.OPT_SEG_COUNT, v)
            c.push_splat(scene.rows)
            idx = c.sort(scene.cam["view"])
            got[v] = [c.render(scene.params()), c.stats()]
        assert got[v][1]["seg_count"] == 0 and got[v][1]["binning"] == 1, (v, got[v][1]["seg_count"], got[v][1]["binning"])
    assert np.array_equal(got[0][0], got[2][0])
    pix_check("forced_form_tall", got[2][0], scene.oracle(idx)[0])


def test_paired_queued_frames_forced_form(cloud):
    """GS_OPT_FRAME_BATCH 2 with the form forced (the twin of k_seg_count and of k_lists<0, true>) == the synchronous segc frames, one
    round and two."""
    _paired_equal_synchronous(cloud, "segc")
    _paired_equal_synchronous(cloud, "segc", near_permille=400)


# ---------------------------------------------------------------- k_emit_runs: its three traversal classes in one chunk

SPANS = (1, 2, 3, 16, 17, 64, 65, 66, 129, 256)                    # tile rows: own thread (1-2), 16 lanes (3-16), a wavefront (17 and more)


def _class_scene(spans, seed, with_half_present):
    """One chunk (GS_BLOCK sorted positions) of a 64 x 4096 frame: position p is a splat of spans[p % len] tile rows (tall(); one row: a
    run of one tile)."""
    g = np.random.Generator(np.random.PCG64(seed))
    W, H = 64, 16 * BLOCK
    shapes = []
    for p in range(BLOCK):
        R = spans[p % len(spans)]
        r0 = int(g.integers(0, BLOCK - R + 1))
        if R == 1:
            col = int(g.integers(0, 4))
            shapes.append(("run", r0, col, col, PALETTE[p % len(PALETTE)] + (150,)))
        else:
            shapes.append(("tall", r0, r0 + R - 1, PALETTE[p % len(PALETTE)] + (40,)))
    half = None
    if with_half_present:
        # a two-row splat, 40 x 16 px around (46, 16 r0 + 10): 2 px of it reach into row r0 + 1, a cap between x = 32.8 and 59.2 (by
        # area; 34.3 .. 57.7 by pixel centres: the same tiles).  Row r0: x from 26 on -> columns 1..3; row r0 + 1: columns 2..3.  In the
        # strip [8, 28) only row r0 has a tile: the packed record's two `present` bits differ.
        half, r0 = 37, 150
        shapes[half] = ("raw", 46.0, 16.0 * r0 + 10.0, 20.0, 8.0, (255, 255, 255, 200), [(r0, 1, 3), (r0 + 1, 2, 3)])
    return Built(W, H, shapes), half


@pytest.fixture(scope="module")
def classes():
    return _class_scene(SPANS, 11, True)


def test_emit_classes_layout(classes):
    scene, half = classes
    assert scene.n == BLOCK and scene.n % BLOCK == 0             # one aligned chunk (asserted kept and visible by assert_layout)
    assert sorted(set(int(t) for k, t in enumerate(scene.tiles) if k != half)) == sorted(4 * s if s > 1 else 1 for s in SPANS)
    assert_layout(scene, "classes")


def test_emit_classes_frame_and_strips_off_a_tile_boundary(classes):
    scene, half = classes
    views = [(0, None), (8, 64), (8, 28), (5, 37)]
    assert_forms(scene, views, views, "classes", frags_views=views)
    for p in FORMS:                                                 # only one of the two rows has a tile inside [8, 28)
        _, st, lens, _, tc = frame(scene, p, 8, 28, staged=True)
        assert tc[half] == 1, (p, int(tc[half]))
        assert lens.shape == (BLOCK, 2)


def test_emit_a_chunk_of_wavefront_splats_only():
    scene, _ = _class_scene(tuple(s for s in SPANS if s >= 17), 12, False)
    assert_layout(scene, "big_only")
    assert_forms(scene, [(0, None), (12, 60)], [(0, None), (12, 60)], "big_only", frags_views=[(0, None), (12, 60)])


# ---------------------------------------------------------------- k_row_scan: 256 runs and 65 536 tiles in one row word

def _wide_chunk_scene(k, H):
    """k splats that cover every tile of a 4096 x H frame at consecutive sorted positions.  k == GS_BLOCK: the scene is one chunk and
    nothing else.  Otherwise two chunks, the k splats last (one less: chunk 1 starts with a single-tile run; one more: the surplus is
    chunk 0's last position) and single-tile runs of row 0 at every other position."""
    W, n = 16 * BLOCK, BLOCK if k == BLOCK else 2 * BLOCK
    rows_y = (H + 15) // 16
    shapes = []
    for p in range(n):
        if p >= n - k:
            # (the half extent asked for is clamped at 2048 px, index.js:148: x = 0 .. 4096; 400 px high: every corner tile is inside)
            shapes.append(("raw", W / 2.0, H / 2.0, 2300.0, 400.0, PALETTE[p % len(PALETTE)] + (5 + p % 7,), [(r, 0, BLOCK - 1) for r in range(rows_y)]))
        else:
            shapes.append(("run", 0, p % BLOCK, p % BLOCK, (255 - p % 200, 40 + p % 190, 20, 120)))
    return Built(W, H, shapes, off=40.0)


@pytest.mark.parametrize("k,H", [(BLOCK, 48), (BLOCK - 1, 16), (BLOCK + 1, 16)])
def test_row_word_of_256_runs_and_65536_tiles(k, H):
    scene = _wide_chunk_scene(k, H)
    rows_y = (H + 15) // 16
    if k == BLOCK:
        assert scene.n == BLOCK and (scene.want == BLOCK).all() and scene.want.sum() == BLOCK * BLOCK * rows_y
    else:
        assert scene.want.min() >= k and scene.want.sum() == k * BLOCK * rows_y + 2 * BLOCK - k
    assert_layout(scene, "row_word_%d" % k)                         # n_pairs, and k entries (and the single tiles) in every tile
    strips = [(0, 32), (2040, 2072), (4064, 4096)]
    assert_forms(scene, [(0, None)] + strips, strips, "row_word_%d" % k, paths=FORMS + ("walk",))


# ---------------------------------------------------------------- chunk seams, one round and two

def near_count(permille, n):
    """gs_share_near_count of csrc/gs_share.h: ceil((double)(float)(permille / 1000) * n), at least 1.  (A mirror the scenes are placed
    from; test_chunk_seams proves from the frames' own per-tile records that round 0 covered exactly this many positions.)"""
    return max(1, int(math.ceil(float(np.float32(permille) / np.float32(1000.0)) * n)))


def _seam_scene(n, nc):
    """Tile row 0 holds runs at the seams of the rounds' chunks only -- relative to a round's first position: 0, 255, 256, 257, 511, 512
    and the round's last (the last position of a partial final chunk) --, tile row 1 the runs of every other position.  Round 0 of a
    two-round frame covers the last nc positions, round 1 the others: a chunk starts at the ROUND's first position."""
    ranges = [(0, n)] if nc >= n else [(n - nc, n), (0, n - nc)]
    seams = set()
    for lo, hi in ranges:
        seams |= {lo + o for o in (0, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK) if lo + o < hi} | {hi - 1}
    shapes, k = [], 0
    for p in range(n):
        if p in seams:
            shapes.append(("run", 0, k % 4, 4 + k % 5, PALETTE[k % len(PALETTE)] + (110,)))    # all of them cover column 4
            k += 1
        else:
            shapes.append(("run", 1, p % 10, p % 10, (60 + p % 190, 200 - p % 150, 250 - p % 240, 50)))
    return Built(160, 32, shapes), len(seams)


SEAM_CASES = [(1000, 1000), (1000, 255), (1024, 250), (1000, 256)]     # (splats, permille): one round; near_count 255, 256, 257


def test_seam_cases_are_what_they_claim():
    assert [near_count(p, n) for n, p in SEAM_CASES[1:]] == [BLOCK - 1, BLOCK, BLOCK + 1]
    assert all(n % BLOCK for n, _ in SEAM_CASES[:2])                # a partial final chunk


@pytest.mark.parametrize("n,permille", SEAM_CASES)
def test_chunk_seams(n, permille):
    scene, nseams = _seam_scene(n, near_count(permille, n) if permille < 1000 else n)
    assert scene.want[0, 4] == nseams and scene.want[0].max() == nseams and scene.want[1].sum() == n - nseams
    assert_layout(scene, "seams_%d_%d" % (n, permille))
    imgs, idx = assert_forms(scene, [(0, None), (64, 80)], [(0, None)], "seams_%d_%d" % (n, permille), paths=FORMS + ("walk",), near=permille)
    if permille < 1000:                                             # two rounds draw the one-round frame
        one, _, _ = draw(scene, "segc")
        assert np.array_equal(imgs["segc"][0], one[0])
        # what the frame itself says about the rounds' extents: a recording frame leaves every tile the length of the list it was
        # drawn from LAST -- round 1's (no tile of this scene saturates: rows 0..2 of every tile are bare) --, and those are the lengths
        # of the positions before n - near_count alone, so round 0 covered the near_count positions the seams were placed from
        nc = near_count(permille, n)
        for p in FORMS:
            _, st, lens, _, _ = frame(scene, p, near=permille, staged=True)
            assert st["n_pairs"] == scene.want.sum() and (p == "pairs" or st["n_runs"] == scene.runs), (p, st["n_runs"], st["n_pairs"])
            assert np.array_equal(lens, scene.want_of(0, n - nc)), (p, n, nc, int(lens.sum()), int(scene.want_of(0, n - nc).sum()))
            assert not np.array_equal(lens, scene.want_of(0, n - nc - 1)) and not np.array_equal(lens, scene.want_of(0, n - nc + 1))
