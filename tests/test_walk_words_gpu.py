"""GPU tier: the row walk's 16-bit run words (csrc/gs_render.hip: k_emit_runs_body<0, true> writes first column | (tiles - 1) << 8 per
run, the WALK branch of k_blend_body examines 128 of them per step -- lane l the dword of runs 2 (D - l) and 2 (D - l) + 1 -- and reads
a hit's sorted position only when its slot is staged).  The standard is test_row_walk_gpu's: a walked frame IS the list frame
(GS_OPT_ROW_WALK 0) of the same scene and pose, bit for bit -- image, unsaturated-tile mask, need record, completion word, unsat_tiles.

What a 2-byte word can get wrong, each a case here: rows that begin or end in the middle of a dword (the other half is the
neighbouring row's run: a loud splat of both rows, which a walk that took that half would blend twice); first column 0 and last column 255, 256 tiles stored
as 255, one tile stored as 0; the run that takes a batch's last slot in either half of lane 0's, a middle lane's and lane 63's
dword with more hits behind it; last steps of 1, 2 and 127 runs; strips off the tile grid; frames drawn in pairs; and a list frame
after a walked one on the same context (32-bit words again where k_lists reads them).

Scenes are test_binning_edges_gpu.Built's (one shape per sorted position, 0 = farthest; a tile row's runs keep that order).  The
cases are placed from `steps()`, a mirror of the walk's step schedule in plain Python, and every case asserts from it that it is
the case it claims to be; the list lengths the construction gives are asserted on the lists path before a frame is compared."""
import numpy as np
import pytest

from conftest import pkg
from test_binning_edges_gpu import PALETTE, Built
from test_blend_paths_gpu import list_lengths
from test_gpu_parity import assert_path, force_path, pix_check

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

TARGET = 4                                                 # the compared tile column of the 10-column scenes
HIT_SHAPES = [(4, 4), (2, 6), (4, 9), (0, 4), (3, 5)]
MISS_SHAPES = [(3, 3), (0, 3), (5, 5), (5, 9), (1, 3), (6, 8)]
KEPT = ("n_pairs", "n_visible", "need_splats", "near_permille", "unsat_tiles")


def steps(first, hits):
    """The walk of a tile row whose runs are [first, first + len(hits)) of the run array, hits[k]: run first + k covers the column.
    Per step (lo, cur, entries before, hits, seam) with seam = None, or (index of the run that takes slot 63, half, lane) when the
    step holds more hits than free slots; then the batches' sizes."""
    cur, nb, out, batches = first + len(hits), 0, [], []
    while cur > first:
        D = (cur - 1) >> 1
        lo = max(first, 2 * (D - 63))
        idx = [i for i in range(cur - 1, lo - 1, -1) if hits[i - first]]
        if nb + len(idx) > 64:
            s = idx[63 - nb]
            out.append((lo, cur, nb, len(idx), (s, s & 1, D - (s >> 1))))
            cur, nb = s, 64
        else:
            out.append((lo, cur, nb, len(idx), None))
            cur, nb = lo, nb + len(idx)
        if nb == 64 or cur == first:
            if nb:
                batches.append(nb)
            nb = 0
    return out, batches


def row_shapes(ty, hits, loud=(), alpha=3, seed=0):
    """Tile row ty: run k covers TARGET iff hits[k]; `loud` runs are strong and saturated in colour, the others faint."""
    g = np.random.Generator(np.random.PCG64(seed + 1000 * ty))
    out, nh, nm = [], 0, 0
    for k, h in enumerate(hits):
        if h:
            a, b = HIT_SHAPES[nh % len(HIT_SHAPES)]; nh += 1
        else:
            a, b = MISS_SHAPES[nm % len(MISS_SHAPES)]; nm += 1
        if k in loud:
            rgba = PALETTE[(k + 3 * ty) % len(PALETTE)] + (90,)
        else:
            rgba = (int(g.integers(0, 256)), int(g.integers(0, 256)), int(g.integers(0, 256)), alpha if h else 6)
        out.append(("run", ty, a, b, rgba))
    return out


def record(c, scene, x0=0, x1=None, **kw):
    """One frame and everything the blend leaves behind."""
    img = c.render(scene.params(x0, x1, **kw))
    st = c.stats()
    tx, ty = (scene.W + 15) // 16, (scene.H + 15) // 16
    mask = c.download(capi.BUF_UNSAT_MASK, ty, np.uint32, (tx + 31) // 32)
    return img, mask, c.frame_status(), {k: st[k] for k in KEPT}


def walk_equals_lists(scene, views, tag, near=(1000,), oracle_views=()):
    """Every view at every first-round share: walked == listed in image, mask, completion word and statistics; the list frame within
    the oracle's bar on oracle_views."""
    got = {}
    for p in ("lists", "walk"):
        got[p] = []
        with capi.Context(0) as c:
            force_path(c, p)
            c.push_splat(scene.rows)
            idx = c.sort(scene.cam["view"])
            assert np.array_equal(idx, np.arange(scene.n, dtype=idx.dtype)), (tag, "the order is not the one built")
            for permille in near:
                c.set_option(capi.OPT_NEAR_PERMILLE, permille)
                for x0, x1 in views:
                    got[p].append(((permille, x0, x1), record(c, scene, x0, x1)))
                    assert_path(c, p, (tag, permille, x0, x1))
    for (ka, a), (kb, b) in zip(got["lists"], got["walk"]):
        assert ka == kb
        assert np.array_equal(a[0], b[0]), (tag, ka, "pixels", int(np.abs(a[0].astype(int) - b[0].astype(int)).max()))
        assert np.array_equal(a[1], b[1]), (tag, ka, "unsaturated-tile mask")
        assert a[2] == b[2], (tag, ka, "completion word", a[2], b[2])
        assert a[3] == b[3], (tag, ka, a[3], b[3])
    for (permille, x0, x1), a in got["lists"]:
        if permille == near[0] and (x0, x1) in oracle_views:
            pix_check("%s_%d_%s" % (tag, x0, x1), a[0], scene.oracle(idx, x0, x1)[0])
    return got


def assert_lengths(scene, tag):
    lens = list_lengths(scene).astype(np.int64)
    bad = np.argwhere(lens != scene.want)
    assert not len(bad), "%s: %d tiles differ from the construction, first (row, column) %s: %d entries, built %d" % (
        tag, len(bad), bad[0].tolist(), lens[tuple(bad[0])], scene.want[tuple(bad[0])])


def count_frags_equal_oracle(scene, x0, x1, tag):
    """The entries of the compared tiles, counted by the list path (a counting frame never walks) == the oracle's fragments."""
    with capi.Context(0) as c:
        force_path(c, "lists")
        c.push_splat(scene.rows)
        idx = c.sort(scene.cam["view"])
        c.render(scene.params(x0, x1, flags=capi.RENDER_COUNT_FRAGS))
        got = c.stats()["n_frags"]
    want = scene.oracle(idx, x0, x1)[1]
    print("fragments", tag, (x0, x1), got, "oracle", want)
    assert got == want, (tag, got, want)


# ---------------------------------------------------------------- row length and alignment

ROW_RUNS = [0, 1, 2, 63, 64, 65, 127, 128, 129, 257]


def _aligned_scene(lead):
    """Tile row r holds ROW_RUNS[r] runs -- behind `lead` runs of a tile row in front, so that a row that begins at an even offset of
    the run array in one scene begins at an odd one in the other.  Every third run of a row's own covers TARGET.  Between two
    neighbouring rows lies a loud splat of BOTH rows, column TARGET alone in each, nearer than every run of the upper row and farther
    than every run of the lower: it is the upper row's last run and the lower row's first, the two halves a shared dword holds.  A
    walk that took the half of the neighbouring row would blend that splat twice.  (A run of another row that is not in the tile's
    own list never shows: it covers no pixel of the tile.)"""
    counts = ([lead] if lead else []) + ROW_RUNS
    budget = list(counts)
    joint = []
    for r in range(len(counts) - 1):                               # (a row of one run has one such neighbour, an empty row none)
        joint.append(budget[r] >= 1 and budget[r + 1] >= 1)
        if joint[-1]:
            budget[r] -= 1; budget[r + 1] -= 1
    shapes, first, firsts = [], 0, []
    for ty, n in enumerate(counts):
        m = budget[ty]
        shapes += row_shapes(ty, [k % 3 == 0 or k == m - 1 for k in range(m)], loud={0, m - 1}, seed=lead)
        if ty < len(joint) and joint[ty]:
            shapes.append(("raw", 16.0 * TARGET + 8.0, 16.0 * (ty + 1), 7.5, 12.0, PALETTE[ty % len(PALETTE)] + (90,), [(ty, TARGET, TARGET), (ty + 1, TARGET, TARGET)]))
        firsts.append(first)
        first += n
    return Built(160, 16 * len(counts), shapes), counts, firsts, joint


@pytest.mark.parametrize("lead", [0, 1])
def test_rows_of_every_length_at_even_and_odd_offsets(lead):
    scene, counts, firsts, joint = _aligned_scene(lead)
    base = np.cumsum([0] + ROW_RUNS[:-1])
    assert [f - lead for f in firsts[-len(ROW_RUNS):]] == base.tolist() and {int(f) & 1 for f in base} == {0, 1}   # either parity, then the other
    assert counts[-1] == 257 and scene.runs == sum(counts)         # (the frame's first and last tile rows are cases too)
    assert all(joint[r] for r in range(len(counts) - 1) if counts[r] >= 2 and counts[r + 1] >= 2)
    assert_lengths(scene, "aligned%d" % lead)
    with capi.Context(0) as c:                                      # the runs of every tile row, as the walked frame counts them
        force_path(c, "walk")
        c.push_splat(scene.rows)
        c.sort(scene.cam["view"])
        c.render(scene.params())
        assert c.stats()["n_runs"] == sum(counts)
    strip = (16 * TARGET, 16 * TARGET + 16)
    count_frags_equal_oracle(scene, *strip, "aligned%d" % lead)
    walk_equals_lists(scene, [(0, None), strip], "aligned%d" % lead, oracle_views=[strip])


# ---------------------------------------------------------------- the word's range

def _wide(full):
    """4096 x 16: runs that start in column 0 and end in column 255, single tiles in columns 0, 100 and 255 and -- `full` -- runs of
    all 256 tiles (tiles - 1 = 255 in the word's high byte; index.js:148 clamps the quad at 2 x 1024 px: asked for wider, the run is
    the frame).  Without them columns 4..99 are covered by nothing: empty lists, the background."""
    shapes = []
    for k in range(3):
        shapes += [("run", 0, 0, 3, PALETTE[0] + (70,)), ("run", 0, 250, 255, PALETTE[1] + (70,)), ("run", 0, 0, 0, PALETTE[2] + (70,)),
                   ("run", 0, 255, 255, PALETTE[3] + (70,)), ("run", 0, 100, 100, PALETTE[4] + (70,)), ("run", 0, 101, 249, PALETTE[6] + (30,))]
        if full:
            shapes.append(("raw", 2048.0, 8.0, 2300.0, 5.0, PALETTE[5] + (60,), [(0, 0, 255)]))
    return Built(4096, 16, shapes, off=40.0)


@pytest.mark.parametrize("full", [True, False])
def test_first_column_0_last_column_255_one_tile_and_256_tiles(full):
    scene = _wide(full)
    assert scene.want[0, 0] == (9 if full else 6) and scene.want[0, 255] == (9 if full else 6) and scene.want[0, 50] == (3 if full else 0)
    assert scene.want[0, 100] == (6 if full else 3) and scene.want[0, 4] == (3 if full else 0)
    assert_lengths(scene, "wide%d" % full)
    strips = [(0, 32), (784, 816), (1600, 1632), (4064, 4096)]
    for s in strips:
        count_frags_equal_oracle(scene, *s, "wide%d" % full)
    got = walk_equals_lists(scene, [(0, None)] + strips, "wide%d" % full, oracle_views=strips)
    if not full:                                                    # tile 50: no run, the background
        assert (got["walk"][0][1][0][:, 784:816] == np.array([0, 0, 0, 255], np.uint8)).all()


# ---------------------------------------------------------------- the overflow seam

def _seam_hits(kind, n):
    """hits of a row of n runs (index 0 = farthest) so that the first batch's last slot is taken as `kind` says, by a step with more
    than 64 hits in it (n even, the row at offset 0: a step is 128 runs, lane l holds runs n - 2 - 2 l and n - 1 - 2 l)."""
    h = [True] * n
    if kind in ("lane0", "lane63"):
        miss = range(n - 128, n, 2) if kind == "lane0" else range(n - 126, n, 2)
        for i in list(miss) + ([n - 127] if kind == "lane0" else []):   # 63 hits in front of the seam run
            h[i] = False
    return h


SEAMS = {  # kind: (lead runs in a row in front, runs, (half, lane) of the run that takes slot 63)
    "even": (0, 330, (0, 31)), "odd": (1, 330, (1, 32)), "lane0": (0, 400, (1, 0)), "lane63": (0, 330, (1, 63)),
}


@pytest.mark.parametrize("kind", sorted(SEAMS))
def test_batch_ends_inside_a_step_in_either_half(kind):
    lead, n, where = SEAMS[kind]
    hits = _seam_hits(kind, n)
    sched, batches = steps(lead, hits)
    seams = [s for s in sched if s[4] is not None]
    first = seams[0]
    print(kind, "steps", sched[:4], "batches", batches)
    assert first[3] > 64 and first[1] - first[0] <= 128 and first[4][1:] == where, (kind, first)
    assert len(batches) >= 3 and sum(batches) == sum(hits)
    # the seam run and its neighbours loud: taken twice or skipped, each shows
    s = first[4][0] - lead
    loud = {i for i in (s - 2, s - 1, s, s + 1, s + 2) if 0 <= i < n}
    shapes = (row_shapes(0, [True] * lead, loud={0}) if lead else []) + row_shapes(1 if lead else 0, hits, loud=loud, alpha=2)
    scene = Built(160, 32 if lead else 16, shapes)
    assert scene.want[-1, TARGET] == sum(hits)
    assert_lengths(scene, "seam_" + kind)
    strip = (16 * TARGET, 16 * TARGET + 16)
    count_frags_equal_oracle(scene, *strip, "seam_" + kind)
    walk_equals_lists(scene, [(0, None), strip], "seam_" + kind, oracle_views=[strip])
    with capi.Context(0) as c:                                      # low opacity: the tile reads its whole list, every batch is compared
        force_path(c, "lists")
        c.set_option(capi.OPT_RECORD_STAGED, 2)
        c.push_splat(scene.rows)
        c.sort(scene.cam["view"])
        c.render(scene.params())
        evaluated = int(c.download(capi.BUF_TILE_STATS, scene.want.size, np.uint32, 2)[scene.want.size - 10 + TARGET, 0])
    assert evaluated >= sum(hits) - 1, (kind, evaluated, sum(hits))


# ---------------------------------------------------------------- a last partial step

@pytest.mark.parametrize("lead,n,last", [(1, 256, 1), (0, 258, 2), (1, 255, 127)])
def test_last_step_of_1_2_and_127_runs(lead, n, last):
    hits = [k % 9 == 0 or k < 3 or k == n - 1 for k in range(n)]   # sparse: no batch fills, every step is a whole one
    sched, batches = steps(lead, hits)
    assert all(s[4] is None for s in sched) and len(batches) == 1 and batches[0] < 64
    assert sched[-1][1] - sched[-1][0] == last and len(sched) >= 2 and all(s[1] - s[0] >= 127 for s in sched[:-1]), sched
    shapes = (row_shapes(0, [True] * lead, loud={0}) if lead else []) + row_shapes(1 if lead else 0, hits, loud={0, 1, 2, n - 1})
    scene = Built(160, 32 if lead else 16, shapes)
    assert_lengths(scene, "partial%d" % last)
    strip = (16 * TARGET, 16 * TARGET + 16)
    walk_equals_lists(scene, [(0, None), strip], "partial%d" % last, oracle_views=[strip])


# ---------------------------------------------------------------- strips, two rounds, pairs, a list frame after a walked one

def test_strips_off_the_tile_grid():
    """x0 off a tile boundary (the tile columns shift: other runs, other words) and a right edge inside a lane's group of 4 pixels."""
    scene = _aligned_scene(1)[0]
    views = [(52, 68), (56, 150), (4, 21), (12, 160)]
    walk_equals_lists(scene, views, "strips", oracle_views=views[:1])


@pytest.fixture(scope="module")
def cloud():
    return synth.make_splat_rows(20000, seed=4242)


def _cloud_params(cam, w, h, flags=0):
    return capi.make_params(cam["gs_mv"], cam["gs_proj"], w, h, focal_=cam["focal"], flags=flags)


def test_twelve_queued_frames_in_pairs_equal_their_synchronous_twins(cloud):
    w, h = 320, 180
    cams = [synth.index_html_camera(w, h, 30.0 * k, capi=capi) for k in range(12)]
    with capi.Context(0) as c:
        force_path(c, "lists")
        c.push_splat(cloud)
        want = []
        for cam in cams:
            c.sort(cam["view"])
            want.append(c.render(_cloud_params(cam, w, h)))
            assert_path(c, "lists")
    with capi.Context(0) as c:
        force_path(c, "walk")
        c.set_option(capi.OPT_FRAME_BATCH, 2)
        c.push_splat(cloud)
        bufs = [capi.host_frame(h, w) for _ in cams]
        for (b, _), cam in zip(bufs, cams):
            c.sort(cam["view"], want_indices=False)
            c.render_into(_cloud_params(cam, w, h, capi.RENDER_ASYNC), b)
        c.sync()
        assert_path(c, "walk", "paired")
        for k, ((b, o), wnt) in enumerate(zip(bufs, want)):
            d = int(np.abs(b.astype(int) - wnt.astype(int)).max())
            o.free()
            assert d == 0, ("queued walked frame", k, d)


def test_list_frame_and_two_round_frame_after_a_walked_one(cloud):
    """One context: walked, listed (k_lists reads 32-bit run words where the walked frame left 16-bit ones), walked over two rounds
    (round 1 keeps the lists), listed over two rounds, walked again -- each the frame a fresh list context draws, with its records."""
    w, h = 640, 360
    cam = synth.index_html_camera(w, h, 200.0, capi=capi)
    tx, ty = (w + 15) // 16, (h + 15) // 16
    seq = [(2, 1000), (0, 1000), (2, 3), (0, 3), (2, 400), (0, 400), (2, 1000)]

    def one(c, walk, permille):
        c.set_option(capi.OPT_ROW_WALK, walk)
        c.set_option(capi.OPT_NEAR_PERMILLE, permille)
        img = c.render(_cloud_params(cam, w, h))
        st = c.stats()
        assert st["row_walk"] == (1 if walk else 0) and st["binning"] == 0
        return img, c.download(capi.BUF_UNSAT_MASK, ty, np.uint32, (tx + 31) // 32), c.frame_status(), {k: st[k] for k in KEPT}

    with capi.Context(0) as c:
        force_path(c, "walk")
        c.push_splat(cloud)
        c.sort(cam["view"])
        got = [one(c, wk, pm) for wk, pm in seq]
    want = {}
    for pm in (1000, 3, 400):
        with capi.Context(0) as c:
            force_path(c, "lists")
            c.push_splat(cloud)
            c.sort(cam["view"])
            want[pm] = one(c, 0, pm)
    assert want[3][1].any(), "no frame left a tile to the second round"
    for (wk, pm), g in zip(seq, got):
        r = want[pm]
        assert np.array_equal(g[0], r[0]), (wk, pm, "pixels")
        assert np.array_equal(g[1], r[1]) and g[2] == r[2] and g[3] == r[3], (wk, pm, g[2], r[2], g[3], r[3])
