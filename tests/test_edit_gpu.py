"""GPU tier: editing the resident cloud (include/gs_splat.h: gs_set_state ... gs_compact).

The one claim everything rests on: a splat whose state byte has GS_STATE_HIDDEN is, in every depth sort, a splat outside the cutout.  So a
context with the set H hidden sorts exactly as the reference sorts the scene WITHOUT the rows of H, and the unchanged CPU oracle checks it
bit for bit: with kept = flatnonzero(~H), ctx.sort(view, cut) == kept[oracle.sort(rows[kept], view, cut)].  Frames are compared with those
of a fresh context that was pushed rows[kept] (bit-identical), region selections with f64 numpy mirrors written in the operation order the
header states, gs_compact with a fresh context fed the kept rows.

Sizes are placed from the depth pass' own chunking, DCHUNK = GS_DEPTH_IPT * GS_BLOCK, read out of the sources.  Where a case claims
something about its own input, the claim is asserted from the input before the GPU's answer is looked at."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT, cached_rows, pkg
from oracle import oracle
from test_gpu_parity import _hostile_floats
from test_sort_paths_gpu import _constant

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

DCHUNK = _constant("GS_DEPTH_IPT", "gs_sort.hip") * _constant("GS_BLOCK", "gs_internal.h")
PAIR_MIN_N = _constant("GS_DEPTH_PAIR_MIN_N", "gs_sort.hip")
HIDDEN, SELECTED, INVERT = capi.STATE_HIDDEN, capi.STATE_SELECTED, capi.SELECT_INVERT
VIEW = np.array([0.0, 0.0, 1.0, 0.0], np.float32)
SIZES = [1, 2, DCHUNK - 1, DCHUNK, DCHUNK + 1, 3 * DCHUNK + 17]


def mats_of(rows4):
    m = np.zeros((len(rows4), 16), np.float32)
    m[:, 12:16] = rows4
    return m


def sort_ctx(rows4, states=None, wide=False):
    c = capi.Context(0)
    if wide:
        c.set_option(capi.OPT_WIDE_PAIRS, 1)
    c.push_matrices(mats_of(rows4))
    if states is not None and len(states):
        c.set_state(0, states)
    return c


def want_order(rows4, H, view, cut=None):
    kept = np.flatnonzero(~H).astype(np.uint32)
    if not kept.size:
        return np.zeros(0, np.uint32)
    return kept[oracle.sort(rows4[kept], view, cut)]


def plain_rows(g, n):
    """well-behaved rows: nothing culled by size, distinct depths likely"""
    r = np.zeros((n, 4), np.float32)
    r[:, :3] = g.normal(0.0, 2.0, (n, 3))
    r[:, 2] = -np.abs(r[:, 2]) - 0.5
    r[:, 3] = 100.0
    return r


def hostile_rows(g, n):
    r = _hostile_floats(g, n * 4).reshape(n, 4)
    r[:, 3] = np.abs(r[:, 3]) * 0.01
    return r


def extreme_rows(g, n, which):
    """One splat alone holds minDepth (or maxDepth), far from the others, whose depths are a quarter of a bucket apart: with the lone
    splat the bucket scale is ~1 per unit of depth and four depths share a bucket (ordered by index); without it the range halves, the
    scale doubles and they part -- the order of the OTHERS must change."""
    r = np.zeros((n, 4), np.float32)
    r[:, 3] = 100.0
    q = g.integers(0, 4 * 32000, n).astype(np.float64) * 0.25
    lone = int(g.integers(0, n))
    if which == "min":
        r[:, 2] = (-1.0 - q).astype(np.float32); r[lone, 2] = -65536.0
        assert (r[:, 2] == r[:, 2].min()).sum() == 1 and int(np.argmin(r[:, 2])) == lone
    else:
        r[:, 2] = (-65536.0 + q).astype(np.float32); r[lone, 2] = -1.0
        assert (r[:, 2] == r[:, 2].max()).sum() == 1 and int(np.argmax(r[:, 2])) == lone
    return r, lone


# ---------------------------------------------------------------- hidden equals removed

def hidden_cases(n):
    """(name, rows, view, hidden set, store length) for n splats: only splat 0, only splat n - 1 (the clamped load index), every splat,
    a random half, a store that ends mid-chunk -- on well-behaved and on hostile rows -- and, from DCHUNK - 1 splats on, the splat that
    alone holds minDepth / maxDepth (asserted: the oracle's order of the others changes)."""
    g = np.random.Generator(np.random.PCG64(4100 + n))
    cases = []
    for fam, rows, view in (("plain", plain_rows(g, n), VIEW), ("hostile", hostile_rows(g, n), g.normal(0.0, 1.0, 4).astype(np.float32))):
        first = np.zeros(n, bool); first[0] = True
        last = np.zeros(n, bool); last[n - 1] = True
        half = g.random(n) < 0.5
        cases += [(fam + "/first", rows, view, first, n), (fam + "/last", rows, view, last, n), (fam + "/all", rows, view, np.ones(n, bool), n),
                  (fam + "/half", rows, view, half, n)]
        short = max(1, n - DCHUNK // 2 - 3)                          # a store that ends mid-chunk: the splats behind it are state 0
        Hs = half.copy(); Hs[short:] = False
        cases.append((fam + "/short", rows, view, Hs, short))
    if n >= DCHUNK - 1:
        for which in ("min", "max"):
            rows, lone = extreme_rows(g, n, which)
            H = np.zeros(n, bool); H[lone] = True
            full = oracle.sort(rows, VIEW)
            assert full.size == n and not np.array_equal(full[full != lone], want_order(rows, H, VIEW)), "the bucket scale did not move"
            cases.append(("extreme/" + which, rows, VIEW, H, n))
    return g, cases


@pytest.mark.parametrize("n", SIZES)
def test_hidden_equals_removed(n):
    g, cases = hidden_cases(n)
    for name, rows, view, H, store in cases:
        want = want_order(rows, H, view)
        with sort_ctx(rows, H[:store].astype(np.uint8) | (g.integers(0, 64, store).astype(np.uint8) << 2)) as c:   # (user bits change nothing)
            got = c.sort(view)
            assert np.array_equal(got, want), (name, n)
            assert c.state_count() == (store, int(H.sum())), name
            assert c.stats()["n_hidden"] == int(H.sum()), name


# the box of the cutout variant: 0.2 x the position, centred at z = -2 -- keeps |x|, |y| <= 2.5 and -4.5 <= z <= 0.5
CUT = np.zeros(16, np.float32); CUT[0] = CUT[5] = CUT[10] = 0.2; CUT[14] = 0.4; CUT[15] = 1.0


@pytest.mark.parametrize("variant", ["wide", "cutout", "posted"])
@pytest.mark.parametrize("n", SIZES)
def test_hidden_equals_removed_variants(n, variant):
    """the same check -- every size, every hidden set -- with GS_OPT_WIDE_PAIRS 1, with a cutout, and through gs_sort_begin / gs_sort_poll"""
    _, cases = hidden_cases(n)
    cut = CUT if variant == "cutout" else None
    some = 0
    for name, rows, view, H, store in cases:
        want = want_order(rows, H, view, cut)
        some += 0 < want.size < (~H).sum()
        with sort_ctx(rows, H[:store].astype(np.uint8), wide=variant == "wide") as c:
            if variant == "posted":
                c.sort_begin(view)
                got = c.sort_poll(wait=True)
            else:
                got = c.sort(view, cut)
            assert np.array_equal(got, want), (name, n, variant)
    assert variant != "cutout" or n < DCHUNK - 1 or some >= 2, "the cutout never cut"


def test_state_change_or_compact_under_a_posted_sort():
    """a sort begun before an edit is run again over what is resident when it is collected -- gs_compact included"""
    n = DCHUNK + 1
    g = np.random.Generator(np.random.PCG64(4250))
    rows = plain_rows(g, n)
    H = g.random(n) < 0.5
    kept = np.flatnonzero(~H)
    with sort_ctx(rows, H.astype(np.uint8)) as c:
        c.sort_begin(VIEW)
        c.set_state(0, np.zeros(n, np.uint8))
        assert np.array_equal(c.sort_poll(wait=True), oracle.sort(rows, VIEW)), "states cleared meanwhile"
        c.set_state(0, H.astype(np.uint8))
        c.sort_begin(VIEW)
        assert np.array_equal(c.compact(), kept)
        assert np.array_equal(c.sort_poll(wait=True), oracle.sort(rows[kept], VIEW)), "compacted meanwhile"
        c.set_state(0, np.ones(kept.size, np.uint8))
        c.sort_begin(VIEW)
        assert c.compact().size == 0 and c.count() == 0
        assert np.array_equal(c.sort_poll(wait=True), np.zeros(1, np.uint32)), "everything deleted meanwhile: the empty context's [0]"


# ---------------------------------------------------------------- frames

class Scene:
    def __init__(self, n=4096, W=256, H=144, seed=77, dense=False):
        self.n, self.W, self.H = n, W, H
        self.rows = synth.make_splat_rows(n, seed=seed).reshape(n, 32).copy()
        if dense:                                                        # large opaque splats: every tile saturates within a few of them
            self.rows[:, 12:24] = np.full((n, 3), 0.6, "<f4").view(np.uint8).reshape(n, 12)
            self.rows[:, 27] = 255
        self.cam = synth.index_html_camera(W, H, yaw_deg=15.0, capi=capi)
        self.params = capi.make_params(self.cam["gs_mv"], self.cam["gs_proj"], W, H, focal_=self.cam["focal"])
        _, _, mats = oracle.pack(self.rows.reshape(-1))
        order = oracle.sort(mats, self.cam["view"])
        assert order.size > n // 2
        self.hid = np.zeros(n, bool); self.hid[order[-(n // 4):]] = True      # the nearest quarter of the order
        self.kept = np.flatnonzero(~self.hid).astype(np.uint32)


def orbit(W, H, k, step=3.0):
    cam = synth.index_html_camera(W, H, yaw_deg=15.0 + step * k, capi=capi)
    return cam, capi.make_params(cam["gs_mv"], cam["gs_proj"], W, H, focal_=cam["focal"])


@functools.lru_cache(maxsize=None)
def scene(dense=False, n=4096):
    return Scene(n=n, dense=dense)


def pair_of_contexts(sc, opts=()):
    a, b = capi.Context(0), capi.Context(0)
    for c in (a, b):
        for o, v in opts:
            c.set_option(o, v)
    a.push_splat(sc.rows); a.set_state(0, sc.hid.astype(np.uint8))
    b.push_splat(sc.rows[sc.kept])
    return a, b


def test_frame_sync_stereo_surface():
    sc = scene()
    a, b = pair_of_contexts(sc)
    with a, b, capi.Context(0) as full:
        full.push_splat(sc.rows); full.sort(sc.cam["view"], want_indices=False)
        ia, ib = a.sort(sc.cam["view"]), b.sort(sc.cam["view"])
        assert np.array_equal(ia, sc.kept[ib])
        fa, fb = a.render(sc.params), b.render(sc.params)
        assert not np.array_equal(fa, full.render(sc.params)), "hiding the nearest quarter did not change the picture"
        assert np.array_equal(fa, fb)
        assert a.stats()["n_hidden"] == sc.hid.sum() and b.stats()["n_hidden"] == 0
        l, r, head = synth.xr_eye_cameras(yaw_deg=10.0, xr_pixel_ratio=0.1, capi=capi)
        eyes = [capi.make_params(e["gs_mv"], e["gs_proj"], e["vw"], e["vh"], focal_=e["focal"]) for e in (l, r)]
        a.sort(head["view"], want_indices=False); b.sort(head["view"], want_indices=False)
        for x, y in zip(a.render_stereo(*eyes), b.render_stereo(*eyes)):
            assert x.any() and np.array_equal(x, y)
        a.sort(sc.cam["view"], want_indices=False); b.sort(sc.cam["view"], want_indices=False)
        ca, ida, da, aa = a.render_surface(sc.params)
        cb, idb, db, ab = b.render_surface(sc.params)
        none = idb == capi.SURFACE_NONE
        assert (~none).any() and np.array_equal(ca, cb) and np.array_equal(da, db) and np.array_equal(aa, ab)
        assert np.array_equal(ida, np.where(none, capi.SURFACE_NONE, sc.kept[np.where(none, 0, idb)]))
        assert not sc.hid[ida[~none]].any()


def orbit_frames(c, W, H, nframes=12, step=3.0):
    frames = [capi.host_frame(H, W) for _ in range(nframes)]
    modes = []
    for f in range(nframes):
        cam, p = orbit(W, H, f, step)
        p.flags = capi.RENDER_ASYNC
        c.sort(cam["view"], want_indices=False)
        c.render_into(p, frames[f][0])
        if f % 2 == 1:
            c.sync()
            st = c.stats()
            modes.append((st["sort_mode"], st["spec_sorts"]))
    out = [fr[0].copy() for fr in frames]
    for _, owner in frames:
        owner.free()
    return out, modes


def _min_positions():
    """GS_SHARE_MIN_POSITIONS (csrc/gs_share.h): the first binning round never covers fewer positions than this"""
    with open(os.path.join(ROOT, PKG_NAME, "csrc", "gs_share.h")) as h:
        m = re.search(r"^#define\s+GS_SHARE_MIN_POSITIONS\s+(\d+)(?:\.0)?f?\b", h.read(), re.M)
    assert m, "GS_SHARE_MIN_POSITIONS not found"
    return int(m.group(1))


def test_frames_async_paired_orbit():
    """Twelve frames of an orbit, queued in pairs, with near-only sorts among them.

    Size.  A sort is near-only only while the first binning round covers a share below 100 % of the RESIDENT splats, and that round never
    covers fewer than GS_SHARE_MIN_POSITIONS (4096) positions (gs_share.h: gs_share_from_need) -- so with the 4096 splats of this
    module's other frames the share is 100 % by construction and every sort is whole, whatever the scene (measured: sort_mode 0 and
    spec_sorts 0 in every collection of eight laps).  The smallest scene in which the path exists at all has a multiple of that floor
    resident: 5 x 4096 splats here, a floor of 20 % for the context that hides a quarter and of 27 % for the fresh one fed the kept rows,
    both below the 85 % above which the share becomes one round.  The frame stays 256x144, a quarter is hidden, nearest first.

    Near-only sorts begin once the share has been measured and four clean frames have been collected, and only while every tile of the
    collected frames saturates (one tile of sky and the share goes to what covers every kept splat: measured, 83 .. 100 % here from a
    yaw of 24 degrees on), so the scene is one whose tiles all saturate early (large opaque splats), the orbit is twelve poses half a
    degree apart from the yaw of 15 degrees at which the quarter was hidden, GS_OPT_SORT_NEAR is 2 (1 leaves sorts whole where the share is more than half of what is
    kept) and the hidden context runs laps of the orbit until a lap's collections report such a sort -- at most eight; the lap that is
    compared is that lap, and it must contain one."""
    floor = _min_positions()
    sc = scene(dense=True, n=5 * floor)
    assert floor / sc.kept.size < 0.85 and floor / sc.n < 0.85
    a, b = pair_of_contexts(sc, [(capi.OPT_PIPELINE_DEPTH, 3), (capi.OPT_FRAME_BATCH, 2), (capi.OPT_SORT_NEAR, 2)])
    with a, b, capi.Context(0) as full:
        full.push_splat(sc.rows); full.sort(sc.cam["view"], want_indices=False)
        a.sort(sc.cam["view"], want_indices=False)
        assert not np.array_equal(a.render(sc.params), full.render(sc.params)), "hiding the nearest quarter did not change the picture"
        for lap in range(8):
            fa, modes = orbit_frames(a, sc.W, sc.H, step=0.5)
            if lap >= 1 and any(m != 0 or s > 0 for m, s in modes):
                break
        fb, _ = orbit_frames(b, sc.W, sc.H, step=0.5)
        print("laps:", lap + 1, "sort modes / spec sorts per collection:", modes)
        assert any(m != 0 or s > 0 for m, s in modes), "no near-only or stash sort occurred: the case proves nothing"
        for k in range(len(fa)):
            assert fa[k].any() and np.array_equal(fa[k], fb[k]), k


def test_frame_multi_world2():
    sc = scene()
    out = []
    for rows, st in ((sc.rows, sc.hid.astype(np.uint8)), (sc.rows[sc.kept], None)):
        with capi.Multi([0, 0]) as m:
            m.push_splat(rows)
            if st is not None:
                m.set_state(0, st)
            frame, owner = capi.host_frame(sc.H, sc.W)
            m.sort(sc.cam["view"], None, sc.params)
            m.render(sc.params, frame)
            m.sync()
            out.append(frame.copy()); owner.free()
    assert out[0].any() and np.array_equal(out[0], out[1])


def test_multi_world2_select_and_compact():
    """the gs_multi forms of the editing calls on two "devices" of one GPU: hit counts and the index map come from device 0, and the
    frame after them equals a single context's"""
    sc = scene()
    pos = sc.rows[:, :12].copy().view("<f4").reshape(sc.n, 3)
    _, _, mats = oracle.pack(sc.rows.reshape(-1))
    box = np.zeros(16, np.float32); box[0] = box[5] = box[10] = 0.2; box[15] = 1.0
    inside = box_mirror(mats[:, 12:16], box)
    assert 0.1 * sc.n < inside.sum() < 0.9 * sc.n
    d = pos.astype(np.float64) - pos[3].astype(np.float64)
    ball = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= 1.5 * 1.5
    ids = np.array([5, 9, 9, sc.n - 1], np.uint32)
    hid = ~inside | ball
    hid[ids] = True
    kept = np.flatnonzero(~hid).astype(np.uint32)
    assert ball[inside].any() and 0 < kept.size < inside.sum()
    with capi.Multi([0, 0]) as m, capi.Context(0) as one:
        m.push_splat(sc.rows)
        assert m.select_box(box, set_bits=HIDDEN, flags=INVERT) == sc.n - inside.sum()
        assert m.select_sphere(pos[3], 1.5, set_bits=HIDDEN) == ball.sum()
        m.set_state_ids(ids, set_bits=HIDDEN)
        m.sort(sc.cam["view"], None, sc.params)
        frame, owner = capi.host_frame(sc.H, sc.W)
        m.render(sc.params, frame); m.sync()
        n_sel = m.select_rect(sc.params, (0, 0, sc.W, sc.H), set_bits=SELECTED)
        assert 0 < n_sel <= kept.size
        old = m.compact()
        assert np.array_equal(old, kept) and m.count() == kept.size
        m.sort(sc.cam["view"], None, sc.params)
        frame2, owner2 = capi.host_frame(sc.H, sc.W)
        m.render(sc.params, frame2); m.sync()
        one.push_splat(sc.rows[kept]); one.sort(sc.cam["view"], want_indices=False)
        want = one.render(sc.params)
        assert want.any() and np.array_equal(frame, want) and np.array_equal(frame2, want)
        owner.free(); owner2.free()


def test_long_paired_depth_pass():
    """n > GS_DEPTH_PAIR_MIN_N: two queued frames that go out as a pair run k_sort_depth_pair<.., HID>, one sweep for both frames.  Whether a
    pair forms depends on both frames waiting in the lane's queue when its thread looks (a matter of timing), and no statistic says
    which depth kernel ran: frames that went out alone match through k_sort_depth<.., HID> just as well.  What this case guarantees is the
    size and the call pattern at which the paired kernel is the one that runs whenever a pair forms."""
    n = PAIR_MIN_N + 1000
    rows = cached_rows("make_splat_rows_fast", n).reshape(n, 32)
    g = np.random.Generator(np.random.PCG64(9))
    hid = g.random(n) < 0.25
    kept = np.flatnonzero(~hid)
    assert 0.2 * n < hid.sum() < 0.3 * n
    res = []
    for r, st in ((rows, hid.astype(np.uint8)), (rows[kept], None)):
        with capi.Context(0) as c:
            c.set_option(capi.OPT_PIPELINE_DEPTH, 2); c.set_option(capi.OPT_FRAME_BATCH, 2)
            c.push_splat(r)
            if st is not None:
                c.set_state(0, st)
            res.append(orbit_frames(c, 64, 64, nframes=4)[0])
    for k in range(4):
        assert res[0][k].any() and np.array_equal(res[0][k], res[1][k]), k


def test_empty_store_after_clear_is_a_context_that_never_edited():
    sc = scene()
    with capi.Context(0) as a, capi.Context(0) as b:
        a.push_splat(sc.rows); a.set_state(0, sc.hid.astype(np.uint8)); a.sort(sc.cam["view"], want_indices=False)
        a.clear()
        assert a.state_count() == (0, 0)
        a.push_splat(sc.rows); b.push_splat(sc.rows)
        assert np.array_equal(a.sort(sc.cam["view"]), b.sort(sc.cam["view"]))
        assert np.array_equal(a.render(sc.params), b.render(sc.params))
        assert a.stats()["n_hidden"] == 0 and a.download_state().size == 0
        a.set_state(1, np.array([4], np.uint8))                      # grows zero-filled: nothing of the old store comes back
        assert np.array_equal(a.download_state(), np.array([0, 4], np.uint8)) and a.state_count() == (2, 0)


def test_sort_for_strip():
    sc = scene()
    a, b = pair_of_contexts(sc)
    strip = capi.make_params(sc.cam["gs_mv"], sc.cam["gs_proj"], sc.W, sc.H, x0=64, x1=128, focal_=sc.cam["focal"])
    with a, b:
        ia, ib = a.sort_for(sc.cam["view"], None, strip), b.sort_for(sc.cam["view"], None, strip)
        assert 0 < ib.size < sc.kept.size and np.array_equal(ia, sc.kept[ib])
        assert np.array_equal(a.render(strip), b.render(strip))


# ---------------------------------------------------------------- box

def box_mirror(rows4, c):
    """index.js:533-540 in f64, operation by operation"""
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        x, y, z = rows4[:, 0].astype(np.float64), -rows4[:, 1].astype(np.float64), rows4[:, 2].astype(np.float64)
        w = 1.0 / (((c[3] * x + c[7] * y) + c[11] * z) + c[15])
        q = [(((c[i] * x + c[4 + i] * y) + c[8 + i] * z) + c[12 + i]) * w for i in range(3)]
        out = np.zeros(len(rows4), bool)
        for v in q:
            out |= (v < -0.5) | (v > 0.5)
    return ~out


@pytest.mark.parametrize("persp", [False, True])
def test_select_box_is_the_cutout(persp):
    n = 3 * DCHUNK + 17
    g = np.random.Generator(np.random.PCG64(4300 + persp))
    rows = plain_rows(g, n)
    rows[:, :3] = g.normal(0.0, 1.0, (n, 3))
    rows[g.integers(0, n, 40), g.integers(0, 3, 40)] = np.array([np.nan, np.inf, -np.inf, np.nan], np.float32)[g.integers(0, 4, 40)]
    view = np.array([0.1, -0.2, -1.0, -6.0], np.float32)
    cut = np.zeros(16, np.float32); cut[0] = cut[5] = cut[10] = 0.5; cut[15] = 1.0; cut[12] = 0.1; cut[13] = -0.05
    if persp:
        cut[3] = 0.05; cut[11] = -0.02
    inside = box_mirror(rows, cut)
    assert 0.1 * n < inside.sum() < 0.9 * n and inside[np.isnan(rows[:, :3]).any(axis=1)].all()
    want = oracle.sort(rows, view, cut)
    assert 0 < want.size <= inside.sum()
    with sort_ctx(rows) as c:
        hit = c.select_box(cut, set_bits=HIDDEN, flags=INVERT)
        assert hit == n - inside.sum()
        assert np.array_equal(c.download_state(), (~inside).astype(np.uint8))
        assert np.array_equal(c.sort(view), want)
        assert c.select_box(cut, set_bits=SELECTED) == inside.sum()
        assert np.array_equal(c.download_state(), np.where(inside, SELECTED, HIDDEN).astype(np.uint8))
        assert np.array_equal(c.sort(view), want), "the SELECTED bit changes no order"


# ---------------------------------------------------------------- sphere

def test_select_sphere():
    n = 3000
    rows = synth.make_splat_rows(n, seed=5).reshape(n, 32).copy()
    pos = rows[:, :12].copy().view("<f4").reshape(n, 3)
    pos[5, 0] = np.nan
    rows[:, :12] = pos.view(np.uint8).reshape(n, 12)
    with capi.Context(0) as c:
        c.push_splat(rows)
        for centre, radius in ((pos[7], 0.0), (np.array([0.3, -0.2, 0.5], np.float32), 2.0), (pos[9], np.float32(1e-3))):
            centre = np.asarray(centre, np.float32)
            with np.errstate(all="ignore"):
                d = pos.astype(np.float64) - centre.astype(np.float64)
                d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                inside = d2 <= float(np.float32(radius)) * float(np.float32(radius))
            assert not inside[5] and (radius != 0.0 or (inside[7] and inside.sum() >= 1)) and (radius != 2.0 or 30 < inside.sum() < n - 30)
            c.set_state(0, np.full(n, 8, np.uint8))
            assert c.select_sphere(centre, radius, set_bits=SELECTED) == inside.sum()
            assert np.array_equal(c.download_state(), np.where(inside, 8 | SELECTED, 8).astype(np.uint8))
            assert c.select_sphere(centre, radius, set_bits=HIDDEN, clear_bits=SELECTED, flags=INVERT) == n - inside.sum()
            assert np.array_equal(c.download_state(), np.where(inside, 8 | SELECTED, 8 | HIDDEN).astype(np.uint8))
    with sort_ctx(plain_rows(np.random.Generator(np.random.PCG64(1)), 8)) as c:
        with pytest.raises(capi.GsError) as e:
            c.select_sphere([0, 0, 0], 1.0, set_bits=HIDDEN)
        assert e.value.code == capi.E_STATE


# ---------------------------------------------------------------- rect

def test_select_rect():
    """oracle.project's `visible` is set on exactly the paths on which gsm::project_splat returns true (oracle/gs_oracle.c: gso_project
    returns early, visible = 0, at the same five tests), so no pose has to be chosen for the two to agree."""
    n, W, Hh = 2048, 320, 180
    rows = synth.make_splat_rows(n, seed=21).reshape(n, 32)
    cam = synth.index_html_camera(W, Hh, yaw_deg=25.0, capi=capi)
    p = capi.make_params(cam["gs_mv"], cam["gs_proj"], W, Hh, focal_=cam["focal"])
    cs, cc, mats = oracle.pack(rows.reshape(-1))
    hid = np.zeros(n, bool); hid[::7] = True
    order = want_order(mats[:, 12:16], hid, cam["view"])
    mv, P = cam["gs_mv"].astype(np.float32), cam["gs_proj"].astype(np.float32)
    px, py = np.full(n, -10 ** 6), np.full(n, -10 ** 6)
    for i in order:
        o = oracle.project(cs, cc, int(i), mv, P, cam["focal"], W, Hh)
        if o.visible and np.isfinite(o.cx) and np.isfinite(o.cy):
            px[i], py[i] = int(np.floor(o.cx)), Hh - 1 - int(np.floor(o.cy))
    in_order = np.zeros(n, bool); in_order[order] = True
    assert len(np.unique(order)) == order.size                       # (no zero tail in this scene: positions are splats)
    on = np.flatnonzero((px >= 0) & (px < W) & (py >= 0) & (py < Hh))
    assert on.size > 100
    one = (int(px[on[3]]), int(py[on[3]]))
    with capi.Context(0) as c:
        c.push_splat(rows); c.set_state(0, hid.astype(np.uint8))
        with pytest.raises(capi.GsError) as e:
            c.select_rect(p, (0, 0, W, Hh), set_bits=SELECTED)
        assert e.value.code == capi.E_STATE
        for rect in ((0, 0, W, Hh), (one[0], one[1], one[0] + 1, one[1] + 1), (W - 40, -25, W + 300, 60), (50, 50, 50, 90)):
            x0, y0, x1, y1 = rect
            want = in_order & (px >= max(x0, 0)) & (px < min(x1, W)) & (py >= max(y0, 0)) & (py < min(y1, Hh))
            assert want.sum() == 0 if x0 == x1 else want.sum() >= 1
            for inv in (0, INVERT):
                w = (in_order & ~want) if inv else want
                c.set_state(0, hid.astype(np.uint8))
                c.sort(cam["view"], want_indices=False)
                assert c.select_rect(p, rect, set_bits=SELECTED, flags=inv) == w.sum(), (rect, inv)
                assert np.array_equal(c.download_state(), hid.astype(np.uint8) | np.where(w, SELECTED, 0).astype(np.uint8)), (rect, inv)
        # after a near-only / strip sort the rectangle still walks the WHOLE order
        strip = capi.make_params(cam["gs_mv"], cam["gs_proj"], W, Hh, x0=0, x1=64, focal_=cam["focal"])
        c.set_state(0, hid.astype(np.uint8))
        c.sort_for(cam["view"], None, strip, want_indices=False)
        want = in_order & (px >= 0) & (px < W) & (py >= 0) & (py < Hh)
        assert c.select_rect(p, (0, 0, W, Hh), set_bits=SELECTED) == want.sum()


# ---------------------------------------------------------------- compact

@pytest.mark.parametrize("n,mode", [(1, "hidden"), (1, "kept"), (65537, "third")])
def test_compact(n, mode):
    g = np.random.Generator(np.random.PCG64(4400 + n))
    rows = synth.make_splat_rows(n, seed=33).reshape(n, 32)
    hid = {"hidden": np.ones(n, bool), "kept": np.zeros(n, bool), "third": g.random(n) < 1.0 / 3.0}[mode]
    kept = np.flatnonzero(~hid).astype(np.uint32)
    nsh = (3 * n) // 4
    sh = (g.normal(0.0, 0.2, (nsh, 27))).astype(np.float32)
    user = (g.integers(0, 64, n).astype(np.uint8) << 2)
    cam = synth.index_html_camera(256, 144, yaw_deg=15.0, capi=capi)
    p = capi.make_params(cam["gs_mv"], cam["gs_proj"], 256, 144, focal_=cam["focal"])
    strip = capi.make_params(cam["gs_mv"], cam["gs_proj"], 256, 144, x0=64, x1=128, focal_=cam["focal"])
    with capi.Context(0) as a, capi.Context(0) as b:
        for c in (a, b):
            c.set_option(capi.OPT_SH_DEGREE, 2)
        a.push_splat(rows)
        if nsh:
            a.push_sh(sh, 2)
        a.set_state(0, user | hid.astype(np.uint8))
        a.sort(cam["view"], want_indices=False)
        old = a.compact()
        assert np.array_equal(old, kept) and a.count() == kept.size and a.state_count() == (kept.size, 0)
        assert np.array_equal(a.compact(), np.arange(kept.size, dtype=np.uint32)), "nothing hidden: nothing happens"
        if kept.size:
            b.push_splat(rows[kept])
            ksh = kept[kept < nsh]
            if ksh.size:
                b.push_sh(sh[ksh], 2)
            b.set_state(0, user[kept])
        assert a.sh_count() == b.sh_count()
        m = kept.size
        for buf, dt, w in ((capi.BUF_CENTER_SCALE, np.uint32, 4), (capi.BUF_COV_COLOR, np.uint32, 4), (capi.BUF_SORT_ROWS, np.uint32, 4)):
            assert np.array_equal(a.download(buf, m, dt, w), b.download(buf, m, dt, w)), buf
        assert np.array_equal(a.download_sh().view(np.uint32), b.download_sh().view(np.uint32))
        assert np.array_equal(a.download_state(), user[kept]) and np.array_equal(b.download_state(), user[kept])
        assert np.array_equal(a.sort(cam["view"]), b.sort(cam["view"]))
        if m:
            fa, fb = a.render(p), b.render(p)
            assert np.array_equal(fa, fb) and a.stats()["sh_degree"] == (2 if kept[kept < nsh].size else 0)
            assert np.array_equal(a.sort_for(cam["view"], None, strip), b.sort_for(cam["view"], None, strip))
            assert np.array_equal(a.render(strip), b.render(strip))


# ---------------------------------------------------------------- arguments

def test_arguments():
    g = np.random.Generator(np.random.PCG64(3))
    rows = plain_rows(g, 100)
    with sort_ctx(rows) as c:
        L = capi.load()
        st = np.zeros(101, np.uint8)
        for first, k in ((0, 101), (100, 1), (101, 0), (50, 51)):
            assert L.gs_set_state(c._h, first, st.ctypes.data, k) == capi.E_BADARG, (first, k)
        assert L.gs_set_state(c._h, 0, None, 5) == capi.E_BADARG
        assert c.state_count() == (0, 0)
        c.set_state(10, np.array([HIDDEN | 32], np.uint8))
        assert c.state_count() == (11, 1)
        before = c.download_state()
        with pytest.raises(capi.GsError) as e:
            c.set_state_ids([3, 100, 4], set_bits=HIDDEN)
        assert e.value.code == capi.E_BADARG and np.array_equal(c.download_state(), before) and c.state_count() == (11, 1)
        c.set_state_ids([3, 3, 10, 99, 3], set_bits=SELECTED, clear_bits=HIDDEN)      # duplicates are harmless
        want = np.zeros(100, np.uint8); want[[3, 99]] = SELECTED; want[10] = 32 | SELECTED
        assert np.array_equal(c.download_state(), want) and c.state_count() == (100, 0)
        assert L.gs_select_box(c._h, None, 1, 0, 0, None) == capi.E_BADARG
        assert L.gs_select_box(c._h, np.zeros(16, np.float32).ctypes.data, 1, 0, 2, None) == capi.E_BADARG
        p = capi.make_params(np.eye(4).reshape(-1), np.eye(4).reshape(-1), 64, 64)
        c.sort(VIEW, want_indices=False)
        with pytest.raises(capi.GsError) as e:
            c.select_rect(p, (0, 0, 8, 8), set_bits=HIDDEN)             # matrices-only context
        assert e.value.code == capi.E_STATE
        out = np.zeros(4, np.uint8)
        assert L.gs_download(c._h, capi.BUF_STATE, out.ctypes.data, 101) == capi.E_BADARG
        assert L.gs_state_count(None, None, None) == capi.E_BADARG
