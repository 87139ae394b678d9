"""GPU tier of the in-place changes (include/gs_splat.h: gs_adjust_colour, gs_replace_splat, gs_replace_sh).

The adjusted colour words and SH rows are exact: capi.adjust_word / capi.adjust_sh_rows -- the kernels' own functions on the host, pinned to
the header's rule by tests/test_adjust_cpu.py -- applied to what the context held before (gs_download), for the splats the state filter
passes; everything else of the resident arrays is byte-identical to before.  Replaced rows are held against a fresh context that was pushed
the spliced rows.  Frames are 64 x 48 with the blend path pinned (tile lists, whole order), so every comparison is bit for bit."""
import numpy as np
import pytest

from conftest import pkg
from test_sort_paths_gpu import _constant

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

# the grid cap of the two kernels: the grid-strided loop of k_adjust_colour takes a second trip first at GRID * BLOCK + 1 splats
GRID, BLOCK = _constant("GS_EDIT_GRID", "gs_cloud_pass.h"), _constant("GS_BLOCK", "gs_internal.h")
assert (GRID, BLOCK) == (2048, 256)
SIZES = [1, 255, 256, 257, 2049, GRID * BLOCK + 1]
HIDDEN, SELECTED, CALLER = capi.STATE_HIDDEN, capi.STATE_SELECTED, 0x40
FILTERS = [(0, 0), (HIDDEN, 0), (3, SELECTED), (CALLER, CALLER)]
W, H = 64, 48
STAT_KEYS = ("n_splats", "n_sorted", "n_visible", "n_pairs", "n_tiles", "unsat_tiles", "near_permille", "binning", "row_walk", "subtile", "surface",
             "seg_count", "n_runs", "sh_degree", "n_hidden")
PINK = (0x80 << 24) | 0xC040FF

# a map with every kind of entry: mixing, negative weights, an offset that clamps, alpha scaled and shifted
ADJ = capi.colour_adjust([[0.75, 0.5, -0.25], [-0.125, 1.5, 0.0], [0.25, 0.25, 0.5]], (12.5, -20.0, 300.0), 0.75, 16.5)
WARM = capi.colour_adjust([[1.25, 0.0, 0.0], [0.0, 1.0, 0.0], [0.125, 0.0, 0.625]], (10.0, 0.0, -6.0), 0.875, 0.0)


def context():
    c = capi.Context(0)
    for k, v in ((capi.OPT_NEAR_PERMILLE, 1000), (capi.OPT_ROW_WALK, 0), (capi.OPT_SUBTILE, 0)):
        c.set_option(k, v)
    return c


def make_rows(n, seed):
    rows = (synth.make_splat_rows_fast(n, seed=seed) if n > 100000 else synth.make_splat_rows(n, seed=seed)).reshape(n, 32).copy()
    if n > 100000:                                               # colour words out of 65536: the host rule is applied to the distinct ones
        g = np.random.Generator(np.random.PCG64(seed))
        palette = g.integers(0, 1 << 32, size=65536, dtype=np.uint64).astype(np.uint32)
        rows[:, 24:28] = palette[g.integers(0, 65536, n)].view(np.uint8).reshape(n, 4)
    return rows


def host_words(words, a):
    u, inv = np.unique(np.asarray(words, np.uint32), return_inverse=True)
    return capi.adjust_word(u, a)[inv] if u.size else np.zeros(0, np.uint32)


def host_rows(rows, a, ok=None):
    """.splat rows with the colour bytes of the rows `ok` adjusted on the host"""
    out = np.array(rows, np.uint8).reshape(-1, 32).copy()
    ok = np.ones(len(out), bool) if ok is None else ok
    w = out[:, 24:28].copy().view("<u4").reshape(-1)
    w[ok] = host_words(w[ok], a)
    out[:, 24:28] = w.astype("<u4").view(np.uint8).reshape(-1, 4)
    return out


def passing_of(n, store, mask, value):
    st = np.zeros(n, np.uint8)
    st[:len(store)] = store
    return (st & np.uint8(mask)) == value


def random_store(g, length):
    st = g.integers(0, 4, length).astype(np.uint8)
    st[::3] |= CALLER
    return st


def snapshot(c, n):
    return (c.download(capi.BUF_CENTER_SCALE, n, np.uint32, 4), c.download(capi.BUF_COV_COLOR, n, np.uint32, 4),
            c.download(capi.BUF_SORT_ROWS, n, np.uint32, 4), c.download_state().copy() if c.state_count()[0] else np.zeros(0, np.uint8))


def stats_of(c):
    s = c.stats()
    return {k: s[k] for k in STAT_KEYS}


def camera():
    cam = synth.index_html_camera(W, H, 25.0, capi=capi)
    return cam, capi.make_params(cam["gs_mv"], cam["gs_proj"], W, H, focal_=cam["focal"])


# ---------------------------------------------------------------- 7. the records

@pytest.mark.parametrize("n", SIZES)
def test_records_against_the_host_rule(n):
    g = np.random.Generator(np.random.PCG64(9100 + n))
    with context() as c:
        c.push_splat(make_rows(n, seed=300 + n % 1000))
        short = n - max(n // 3, 1) if n > 1 else 0               # no store, a store shorter than N, a full one
        for length in sorted({0, short, n}):
            store = random_store(g, length)
            if length:
                c.set_state(0, store)
            for mask, value in FILTERS:
                cs, cc, sr, st = snapshot(c, n)
                ok = passing_of(n, store, mask, value)
                hit = c.adjust_colour(ADJ, (mask, value))
                cs2, cc2, sr2, st2 = snapshot(c, n)
                assert hit == int(ok.sum()), (length, mask, value)
                want = cc.copy()
                want[ok, 3] = host_words(cc[ok, 3], ADJ)
                assert np.array_equal(cc2[:, 3], want[:, 3]), (length, mask, value, np.flatnonzero(cc2[:, 3] != want[:, 3])[:8])
                assert np.array_equal(cc2[:, :3], cc[:, :3]) and np.array_equal(cs2, cs) and np.array_equal(sr2, sr)
                assert np.array_equal(st2, st) and len(st2) == length and c.state_count()[0] == length   # the store is neither grown nor changed
                if ok.sum() > 8:
                    assert not np.array_equal(cc2[ok, 3], cc[ok, 3])


# ---------------------------------------------------------------- 8. the SH store

def check_sh(c, n, sh_n, degree, store, mask, value):
    before = c.download_sh()
    words = c.download(capi.BUF_COV_COLOR, n, np.uint32, 4)[:, 3]
    ok = passing_of(n, store, mask, value)
    assert c.adjust_colour(WARM, (mask, value)) == int(ok.sum())
    after = c.download_sh()
    want = before.copy()
    sel = np.flatnonzero(ok[:sh_n])
    want[sel] = capi.adjust_sh_rows(before[sel], degree, WARM)
    assert after.shape == (sh_n, 3 * (degree + 1) ** 2) and c.sh_count() == (sh_n, degree)
    assert np.array_equal(after.view(np.uint32), want.view(np.uint32)), (degree, mask, value)
    if sel.size:
        assert not np.array_equal(after[sel], before[sel])
    got = c.download(capi.BUF_COV_COLOR, n, np.uint32, 4)[:, 3]
    exp = words.copy(); exp[ok] = host_words(words[ok], WARM)
    assert np.array_equal(got, exp)                               # the bytes of splats without an SH row are adjusted all the same


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_sh_rows_against_the_host_rule(degree):
    n, sh_n = 700, 500                                            # (degrees 1 and 3: 4 and 16 coefficients per channel; 2: 9 padded to 12)
    g = np.random.Generator(np.random.PCG64(9200 + degree))
    sh = (g.normal(size=(sh_n, 3 * (degree + 1) ** 2)) * 0.4).astype(np.float32)
    with context() as c:
        c.push_splat(make_rows(n, seed=41))
        c.push_sh(sh, degree)
        check_sh(c, n, sh_n, degree, np.zeros(0, np.uint8), 0, 0)
        for edge in (300, 600):                                   # the filter's boundary inside the SH store, then beyond it
            store = np.zeros(n, np.uint8)
            store[:edge] = CALLER
            c.set_state(0, store)
            check_sh(c, n, sh_n, degree, store, CALLER, CALLER)
        store = random_store(g, n - 40)
        c.set_state(0, np.concatenate([store, np.zeros(40, np.uint8)]))
        for mask, value in FILTERS:
            check_sh(c, n, sh_n, degree, np.concatenate([store, np.zeros(40, np.uint8)]), mask, value)


def test_sh_kernel_second_trip_of_the_grid():
    degree, K = 3, 16
    sh_n = GRID * BLOCK // K + 1                                  # one (row, k) item more than the capped grid covers in one trip
    n = sh_n + 31
    g = np.random.Generator(np.random.PCG64(9300))
    sh = (g.normal(size=(sh_n, 3 * K)) * 0.4).astype(np.float32)
    store = random_store(g, n)
    with context() as c:
        c.push_splat(make_rows(n, seed=43))
        c.push_sh(sh, degree)
        c.set_state(0, store)
        check_sh(c, n, sh_n, degree, store, HIDDEN, 0)


# ---------------------------------------------------------------- 9. frames

def scene_of(n=4096, seed=77):
    """rows whose size (largest scale x alpha / 255, the sort row's fourth word) stays far above the depth sort's cull 0.0001 |depth|
    (index.js:548) under WARM's alpha scale too: scales >= 0.02, alpha >= 64 -> size >= 0.004 against a cull below 0.002.  The sort row is
    packed at push time and an adjustment leaves it alone, so only then is the order of a fresh push of adjusted rows the same order."""
    rows = make_rows(n, seed)
    scale = rows[:, 12:24].copy().view("<f4").reshape(n, 3)
    rows[:, 12:24] = np.maximum(scale, np.float32(0.02)).view(np.uint8).reshape(n, 12)
    rows[:, 27] = np.maximum(rows[:, 27], 64)
    store = np.zeros(n, np.uint8)
    store[::2] = SELECTED
    store[5::7] |= CALLER
    return rows, store


@pytest.mark.parametrize("variant", ["bytes", "sh", "highlight"])
def test_frame_after_an_adjust_equals_a_fresh_context(variant):
    cam, p = camera()
    rows, store = scene_of()
    n = len(rows)
    ok = passing_of(n, store, 3, SELECTED)
    g = np.random.Generator(np.random.PCG64(9400))
    sh = (g.normal(size=(n, 27)) * 0.25).astype(np.float32)

    def prepare(c, rows_, sh_):
        if variant == "sh":
            c.set_option(capi.OPT_SH_DEGREE, 2)
        if variant == "highlight":
            c.set_option(capi.OPT_HIGHLIGHT, PINK)
        c.push_splat(rows_)
        if variant == "sh":
            c.push_sh(sh_, 2)
        c.set_state(0, store)
        return c.sort(cam["view"])

    with context() as a, context() as b:
        order = prepare(a, rows, sh)
        first = a.render(p)
        assert a.adjust_colour(WARM, "selected") == int(ok.sum())
        second, stats_a = a.render(p), stats_of(a)                # no new sort
        sh_b = sh.copy()
        sh_b[ok] = capi.adjust_sh_rows(sh[ok], 2, WARM)
        assert np.array_equal(prepare(b, host_rows(rows, WARM, ok), sh_b), order), "the scene sits at the sort's size cull: see scene_of"
        want, stats_b = b.render(p), stats_of(b)
    assert first.any() and not np.array_equal(first, second), "the adjustment does not show"
    assert np.array_equal(second, want)
    assert stats_a == stats_b and stats_a["n_sorted"] > 0
    if variant == "sh":
        assert stats_a["sh_degree"] == 2


# ---------------------------------------------------------------- 10. orders

def test_an_adjust_keeps_the_order_and_a_replace_drops_it():
    cam, p = camera()
    rows, store = scene_of(2500, 78)
    with context() as c, context() as pushed:
        c.push_splat(rows)
        order = c.sort(cam["view"])
        info, idx = c.sort_inspect()
        c.adjust_colour(ADJ, "all")
        info2, idx2 = c.sort_inspect()
        assert info2 == info and np.array_equal(idx2, idx) and info["n_records"] == len(order) > 0
        assert c.render(p).any()
        c.replace_splat(10, rows[100:120])
        pushed.push_splat(rows)                                   # as after a push: a render before the next sort draws the background only
        blank = c.render(p)
        assert np.array_equal(blank, pushed.render(p)) and (blank == blank[0, 0]).all()
        c.sort(cam["view"], want_indices=False)
        assert c.render(p).any()


def test_the_sorts_size_cull_keeps_the_alpha_of_the_push():
    """The sort row's fourth word is (largest scale) x alpha / 255 as packed at push time, and the depth sort culls on it (index.js:548).  An
    adjustment rewrites the colour word alone (the header says so): a splat faded to alpha 0 in place stays in the order -- it draws with
    weight 0 -- while a fresh push of the same row is culled.  gs_replace_splat packs the row again and the cull follows."""
    cam, p = camera()
    rows, _ = scene_of(512, 84)
    fade = capi.colour_adjust(alpha_scale=0.0)
    with context() as a, context() as b:
        a.push_splat(rows)
        order = a.sort(cam["view"])
        assert len(order) > 100
        assert a.adjust_colour(fade) == len(rows)
        assert np.array_equal(a.sort(cam["view"]), order)         # still sorted ...
        blank = a.render(p)
        assert (blank == blank[0, 0]).all()                       # ... and invisible
        faded = host_rows(rows, fade)
        assert not faded[:, 27].any()
        b.push_splat(faded)
        assert len(b.sort(cam["view"])) == 0                      # pushed with alpha 0: size 0, culled
        a.replace_splat(0, faded)
        assert len(a.sort(cam["view"])) == 0


# ---------------------------------------------------------------- 11. replaced rows

REPLACE_N = 6149
RANGES = [(0, 100), (REPLACE_N - 77, REPLACE_N), (3000, 3001), (2000, 2100)]     # from 0; ending at N; one row; across index 2048


@pytest.mark.parametrize("first,last", RANGES)
def test_replace_splat_against_a_fresh_context(first, last):
    n, sh_n, degree = REPLACE_N, 4000, 1
    cam, p = camera()
    strip = capi.make_params(cam["gs_mv"], cam["gs_proj"], W, H, x0=16, x1=40, focal_=cam["focal"])
    rows, other = make_rows(n, 81), make_rows(n, 82)
    g = np.random.Generator(np.random.PCG64(9500 + first))
    store = random_store(g, n - 100) & np.uint8(~HIDDEN & 0xFF)
    sh = (g.normal(size=(sh_n, 12)) * 0.3).astype(np.float32)
    spliced = rows.copy()
    spliced[first:last] = other[first:last]
    with context() as a, context() as b:
        a.push_splat(rows); a.push_sh(sh, degree); a.set_state(0, store)
        a.sort(cam["view"], want_indices=False)
        a.render_contrib(p, want_rgba=False)
        seen, states, shs = a.download_contrib().copy(), a.download_state().copy(), a.download_sh().copy()
        assert seen.any()
        a.sort_begin(cam["view"])                                 # posted before the change, collected after it
        a.replace_splat(first, other[first:last])
        b.push_splat(spliced); b.push_sh(sh, degree); b.set_state(0, store)
        assert a.count() == n
        for x, y in zip(snapshot(a, n), snapshot(b, n)):
            assert np.array_equal(x, y)
        assert np.array_equal(a.download_state(), states) and np.array_equal(a.download_sh().view(np.uint32), shs.view(np.uint32))
        assert np.array_equal(a.download_contrib(), seen) and a.sh_count() == (sh_n, degree)
        want_order = b.sort(cam["view"])
        assert np.array_equal(a.sort_poll(wait=True), want_order)
        assert np.array_equal(a.render(p), b.render(p)) and stats_of(a) == stats_of(b)
        oa, ob = a.sort_for(cam["view"], None, strip), b.sort_for(cam["view"], None, strip)      # the strip sort reads bound_r
        assert np.array_equal(oa, ob) and 0 < len(oa)
        fa, fb = a.render(strip), b.render(strip)
        assert np.array_equal(fa, fb) and fa.any()
        # ... and SH rows likewise
        sh2 = (g.normal(size=(sh_n, 12)) * 0.3).astype(np.float32)
        s0, s1 = min(first, sh_n - 1), min(last, sh_n)
        lies = a.sort_inspect()
        a.replace_sh(s0, sh2[s0:s1], degree)
        sp = sh.copy(); sp[s0:s1] = sh2[s0:s1]
        with context() as d:
            d.push_splat(spliced); d.push_sh(sp, degree)
            assert np.array_equal(a.download_sh().view(np.uint32), d.download_sh().view(np.uint32))
        assert a.sh_count() == (sh_n, degree)
        again = a.sort_inspect()                                  # gs_replace_sh drops no order
        assert again[0] == lies[0] and np.array_equal(again[1], lies[1]) and lies[0]["n_records"] > 0


# ---------------------------------------------------------------- 12. export -> transform on the host -> replace

def test_round_trip_export_translate_replace():
    n = 3001
    rows = make_rows(n, 91)
    pos = rows[:, :12].copy().view("<f4").reshape(n, 3)
    pos = (np.rint(pos * 1024) / 1024).astype(np.float32)        # multiples of 2^-10 below 2^4: the offset below adds exactly
    rows[:, :12] = pos.view(np.uint8).reshape(n, 12)
    offset = np.array([0.5, -0.25, 2.0], np.float32)
    first, last = 1000, 2500
    with context() as a, context() as b:
        a.push_splat(rows)
        out = a.export_splat()
        assert np.array_equal(out[:, :12], rows[:, :12])
        moved = out[first:last].copy()
        mp = moved[:, :12].copy().view("<f4").reshape(-1, 3) + offset
        assert np.array_equal(mp.astype(np.float64), pos[first:last].astype(np.float64) + offset.astype(np.float64))   # exact
        moved[:, :12] = mp.astype("<f4").view(np.uint8).reshape(-1, 12)
        a.replace_splat(first, moved)
        full = out.copy(); full[first:last] = moved
        b.push_splat(full)
        ca, cb = a.download(capi.BUF_CENTER_SCALE, n, np.float32, 4), b.download(capi.BUF_CENTER_SCALE, n, np.float32, 4)
        assert np.array_equal(ca[:, :3].view(np.uint32), cb[:, :3].view(np.uint32))
        want = pos.copy(); want[first:last] += offset
        assert np.array_equal(ca[:, :3], want * np.array([1, 1, -1], np.float32))           # the packed centre is (x, y, -z)


# ---------------------------------------------------------------- 13. errors

def test_errors_change_nothing():
    n = 300
    rows = make_rows(n, 95)
    with context() as c:
        assert c.adjust_colour(ADJ) == 0                          # nothing resident
        c.replace_splat(0, np.zeros((0, 32), np.uint8))
        c.push_splat(rows)
        c.push_sh(np.ones((100, 12), np.float32), 1)
        before, sh = snapshot(c, n), c.download_sh()
        for first, k in ((n, 1), (n - 1, 2), (0, n + 1), (n + 5, 0)):
            with pytest.raises(capi.GsError) as e:
                c.replace_splat(first, rows[:k] if k <= n else np.zeros((k, 32), np.uint8))
            assert e.value.code == capi.E_BADARG
        assert c._L.gs_replace_splat(c._h, (1 << 64) - 1, capi._p(rows), 2) == capi.E_BADARG     # first + nrows wraps around
        assert c._L.gs_replace_splat(c._h, 0, None, 2) == capi.E_BADARG
        for first, k, degree in ((100, 1, 1), (99, 2, 1), (0, 1, 2), (0, 1, 0), (0, 1, 4)):
            with pytest.raises(capi.GsError) as e:
                c.replace_sh(first, np.zeros((k, 3 * (degree + 1) ** 2), np.float32), degree)
            assert e.value.code == capi.E_BADARG
        bad = capi.colour_adjust(offset=(0.0, np.nan, 0.0))
        with pytest.raises(capi.GsError) as e:
            c.adjust_colour(bad)
        assert e.value.code == capi.E_BADARG
        assert c._L.gs_adjust_colour(c._h, None, 0, 0, None) == capi.E_BADARG
        for x, y in zip(snapshot(c, n), before):
            assert np.array_equal(x, y)
        assert np.array_equal(c.download_sh(), sh)
        c.replace_splat(n, np.zeros((0, 32), np.uint8))           # nrows == 0 at the end: GS_OK
    with capi.Context(0) as c:
        c.push_matrices(np.zeros((4, 16), np.float32))
        for call in (lambda: c.adjust_colour(ADJ), lambda: c.replace_splat(0, rows[:1])):
            with pytest.raises(capi.GsError) as e:
                call()
            assert e.value.code == capi.E_STATE


# ---------------------------------------------------------------- 14. a context that never calls these

def test_an_identity_adjust_changes_no_frame_and_no_statistic():
    cam, p = camera()
    rows, store = scene_of(4096, 79)
    store[1::5] |= HIDDEN

    def two_frames(adjust):
        with context() as c:
            c.push_splat(rows)
            c.set_state(0, store)
            c.sort(cam["view"], want_indices=False)
            before = c.render(p)
            if adjust:
                assert c.adjust_colour(capi.colour_adjust(), "all") == len(rows)
            after = c.render(p)
            return before, after, stats_of(c), c.state_count()

    b1, a1, s1, h1 = two_frames(True)
    b0, a0, s0, h0 = two_frames(False)
    assert b1.any() and np.array_equal(b1, a1)
    assert np.array_equal(b0, b1) and np.array_equal(a0, a1) and s0 == s1 and h0 == h1


# ---------------------------------------------------------------- 15. two contexts of one GPU

def test_multi_forms_on_two_contexts_of_one_gpu():
    cam, p = camera()
    rows, store = scene_of(4096, 80)
    n = len(rows)
    g = np.random.Generator(np.random.PCG64(9600))
    sh = (g.normal(size=(n, 12)) * 0.3).astype(np.float32)
    sh2 = (g.normal(size=(50, 12)) * 0.3).astype(np.float32)
    other = make_rows(64, 83)
    ok = passing_of(n, store, 3, SELECTED)
    L = capi.load()

    def download(h, which, count, dtype, width):
        out = np.zeros((count, width), dtype)
        assert L.gs_download(h, which, capi._p(out), out.nbytes) == capi.GS_OK
        return out

    with capi.Multi([0, 0]) as m, context() as one:
        hs = [L.gs_multi_ctx(m._h, i) for i in range(2)]
        for h in hs:
            for k, v in ((capi.OPT_NEAR_PERMILLE, 1000), (capi.OPT_ROW_WALK, 0), (capi.OPT_SUBTILE, 0)):
                assert L.gs_set_option(h, k, v) == capi.GS_OK
        for c in (m, one):
            c.push_splat(rows); c.push_sh(sh, 1); c.set_state(0, store)
        m.sort(cam["view"], None, p)
        one.sort(cam["view"], want_indices=False)
        assert m.adjust_colour(WARM, "selected") == one.adjust_colour(WARM, "selected") == int(ok.sum())
        frame, owner = capi.host_frame(H, W)
        m.render(p, frame); m.sync()                              # the sort from before the adjustment: no order was dropped
        assert frame.any() and np.array_equal(frame, one.render(p))
        m.replace_splat(2040, other); m.replace_sh(7, sh2, 1)
        one.replace_splat(2040, other); one.replace_sh(7, sh2, 1)
        want = [one.download(capi.BUF_CENTER_SCALE, n, np.uint32, 4), one.download(capi.BUF_COV_COLOR, n, np.uint32, 4),
                one.download(capi.BUF_SORT_ROWS, n, np.uint32, 4), one.download(capi.BUF_SH, n, np.uint32, 12)]
        for h in hs:
            got = [download(h, capi.BUF_CENTER_SCALE, n, np.uint32, 4), download(h, capi.BUF_COV_COLOR, n, np.uint32, 4),
                   download(h, capi.BUF_SORT_ROWS, n, np.uint32, 4), download(h, capi.BUF_SH, n, np.uint32, 12)]
            for x, y in zip(got, want):
                assert np.array_equal(x, y)
        m.sort(cam["view"], None, p)
        one.sort(cam["view"], want_indices=False)
        m.render(p, frame); m.sync()
        assert np.array_equal(frame, one.render(p))
        owner.free()
