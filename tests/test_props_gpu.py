"""GPU tier of the per-splat properties (include/gs_splat.h: gs_prop_range, gs_histogram, gs_select_range).

Everything is exact.  The mirror: the records the context holds (GS_BUF_CENTER_SCALE, GS_BUF_COV_COLOR -- asserted equal to oracle.pack's)
through capi.prop_eval, the kernels' own function on the host, then the header's bin rule and state filter in numpy.  Sizes are placed
from the editing kernels' own constants, read out of the sources: one workgroup step is GS_BLOCK splats, the grid ends at GS_EDIT_GRID
workgroups, so GS_EDIT_GRID * GS_BLOCK + 1 is the smallest cloud at which a workgroup takes a second step."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_props_cpu import bin_mirror
from test_sort_paths_gpu import _constant

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

BLOCK = _constant("GS_BLOCK", "gs_internal.h")
CHUNK = _constant("GS_EDIT_IPT", "gs_cloud_pass.h") * BLOCK
GRID = _constant("GS_EDIT_GRID", "gs_cloud_pass.h")
HIDDEN, SELECTED, INVERT = capi.STATE_HIDDEN, capi.STATE_SELECTED, capi.SELECT_INVERT
VIEW = np.array([0.0, 0.0, 1.0, 0.0], np.float32)
FILTERS = [(0, 0), (1, 0), (3, 2), (0x40, 0x40)]
NBINS = [1, 100, 256, 4096]
SIZES = [1, 255, 256, 257, CHUNK - 1, CHUNK + 1]
assert BLOCK == 256 and CHUNK == 2048 and GRID == 2048


def make_rows(n, seed):
    return synth.make_splat_rows(n, seed=seed).reshape(n, 32).copy()


def set_pos(rows, i, axis, value):
    rows[i, 4 * axis:4 * axis + 4] = np.array([value], "<f4").view(np.uint8)


def records(c, rows):
    """the context's records, asserted to be the oracle's"""
    n = len(rows)
    cs = c.download(capi.BUF_CENTER_SCALE, n, np.float32, 4)
    cc = c.download(capi.BUF_COV_COLOR, n, np.uint32, 4)
    ocs, occ, _ = oracle.pack(rows.reshape(-1))
    assert np.array_equal(cs.view(np.uint32), ocs.view(np.uint32)) and np.array_equal(cc, occ)
    return cs, cc


def passing_of(n, store, mask, value):
    st = np.zeros(n, np.uint8)
    st[:len(store)] = store
    return (st & np.uint8(mask)) == value


def hist_mirror(v, passing, lo, hi, nbins):
    with np.errstate(all="ignore"):
        b = bin_mirror(v[passing], lo, hi, nbins)
    counts = np.bincount(b[b >= 0], minlength=nbins).astype(np.uint32)
    tally = np.array([passing.sum(), (b == -1).sum(), (b == -2).sum(), (b == -3).sum()], np.uint64)
    assert counts.sum() + tally[1:].sum() == tally[0]
    return counts, tally


def range_mirror(v, passing):
    w = v[passing]
    w = w[~np.isnan(w)]
    return (w.min() if w.size else np.inf, w.max() if w.size else -np.inf, int(passing.sum()))


def check_hist(c, v, prop, lo, hi, nbins, store, mask=0, value=0):
    counts, tally = c.histogram(prop, lo, hi, nbins, mask, value)
    wc, wt = hist_mirror(v, passing_of(len(v), store, mask, value), lo, hi, nbins)
    assert counts.dtype == np.uint32 and counts.shape == (nbins,)
    assert np.array_equal(counts, wc), (prop, lo, hi, nbins, mask, value, np.flatnonzero(counts != wc)[:8])
    assert np.array_equal(tally, wt), (prop, lo, hi, nbins, mask, value, tally, wt)
    assert int(counts.sum()) + int(tally[1:].sum()) == int(tally[0])
    return counts, tally


def span_of(v):
    """a range from the input that leaves values on both sides and some inside"""
    f = v[np.isfinite(v)]
    lo, hi = np.quantile(f, 0.1), np.quantile(f, 0.9)
    return (float(lo), float(hi)) if lo < hi else (float(lo) - 1.0, float(lo) + 1.0)


def random_store(g, n, length):
    st = g.integers(0, 4, length).astype(np.uint8)
    st[::3] |= 0x40                                                      # a caller bit on every third splat
    return st


# ---------------------------------------------------------------- sizes x properties x bins

@pytest.mark.parametrize("n", SIZES)
def test_histogram_and_range_equal_the_mirror(n):
    g = np.random.Generator(np.random.PCG64(9100 + n))
    rows = make_rows(n, seed=300 + n)
    store = random_store(g, n, n)
    with capi.Context(0) as c:
        c.push_splat(rows)
        cs, cc = records(c, rows)
        for prop in range(8):
            v = capi.prop_eval(cs, cc, prop).reshape(-1)
            assert c.prop_range(prop) == range_mirror(v, np.ones(n, bool))
            lo, hi = span_of(v)
            for nbins in NBINS:
                check_hist(c, v, prop, lo, hi, nbins, store[:0])
                if capi.PROP_RED <= prop <= capi.PROP_ALPHA:
                    check_hist(c, v, prop, 0.0, 255.0, nbins, store[:0])
        c.set_state(0, store)
        for prop in (capi.PROP_Y, capi.PROP_BLUE, capi.PROP_SIZE2):
            v = capi.prop_eval(cs, cc, prop).reshape(-1)
            lo, hi = span_of(v)
            for mask, value in FILTERS:
                check_hist(c, v, prop, lo, hi, 256, store, mask, value)
                assert c.prop_range(prop, mask, value) == range_mirror(v, passing_of(n, store, mask, value))


def test_second_grid_stride():
    """GS_EDIT_GRID * GS_BLOCK + 1 splats: workgroup 0 alone comes round a second time, for one splat -- the last one, given a value no
    other splat has, in a store that ends one byte before it"""
    n = GRID * BLOCK + 1
    g = np.random.Generator(np.random.PCG64(77))
    rows = synth.make_splat_rows_fast(n, seed=41).reshape(n, 32).copy()
    rows[:, 27] = np.minimum(rows[:, 27], 250)
    rows[n - 1, 27] = 253
    set_pos(rows, n - 1, 0, 1000.0)
    store = random_store(g, n, n - 1)
    with capi.Context(0) as c:
        c.push_splat(rows)
        cs, cc = records(c, rows)
        c.set_state(0, store)
        for prop, lo, hi in ((capi.PROP_ALPHA, 0.0, 255.0), (capi.PROP_X, -8.0, 1000.0)):
            v = capi.prop_eval(cs, cc, prop).reshape(-1)
            assert (v == v[n - 1]).sum() == 1
            for nbins, (mask, value) in ((256, (0, 0)), (4096, (1, 0))):
                counts, _ = check_hist(c, v, prop, lo, hi, nbins, store, mask, value)
                assert counts[bin_mirror(v[n - 1:], lo, hi, nbins)[0]] >= 1
            assert c.prop_range(prop, 1, 0) == range_mirror(v, passing_of(n, store, 1, 0))
            assert c.prop_range(prop)[1] == v[n - 1]
        assert c.select_range(capi.PROP_X, 999.0, 1001.0, set_bits=SELECTED) == 1
        st = c.download_state()
        assert st.size == n and st[n - 1] == SELECTED and np.array_equal(st[:n - 1], store)


# ---------------------------------------------------------------- pile-up

def test_pile_up_in_one_bin():
    """every lane of every wave wants the same word: constant alpha, then constant positions"""
    n = 4096
    rows = make_rows(n, seed=12)
    rows[:, 27] = 255
    with capi.Context(0) as c:
        c.push_splat(rows)
        cs, cc = records(c, rows)
        v = capi.prop_eval(cs, cc, capi.PROP_ALPHA).reshape(-1)
        assert (v == 255.0).all()
        counts, tally = check_hist(c, v, capi.PROP_ALPHA, 0.0, 255.0, 256, [])
        assert counts[255] == n and counts[:255].sum() == 0 and list(tally) == [n, 0, 0, 0]
        counts, tally = check_hist(c, v, capi.PROP_ALPHA, 0.0, 255.0, 1, [])
        assert list(counts) == [n] and list(tally) == [n, 0, 0, 0]
        assert c.prop_range(capi.PROP_ALPHA) == (255.0, 255.0, n)
    rows[:, :12] = rows[7, :12]
    with capi.Context(0) as c:
        c.push_splat(rows)
        cs, cc = records(c, rows)
        for prop in (capi.PROP_X, capi.PROP_Y, capi.PROP_Z):
            v = capi.prop_eval(cs, cc, prop).reshape(-1)
            assert (v == v[0]).all()
            for nbins in (1, 256, 4096):
                counts, tally = check_hist(c, v, prop, float(v[0]) - 1.0, float(v[0]) + 2.0, nbins, [])
                assert counts.max() == n and list(tally) == [n, 0, 0, 0]
    # two values, interleaved lane by lane, and a run of a third: a wave holds 2 or 3 distinct bins
    rows = make_rows(n, seed=12)
    rows[:, 27] = np.where(np.arange(n) % 2, 255, 254).astype(np.uint8)
    rows[100:140, 27] = 3
    with capi.Context(0) as c:
        c.push_splat(rows)
        cs, cc = records(c, rows)
        v = capi.prop_eval(cs, cc, capi.PROP_ALPHA).reshape(-1)
        counts, _ = check_hist(c, v, capi.PROP_ALPHA, 0.0, 255.0, 256, [])
        assert counts[3] == 40 and counts[254] + counts[255] == n - 40


# ---------------------------------------------------------------- edges, NaN, +-Inf

def test_edges_and_non_finite_values():
    n = 1500
    rows = make_rows(n, seed=31)
    f32 = np.float32
    x_lo, x_hi = f32(-1.5), f32(2.25)
    plant = {3: x_lo, 4: x_hi, 5: np.nextafter(x_lo, f32(-np.inf)), 6: np.nextafter(x_hi, f32(np.inf)), 7: np.nextafter(x_lo, f32(np.inf)),
             8: np.nextafter(x_hi, f32(-np.inf)), 300: f32(np.nan), 301: f32(np.nan), 700: f32(np.inf), 701: f32(-np.inf), 702: f32(-np.inf),
             n - 1: f32(np.nan)}
    for i, x in plant.items():
        set_pos(rows, i, 0, x)
    set_pos(rows, 9, 2, np.inf); set_pos(rows, 10, 2, np.nan)
    g = np.random.Generator(np.random.PCG64(5))
    store = random_store(g, n, n // 2)
    with capi.Context(0) as c:
        c.push_splat(rows)
        cs, cc = records(c, rows)
        v = capi.prop_eval(cs, cc, capi.PROP_X).reshape(-1)
        assert np.isnan(v).sum() == 3 and np.isposinf(v).sum() == 1 and np.isneginf(v).sum() == 2
        lo, hi = float(x_lo), float(x_hi)
        inner = (np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf))     # the planted edge values now lie one f64 step outside
        for a, b in ((lo, hi), inner):
            for nbins in NBINS:
                counts, tally = check_hist(c, v, capi.PROP_X, a, b, nbins, [])
                assert tally[3] == 3 and tally[1] >= 3 and tally[2] >= 2
        counts, tally = check_hist(c, v, capi.PROP_X, lo, hi, 256, [])
        c2, t2 = check_hist(c, v, capi.PROP_X, inner[0], inner[1], 256, [])
        assert counts[0] >= 1 and counts[255] >= 1 and t2[1] == tally[1] + 1 and t2[2] == tally[2] + 1
        assert c.prop_range(capi.PROP_X) == (-np.inf, np.inf, n)
        vz = capi.prop_eval(cs, cc, capi.PROP_Z).reshape(-1)
        assert np.isposinf(vz[9]) and np.isnan(vz[10])                    # (the packed z is negated, and negated back: the row's own)
        assert c.prop_range(capi.PROP_Z) == range_mirror(vz, np.ones(n, bool))
        check_hist(c, vz, capi.PROP_Z, -3.0, 3.0, 100, [])
        # a store shorter than the cloud: the splats behind it have state 0
        c.set_state(0, store)
        for mask, value in FILTERS:
            check_hist(c, v, capi.PROP_X, lo, hi, 100, store, mask, value)
            assert c.prop_range(capi.PROP_X, mask, value) == range_mirror(v, passing_of(n, store, mask, value))
        # only NaN values pass: the range is empty, the count is not
        only = np.zeros(n, np.uint8); only[[300, 301, n - 1]] = 0x80
        c.set_state(0, only)
        assert c.prop_range(capi.PROP_X, 0x80, 0x80) == (np.inf, -np.inf, 3)
        counts, tally = c.histogram(capi.PROP_X, lo, hi, 4, 0x80, 0x80)
        assert not counts.any() and list(tally) == [3, 0, 0, 3]
        # a filter nothing passes
        assert c.prop_range(capi.PROP_X, 0x20, 0x20) == (np.inf, -np.inf, 0)
        assert c.prop_range(capi.PROP_X, 0, 1) == (np.inf, -np.inf, 0)     # (a value outside the mask)


def test_filters_on_an_empty_store():
    n = 600
    rows = make_rows(n, seed=8)
    with capi.Context(0) as c:
        c.push_splat(rows)
        cs, cc = records(c, rows)
        assert c.state_count() == (0, 0)
        v = capi.prop_eval(cs, cc, capi.PROP_GREEN).reshape(-1)
        for mask, value in FILTERS + [(1, 1)]:
            counts, tally = check_hist(c, v, capi.PROP_GREEN, 0.0, 255.0, 256, [], mask, value)
            assert tally[0] == (n if value == 0 else 0)
            assert c.prop_range(capi.PROP_GREEN, mask, value)[2] == tally[0]
        assert c.state_count() == (0, 0)                                  # reading allocates no store


# ---------------------------------------------------------------- gs_select_range

def test_select_range():
    n = 3000
    rows = make_rows(n, seed=5)
    set_pos(rows, 5, 1, np.nan)
    with capi.Context(0) as c:
        c.push_splat(rows)
        cs, cc = records(c, rows)
        for prop in (capi.PROP_Y, capi.PROP_ALPHA, capi.PROP_SIZE2):
            v = capi.prop_eval(cs, cc, prop).reshape(-1)
            lo, hi = span_of(v)
            exists = float(v[11])
            for a, b in ((lo, hi), (exists, exists), (hi, lo), (-np.inf, np.inf)):
                with np.errstate(all="ignore"):
                    inside = (a <= v) & (v <= b)
                if (a, b) == (lo, hi):
                    assert 30 < inside.sum() < n - 30
                if a == b:
                    assert inside[11]
                if a > b:
                    assert not inside.any()
                c.set_state(0, np.full(n, 8, np.uint8))
                assert c.select_range(prop, a, b, set_bits=SELECTED) == inside.sum()
                assert np.array_equal(c.download_state(), np.where(inside, 8 | SELECTED, 8).astype(np.uint8))
                assert c.select_range(prop, a, b, set_bits=HIDDEN, clear_bits=SELECTED, flags=INVERT) == n - inside.sum()
                want = np.where(inside, 8 | SELECTED, 8 | HIDDEN).astype(np.uint8)
                assert np.array_equal(c.download_state(), want)
                assert c.state_count() == (n, n - inside.sum())
                order = c.sort(VIEW)                                      # (read back: the sort is collected, and its statistics with it)
                assert c.stats()["n_hidden"] == n - inside.sum() and inside[order].all()
                # the inverse the editing calls lacked: how many carry a state, and what
                counts, tally = check_hist(c, v, prop, lo, hi, 100, want, 3, SELECTED)
                assert tally[0] == inside.sum()
        vy = capi.prop_eval(cs, cc, capi.PROP_Y).reshape(-1)
        assert np.isnan(vy[5])
        c.set_state(0, np.zeros(n, np.uint8))
        assert c.select_range(capi.PROP_Y, -np.inf, np.inf, set_bits=SELECTED) == n - 1 and c.download_state()[5] == 0
        assert c.select_range(capi.PROP_Y, -np.inf, np.inf, set_bits=HIDDEN, flags=INVERT) == 1 and c.download_state()[5] == HIDDEN


# ---------------------------------------------------------------- read-only

def test_reading_calls_disturb_nothing():
    n, W, H = 4096, 256, 144
    rows = make_rows(n, seed=77)
    cam = synth.index_html_camera(W, H, yaw_deg=15.0, capi=capi)
    params = capi.make_params(cam["gs_mv"], cam["gs_proj"], W, H, focal_=cam["focal"])
    with capi.Context(0) as c:
        c.push_splat(rows)
        c.set_state(0, np.where(np.arange(n) % 5 == 0, SELECTED, 0).astype(np.uint8))
        c.sort(cam["view"], want_indices=False)
        a = c.render(params)
        before = (c.stats(), c.state_count(), c.highlight_info(), c.download_state())
        counts, tally = c.histogram(capi.PROP_ALPHA, 0.0, 255.0, 256)
        mn, mx, cnt = c.prop_range(capi.PROP_SIZE2, 3, SELECTED)
        assert tally[0] == n and counts.sum() == n and cnt == (n + 4) // 5 and 0 < mn < mx
        after = (c.stats(), c.state_count(), c.highlight_info(), c.download_state())
        assert before[:3] == after[:3] and np.array_equal(before[3], after[3])
        b = c.render(params)                                              # no new sort: the order is still there
        assert a[..., :3].any(), "the frame is the bare background"
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- with the rest of the editor

def test_select_range_then_compact():
    n = 4096
    rows = make_rows(n, seed=77)
    rows[::9, 27] = (np.arange(len(rows[::9])) % 40).astype(np.uint8)      # alpha bytes on both sides of 16
    with capi.Context(0) as c:
        c.push_splat(rows)
        cs, cc = records(c, rows)
        v = capi.prop_eval(cs, cc, capi.PROP_ALPHA).reshape(-1)
        low = v <= 16
        assert 50 < low.sum() < n // 2
        assert c.select_range(capi.PROP_ALPHA, 0, 16, set_bits=HIDDEN) == low.sum()
        drawn, t0 = c.histogram(capi.PROP_ALPHA, 0.0, 255.0, 256, HIDDEN, 0)
        assert t0[0] == n - low.sum() and not drawn[:17].any()
        old = c.compact()
        assert np.array_equal(old, np.flatnonzero(~low)) and c.count() == n - low.sum()
        kept, t1 = c.histogram(capi.PROP_ALPHA, 0.0, 255.0, 256)
        want = np.bincount(rows[~low, 27], minlength=256).astype(np.uint32)
        assert np.array_equal(kept, want) and np.array_equal(kept, drawn) and list(t1) == [n - low.sum(), 0, 0, 0]
        records(c, rows[~low])


# ---------------------------------------------------------------- errors, empty contexts, gs_multi

def _code(fn, *a, **k):
    with pytest.raises(capi.GsError) as e:
        fn(*a, **k)
    return e.value.code


def test_arguments_and_empty_contexts():
    L = capi.load()
    with capi.Context(0) as c:
        for ctx_has_rows in (False, True):
            if ctx_has_rows:
                c.push_splat(make_rows(10, seed=1))
            for prop in (-1, 8, 1000):
                assert _code(c.prop_range, prop) == capi.E_BADARG
                assert _code(c.histogram, prop, 0.0, 1.0, 4) == capi.E_BADARG
                assert _code(c.select_range, prop, 0.0, 1.0) == capi.E_BADARG
            for lo, hi, nbins in ((1.0, 1.0, 4), (2.0, 1.0, 4), (np.nan, 1.0, 4), (0.0, np.nan, 4), (0.0, np.inf, 4), (-np.inf, 0.0, 4), (0.0, 1.0, 0),
                                  (0.0, 1.0, 4097)):
                assert _code(c.histogram, 0, lo, hi, nbins) == capi.E_BADARG, (lo, hi, nbins)
            assert _code(c.select_range, 0, np.nan, 1.0) == capi.E_BADARG and _code(c.select_range, 0, 0.0, np.nan) == capi.E_BADARG
            assert _code(c.select_range, 0, 0.0, 1.0, flags=2) == capi.E_BADARG
            t = np.zeros(4, np.uint64)
            assert L.gs_histogram(c._h, 0, 0.0, 1.0, 4, 0, 0, None, t.ctypes.data) == capi.E_BADARG
            assert L.gs_prop_range(c._h, 0, 0, 0, None, None, None) == capi.E_BADARG
            n_out = C.c_size_t(99)
            assert L.gs_prop_range(c._h, 0, 0, 0, None, None, C.byref(n_out)) == capi.GS_OK and n_out.value == (10 if ctx_has_rows else 0)
            cnt = np.full(4, 9, np.uint32)
            assert L.gs_histogram(c._h, 0, -100.0, 100.0, 4, 0, 0, cnt.ctypes.data, None) == capi.GS_OK     # (the tally is optional)
            assert cnt.sum() == (10 if ctx_has_rows else 0)
            if not ctx_has_rows:                                          # nothing resident: zero counts, an empty range, no hit
                counts, tally = c.histogram(capi.PROP_ALPHA, 0.0, 255.0, 256, 1, 0)
                assert not counts.any() and not tally.any()
                assert c.prop_range(capi.PROP_X) == (np.inf, -np.inf, 0)
                assert c.select_range(capi.PROP_X, -1.0, 1.0, set_bits=HIDDEN) == 0 and c.state_count() == (0, 0)
        c.clear()
        assert c.prop_range(capi.PROP_X) == (np.inf, -np.inf, 0)
    with capi.Context(0) as c:                                            # worker matrices only: no packed records
        m = np.zeros((8, 16), np.float32); m[:, 15] = 1.0
        c.push_matrices(m)
        assert _code(c.prop_range, 0) == capi.E_STATE
        assert _code(c.histogram, 0, 0.0, 1.0, 4) == capi.E_STATE
        assert _code(c.select_range, 0, 0.0, 1.0, set_bits=HIDDEN) == capi.E_STATE
        assert _code(c.histogram, 9, 0.0, 1.0, 4) == capi.E_BADARG


def _multi_store(m, i):
    L = capi.load()
    h = L.gs_multi_ctx(m._h, i)
    rows, hidden = C.c_size_t(0), C.c_size_t(0)
    assert L.gs_state_count(h, C.byref(rows), C.byref(hidden)) == capi.GS_OK
    out = np.zeros(max(rows.value, 1), np.uint8)
    assert L.gs_download(h, capi.BUF_STATE, out.ctypes.data, rows.value) == capi.GS_OK
    return out[:rows.value], hidden.value


def test_multi_world2():
    n = 3000
    rows = make_rows(n, seed=21)
    with capi.Multi([0, 0]) as m, capi.Context(0) as one:
        m.push_splat(rows); one.push_splat(rows)
        cs, cc = records(one, rows)
        v = capi.prop_eval(cs, cc, capi.PROP_SIZE2).reshape(-1)
        lo, hi = span_of(v)
        inside = (lo <= v) & (v <= hi)
        assert m.select_range(capi.PROP_SIZE2, lo, hi, set_bits=HIDDEN, flags=INVERT) == n - inside.sum()
        assert one.select_range(capi.PROP_SIZE2, lo, hi, set_bits=HIDDEN, flags=INVERT) == n - inside.sum()
        m.sync()
        s0, h0 = _multi_store(m, 0)
        s1, h1 = _multi_store(m, 1)
        want = np.where(inside, 0, HIDDEN).astype(np.uint8)
        assert np.array_equal(s0, want) and np.array_equal(s1, want) and h0 == h1 == n - inside.sum()
        for mask, value in ((0, 0), (1, 0)):
            mc, mt = m.histogram(capi.PROP_SIZE2, lo, hi, 100, mask, value)
            oc, ot = one.histogram(capi.PROP_SIZE2, lo, hi, 100, mask, value)
            wc, wt = hist_mirror(v, passing_of(n, want, mask, value), lo, hi, 100)
            assert np.array_equal(mc, oc) and np.array_equal(mt, ot) and np.array_equal(mc, wc) and np.array_equal(mt, wt)
            assert m.prop_range(capi.PROP_SIZE2, mask, value) == one.prop_range(capi.PROP_SIZE2, mask, value) == range_mirror(v, passing_of(n, want, mask, value))
