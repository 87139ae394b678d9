"""GPU tier of gs_transform (include/gs_splat.h): the similarity baked into resident splats by k_transform_records / k_transform_sh.

The moved records, sort rows and SH rows are exact: capi.transform_records / capi.transform_sh_rows -- the kernels' own functions on the host,
pinned to the header's rule by tests/test_transform_cpu.py -- applied to what the context held before (gs_download), for the splats the state
filter passes; everything else of the resident arrays is byte-identical to before.  Where the rule is exact (a translation, a scale by a
power of two) the context is held against a fresh one that was pushed the rows moved in numpy.  Frames are 64 x 48 with the blend path
pinned as tests/test_adjust_gpu.py pins it, so every comparison is bit for bit."""
import math

import numpy as np
import pytest

from conftest import pkg
from test_adjust_gpu import (CALLER, FILTERS, GRID, BLOCK, H, HIDDEN, SELECTED, SIZES, W, camera, context, make_rows, passing_of, random_store,
                             scene_of, snapshot, stats_of)

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

assert SIZES == [1, 255, 256, 257, 2049, GRID * BLOCK + 1]
U32 = np.uint32


def quat(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    h = math.radians(deg) / 2
    return (math.cos(h), *(math.sin(h) * a))


# a general similarity: a rotation about a skew axis, a scale, a translation
GENERAL = capi.similarity(rotation=quat((0.3, -0.8, 0.52), 37.0), scale=1.75, translation=(0.5, -1.25, 3.0))
TURN = capi.similarity(rotation=quat((-0.6, 0.1, 0.79), 112.0))
MOVE = capi.similarity(translation=(0.5, -0.25, 2.0))
DOUBLE = capi.similarity(scale=2.0)


def contrib_of(c):
    return c.download_contrib().copy()


# ---------------------------------------------------------------- the records

@pytest.mark.parametrize("n", SIZES)
def test_records_against_the_host_rule(n):
    g = np.random.Generator(np.random.PCG64(9700 + n))
    cam, p = camera()
    with context() as c:
        c.push_splat(make_rows(n, seed=500 + n % 1000))
        if n <= 2049:                                            # a contribution store to find untouched
            c.sort(cam["view"], want_indices=False)
            c.render_contrib(p, want_rgba=False)
        seen = contrib_of(c)
        short = n - max(n // 3, 1) if n > 1 else 0               # no store, a store shorter than N, a full one
        for length in sorted({0, short, n}):
            store = random_store(g, length)
            if length:
                c.set_state(0, store)
            for mask, value in FILTERS:
                cs, cc, sr, st = snapshot(c, n)
                ok = passing_of(n, store, mask, value)
                hit = c.transform(GENERAL, (mask, value))
                cs2, cc2, sr2, st2 = snapshot(c, n)
                assert hit == int(ok.sum()), (length, mask, value)
                want = [cs.copy(), cc.copy(), sr.copy()]
                for w, m in zip(want, capi.transform_records(cs[ok], cc[ok], sr[ok], GENERAL)):
                    w[ok] = m
                for name, got, exp, old in (("cs", cs2, want[0], cs), ("cc", cc2, want[1], cc), ("sort rows", sr2, want[2], sr)):
                    assert np.array_equal(got[ok], exp[ok]), (name, length, mask, value, np.flatnonzero((got != exp).any(axis=1))[:8])
                    assert np.array_equal(got[~ok], old[~ok]), (name, "a splat that does not pass was written", length, mask, value)
                assert np.array_equal(cc2[:, 3], cc[:, 3])                                   # the colour word stays
                assert np.array_equal(st2, st) and len(st2) == length and c.state_count()[0] == length   # the store is neither grown nor changed
                assert np.array_equal(contrib_of(c), seen) and c.count() == n
                if ok.sum() > 8:
                    assert not np.array_equal(cs2[ok], cs[ok]) and not np.array_equal(cc2[ok, :3], cc[ok, :3])


# ---------------------------------------------------------------- the SH store

def check_sh(c, n, sh_n, degree, store, mask, value, t, turns):
    before = c.download_sh()
    ok = passing_of(n, store, mask, value)
    assert c.transform(t, (mask, value)) == int(ok.sum())
    after = c.download_sh()
    want = before.copy()
    sel = np.flatnonzero(ok[:sh_n])
    want[sel] = capi.transform_sh_rows(before[sel], degree, t)
    assert after.shape == (sh_n, 3 * (degree + 1) ** 2) and c.sh_count() == (sh_n, degree)
    assert np.array_equal(after.view(U32), want.view(U32)), (degree, mask, value)
    if turns and sel.size:
        assert not np.array_equal(after[sel], before[sel])
    if not turns:
        assert np.array_equal(after.view(U32), before.view(U32))          # a pure translation or scale leaves the whole store untouched


@pytest.mark.parametrize("sh_n", [500, 700])
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_sh_rows_against_the_host_rule(degree, sh_n):
    n = 700                                                       # an SH store shorter than N, and one of length N
    g = np.random.Generator(np.random.PCG64(9800 + degree))
    sh = g.uniform(-1.0, 1.0, size=(sh_n, 3 * (degree + 1) ** 2)).astype(np.float32)
    with context() as c:
        c.push_splat(make_rows(n, seed=45))
        c.push_sh(sh, degree)
        check_sh(c, n, sh_n, degree, np.zeros(0, np.uint8), 0, 0, TURN, True)
        for edge in (300, 600):                                   # the filter's boundary inside the SH store, then beyond it (or at 600 of 700)
            store = np.zeros(n, np.uint8)
            store[:edge] = CALLER
            c.set_state(0, store)
            check_sh(c, n, sh_n, degree, store, CALLER, CALLER, GENERAL, True)
        store = np.concatenate([random_store(g, n - 40), np.zeros(40, np.uint8)])
        c.set_state(0, store)
        for mask, value in FILTERS:
            check_sh(c, n, sh_n, degree, store, mask, value, TURN, True)
        for t in (MOVE, DOUBLE, capi.similarity(scale=0.3, translation=(1.0, 2.0, 3.0))):
            check_sh(c, n, sh_n, degree, store, 0, 0, t, False)


def test_sh_kernel_second_trip_of_the_grid():
    degree, K = 1, 4
    sh_n = GRID * BLOCK // 3 + 1                                  # one (row, channel) item more than the capped grid covers in one trip
    n = sh_n + 31
    g = np.random.Generator(np.random.PCG64(9810))
    sh = g.uniform(-1.0, 1.0, size=(sh_n, 3 * K)).astype(np.float32)
    store = random_store(g, n)
    with context() as c:
        c.push_splat(make_rows(n, seed=46))
        c.push_sh(sh, degree)
        c.set_state(0, store)
        check_sh(c, n, sh_n, degree, store, HIDDEN, 0, TURN, True)


# ---------------------------------------------------------------- equal to a fresh context where the rule is exact

def moved_rows(rows, kind, ok):
    """.splat rows with the rows `ok` moved in numpy: f64, rounded once"""
    out = np.array(rows, np.uint8).reshape(-1, 32).copy()
    pos = out[:, :12].copy().view("<f4").reshape(-1, 3).astype(np.float64)
    scl = out[:, 12:24].copy().view("<f4").reshape(-1, 3).astype(np.float64)
    if kind == "translation":
        pos[ok] += np.array(list(MOVE.translation), np.float64)
    else:
        pos[ok] *= 2.0
        scl[ok] *= 2.0
    out[:, :12] = pos.astype("<f4").view(np.uint8).reshape(-1, 12)
    out[:, 12:24] = scl.astype("<f4").view(np.uint8).reshape(-1, 12)
    return out


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("kind", ["translation", "scale"])
def test_equal_to_a_fresh_context(kind, half):
    cam, p = camera()
    rows, store = scene_of(4096, 97)
    n = len(rows)
    ok = passing_of(n, store, 3, SELECTED) if half else np.ones(n, bool)
    t = MOVE if kind == "translation" else DOUBLE
    with context() as a, context() as b:
        a.push_splat(rows); a.set_state(0, store)
        a.sort(cam["view"], want_indices=False)
        first = a.render(p)
        assert a.transform(t, "selected" if half else "all") == int(ok.sum())
        b.push_splat(moved_rows(rows, kind, ok)); b.set_state(0, store)
        for name, x, y in zip(("cs", "cc", "sort rows", "states"), snapshot(a, n), snapshot(b, n)):
            assert np.array_equal(x, y), (name, np.flatnonzero((x != y).reshape(n, -1).any(axis=1))[:8])
        oa, ob = a.sort(cam["view"]), b.sort(cam["view"])
        assert np.array_equal(oa, ob) and len(oa) > 100
        fa, fb = a.render(p), b.render(p)
        assert np.array_equal(fa, fb) and fa.any() and not np.array_equal(fa, first)
        assert stats_of(a) == stats_of(b)


# ---------------------------------------------------------------- the strip bound follows the scale

def test_strip_bound_follows_the_scale():
    """gs_sort_for culls by bound_r, the bound of the splat's size in object space: after a scale by 8 a stale bound drops splats whose
    grown footprint reaches the strip."""
    cam, p = camera()
    strip = capi.make_params(cam["gs_mv"], cam["gs_proj"], W, H, x0=16, x1=32, focal_=cam["focal"])
    rows, _ = scene_of(4096, 98)
    with context() as c:
        c.push_splat(rows)
        assert c.transform(capi.similarity(scale=8.0)) == len(rows)
        whole = c.sort(cam["view"])
        full = c.render(p)
        sub = c.sort_for(cam["view"], None, strip)
        part = c.render(strip)
        assert 0 < len(sub) <= len(whole) and full[:, 16:32].any()
        assert np.array_equal(part, full[:, 16:32])


# ---------------------------------------------------------------- orders and posted sorts

def test_orders_are_dropped_and_a_posted_sort_runs_again():
    cam, p = camera()
    rows, store = scene_of(2500, 99)
    with context() as c, context() as pushed:
        c.push_splat(rows)
        c.sort(cam["view"], want_indices=False)
        assert c.render(p).any()
        c.sort_begin(cam["view"])                                 # posted before the change, collected after it
        assert c.transform(GENERAL) == len(rows)
        pushed.push_splat(rows)                                   # as after a push: a render before the next sort draws the background only
        blank = c.render(p)
        assert np.array_equal(blank, pushed.render(p)) and (blank == blank[0, 0]).all()
        got = c.sort_poll(wait=True)
        assert np.array_equal(got, c.sort(cam["view"])) and len(got) > 100     # the order of the transformed cloud
        assert c.render(p).any()
        before = c.download(capi.BUF_SORT_ROWS, len(rows), U32, 4)
        pushed.sort(cam["view"], want_indices=False)
        assert not np.array_equal(before, pushed.download(capi.BUF_SORT_ROWS, len(rows), U32, 4))


# ---------------------------------------------------------------- two contexts of one GPU

def test_multi_transform_on_two_contexts_of_one_gpu():
    rows, store = scene_of(4096, 100)
    n = len(rows)
    g = np.random.Generator(np.random.PCG64(9900))
    sh = g.uniform(-1.0, 1.0, size=(n, 12)).astype(np.float32)
    ok = passing_of(n, store, 3, SELECTED)
    L = capi.load()

    def download(h, which, width):
        out = np.zeros((n, width), U32)
        assert L.gs_download(h, which, capi._p(out), out.nbytes) == capi.GS_OK
        return out

    with capi.Multi([0, 0]) as m, context() as one:
        hs = [L.gs_multi_ctx(m._h, i) for i in range(2)]
        for c in (m, one):
            c.push_splat(rows); c.push_sh(sh, 1); c.set_state(0, store)
        assert m.transform(GENERAL, "selected") == one.transform(GENERAL, "selected") == int(ok.sum())
        want = [one.download(capi.BUF_CENTER_SCALE, n, U32, 4), one.download(capi.BUF_COV_COLOR, n, U32, 4),
                one.download(capi.BUF_SORT_ROWS, n, U32, 4), one.download(capi.BUF_SH, n, U32, 12)]
        for h in hs:
            got = [download(h, capi.BUF_CENTER_SCALE, 4), download(h, capi.BUF_COV_COLOR, 4), download(h, capi.BUF_SORT_ROWS, 4), download(h, capi.BUF_SH, 12)]
            for x, y in zip(got, want):
                assert np.array_equal(x, y)
        assert not np.array_equal(want[3].view(np.float32)[ok], sh[ok])


# ---------------------------------------------------------------- errors

def test_errors_change_nothing():
    n = 300
    rows = make_rows(n, 96)
    with context() as c:
        assert c.transform(GENERAL) == 0                          # nothing resident
        c.push_splat(rows)
        c.push_sh(np.ones((100, 12), np.float32), 1)
        before, sh = snapshot(c, n), c.download_sh()
        bad = [capi.similarity(scale=0.0), capi.similarity(scale=-2.0), capi.similarity(rotation=(0.0, 0.0, 0.0, 0.0)),
               capi.similarity(translation=(0.0, np.nan, 0.0)), capi.similarity(rotation=(1.0, np.inf, 0.0, 0.0)), capi.similarity(scale=np.inf)]
        for t in bad:
            with pytest.raises(capi.GsError) as e:
                c.transform(t)
            assert e.value.code == capi.E_BADARG
        assert c._L.gs_transform(c._h, None, 0, 0, None) == capi.E_BADARG
        for x, y in zip(snapshot(c, n), before):
            assert np.array_equal(x, y)
        assert np.array_equal(c.download_sh(), sh)
    with capi.Context(0) as c:
        c.push_matrices(np.zeros((4, 16), np.float32))
        with pytest.raises(capi.GsError) as e:
            c.transform(GENERAL)
        assert e.value.code == capi.E_STATE
