"""GPU tier: gs_compact and the region selections (csrc/gs_edit.hip) at the sizes where their own chunking changes behaviour.

gs_compact: one workgroup per CH = GS_EDIT_IPT * GS_BLOCK splats, one thread per IPT consecutive ones, and ONE workgroup that scans the
per-chunk counts STEP = GS_BLOCK at a time with a carry between steps -- so the sizes lie around a thread (IPT), a wave (WAVE), a chunk (CH)
and the first and second step of the offsets loop (STEP * CH, 2 * STEP * CH).  The reference is numpy: kept = flatnonzero(~hid), and every
array the context holds, downloaded BEFORE the call, indexed with it -- bit for bit.  bound_r has no download: it is seen through gs_sort_for
of a 64-pixel strip against a fresh context fed rows[kept].
The grid-strided kernels end their grid at GRID = GS_EDIT_GRID workgroups: their loop comes round only beyond GRID * BLOCK items, so they
run at N1 = GRID * BLOCK + 1 and N2 = 2 * GRID * BLOCK + BLOCK + 1 against the f64 mirrors of test_edit_gpu / test_select_mask_gpu; the two
that walk the order run on a scene of 4096 rows pushed T times (the decision for splat i is the oracle's for row i % 4096).
The store across ensure_capacity's doublings, and the sphere / box predicates on their boundaries (hand-built rows, exact in f64).

Every size is an expression in the constants read out of the sources.  Where a case claims something about its own input, the claim is
asserted from the input before the GPU's answer is looked at."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT, cached_rows, pkg
from oracle import oracle
from test_edit_gpu import box_mirror, mats_of, plain_rows, scene, sort_ctx, want_order
from test_sort_paths_gpu import _constant

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

IPT = _constant("GS_EDIT_IPT", "gs_cloud_pass.h")
GRID = _constant("GS_EDIT_GRID", "gs_cloud_pass.h")
BLOCK = _constant("GS_BLOCK", "gs_internal.h")
CH, WAVE, STEP = IPT * BLOCK, 64 * IPT, BLOCK
GB = GRID * BLOCK
N1, N2 = GB + 1, 2 * GB + BLOCK + 1
SMALL = [IPT - 1, IPT, IPT + 1, WAVE - 1, WAVE + 1, CH - 1, CH, CH + 1]
LARGE = [STEP * CH - 1, STEP * CH, STEP * CH + 1, (2 * STEP + 1) * CH + 3]
NBIG = max(LARGE[-1], N2)
BOUND_AT = (CH + 1, LARGE[-1])                                      # where bound_r is seen through a strip sort: one size per family
HIDDEN, SELECTED, INVERT = capi.STATE_HIDDEN, capi.STATE_SELECTED, capi.SELECT_INVERT
VIEW = np.array([0.0, 0.0, 1.0, 0.0], np.float32)
W, H = 256, 144


def big_rows(n):
    assert n <= NBIG
    return cached_rows("make_splat_rows_fast", NBIG).reshape(NBIG, 32)[:n]


def rng(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


@functools.lru_cache(maxsize=None)
def camera():
    cam = synth.index_html_camera(W, H, yaw_deg=15.0, capi=capi)
    p = capi.make_params(cam["gs_mv"], cam["gs_proj"], W, H, focal_=cam["focal"])
    strip = capi.make_params(cam["gs_mv"], cam["gs_proj"], W, H, x0=64, x1=128, focal_=cam["focal"])
    return cam, p, strip


# ---------------------------------------------------------------- 1. compaction against numpy

def chunk_counts(hid):
    """kept splats per chunk of CH, as k_compact_count sees them"""
    return np.add.reduceat((~hid).astype(np.int64), np.arange(0, hid.size, CH))


def hidden_sets(n, g):
    """(name, hidden set) for n splats, each where it means something at this size"""
    i = np.arange(n)
    out = []

    def add(name, hid):
        if hid.any():
            out.append((name, hid))
    add("first", i == 0)
    add("last", i == n - 1)
    if n > 1:
        add("all_but_first", i != 0)
        add("all_but_last", i != n - 1)
    add("all", np.ones(n, bool))
    add("alternate", i % 2 == 0)
    if n > IPT:
        add("threads", (i // IPT) % 2 == 0)
    if n > WAVE:
        add("waves", (i // WAVE) % 2 == 1)
    if n > CH:
        add("chunks", (i // CH) % 2 == 0)
    for p in (0.01, 0.5, 0.99):
        hid = g.random(n) < p
        if not hid.any():
            hid[int(g.integers(0, n))] = True
        add("random_%g" % p, hid)
    if n >= STEP * CH - 1:                                              # count 0 on either side of the carry, the neighbours full
        hid = (i // CH == STEP - 1) | (i // CH == STEP)
        cnt = chunk_counts(hid)
        assert cnt[STEP - 1] == 0 and cnt[STEP - 2] == CH and (cnt.size <= STEP or cnt[STEP] == 0) and (cnt.size <= STEP + 1 or cnt[STEP + 1] > 0)
        add("carry_chunks", hid)
        hid = i // CH < (n - 1) // CH                                   # every chunk but the last: a carry of 0 into a non-empty tail
        cnt = chunk_counts(hid)
        assert not cnt[:-1].any() and cnt[-1] > 0 and cnt.size == (n + CH - 1) // CH and (n <= STEP * CH or cnt.size > STEP)
        add("only_last_chunk", hid)
    return out


def snapshot(c, renderable=True):
    """the context's own arrays; the state store padded with the zeros the header promises behind its end"""
    n = c.count()
    s = {"rows": c.download(capi.BUF_SORT_ROWS, n, np.uint32, 4), "sh": c.download_sh().view(np.uint32)}
    if renderable:
        s["cs"] = c.download(capi.BUF_CENTER_SCALE, n, np.uint32, 4)
        s["cc"] = c.download(capi.BUF_COV_COLOR, n, np.uint32, 4)
    st = c.download_state()
    s["store"] = st.size
    s["state"] = np.concatenate([st, np.zeros(n - st.size, np.uint8)])
    return s


def compact_and_check(c, hid, tag, renderable=True, grow=True):
    """gs_compact of the context, whose hidden set is `hid` (asserted from the downloaded store), against numpy -> (kept, before)"""
    n = c.count()
    before = snapshot(c, renderable)
    store, nh = c.state_count()
    nsh, deg = c.sh_count()
    assert hid.size == n and store == before["store"] and nh == hid.sum() and np.array_equal((before["state"] & HIDDEN) != 0, hid), tag
    kept = np.flatnonzero(~hid).astype(np.uint32)
    old = c.compact()
    assert old.size == kept.size and np.array_equal(old, kept), (tag, "the index map")
    assert c.count() == kept.size and c.state_count() == (store - nh, 0), tag
    ksh = kept[kept < nsh]
    assert c.sh_count() == (ksh.size, deg if ksh.size else 0), tag
    after = snapshot(c, renderable)
    for k in ("rows", "cs", "cc") if renderable else ("rows",):
        assert np.array_equal(after[k], before[k][kept]), (tag, k)
    assert np.array_equal(after["sh"].reshape(-1), before["sh"][ksh].reshape(-1)), (tag, "sh")
    assert after["store"] == store - nh and np.array_equal(after["state"][:store - nh], before["state"][kept][:store - nh]), (tag, "state")
    if kept.size and grow:
        # the splats behind the store are kept and arrive with state 0: an id list that changes no bit grows the store to gs_count()
        c.set_state_ids([kept.size - 1])
        assert c.state_count() == (kept.size, 0) and np.array_equal(c.download_state(), before["state"][kept]), (tag, "state behind the store")
    return kept, before


def states_of(hid, g, store=None):
    store = hid.size if store is None else store
    assert not hid[store:].any()
    return hid[:store].astype(np.uint8) | (g.integers(0, 64, store).astype(np.uint8) << 2)        # user bits 2..7 random


def strip_check(c, rows_kept, tag):
    """bound_r after the scatter: the strip's order (its reach test reads bound_r) equals a fresh context's that was pushed the kept rows"""
    cam, _, strip = camera()
    with capi.Context(0) as b:
        b.push_splat(rows_kept)
        want = b.sort_for(cam["view"], None, strip)
    got = c.sort_for(cam["view"], None, strip)
    assert 0 < want.size < len(rows_kept) and np.array_equal(got, want), tag


@pytest.mark.parametrize("n", SMALL + LARGE)
def test_compact_sizes_and_hidden_sets(n):
    g = rng(5100, n)
    rows = big_rows(n)
    sets = hidden_sets(n, g)
    names = [s[0] for s in sets]
    assert {"first", "last", "all", "random_0.5"} <= set(names) and (n < STEP * CH - 1 or {"carry_chunks", "only_last_chunk"} <= set(names))
    with capi.Context(0) as c:
        for name, hid in sets:
            c.clear()
            c.push_splat(rows)
            c.set_state(0, states_of(hid, g))
            kept, _ = compact_and_check(c, hid, (n, name))
            if n in BOUND_AT and name == "random_0.5":
                strip_check(c, rows[kept], (n, name))
            assert np.array_equal(c.compact(), np.arange(kept.size, dtype=np.uint32)), "nothing hidden: nothing happens"


STORE_N = STEP * CH + WAVE + 3
STORES = {"full": STORE_N, "one": 1, "mid_thread_in_chunk_1": CH + 3 * IPT + 3, "at_CH": CH, "at_STEP_CH": STEP * CH}


@pytest.mark.parametrize("shape", list(STORES))
def test_compact_store_shorter_than_count(shape):
    n, store = STORE_N, STORES[shape]
    assert store <= n and (shape == "full") == (store == n)
    assert shape != "mid_thread_in_chunk_1" or (store // CH == 1 and store % IPT != 0)
    g = rng(5200, store)
    hid = np.zeros(n, bool)
    hid[:store] = g.random(store) < 0.5
    if store == 1:
        hid[0] = True                                                   # (only splat 0 can be hidden)
    assert hid[:store].any()
    with capi.Context(0) as c:
        c.push_splat(big_rows(n))
        c.set_state(0, states_of(hid, g, store))
        kept, before = compact_and_check(c, hid, shape)
        assert kept.size - (store - hid.sum()) == n - store             # everything behind the store was kept


SH_N, SH_STORE = 2 * CH + 5, CH + 3 * IPT + 3
SH_CASES = [(SH_N, SH_STORE, 0), (SH_N, SH_STORE, CH // 2 + 1), (SH_N, SH_STORE, SH_STORE + IPT + 1), (SH_N, SH_STORE, SH_N),
            (STEP * CH + 1, STEP * CH + 1, (STEP * CH) // 2)]       # the last: k_compact_sh's own grid comes round (asserted)


@pytest.mark.parametrize("n,store,nsh", SH_CASES)
def test_compact_sh_rows(n, store, nsh):
    assert nsh == 0 or nsh < store or store < nsh < n or nsh == n
    g = rng(5300, n, nsh)
    hid = np.zeros(n, bool)
    hid[:store] = g.random(store) < 0.5
    sh = g.normal(0.0, 0.2, (nsh, 27)).astype(np.float32)
    if n > SH_N:
        assert (~hid[:nsh]).sum() * 27 // 4 > GB                        # (a stored row is at least its 27 floats: more 16-byte words than one pass)
    with capi.Context(0) as c:
        c.set_option(capi.OPT_SH_DEGREE, 2)
        c.push_splat(big_rows(n))
        if nsh:
            c.push_sh(sh, 2)
        assert c.sh_count() == ((nsh, 2) if nsh else (0, 0))
        c.set_state(0, states_of(hid, g, store))
        kept, before = compact_and_check(c, hid, (n, store, nsh))
        assert before["sh"].size == nsh * 27 and np.array_equal(before["sh"].reshape(-1), sh.view(np.uint32).reshape(-1))


@pytest.mark.parametrize("n", [CH + 1, STEP * CH + 1])
def test_compact_matrices_only(n):
    g = rng(5400, n)
    rows4 = plain_rows(g, n)
    hid = g.random(n) < 0.5
    kept = np.flatnonzero(~hid)
    with sort_ctx(rows4, states_of(hid, g)) as c:
        k2, before = compact_and_check(c, hid, n, renderable=False)
        assert np.array_equal(before["rows"], rows4.view(np.uint32))
        assert np.array_equal(c.sort(VIEW), oracle.sort(rows4[kept], VIEW))
        with pytest.raises(capi.GsError) as e:
            c.select_sphere([0, 0, 0], 1.0, set_bits=HIDDEN)
        assert e.value.code == capi.E_STATE


@pytest.mark.parametrize("n", [3 * CH + 17, STEP * CH + 1])
def test_compact_twice_then_push_and_hide(n):
    """the map composes over two compactions; rows pushed afterwards arrive with state 0 behind a store that ends 5 splats early"""
    g = rng(5500, n)
    cam, _, _ = camera()
    rows = big_rows(n)
    store = n - 5
    hid1 = np.zeros(n, bool); hid1[:store] = g.random(store) < 0.4
    kept1 = np.flatnonzero(~hid1)
    hid2 = np.zeros(kept1.size, bool); hid2[:kept1.size - 5] = g.random(kept1.size - 5) < 0.6
    both = hid1.copy(); both[kept1[hid2]] = True
    kept = np.flatnonzero(~both)
    m = CH + 3
    more = synth.make_splat_rows_fast(m, seed=977).reshape(m, 32)
    assert not np.array_equal(more[:8], rows[:8])
    with capi.Context(0) as c:
        c.push_splat(rows)
        st1 = states_of(hid1, g, store)
        c.set_state(0, st1)
        old1, _ = compact_and_check(c, hid1, (n, "first"), grow=False)
        user = c.download_state()
        assert user.size == kept1.size - 5 and np.array_equal(user, st1[kept1[kept1 < store]])
        c.set_state(0, user | hid2[:user.size].astype(np.uint8))
        old2, _ = compact_and_check(c, hid2, (n, "second"), grow=False)
        assert np.array_equal(old1[old2], kept)
        user = c.download_state()
        assert user.size == kept.size - 5 and user.any()
        c.push_splat(more)
        assert c.count() == kept.size + m and c.state_count() == (kept.size - 5, 0)
        tail = (g.random(m) < 0.5).astype(np.uint8) | np.uint8(64)
        c.set_state(c.count() - m, tail)
        assert c.state_count() == (kept.size + m, int((tail & 1).sum()))
        assert np.array_equal(c.download_state(), np.concatenate([user, np.zeros(5, np.uint8), tail]))
        allrows = np.concatenate([rows[kept], more])
        _, _, mats = oracle.pack(allrows.reshape(-1))
        Hh = np.concatenate([np.zeros(kept.size, bool), (tail & 1) != 0])
        want = want_order(mats[:, 12:16], Hh, cam["view"])
        assert 0 < want.size and np.array_equal(c.sort(cam["view"]), want)


# ---------------------------------------------------------------- 2. the store across a capacity change

def first_capacity():
    """gs_lanes.hip: ensure_capacity starts at (size_t)1 << 16 and doubles -- plain code, no #define, so read from the text"""
    with open(os.path.join(ROOT, PKG_NAME, "csrc", "gs_lanes.hip")) as f:
        body = f.read().split("int gs_ctl::ensure_capacity(", 1)[1].split("\n}\n", 1)[0]
    m = re.search(r"size_t cap = ctx->cap \? ctx->cap : \(size_t\)1 << (\d+);\s*while \(cap < want\) cap \*= 2;", body)
    assert m, "ensure_capacity's growth rule not found"
    return 1 << int(m.group(1))


@pytest.mark.parametrize("store", ["full", "one"])
def test_store_survives_two_doublings(store):
    cap0 = first_capacity()
    n0, more = cap0, (1, 70000)
    assert n0 + more[0] > cap0 and n0 + sum(more) > 2 * cap0
    g = rng(5600, n0)
    cam, _, _ = camera()
    rows = big_rows(n0 + sum(more))
    _, _, mats = oracle.pack(rows.reshape(-1))
    rows4 = mats[:, 12:16]
    st = g.integers(0, 256, n0 if store == "full" else 1).astype(np.uint8)
    st[-1] |= HIDDEN | 4                                               # (the store's last byte is not a zero)
    assert store == "one" or (0.4 * n0 < (st & 1).sum() < 0.6 * n0 and (st & SELECTED).any() and (st >> 2).any())
    with capi.Context(0) as c:
        c.push_splat(rows[:n0])
        c.set_state(0, st)
        at = n0
        for k in more:
            c.push_splat(rows[at:at + k]); at += k
            assert c.count() == at
            assert np.array_equal(c.download_state(), st) and c.state_count() == (st.size, int((st & 1).sum())), at
            Hh = np.zeros(at, bool); Hh[:st.size] = (st & 1) != 0
            want = want_order(rows4[:at], Hh, cam["view"])
            assert 0 < want.size and np.array_equal(c.sort(cam["view"]), want), at
        box = np.zeros(16, np.float32); box[0] = box[5] = box[10] = 0.125; box[12] = 0.25; box[15] = 1.0
        inside = box_mirror(rows4, box)
        assert all(a[sl].any() for a in (inside, ~inside) for sl in (slice(0, n0), slice(n0, 2 * cap0), slice(2 * cap0, at)))
        full = np.zeros(at, np.uint8); full[:st.size] = st
        assert c.select_box(box, set_bits=SELECTED, clear_bits=4, flags=INVERT) == (~inside).sum()
        assert c.state_count()[0] == at
        assert np.array_equal(c.download_state(), np.where(~inside, (full & ~np.uint8(4)) | SELECTED, full).astype(np.uint8))


# ---------------------------------------------------------------- 3. the grid stride of the six older kernels

@pytest.mark.parametrize("n", [N1, N2])
def test_count_hidden_and_ids_grid_stride(n):
    g = rng(5700, n)
    i = np.arange(n)
    with sort_ctx(plain_rows(g, n)) as c:
        for name, hid in (("beyond_the_grid", i >= GB), ("first_block", i < BLOCK), ("tenth", g.random(n) < 0.1)):
            st = hid.astype(np.uint8) | (g.integers(0, 64, n).astype(np.uint8) << 2)
            assert (st & 1).sum() == hid.sum() > 0
            c.set_state(0, st)
            assert c.state_count() == (n, int((st & 1).sum())), name
        ids = g.integers(0, n, N2).astype(np.uint32)
        ids[:4] = (0, GB - 1, GB, n - 1)
        assert np.unique(ids).size < ids.size and (ids < GB).sum() > 1000 and (ids >= GB).any() and (n < N2 or (ids >= GB).sum() > 1000)
        for set_bits, clear_bits in ((SELECTED | 16, HIDDEN | 32), (0, SELECTED | 4), (HIDDEN, 0)):
            want = st.copy()
            want[ids] = (st[ids] & ~np.uint8(clear_bits)) | np.uint8(set_bits)
            assert not np.array_equal(want, st)
            c.set_state_ids(ids, set_bits=set_bits, clear_bits=clear_bits)
            assert np.array_equal(c.download_state(), want), (set_bits, clear_bits)
            assert c.state_count() == (n, int((want & 1).sum()))
            st = want


def region_check(regions, n):
    """each region: (argument tuple, f64 mirror's inside[n]); plain and INVERT; members of region and complement on both sides of GB
    -- at N1 a single splat lies beyond GB, so there the claim is made over the regions together"""
    sides = np.zeros((2, 2), bool)
    for args, inside in regions:
        for s, sl in enumerate((slice(0, GB), slice(GB, n))):
            sides[s, 0] |= inside[sl].any(); sides[s, 1] |= (~inside[sl]).any()
        assert n < N2 or all(a[sl].any() for a in (inside, ~inside) for sl in (slice(0, GB), slice(GB, n)))
    assert sides.all()
    return [(args, inside, inv) for args, inside in regions for inv in (0, INVERT)]


@pytest.mark.parametrize("n", [N1, N2])
def test_select_box_grid_stride(n):
    g = rng(5800, n)
    rows4 = plain_rows(g, n)
    rows4[GB, :3] = (0.125, 0.125, -1.0)
    box1 = np.zeros(16, np.float32); box1[0] = box1[5] = box1[10] = 0.25; box1[15] = 1.0
    box2 = box1.copy(); box2[12] = 0.625                                # keeps -4.5 <= x <= -0.5: not the splat at GB
    persp = box1.copy(); persp[11] = -0.0625
    regions = [((b,), box_mirror(rows4, b)) for b in (box1, box2, persp)]
    assert regions[0][1][GB] and not regions[1][1][GB]
    base = (g.integers(0, 64, n).astype(np.uint8) << 2)
    with sort_ctx(rows4) as c:
        for (b,), inside, inv in region_check(regions, n):
            w = ~inside if inv else inside
            c.set_state(0, base)
            assert c.select_box(b, set_bits=SELECTED, clear_bits=8, flags=inv) == w.sum(), inv
            assert np.array_equal(c.download_state(), np.where(w, (base & ~np.uint8(8)) | SELECTED, base).astype(np.uint8)), inv


@pytest.mark.parametrize("n", [N1, N2])
def test_select_sphere_grid_stride(n):
    g = rng(5900, n)
    rows = big_rows(n)
    pos = rows[:, :12].copy().view("<f4").reshape(n, 3)
    regions = []
    for centre, radius in ((pos[GB], 2.0), (pos[GB] + np.float32(4.0), 2.0), (np.zeros(3, np.float32), 3.0)):
        centre = np.asarray(centre, np.float32)
        d = pos.astype(np.float64) - centre.astype(np.float64)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        regions.append(((centre, radius), d2 <= float(np.float32(radius)) * float(np.float32(radius))))
    assert regions[0][1][GB] and not regions[1][1][GB]
    base = (g.integers(0, 64, n).astype(np.uint8) << 2)
    with capi.Context(0) as c:
        c.push_splat(rows)
        for (centre, radius), inside, inv in region_check(regions, n):
            w = ~inside if inv else inside
            c.set_state(0, base)
            assert c.select_sphere(centre, radius, set_bits=HIDDEN, clear_bits=16, flags=inv) == w.sum(), inv
            assert np.array_equal(c.download_state(), np.where(w, (base & ~np.uint8(16)) | HIDDEN, base).astype(np.uint8)), inv


class Tiled:
    """m = 4096 rows pushed T times.  The sort's keep test and the projection are per row, so copy i + k m shares the decision of row i:
    the truth is computed once on the m rows, as test_select_rect / test_select_mask_gpu.Frame do it, and tiled."""

    def __init__(self):
        sc = scene()
        self.m, self.rows = sc.n, sc.rows
        self.cam, self.p, _ = camera()
        assert (sc.W, sc.H) == (W, H)
        cs, cc, mats = oracle.pack(self.rows.reshape(-1))
        self.hid = np.zeros(self.m, bool); self.hid[::7] = True
        order = want_order(mats[:, 12:16], self.hid, self.cam["view"])
        self.kept_m = order.size
        culled = (~self.hid).sum() - order.size
        assert len(np.unique(order)) == order.size and 0 < culled < self.m // 4, culled
        self.T = -(-(GB + 1) // self.kept_m) + 1
        assert self.T * self.kept_m > GB and (self.T - 2) * self.kept_m <= GB
        mv, P = self.cam["gs_mv"].astype(np.float32), self.cam["gs_proj"].astype(np.float32)
        self.col, self.row = np.full(self.m, -1, np.int64), np.full(self.m, -1, np.int64)
        self.zwin = np.full(self.m, np.nan, np.float32)
        for i in order:
            o = oracle.project(cs, cc, int(i), mv, P, self.cam["focal"], W, H)
            if o.visible and np.isfinite(o.cx) and np.isfinite(o.cy):
                col, row = int(np.floor(o.cx)), H - 1 - int(np.floor(o.cy))
                if 0 <= col < W and 0 <= row < H:
                    self.col[i], self.row[i] = col, row
                    self.zwin[i] = np.float32(np.float32(o.zndc) * np.float32(0.5)) + np.float32(0.5)   # what k_project writes to zwin
        self.in_order = np.zeros(self.m, bool); self.in_order[order] = True
        self.on = np.flatnonzero(self.col >= 0)
        assert self.on.size > 200

    def context(self):
        c = capi.Context(0)
        for _ in range(self.T):
            c.push_splat(self.rows)
        c.set_state(0, np.tile(self.hid.astype(np.uint8), self.T))
        got = c.sort(self.cam["view"])                                  # the claim the tiling rests on: every copy of a row shares its fate
        assert got.size == self.T * self.kept_m > GB
        assert np.array_equal(np.bincount(got % self.m, minlength=self.m), np.where(self.in_order, self.T, 0))
        return c

    def check(self, c, select, want_m, tag):
        """want_m: the splats of the m rows the rule takes; with and without INVERT: T times the hits, the tiled store"""
        assert 0 < want_m.sum() < self.in_order.sum() and not (want_m & ~self.in_order).any(), tag
        for inv in (0, INVERT):
            w = (self.in_order & ~want_m) if inv else want_m
            c.set_state(0, np.tile(self.hid.astype(np.uint8), self.T))
            c.sort(self.cam["view"], want_indices=False)
            assert select(inv) == self.T * int(w.sum()), (tag, inv)
            assert np.array_equal(c.download_state(), np.tile(self.hid.astype(np.uint8) | np.where(w, SELECTED, 0).astype(np.uint8), self.T)), (tag, inv)


@functools.lru_cache(maxsize=None)
def tiled():
    return Tiled()


def test_select_rect_grid_stride():
    t = tiled()
    with t.context() as c:
        for rect in ((0, 0, W, H), (W // 4, H // 4, 3 * W // 4, 3 * H // 4)):
            x0, y0, x1, y1 = rect
            want = t.in_order & (t.col >= x0) & (t.col < x1) & (t.row >= y0) & (t.row < y1)
            if rect != (0, 0, W, H):
                assert want.sum() < (t.in_order & (t.col >= 0)).sum()
            t.check(c, lambda inv: c.select_rect(t.p, rect, set_bits=SELECTED, flags=inv), want, rect)


def test_select_mask_grid_stride():
    t = tiled()
    mask = np.full((H, W), 255, np.uint8)
    mask[H // 3:2 * H // 3, W // 3:2 * W // 3] = 0                     # a hole
    seen = t.in_order & (t.col >= 0)
    med = np.sort(t.zwin[seen])[seen.sum() // 2]
    plane = np.full((H, W), med, np.float32)
    on = t.on
    in_mask = np.zeros(t.m, bool); in_mask[on] = mask[t.row[on], t.col[on]] != 0
    near = np.zeros(t.m, bool); near[on] = t.zwin[on] <= plane[t.row[on], t.col[on]]
    assert (seen & ~in_mask).any() and (seen & in_mask & ~near).any() and (seen & in_mask & near).any()
    with t.context() as c:
        t.check(c, lambda inv: c.select_mask(t.p, mask, None, set_bits=SELECTED, flags=inv), t.in_order & in_mask, "hole")
        t.check(c, lambda inv: c.select_mask(t.p, mask, plane, set_bits=SELECTED, flags=inv), t.in_order & in_mask & near, "hole_and_plane")


# ---------------------------------------------------------------- 4. the predicates on their boundaries

def hand_rows(pos):
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    n = len(pos)
    rows = np.zeros((n, 32), np.uint8)
    rows[:, 0:12] = pos.astype("<f4").view(np.uint8).reshape(n, 12)
    rows[:, 12:24] = np.full((n, 3), 0.01, "<f4").view(np.uint8).reshape(n, 12)
    rows[:, 24:28] = 255
    rows[:, 28:32] = (255, 128, 128, 128)
    return rows, pos


def up(x):
    """one float32 ulp away from zero"""
    x = np.float32(x)
    return np.nextafter(x, np.float32(np.inf if x > 0 else -np.inf), dtype=np.float32)


def down(x):
    """one float32 ulp towards zero"""
    return np.nextafter(np.float32(x), np.float32(0.0), dtype=np.float32)


def sphere_mirror(pos, centre, radius):
    """the header's rule in f64, operation by operation (test_edit_gpu.test_select_sphere's expression)"""
    with np.errstate(all="ignore"):
        d = pos.astype(np.float64) - np.asarray(centre, np.float32).astype(np.float64)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        return d2 <= float(np.float32(radius)) * float(np.float32(radius))


def test_sphere_on_its_boundary():
    r = np.float32(1.7)
    s = np.float32(0.25)
    on, outside, inner = [], [], []
    for axis in range(3):
        for sign in (1.0, -1.0):
            for lst, v in ((on, r), (outside, up(r)), (inner, down(r))):
                p = np.zeros(3, np.float32); p[axis] = np.float32(sign) * v
                lst.append(p)
    pyth = [np.array([3 * s, 4 * s, 0], np.float32), np.array([up(3 * s), 4 * s, 0], np.float32), np.array([3 * s, down(4 * s), 0], np.float32)]
    odd = [np.array(v, np.float32) for v in ((np.nan, 0, 0), (0, np.nan, 0), (0, 0, np.nan), (np.inf, 0, 0), (0, -np.inf, 0), (0, 0, np.inf), (np.inf, np.nan, 0))]
    zz = [np.array([0, 0, 1.25], np.float32), np.array([0, 0, -1.25], np.float32)]
    groups = {"on": on, "outside": outside, "inner": inner, "pyth": pyth, "odd": odd, "zz": zz}
    idx, at = {}, 0
    for k, v in groups.items():
        idx[k] = np.arange(at, at + len(v)); at += len(v)
    rows, pos = hand_rows(np.concatenate([np.stack(v) for v in groups.values()]))
    n = len(pos)
    finite = np.isfinite(pos).all(axis=1)
    zero = np.zeros(3, np.float32)
    cases = []
    for radius in (r, -r):                                              # the rule is on radius * radius: -r selects like r
        m = sphere_mirror(pos, zero, radius)
        assert m[idx["on"]].all() and not m[idx["outside"]].any() and m[idx["inner"]].all() and not m[idx["odd"]].any()
        cases.append(("r=%g" % radius, zero, radius, m))
    assert np.array_equal(cases[0][3], cases[1][3])
    m = sphere_mirror(pos, zero, 5 * s)
    assert float(3 * s) ** 2 + float(4 * s) ** 2 == float(5 * s) ** 2 and list(m[idx["pyth"]]) == [True, False, True]
    cases.append(("pythagorean", zero, 5 * s, m))
    m = sphere_mirror(pos, zero, np.inf)                                 # (+-inf positions: inf <= inf -- whatever the mirror says)
    assert m[finite].all() and not m[np.isnan(pos).any(axis=1)].any()
    cases.append(("inf", zero, np.float32(np.inf), m))
    m = sphere_mirror(pos, zero, np.nan)
    assert not m.any()
    cases.append(("nan", zero, np.float32(np.nan), m))
    off = np.array([0, 0, 0.5], np.float32)                             # the packed centre stores -z: a lost sign swaps these two
    m = sphere_mirror(pos, off, 1.0)
    assert list(m[idx["zz"]]) == [True, False] and list(sphere_mirror(pos * np.float32([1, 1, -1]), off, 1.0)[idx["zz"]]) == [False, True]
    cases.append(("off_centre_z", off, 1.0, m))
    with capi.Context(0) as c:
        c.push_splat(rows)
        for name, centre, radius, inside in cases:
            for inv in (0, INVERT):
                w = ~inside if inv else inside
                c.set_state(0, np.full(n, 8, np.uint8))
                assert c.select_sphere(centre, radius, set_bits=SELECTED, flags=inv) == w.sum(), (name, inv)
                assert np.array_equal(c.download_state(), np.where(w, 8 | SELECTED, 8).astype(np.uint8)), (name, inv)


def test_box_on_its_boundary():
    """powers of two in the matrices: every product and sum of the mirror is exact, so on / one ulp off the face is decided by the input"""
    aff = np.zeros(16, np.float32); aff[0] = aff[5] = aff[10] = 0.5; aff[12], aff[13], aff[14], aff[15] = 0.25, -0.125, 0.0, 1.0
    # affine: q0 = x / 2 + 1/4, q1 = -y / 2 - 1/8, q2 = z / 2: the faces at x = 1/2, -3/2; y = -5/4, 3/4; z = 1, -1
    faces = [(0, 0.5), (0, -1.5), (1, -1.25), (1, 0.75), (2, 1.0), (2, -1.0)]
    centre = np.array([-0.5, -0.25, 0.0], np.float32)
    rows, expect = [], []
    for axis, f in faces:
        away = np.float32(f) > centre[axis]
        step_out = np.nextafter(np.float32(f), np.float32(np.inf if away else -np.inf), dtype=np.float32)
        step_in = np.nextafter(np.float32(f), np.float32(-np.inf if away else np.inf), dtype=np.float32)
        for v, e in ((np.float32(f), True), (step_out, False), (step_in, True)):
            p = centre.copy(); p[axis] = v
            rows.append(p); expect.append(e)
    rows4 = np.zeros((len(rows), 4), np.float32); rows4[:, :3] = np.stack(rows); rows4[:, 3] = 100.0
    expect = np.array(expect)
    m_aff = box_mirror(rows4, aff)
    assert np.array_equal(m_aff, expect) and expect.sum() == 12
    # perspective: w = 1 / (z / 4 + 1); at z = 4: w = 1/2, at z = -2: w = 2, at z = -4: 1 / 0
    per = np.zeros(16, np.float32); per[0] = per[5] = 0.5; per[11] = 0.25; per[15] = 1.0       # (q2 = 0: the box ignores z)
    prow, pexp = [], []
    for z, xf in ((4.0, 2.0), (-2.0, 0.5)):                             # q0 = x / 2 * w = 1/2 exactly at x = xf
        for v, e in ((xf, True), (up(xf), False), (down(xf), True), (-xf, True), (up(-xf), False)):
            prow.append((v, 0.0, z)); pexp.append(e)
    prow += [(1.0, 0.0, -4.0), (0.0, 0.0, -4.0), (-1.0, 0.0, -4.0)]      # w = inf: +-inf outside; 0 * inf = NaN compares false: inside
    prows4 = np.zeros((len(prow), 4), np.float32); prows4[:, :3] = np.array(prow, np.float32); prows4[:, 3] = 100.0
    m_per = box_mirror(prows4, per)
    assert np.array_equal(m_per[:len(pexp)], np.array(pexp)) and list(m_per[-3:]) == [False, True, False]
    assert (0.25 * prows4[-3:, 2].astype(np.float64) + 1.0 == 0.0).all()
    for r4, box, inside, name in ((rows4, aff, m_aff, "affine"), (prows4, per, m_per, "perspective")):
        n = len(r4)
        with sort_ctx(r4) as c:
            for inv in (0, INVERT):
                w = ~inside if inv else inside
                c.set_state(0, np.full(n, 8, np.uint8))
                assert c.select_box(box, set_bits=SELECTED, flags=inv) == w.sum(), (name, inv)
                assert np.array_equal(c.download_state(), np.where(w, 8 | SELECTED, 8).astype(np.uint8)), (name, inv)
