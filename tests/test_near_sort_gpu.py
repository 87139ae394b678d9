"""GPU tier: every near-only form of the depth sort (csrc/gs_sort.hip, csrc/gs_prims.hip) against the WHOLE order, position for position.

A near-only sort promises that the positions a frame reads hold exactly what the whole order holds there.  GS_OPT_SORT_NEAR_FORCE asks
for a chosen number of positions, gs_sort_inspect shows the lane's records as they lie, and every case asserts ONE thing, with W the
whole order (oracle.sort), V its length, V' its valid length (W[V':] is the zero tail) and P = info.n_records:

    P >= min(req, V');  the P records == W[V' - P : V'] bit for bit;  n_valid == V';  n_kept == V;  order_incomplete == 0 (but in the
    three constructed cases: a stash of 513, a candidate stash of 129, a hint that is behind);  info.form is the form the case was built for.

Forms and how they are reached (run_sort chooses as always):
    tail       n <= GS_MSD_MAX_N in this process: k_msd_scatter cuts at a segment boundary.  Buckets are chosen (rows_of of
               test_sort_paths_gpu), so the cut segment is known and P must equal the constructed suffix sum EXACTLY -- the one check that
               sees a cut a segment early.
    histogram  GS_MSD_MAX_N < n <= GS_RADIX_LARGE_N here, short inputs in a GS_SORT_MSD=0 child (tests/sort_jobs.py); long inputs with
               req > n / 32.  The numpy mirror of depth_bin (sign-less f32 bits >> 20) gives the threshold bin T, which must be
               info.threshold_bin; P is at most the kept splats in bins <= T + 1 where bins are wider than buckets.
    stash      n = 3 * 2^20 + 4097, req <= n / 32: survivors per 4096-item chunk are placed by index (0, 1, 511, 512, spread, the last
               partial chunk); 513 overflows.
    spec       the sort after a collected one: candidates per 1024-item chunk (kept splats in bins <= hint + GS_SPEC_PAD) at 128 and 129;
               a view whose threshold bin is more than GS_SPEC_PAD bins past the hint.
The long cloud is built once: three independent depth layouts on its x, y and z columns, chosen by the view row.

Not covered here: the paired depth pass (k_sort_depth_pair<..>: two views with a histogram each) and the shared sort's no_tail_sort lane -- reached only through
queued pairs and several contexts, they stay with the 6 M-splat frame tests of test_gpu_parity.py.  The gather's workgroups take one group
of GS_GATHER_CHUNKS chunks each at this size (a workgroup takes several only beyond 33 M splats); the spread survivors cross every seam
between groups.  Frames after a forced sort: the tail form at 4096 splats, and the stash form's overflow at the long cloud; the histogram
form of 4096 splats exists only under GS_SORT_MSD=0 and is pinned by its records in the child.

Budget, as measured on one MI355X: 2.2 .. 2.3 s of wall time for the module's 15 tests; the GS_SORT_MSD=0 child (9 jobs) 0.64 s, the long
cloud's setup 0.35 s, every other test under 0.25 s (docs/LAB_NOTES.md section 9g, with the mutations tried)."""
import time

import numpy as np
import pytest

import sort_jobs
import test_sort_paths_gpu as sp
from conftest import pkg
from oracle import oracle
from sort_jobs import decode, splat_rows
from test_sort_paths_gpu import (CHUNK_L, LARGE_N, MSD_MAX_N, SEG_B, SEG_MAXBLK, VIEW, VIEW_DROP, _constant, dropped_case, population, rows_of,
                                 run_child, run_here)

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

DEPTH_BINS = _constant("GS_DEPTH_BINS", "gs_internal.h")
NEAR_STASH = _constant("GS_NEAR_STASH", "gs_internal.h")
SPEC_SLOT = _constant("GS_SPEC_SLOT", "gs_sort.hip")
SPEC_PAD = _constant("GS_SPEC_PAD", "gs_sort.hip")
DEPTH_IPT = _constant("GS_DEPTH_IPT", "gs_sort.hip")
BLOCK = _constant("GS_BLOCK", "gs_internal.h", "gs_prims.hip", "gs_sort.hip")
SPEC_CHUNK = DEPTH_IPT * BLOCK
assert (DEPTH_BINS, NEAR_STASH, SPEC_SLOT, SPEC_PAD, SPEC_CHUNK, CHUNK_L) == (2048, 512, 128, 2, 1024, 4096), "the long cloud is laid out for these"
WHOLE, HIST, SPEC, TAIL, STASH = capi.SORT_WHOLE, capi.SORT_HISTOGRAM, capi.SORT_SPEC, capi.SORT_TAIL, capi.SORT_STASH
FORCE = capi.OPT_SORT_NEAR_FORCE


# ---------------------------------------------------------------- the mirror and the one assertion

def mirror(rows4, view, inside=None):
    """-> (kept mask, depth bin of every row): index.js:517-555 in f64, left to right; the stored depth is its f32 rounding"""
    v = np.asarray(view, np.float32).astype(np.float64)
    x, y, z, s = (rows4[:, k].astype(np.float64) for k in range(4))
    with np.errstate(all="ignore"):
        d = ((v[0] * x + v[1] * y) + v[2] * z) + v[3]
        keep = (d < 0) & (s > -0.0001 * d)
        f = d.astype(np.float32)
    if inside is not None:
        keep &= inside
    return keep, (f.view(np.uint32) & 0x7FFFFFFF) >> 20


def threshold_bin(bins, keep, req):
    """the first bin T with (kept splats in bins <= T) >= req; the last bin when there are fewer -> (T, cumulative counts)"""
    cum = np.cumsum(np.bincount(bins[keep], minlength=DEPTH_BINS))
    t = int(np.searchsorted(cum, req))
    return min(t, DEPTH_BINS - 1), cum


def near_bad(tag, words, W, Vp, req, form, P=None, incomplete=False, bound=None):
    """the one assertion -> a list of sentences (empty: the case holds)"""
    info, rec = decode(words) if not isinstance(words, tuple) else words
    bad = []
    p = info["n_records"]
    if info["form"] != form:
        bad.append("%s: form %d, built for %d" % (tag, info["form"], form))
    if form == WHOLE:
        d = sp.differs(tag, rec, W)
        return bad + ([d] if d else [])
    if info["near_req"] != req:
        bad.append("%s: near_req %d, asked %d" % (tag, info["near_req"], req))
    if info["n_valid"] != Vp or info["n_kept"] != W.size:
        bad.append("%s: n_valid %d n_kept %d, not V' %d V %d" % (tag, info["n_valid"], info["n_kept"], Vp, W.size))
    if (p < min(req, Vp) and not incomplete) or p > Vp:
        bad.append("%s: P = %d for req %d, V' %d" % (tag, p, req, Vp))
    if P is not None and p != P:
        bad.append("%s: P = %d, constructed %d (req %d)" % (tag, p, P, req))
    if bound is not None and p > bound:
        bad.append("%s: P = %d, more than the %d kept splats up to the bin behind the threshold's" % (tag, p, bound))
    if incomplete:
        if not info["order_incomplete"]:
            bad.append("%s: order_incomplete is 0" % tag)
    else:
        if info["order_incomplete"] or info["near_overflow"] or info["spec_fail"]:
            bad.append("%s: flagged: %r" % (tag, info))
        if p <= Vp:
            d = sp.differs(tag, rec, W[Vp - p:Vp])
            if d:
                bad.append(d)
    return bad


def near_steps(reqs, view, cut, name):
    s = []
    for r in reqs:
        s += [["opt", FORCE, int(r)], ["near", view, cut, "%s.r%d" % (name, r)]]
    return s


def rows_bad(tag, words, rows4):
    return [] if np.array_equal(words, np.ascontiguousarray(rows4, np.float32).view(np.uint32).reshape(-1)) else ["%s: the resident sort rows are not the rows"
                                                                                                                 " the case was built from" % tag]


# ---------------------------------------------------------------- 1. the tail form

def buckets_of(g, n, pops):
    """n buckets with pops[segment] records in each named segment (high bucket byte), random low bytes, the anchors 0 and 65535, shuffled"""
    assert sum(pops.values()) == n and pops.get(0, 0) >= 1 and pops.get(255, 0) >= 1
    b = np.concatenate([(d << 8) | g.integers(0, 256, c) for d, c in sorted(pops.items())])
    b[0], b[-1] = 0, 65535
    b = g.permutation(b)
    pop = population(b)
    assert all(pop[d] == c for d, c in pops.items()) and pop.sum() == n, "the segments do not hold what the case names"
    return b


def tail_P(pop, req):
    """records a tail sort keeps: from the start of the non-empty segment that holds position V' - req; everything for req >= V'"""
    Vp = int(pop.sum())
    if req >= Vp:
        return Vp
    suf = np.cumsum(pop[::-1])[::-1]
    return int(suf[max(d for d in range(256) if pop[d] and suf[d] >= req)])


def tail_reqs(pop, n, segs):
    Vp, suf = int(pop.sum()), np.cumsum(pop[::-1])[::-1]
    r = {1, Vp - 1, Vp, Vp + 1, n + 7}
    for d in segs:
        assert pop[d] > 0
        r |= {int(suf[d]) - 1, int(suf[d]), int(suf[d]) + 1}
    return sorted(x for x in r if x >= 1)


TAIL_POPS = {
    2: ({0: 1, 255: 1}, (255,)),                                                  # a cut at segment 255
    257: ({0: 1, 3: 40, 6: 100, 200: 50, 255: 66}, (3, 6, 200, 255)),            # empty segments on both sides of every cut
    2049: ({0: 1, 2: 500, 9: 700, 0x55: 600, 0xFE: 247, 255: 1}, (2, 0x55, 0xFE, 255)),
    # the cut segment in k_seg_sort's one-item tier (more than GS_SEG_B x GS_SEG_MAXBLK records) and one block below it (GS_SEG_MAXBLK blocks)
    70001: ({0: 1000, 0x40: SEG_B * SEG_MAXBLK + 1, 0x80: SEG_B * SEG_MAXBLK, 0xC0: 2000, 255: 70001 - 3001 - 2 * SEG_B * SEG_MAXBLK}, (0x40, 0x80, 0xC0, 255)),
}


@pytest.mark.parametrize("n", [1, 2, 257, 2049, 70001])
def test_tail_cut_at_every_request_edge(n):
    """req in {1, S - 1, S, S + 1, V' - 1, V', V' + 1, n + 7} for the suffix sum S at chosen non-empty segments: P is the constructed
    suffix sum exactly.  n = 1 and the all-in-one-segment cloud (equal depths: bucket 0) have no cut: P = V'.  The same context then
    sorts whole (the policy's choice on a fresh context) and forced again."""
    g = np.random.Generator(np.random.PCG64(100 + n))
    cases = []
    if n == 1:
        rows = np.array([[0, 0, -5, 100]], np.float32)
        cases.append(("single", rows, np.bincount([0], minlength=256), (0,)))
    else:
        pops, segs = TAIL_POPS[n]
        b = buckets_of(g, n, pops)
        cases.append(("chosen", rows_of(b), population(b), segs))
    if n == 257:
        rows = np.zeros((n, 4), np.float32)
        rows[:, 2], rows[:, 3] = -5.0, 100.0
        cases.append(("one_segment", rows, np.bincount([0], weights=[n], minlength=256).astype(np.int64), (0,)))
    bad = []
    for name, rows, pop, segs in cases:
        W = oracle.sort(rows, VIEW)
        assert W.size == n == pop.sum()
        if name == "chosen":
            assert np.array_equal(W, sp.definition(sp.rows_of_bucket(sp.Case(name, rows, W))))
        else:
            assert np.array_equal(W, np.arange(n, dtype=np.uint32))
        reqs = tail_reqs(pop, n, segs)
        mid = reqs[len(reqs) // 2]
        steps = [["splat", rows], ["rows", "rows"]] + near_steps(reqs, VIEW, None, name) + [["opt", FORCE, 0], ["near", VIEW, None, "whole"]] + \
            near_steps([mid], VIEW, None, name + ".again")
        got = run_here(steps)
        bad += rows_bad(name, got["rows"], rows)
        for r in reqs:
            bad += near_bad("%s n=%d req=%d" % (name, n, r), got["%s.r%d" % (name, r)], W, n, r, TAIL, P=tail_P(pop, r))
        bad += near_bad("%s n=%d whole" % (name, n), got["whole"], W, n, 0, WHOLE)
        bad += near_bad("%s n=%d again req=%d" % (name, n, mid), got["%s.again.r%d" % (name, mid)], W, n, mid, TAIL, P=tail_P(pop, mid))
    assert not bad, "\n".join(bad[:40])


def cutout_x():
    """keeps x in [-0.5, 0.5] (and every z the constructed rows use); affine"""
    c = np.zeros(16, np.float32)
    c[0] = c[5] = c[15] = 1.0
    c[10] = 2.0 ** -18
    return c


def test_tail_with_dropped_buckets_a_cutout_and_hidden_splats():
    """Dropped buckets (the recipe of test_sort_paths_gpu: x in [-0.999, 0.999], 5 .. 50 % of V dropped): V' < V, the records end at V'.
    A cutout that culls a third of a chosen cloud and hidden splats (gs_set_state) in another third, the anchors kept: the buckets stay
    as chosen, the populations are those of the kept splats."""
    bad = []
    case, Vp = dropped_case(2049)
    W = case.want
    reqs = [1, Vp // 3, Vp - 1, Vp, Vp + 1, W.size, W.size + 9]
    got = run_here([["splat", case.rows], ["rows", "rows"]] + near_steps(reqs, VIEW_DROP, None, "drop"))
    bad += rows_bad("dropped", got["rows"], case.rows)
    for r in reqs:
        bad += near_bad("dropped req=%d" % r, got["drop.r%d" % r], W, Vp, r, TAIL)
    g = np.random.Generator(np.random.PCG64(9))
    n = 6001
    b = buckets_of(g, n, {0: 1, 7: 1500, 0x30: 1500, 0x90: 1500, 0xD0: 1499, 255: 1})
    rows = rows_of(b)
    anchors = (b == 0) | (b == 65535)
    third = g.permutation(n)
    out_cut = np.zeros(n, bool); out_cut[third[:2000]] = True; out_cut &= ~anchors
    hidden = np.zeros(n, bool); hidden[third[2000:4000]] = True; hidden &= ~anchors
    rows[out_cut, 0] = 1.0
    for name, gone, cut in (("cutout", out_cut, cutout_x()), ("hidden", hidden, None), ("both", out_cut | hidden, cutout_x())):
        ref = rows.copy()
        ref[gone, 3] = 0.0                                           # (size 0 is culled: the same kept set, the same min / max)
        W = oracle.sort(ref, VIEW)
        kept = np.flatnonzero(~gone)
        assert W.size == kept.size < n - 1500 and np.array_equal(W, kept[np.argsort(b[kept].astype(np.uint16), kind="stable")].astype(np.uint32)), name
        if cut is not None and name == "cutout":
            assert np.array_equal(oracle.sort(rows, VIEW, cut), W), "the cutout does not cull what the case says"
        pop = population(b[kept])
        reqs = tail_reqs(pop, n, (0x30, 0x90, 255))
        steps = [["splat", rows]]
        if name != "cutout":
            steps += [["state", 0, (hidden * capi.STATE_HIDDEN).astype(np.uint8)]]
        got = run_here(steps + near_steps(reqs, VIEW, cut, name))
        for r in reqs:
            bad += near_bad("%s req=%d" % (name, r), got["%s.r%d" % (name, r)], W, W.size, r, TAIL, P=tail_P(pop, r))
    assert not bad, "\n".join(bad[:40])


# ---------------------------------------------------------------- 2. the histogram form

FAR_BIN = (127 + 12) * 8                                 # from |depth| = 2^12 on a bin (12 % of the depth) is wider than 30 buckets of the spread cloud


def spread_rows(g, n):
    """|depth| = 2^e, e uniform over 40 binades: ~320 populated bins in 10 coarse bins; a splat on either side of a coarse-bin edge"""
    z = -np.exp2(g.uniform(-20.0, 20.0, n))
    if n >= 4:
        z[:4] = [-(2.0 ** 12) * 1.9375, -(2.0 ** 12) * 1.97, -(2.0 ** 13) * 1.01, -(2.0 ** 13) * 1.06]    # bins 1119, 1119, 1120, 1120
    rows = np.zeros((n, 4), np.float32)
    rows[:, 2], rows[:, 3] = z, 200.0
    return rows


def hist_requests(rows, view=VIEW):
    """-> (requests, {req: (T, bound)}): C - 1, C, C + 1 for the cumulative count C at a fine-bin edge, a coarse-bin edge (bin 32 k - 1)
    and the last populated bin -- all where bins are wider than buckets, so that P <= kept splats in bins <= T + 1 -- and req > V"""
    keep, bins = mirror(rows, view)
    V = int(keep.sum())
    _, cum = threshold_bin(bins, keep, 1)
    pop = np.flatnonzero(np.diff(np.concatenate([[0], cum])))
    edges = [int(pop[-1])]
    fine = [t for t in pop if t >= FAR_BIN and t % 32 not in (0, 31)]
    coarse = [t for t in pop if t >= FAR_BIN and t % 32 == 31]
    if rows.shape[0] >= 2049:
        assert fine and coarse and 1120 in pop, "the spread cloud lacks an edge"
    edges += fine[:1] + coarse[:1]
    reqs = {V + 5}
    for t in edges:
        reqs |= {int(cum[t]) - 1, int(cum[t]), int(cum[t]) + 1}
    out = {}
    for r in sorted(x for x in reqs if x >= 1):
        T, _ = threshold_bin(bins, keep, r)
        out[r] = (T, int(cum[min(T + 1, DEPTH_BINS - 1)]) if (T >= FAR_BIN or T == DEPTH_BINS - 1) else None)
    return out


def hist_bad(tag, got, name, W, Vp, want):
    bad = []
    for r, (T, bound) in want.items():
        words = got["%s.r%d" % (name, r)]
        bad += near_bad("%s req=%d" % (tag, r), words, W, Vp, r, HIST, bound=bound)
        if decode(words)[0]["threshold_bin"] != T:
            bad.append("%s req=%d: threshold bin %d, the mirror's %d" % (tag, r, decode(words)[0]["threshold_bin"], T))
    return bad


def test_histogram_short_geometry_in_process():
    """n = GS_MSD_MAX_N + 1: the smallest input whose near-only sort is the histogram form without the environment switch."""
    n = MSD_MAX_N + 1
    rows = spread_rows(np.random.Generator(np.random.PCG64(41)), n)
    W = oracle.sort(rows, VIEW)
    assert W.size == n
    want = hist_requests(rows)
    got = run_here([["splat", rows]] + near_steps(want, VIEW, None, "spread"))
    bad = hist_bad("spread n=%d" % n, got, "spread", W, n, want)
    assert not bad, "\n".join(bad[:40])


def degenerate_cases():
    """-> [(name, rows4, view, requests)]: inputs whose bucket scale or threshold edge is degenerate; the one assertion and the bin only"""
    n = 2049
    g = np.random.Generator(np.random.PCG64(43))
    base = np.zeros((n, 4), np.float32)
    base[:, 2], base[:, 3] = -np.exp2(g.uniform(0.0, 8.0, n)), 1.0e36
    equal = base.copy(); equal[:, 2] = -7.0                          # max == min: the scale is infinite, every bucket is 0: keep all
    inf = base.copy(); inf[5, 2] = -3.0e38                           # view row z = 2: the stored depth is -inf (bin 2040; its far edge is no number)
    ends = base.copy(); ends[7, 2] = -1.0e-40; ends[9, 2] = -3.4e38  # bins 0 and 2039
    nan = base.copy(); nan[::3, 2] = np.nan                          # culled
    k, b = mirror(ends, VIEW)
    assert k.all() and b[7] == 0 and b[9] == 2039
    k, b = mirror(inf, np.array([0, 0, 2, 0], np.float32))
    assert k.all() and b[5] == 2040
    k, _ = mirror(nan, VIEW)
    assert k.sum() == n - len(range(0, n, 3))
    return [("equal", equal, VIEW, (1, n - 1, n, n + 3)), ("stored_inf", inf, np.array([0, 0, 2, 0], np.float32), (1, 700, n - 1, n, n + 3)),
            ("both_ends", ends, VIEW, (1, 2, 700, n - 1, n, n + 3)), ("nan", nan, VIEW, (1, 500, int(k.sum()), n))]


def test_histogram_short_inputs_and_degenerate_depths(tmp_path):
    """n in {1, 65, 2049, 30 011} with the LSD passes (a GS_SORT_MSD=0 child): the spread cloud at its bin edges; all depths equal, a
    stored depth of -inf, depths in bins 0 and 2039, NaN depths (culled), and dropped buckets (index 0 culled: a zero is a tail slot)."""
    jobs, checks = [], []
    for n in (1, 65, 2049, 30011):
        rows = spread_rows(np.random.Generator(np.random.PCG64(50 + n)), n)
        W = oracle.sort(rows, VIEW)
        assert W.size == n
        want = hist_requests(rows)
        name = "spread%d" % n
        jobs.append([["splat", rows]] + near_steps(want, VIEW, None, name))
        checks.append((name, W, n, want))
    for name, rows, view, reqs in degenerate_cases():
        W = oracle.sort(rows, view)
        keep, bins = mirror(rows, view)
        assert W.size == keep.sum() and np.array_equal(np.sort(W), np.flatnonzero(keep))
        want = {r: (threshold_bin(bins, keep, r)[0], None) for r in reqs}
        jobs.append([["splat", rows]] + near_steps(want, view, None, name))
        checks.append((name, W, W.size, want))
    case, Vp = dropped_case(2049)
    keep, bins = mirror(case.rows, VIEW_DROP)
    assert keep.sum() == case.want.size
    want = {r: (threshold_bin(bins, keep, r)[0], None) for r in (1, Vp // 2, Vp, case.want.size, case.want.size + 3)}
    jobs.append([["splat", case.rows]] + near_steps(want, VIEW_DROP, None, "dropped"))
    checks.append(("dropped", case.want, Vp, want))
    got = run_child(jobs, tmp_path)
    bad = []
    for name, W, Vp, want in checks:
        bad += hist_bad(name, got, name, W, Vp, want)
    assert not bad, "\n".join(bad[:40])


# ---------------------------------------------------------------- 3. the long cloud: histogram (long geometry), stash, spec

N_LONG = LARGE_N + CHUNK_L + 1
G_LO, G_HI, E_LO, E_HI = 1.01, 1.05, 1.27, 1.30          # the near cluster G (bin 1016 = [1, 1.125)) and the candidates E (bin 1018 = [1.25, 1.375))
BIN_G = 127 * 8
VIEWS = {"x": (1.0, 0, 0, 0), "y": (0, 1.0, 0, 0), "z": (0, 0, 1.0, 0)}


class LongCloud:
    """N_LONG rows whose x, y and z columns are three depth layouts (view rows (1,0,0,0), (0,1,0,0), (0,0,1,0), or multiples):
    a background at |depth| in [1000, 2000) and, placed by index, the near cluster G and the candidates E.
      z  stash: G per 4096-item chunk 512, 511, 1, 0 .. and 40 in each of the chunks 10 .. 700, and the last (one-item) chunk;
         spec:  per 1024-item chunk that is 128 four times, 128 128 128 127, and 1 + 127 of E: candidates at GS_SPEC_SLOT, never beyond
      y  spec:  one 1024-item chunk with 100 of G and 29 of E (129 candidates); G 8 in each of the chunks 100 .. 300
      x  stash: one 4096-item chunk with 513 of G; 5 in each of the chunks 100 .. 300"""

    def __init__(self):
        t0 = time.perf_counter()
        g = np.random.Generator(np.random.PCG64(31))
        n = N_LONG
        self.rows = np.zeros((n, 4), np.float32)
        self.rows[:, :3] = -(1000.0 + 1000.0 * g.random((n, 3), np.float32))
        self.rows[:, 3] = 0.5
        used = np.zeros((3, n), bool)

        def place(axis, start, length, count, lo, hi):
            free = start + np.flatnonzero(~used[axis, start:start + length])
            at = g.choice(free, count, replace=False)
            used[axis, at] = True
            self.rows[at, axis] = -g.uniform(lo, hi, count)

        for sub, cnt in enumerate([128] * 7 + [127]):
            place(2, sub * 1024, 1024, cnt, G_LO, G_HI)
        place(2, 8 * 1024, 1024, 1, G_LO, G_HI)
        place(2, 8 * 1024, 1024, 127, E_LO, E_HI)
        for c in range(10, 701):
            for sub in range(4):
                place(2, c * 4096 + sub * 1024, 1024, 10, G_LO, G_HI)
        place(2, n - 1, 1, 1, G_LO, G_HI)
        place(1, 20 * 1024, 1024, 100, G_LO, G_HI)
        place(1, 20 * 1024, 1024, 29, E_LO, E_HI)
        for c in range(100, 301):
            place(1, c * 4096, 4096, 8, G_LO, G_HI)
        place(0, 5 * 4096, 4096, 513, G_LO, G_HI)
        for c in range(100, 301):
            place(0, c * 4096, 4096, 5, G_LO, G_HI)
        self.records = splat_rows(self.rows)
        self.refs = {}
        print("long cloud: %.2f s" % (time.perf_counter() - t0))

    def view(self, axis, scale=1.0):
        return (np.array(VIEWS[axis], np.float32) * np.float32(scale)).astype(np.float32)

    def ref(self, axis, scale=1.0, n=N_LONG):
        """-> (W, G mask, kept mask, bins) of the first n rows under the layout's view row times scale"""
        key = (axis, scale, n)
        if key not in self.refs:
            v = self.view(axis, scale)
            W = oracle.sort(self.rows[:n], v)
            keep, bins = mirror(self.rows[:n], v)
            assert W.size == n and keep.all(), "a splat of the long cloud is culled"
            G = np.abs(self.rows[:n, "xyz".index(axis)]) < 1.2
            self.refs[key] = (W, G, keep, bins)
        return self.refs[key]

    def counts(self, axis, scale, chunk, upto_bin):
        """kept splats in bins <= upto_bin per `chunk` consecutive rows"""
        _, _, keep, bins = self.ref(axis, scale)
        sel = keep & (bins <= upto_bin)
        return np.add.reduceat(sel.astype(np.int64), np.arange(0, N_LONG, chunk))

    def context(self, n=N_LONG):
        c = capi.Context(0)
        for o in range(0, n, sort_jobs.PUSH_ROWS):
            c.push_splat(self.records[o:min(o + sort_jobs.PUSH_ROWS, n)])
        return c


@pytest.fixture(scope="module")
def cloud():
    c = LongCloud()
    # the constructions, from the rows alone
    for axis in "xyz":
        W, G, keep, bins = c.ref(axis)
        T, _ = threshold_bin(bins, keep, int(G.sum()))
        assert T == BIN_G and (bins[G] == BIN_G).all() and (bins[~G] >= BIN_G + 2).all(), axis
    z = c.counts("z", 1.0, CHUNK_L, BIN_G)
    assert list(z[:4]) == [512, 511, 1, 0] and (z[10:701] == 40).all() and z[-1] == 1 and len(z) == 770 and z.max() == NEAR_STASH
    for scale in (1.0, 1.03):
        zc = c.counts("z", scale, SPEC_CHUNK, BIN_G + SPEC_PAD)
        assert zc.max() == SPEC_SLOT == zc[8] and list(zc[:8]) == [128] * 7 + [127], scale
    assert c.counts("z", 1.0, SPEC_CHUNK, BIN_G)[8] == 1
    yc = c.counts("y", 1.0, SPEC_CHUNK, BIN_G + SPEC_PAD)
    assert yc.max() == SPEC_SLOT + 1 == yc[20] and c.counts("y", 1.0, CHUNK_L, BIN_G).max() <= NEAR_STASH
    x = c.counts("x", 1.0, CHUNK_L, BIN_G)
    assert x[5] == NEAR_STASH + 1 and np.delete(x, 5).max() == 5
    return c


def forced(c, view, req):
    c.set_option(FORCE, int(req))
    c.sort(view, want_indices=False)
    return c.sort_inspect()


def test_long_cloud_rows_are_the_rows_built(cloud):
    with cloud.context(4 * CHUNK_L) as c:
        got = c.download(capi.BUF_SORT_ROWS, 4 * CHUNK_L, np.float32, 4)
    assert np.array_equal(got.view(np.uint32), cloud.rows[:4 * CHUNK_L].view(np.uint32))


def test_histogram_long_geometry(cloud):
    """n = GS_RADIX_LARGE_N + 1 with req > n / 32: the stash is refused, the whole-length passes run with 4096-item chunks."""
    n = LARGE_N + 1
    W, G, keep, bins = cloud.ref("z", 1.0, n)
    bad = []
    with cloud.context(n) as c:
        for req in (n // 32 + 1, n // 2, n + 5):
            T, cum = threshold_bin(bins, keep, req)
            got = forced(c, cloud.view("z"), req)
            bad += near_bad("long histogram req=%d" % req, got, W, n, req, HIST, bound=int(cum[min(T + 1, DEPTH_BINS - 1)]))
            if got[0]["threshold_bin"] != T:
                bad.append("req=%d: threshold bin %d, the mirror's %d" % (req, got[0]["threshold_bin"], T))
    assert not bad, "\n".join(bad)


def test_stash_then_spec_at_their_slot_edges(cloud):
    """Layout z.  Stash: chunks with 0, 1, 511 and 512 survivors, 40 in every chunk across the gather's seams, the last one-item chunk;
    the survivors are exactly G.  Collected, the same view again takes the spec form; the next view is 3 % (a quarter of a bin) away:
    candidates per 1024-item chunk at GS_SPEC_SLOT.  Layout y then holds a chunk of GS_SPEC_SLOT + 1 candidates: spec_fail 2, incomplete
    (constructed case 2), and the context leaves the form: the next sort is a stash sort again, complete."""
    bad = []
    Wz, Gz, _, _ = cloud.ref("z")
    Wz3 = cloud.ref("z", 1.03)[0]
    Wy, Gy, _, _ = cloud.ref("y")
    gz, gy = int(Gz.sum()), int(Gy.sum())
    with cloud.context() as c:
        for req in (gz, gz - 1, 1):
            bad += near_bad("stash req=%d" % req, forced(c, cloud.view("z"), req), Wz, N_LONG, req, STASH if req == gz else SPEC, P=gz)
        bad += near_bad("spec, 3 %% away", forced(c, cloud.view("z", 1.03), gz), Wz3, N_LONG, gz, SPEC, P=gz)
        got = forced(c, cloud.view("y"), gy)
        bad += near_bad("spec, 129 candidates", got, Wy, N_LONG, gy, SPEC, incomplete=True)
        if got[0]["spec_fail"] != 2:
            bad.append("129 candidates: spec_fail %d" % got[0]["spec_fail"])
        bad += near_bad("after the candidate overflow", forced(c, cloud.view("y"), gy), Wy, N_LONG, gy, STASH, P=gy)
        c.set_option(FORCE, 0)
        c.sort(cloud.view("z"), want_indices=False)
        bad += near_bad("whole", c.sort_inspect(), Wz, N_LONG, 0, WHOLE)
    assert not bad, "\n".join(bad)


def test_spec_hint_behind(cloud):
    """A fresh context: a collected stash sort leaves the hint at G's bin; the view row times 1.5 moves the threshold four bins: more
    than GS_SPEC_PAD past the hint: spec_fail 1, incomplete (constructed case 3).  The following sort is complete and equal."""
    bad = []
    Wz, Gz, _, _ = cloud.ref("z")
    W15, _, keep, bins = cloud.ref("z", 1.5)
    gz = int(Gz.sum())
    assert threshold_bin(bins, keep, gz)[0] == BIN_G + 4 > BIN_G + SPEC_PAD
    with cloud.context() as c:
        got = forced(c, cloud.view("z"), gz)
        bad += near_bad("stash", got, Wz, N_LONG, gz, STASH, P=gz)
        if got[0]["threshold_bin"] != BIN_G:
            bad.append("hint %d" % got[0]["threshold_bin"])
        got = forced(c, cloud.view("z", 1.5), gz)
        bad += near_bad("hint behind", got, W15, N_LONG, gz, SPEC, incomplete=True)
        if got[0]["spec_fail"] != 1:
            bad.append("hint behind: spec_fail %d" % got[0]["spec_fail"])
        got = forced(c, cloud.view("z", 1.5), gz)
        bad += near_bad("after the miss", got, W15, N_LONG, gz, SPEC, P=gz)
        if got[0]["threshold_bin"] != BIN_G + 4:
            bad.append("hint after the miss %d" % got[0]["threshold_bin"])
    assert not bad, "\n".join(bad)


def small_camera():
    return synth.index_html_camera(64, 64, 30.0, capi=capi)


def params(cam):
    return capi.make_params(cam["gs_mv"], cam["gs_proj"], cam["vw"], cam["vh"], focal_=cam["focal"])


def test_stash_overflow_and_the_frame_drawn_from_it(cloud):
    """Layout x: a chunk of GS_NEAR_STASH + 1 survivors: near_overflow, incomplete (constructed case 1); after that collection the forced
    sort is the histogram form, complete and equal.  On a second context a synchronous 64 x 64 frame after the overflowing sort equals the
    frame drawn from a whole sort."""
    bad = []
    Wx, Gx, _, _ = cloud.ref("x")
    gx = int(Gx.sum())
    cam = small_camera()
    with cloud.context() as c:
        got = forced(c, cloud.view("x"), gx)
        bad += near_bad("513 survivors", got, Wx, N_LONG, gx, STASH, incomplete=True)
        if not got[0]["near_overflow"]:
            bad.append("513 survivors: near_overflow is 0")
        bad += near_bad("after the overflow", forced(c, cloud.view("x"), gx), Wx, N_LONG, gx, HIST)
        c.set_option(FORCE, 0)
        c.sort(cloud.view("x"), want_indices=False)
        bad += near_bad("whole", c.sort_inspect(), Wx, N_LONG, 0, WHOLE)
        want = c.render(params(cam))
    with cloud.context() as c:
        c.set_option(FORCE, gx)
        c.sort(cloud.view("x"), want_indices=False)
        frame = c.render(params(cam))
        if not np.array_equal(frame, want):
            bad.append("the frame after the overflowing sort differs from the whole sort's in %d bytes" % int((frame != want).sum()))
        if c.stats()["retried_frames"] < 1:
            bad.append("the frame was not drawn again")
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------- 4. frames and the option

def test_frames_after_forced_sorts_equal_the_whole_sorts():
    """64 x 64, 4096 splats: a synchronous gs_render after a forced tail sort of 1, 300, 4095 and 5000 positions equals the frame of a whole
    sort bit for bit.  The share of this fresh context is not settled, so every one of these frames finds its lane's order too short
    and sorts again in full first (ensure_sort_covers): that reaction is what is pinned here.  Frames that READ a partial order at
    j - j_base need a settled share: test_gpu_parity.test_near_only_sorts_fill_the_positions_a_frame_reads_like_whole_sorts."""
    rows = synth.make_splat_rows(4096, seed=5)
    cam = small_camera()
    with capi.Context(0) as c:
        c.push_splat(rows)
        c.set_option(capi.OPT_SORT_NEAR, 0)
        c.sort(cam["view"], want_indices=False)
        info, _ = c.sort_inspect()
        assert info["form"] == WHOLE
        want = c.render(params(cam))
        assert want[..., :3].any()
        for permille in (0, 100):                                    # the adaptive share, and a fixed one a near-only order of 500 covers
            c.set_option(capi.OPT_NEAR_PERMILLE, permille)
            for req in (1, 300, 500, 4095, 5000):
                c.set_option(FORCE, req)
                c.sort(cam["view"], want_indices=False)
                info, _ = c.sort_inspect(want_indices=False)
                assert info["form"] == TAIL and info["near_req"] == req, info
                got = c.render(params(cam))
                assert np.array_equal(got, want), "permille %d req %d: %d bytes differ" % (permille, req, int((got != want).sum()))


def test_option_values():
    """-1: GS_E_BADARG; 0 restores the policy's choice; a fresh context's lane has near_req 0; wide records and worker rows sort whole."""
    g = np.random.Generator(np.random.PCG64(3))
    b = buckets_of(g, 300, {0: 100, 9: 100, 255: 100})
    rows = rows_of(b)
    W = oracle.sort(rows, VIEW)
    with capi.Context(0) as c:
        c.push_splat(splat_rows(rows))
        with pytest.raises(capi.GsError) as e:
            c.set_option(FORCE, -1)
        assert e.value.code == capi.E_BADARG
        with pytest.raises(capi.GsError) as e:
            c.sort_inspect()
        assert e.value.code == capi.E_STATE
        c.sort(VIEW, want_indices=False)
        assert not near_bad("fresh", c.sort_inspect(), W, 300, 0, WHOLE)
        assert not near_bad("forced", forced(c, VIEW, 150), W, 300, 150, TAIL, P=200)
        assert np.array_equal(c.sort(VIEW), W)                       # (asked for the list: all of it)
        assert not near_bad("zero", forced(c, VIEW, 0), W, 300, 0, WHOLE)
        c.set_option(capi.OPT_WIDE_PAIRS, 1)
        assert not near_bad("wide", forced(c, VIEW, 150), W, 300, 0, WHOLE)
    with capi.Context(0) as c:
        c.push_matrices(sort_jobs.expand(rows))
        assert not near_bad("worker rows", forced(c, VIEW, 150), W, 300, 0, WHOLE)
