"""GPU tier: every whole-order path of the depth sort against the CPU oracle AND against the definition of the order (a stable argsort
of the bucket numbers), bit for bit, at the edges of the kernels that make the order: the block tiers of k_seg_sort, the chunk and
group rows of k_msd_scatter, the size switches of run_sort, dropped buckets and the zero tail, culls / cutouts / IEEE specials, the
state one sort leaves for the next, and the posted sort.

Paths.  gs_stats does not name a whole sort's path; a path is reached by (n, options, environment) exactly as run_sort
(csrc/gs_sort.hip) chooses it, and the edges are placed from the constants this module reads out of csrc/gs_internal.h and
csrc/gs_prims.hip (a constant that cannot be found or parsed fails the module; a threshold that moves takes its edges along):

    path                         how it is reached                                   the lines of run_sort it mirrors
    MSD                          n <= GS_MSD_MAX_N, default options                  compact = !wide_pairs && n <= 2^25; gs_msd_ok(): gs_msd_enabled()
                                                                                     && compact && n <= GS_MSD_MAX_N; if (msd) gs_msd_sort<NF>()
    compact LSD, short geometry  GS_MSD_MAX_N < n <= GS_RADIX_LARGE_N,               else if (compact): two gs_radix_pass (9 + 7 bits); gs_radix_chunk(n)
                                 or any such n with GS_SORT_MSD=0                    = n > GS_RADIX_LARGE_N ? GS_CHUNK_L : GS_CHUNK_S
    compact LSD, long geometry   n > GS_RADIX_LARGE_N                                (the same branch, 512-thread workgroups and 4096-item chunks)
    wide records                 GS_OPT_WIDE_PAIRS 1, any n                          else: two gs_radix_pass (8 + 9 bits, GS_CULLED_KEY in the second)

GS_SORT_MSD is read once per process, so the compact LSD sort of a short input runs in a CHILD process (tests/sort_jobs.py, started
with GS_SORT_MSD=0 under `timeout`): one per test function that needs it, one alive at a time; it creates its own contexts, never
replaces its program, runs a list of jobs and leaves every index list as a .npy.  If a child ends on a signal or at its time limit, or
a HIP call fails in this process, nothing further of this module touches the GPU.

Constructed inputs: every splat's bucket is chosen.  Rows (0, 0, b - 65536, 100) with the view row (0, 0, 1, 0) for an integer array
b in [0, 65535] that contains 0 and 65535: min = -65536, max = -1, 65535 / (max - min) is exactly 1.0, every depth is exact in f32,
nothing is culled (100 > 1e-4 * 65536), and splat i lands in bucket b[i].  Every such case asserts, from b alone, the populations
it claims ("segment 0x55 holds exactly 32 769 records") and that oracle.sort equals np.argsort(b, kind="stable") before the GPU's list
is looked at.  Dropped buckets: x uniform in [-0.999, 0.999], z = -1e6, size 1000, view (0.25, 0, 1, 0): the f64 depth range is just under 0.5, the
f32-rounded depths move in steps of 0.0625, so buckets fall below 0 and at or beyond 65536; the oracle alone is the reference and must
leave a zero tail of 5 .. 50 % of V; row 0 is culled (size 0), so a zero in a list is a dropped splat's slot and nothing else.  On the
GPU such a case follows a full sort of as many splats on the same context: the slots of the tail hold stale indices, not fresh memory.

Budget, as measured on one MI355X: 5.3 s of wall time for the module (4.6 s of test time).  The slowest test is test_segment_tiers
with 1.0 s (0.4 s for its 52 contexts in this process, 0.6 s for its child, most of that the child's start); every test with a child
takes 0.6 .. 0.8 s, the size switches 0.12 .. 0.18 s each (both references of 3 M splats: 0.06 s; two fresh contexts of 3 M splats:
0.12 s), the posted sorts 0.04 s.  136 contexts in this process; 5 child processes (one per test function that runs the compact LSD
sort on short inputs, one at a time) with 62 contexts between them.

Not covered here (so that nobody assumes it):
  - the near-only forms (tail, histogram, stash, spec): tests/test_near_sort_gpu.py, through gs_sort_inspect;
  - paired sorts: their lists are only visible through frames, which test_blend_paths_gpu.py and test_as_benched.py compare;
  - strip sorts (gs_sort_for)."""
import functools
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import sort_jobs
from conftest import PKG_NAME, ROOT, pkg
from oracle import oracle
from test_gpu_parity import _hostile_floats

pytestmark = pytest.mark.gpu
capi = pkg("capi")

assert not os.environ.get("GS_SORT_MSD", "").startswith("0"), "this module's own process must run the MSD sort: unset GS_SORT_MSD"


# ---------------------------------------------------------------- the constants the edges are placed from

def _constant(name, *files):
    """The value of `#define name <integer | integer << integer>` (u suffixes, parentheses and a trailing comment allowed)."""
    for f in files:
        with open(os.path.join(ROOT, PKG_NAME, "csrc", f)) as h:
            m = re.search(r"^[ \t]*#[ \t]*define[ \t]+%s[ \t]+(.*)$" % re.escape(name), h.read(), re.M)
        if m:
            expr = re.sub(r"//.*|/\*.*", "", m.group(1)).strip()
            v = re.fullmatch(r"\(?\s*(\d+)[uU]?\s*(?:<<\s*(\d+)[uU]?\s*)?\)?", expr)
            assert v, "cannot parse %s = %r (%s)" % (name, expr, f)
            return int(v.group(1)) << int(v.group(2) or 0)
    raise AssertionError("%s not found in %s" % (name, ", ".join(files)))


MSD_MAX_N = _constant("GS_MSD_MAX_N", "gs_internal.h", "gs_prims.hip")
LARGE_N = _constant("GS_RADIX_LARGE_N", "gs_internal.h", "gs_prims.hip")
CHUNK_S = _constant("GS_CHUNK_S", "gs_internal.h", "gs_prims.hip")
CHUNK_L = _constant("GS_CHUNK_L", "gs_internal.h", "gs_prims.hip")
MSD_GROUP = _constant("GS_MSD_GROUP", "gs_internal.h", "gs_prims.hip")
SEG_B = _constant("GS_SEG_B", "gs_internal.h", "gs_prims.hip")
SEG_MAXBLK = _constant("GS_SEG_MAXBLK", "gs_internal.h", "gs_prims.hip")
G = MSD_GROUP * CHUNK_S                                  # items per group row of k_msd_scatter (the MSD sort runs the short geometry)
# what the mapping in the docstring rests on: MSD sorts are short-geometry sorts, and the four size-switch cases are four paths
assert CHUNK_S < CHUNK_L and 256 <= CHUNK_S and MSD_MAX_N < LARGE_N < (1 << 25), (MSD_MAX_N, LARGE_N)
assert SEG_B >= 256 and SEG_MAXBLK >= 2 and 3 * SEG_MAXBLK * SEG_B + 17 < 200000 and 3 * G + CHUNK_S + 1 < 200000

VIEW = np.array([0.0, 0.0, 1.0, 0.0], np.float32)
VIEW_BACK = np.array([0.0, 0.0, -1.0, 0.0], np.float32)
VIEW_DROP = np.array([0.25, 0.0, 1.0, 0.0], np.float32)
SEG = 0x55                                               # the high bucket byte (= segment of k_seg_sort) the tier cases fill


# ---------------------------------------------------------------- cases and their references

class Case:
    def __init__(self, name, rows, want, view=VIEW, cut=None):
        self.name, self.rows, self.want, self.view, self.cut = name, rows, want, view, cut


def rows_of(b):
    b = np.asarray(b, np.int64)
    assert b.min() == 0 and b.max() == 65535, "both anchors"
    r = np.zeros((b.size, 4), np.float32)
    r[:, 2] = (b - 65536).astype(np.float32)
    r[:, 3] = 100.0
    return r


def definition(b):
    return np.argsort(np.asarray(b).astype(np.uint16), kind="stable").astype(np.uint32)


def constructed(name, b):
    """Splat i in bucket b[i]; the two references -- the oracle and the definition -- must agree."""
    rows = rows_of(b)
    want = oracle.sort(rows, VIEW)
    assert want.size == len(b) and np.array_equal(want, definition(b)), "%s: the oracle is not the stable argsort of the buckets" % name
    return Case(name, rows, want)


def rows_of_bucket(case):
    """The bucket of every row of a constructed case, back from its rows."""
    return case.rows[:, 2].astype(np.int64) + 65536


def population(b):
    return np.bincount(np.asarray(b, np.int64) >> 8, minlength=256)


def seg_buckets(g, low, pad):
    """len(low) records in segment SEG with the low bytes `low` in index order, `pad` records with random low bytes in each of the
    segments 0x00 and 0xFF -- the anchors 0 and 65535 among them --, at shuffled positions."""
    c, n = len(low), len(low) + 2 * pad
    pos = g.permutation(n)
    b = np.empty(n, np.int64)
    b[np.sort(pos[:c])] = (SEG << 8) | np.asarray(low, np.int64)
    fill = np.concatenate([g.integers(0, 256, pad), 0xFF00 | g.integers(0, 256, pad)])
    fill[0], fill[pad] = 0, 65535
    b[pos[c:]] = fill
    pop = population(b)
    assert pop[SEG] == c and pop[0x00] == pad and pop[0xFF] == pad and pop.sum() == n == c + 2 * pad, "segment 0x%02X does not hold %d" % (SEG, c)
    return b


@functools.lru_cache(maxsize=None)
def dropped_case(n, seed=7):
    """The narrow, far depth range whose f32 rounding drops buckets at both ends; row 0 is culled.  -> (case, V')
    x stays 0.001 inside [-1, 1]: the stored depths at the two ends round to -1000000.25 and -999999.75, and they are dropped only
    while the f64 min / max lie more than a bucket (7.6e-6) inside those values -- with x from all of [-1, 1] the extremes of a long
    input come closer than that (0.5 / n on average), the rounded depths land in buckets 0 and 65535, and no tail is left at all."""
    g = np.random.Generator(np.random.PCG64(seed + n))
    rows = np.zeros((n, 4), np.float32)
    rows[:, 0] = g.uniform(-0.999, 0.999, n).astype(np.float32)
    rows[:, 2] = -1.0e6
    rows[:, 3] = 1000.0
    rows[0, 3] = 0.0
    want = oracle.sort(rows, VIEW_DROP)
    V = want.size
    placed = want != 0
    Vp = int(placed.sum())
    assert V == n - 1 and placed[:Vp].all() and not placed[Vp:].any(), "dropped_%d: the zeros are not one tail" % n
    assert 0.05 * V <= V - Vp <= 0.5 * V, "dropped_%d: V = %d, V' = %d" % (n, V, Vp)
    return Case("dropped_%d" % n, rows, want, VIEW_DROP), Vp


@functools.lru_cache(maxsize=None)
def full_case(n, seed=3):
    """n splats in random buckets, all placed: what a context sorts BEFORE a dropped-bucket case, so that the tail's slots hold indices."""
    g = np.random.Generator(np.random.PCG64(seed + n))
    b = g.integers(0, 65536, n)
    b[0], b[1] = 65535, 0
    return constructed("full_%d" % n, b)


def fuzz_case(seed, n=None):
    """test_gpu_parity.test_sort_fuzz_specials_match_oracle's recipe (its generator, its draws in its order); n: instead of the size it draws."""
    g = np.random.Generator(np.random.PCG64(1000 + seed))
    n0 = int(g.choice([1, 2, 63, 64, 65, 255, 257, 2047, 2049, 4097, 30011, 131071, 262145]))
    n = n0 if n is None else n
    rows4 = _hostile_floats(g, n * 4).reshape(n, 4)
    rows4[:, 3] = np.abs(rows4[:, 3]) * 0.01 if seed % 3 else rows4[:, 3]
    view = _hostile_floats(g, 4) if seed % 4 == 3 else g.normal(0.0, 1.0, 4).astype(np.float32)
    cut = None
    if seed % 2:
        cut = g.normal(0.0, 0.4, 16).astype(np.float32)
        if seed % 6 == 5:
            cut[g.integers(0, 16)] = np.float32(np.nan)
    return Case("fuzz%d_n%d" % (seed, n), rows4, oracle.sort(rows4, view, cut), view, cut)


# ---------------------------------------------------------------- running jobs here and in the GS_SORT_MSD=0 child

_DEAD = []                                               # why nothing further touches the GPU


def _alive():
    if _DEAD:
        pytest.fail("not run: " + _DEAD[0])


def run_here(steps):
    _alive()
    try:
        return sort_jobs.run_job(capi, steps)
    except capi.GsError as e:
        if e.code == capi.E_HIP:
            _DEAD.append("a HIP call failed earlier in this module (%s)" % e.message)
        raise


def run_child(jobs, d, limit=180):
    """The jobs in ONE child process with GS_SORT_MSD=0 -> {out name: list}."""
    _alive()
    d = str(d)
    names, keep = {}, []

    def ref(a):
        if a is None or not isinstance(a, np.ndarray):
            return a
        if id(a) not in names:
            names[id(a)] = "in%d" % len(names)
            keep.append(a)
            np.save(os.path.join(d, names[id(a)] + ".npy"), a)
        return names[id(a)]

    outs = [st[3] for steps in jobs for st in steps if st[0] in ("sort", "posted", "near")] + [st[1] for steps in jobs for st in steps if st[0] == "rows"]
    assert len(set(outs)) == len(outs), "output names must be unique over a child's jobs"
    with open(os.path.join(d, "jobs.json"), "w") as f:
        json.dump([[[ref(x) for x in st] for st in steps] for steps in jobs], f)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(sort_jobs.__file__), d]
    t0 = time.perf_counter()
    p = subprocess.run(cmd, env=dict(os.environ, GS_SORT_MSD="0"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print("GS_SORT_MSD=0 child: %d jobs, exit status %d, %.2f s" % (len(jobs), p.returncode, time.perf_counter() - t0))
    if p.returncode < 0 or p.returncode >= 124:
        _DEAD.append("the GS_SORT_MSD=0 child ended on a signal or at its time limit (exit status %d)" % p.returncode)
    assert p.returncode == 0, "GS_SORT_MSD=0 child: exit status %d\n%s" % (p.returncode, p.stdout[-4000:])
    return {o: np.load(os.path.join(d, o + ".npy")) for o in outs}


def differs(tag, got, want):
    """None, or a sentence about the first difference (lists are compared whole: no tolerance, no skipped element)."""
    if got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want):
        return None
    if got.shape != want.shape:
        return "%s: %d entries, not %d" % (tag, got.size, want.size)
    bad = np.flatnonzero(got != want)
    return "%s: %d of %d entries differ, first at %d: %d, not %d" % (tag, bad.size, want.size, bad[0], got[bad[0]], want[bad[0]])


def steps_of(case, name, wide=False, twice=False, before=None):
    """One fresh context's steps: [a full sort of `before`, clear,] push, [wide records,] sort [, sort again]."""
    s = []
    if before is not None:
        s += [["push", before.rows]] + ([["wide", 1]] if wide else []) + [["sort", before.view, before.cut, name + ".before"], ["clear"]]
    s += [["push", case.rows]] + ([["wide", 1]] if wide and before is None else []) + [["sort", case.view, case.cut, name]]
    if twice:
        s += [["sort", case.view, case.cut, name + ".again"]]
    return s


def expect(case, name, twice=False, before=None):
    e = {name: case.want}
    if twice:
        e[name + ".again"] = case.want
    if before is not None:
        e[name + ".before"] = before.want
    return e


def check(cases, tmp_path=None, before=None):
    """Every case on every path its n allows, each on a fresh context: the default path (sorted twice: the second sort meets what the
    first left behind) and wide records in this process, the compact LSD sort with the short geometry in ONE child when tmp_path is
    given.  before: {case name: the case sorted first on the same context}.  All differences are collected, then asserted."""
    before = before or {}
    bad, t0 = [], time.perf_counter()
    for c in cases:
        assert c.rows.shape[0] <= MSD_MAX_N or tmp_path is None
        for tag, wide in (("default", False), ("wide", True)):
            name = "%s.%s" % (c.name, tag)
            got = run_here(steps_of(c, name, wide=wide, twice=not wide, before=before.get(c.name)))
            want = expect(c, name, twice=not wide, before=before.get(c.name))
            assert set(got) == set(want)
            bad += [differs(k, got[k], want[k]) for k in sorted(want)]
    t1 = time.perf_counter()
    if tmp_path is not None:
        got = run_child([steps_of(c, c.name + ".lsd", twice=True, before=before.get(c.name)) for c in cases], tmp_path)
        for c in cases:
            want = expect(c, c.name + ".lsd", twice=True, before=before.get(c.name))
            bad += [differs(k, got[k], want[k]) for k in sorted(want)]
    print("%d cases: %.2f s in this process, %.2f s in the child" % (len(cases), t1 - t0, time.perf_counter() - t1))
    bad = [b for b in bad if b]
    assert not bad, "\n".join(bad[:40])


# ---------------------------------------------------------------- 1. the block tiers of k_seg_sort

def test_segment_tiers(tmp_path):
    """One segment (high bucket byte 0x55) of exactly 1, 63, 64, 65, S - 1, S, S + 1, 2 S, M S, M S + 1 and 3 M S + 17 records
    (S = GS_SEG_B, M = GS_SEG_MAXBLK: one block with 8 or 16 rounds; 2 .. M blocks by as many workgroups, each counting the whole
    segment first; more than M blocks in turn by one workgroup), its low bytes spread over all 256 values, and all equal -- a pure
    stability test: the segment's part of the list ascends in index.  Then the cloud in one segment apart from the anchors, 256
    segments of one record each, and low bytes that descend with the index."""
    S, M = SEG_B, SEG_MAXBLK
    g = np.random.Generator(np.random.PCG64(55))
    cases = []
    for c in (1, 63, 64, 65, S - 1, S, S + 1, 2 * S, M * S, M * S + 1, 3 * M * S + 17):
        cases.append(constructed("seg%d_spread" % c, seg_buckets(g, g.permutation(np.arange(c) % 256), 300)))
        eq = constructed("seg%d_equal" % c, seg_buckets(g, np.full(c, 0xAA), 300))
        part = eq.want[300:300 + c].astype(np.int64)                # (segment 0x00's 300 records come first)
        assert (np.diff(part) > 0).all() and ((rows_of_bucket(eq) >> 8)[part] == SEG).all()
        cases.append(eq)
    lone = seg_buckets(g, g.integers(0, 256, 5 * S + 9), 1)             # the whole cloud in one segment apart from the two anchors
    assert population(lone)[SEG] == lone.size - 2
    cases.append(constructed("one_segment", lone))
    singles = (np.arange(256) << 8) | g.integers(0, 256, 256)           # 256 segments of one record each
    singles[0], singles[255] = 0, 65535
    singles = g.permutation(singles)
    assert (population(singles) == 1).all()
    cases.append(constructed("256_segments_of_1", singles))
    cases.append(constructed("descending_256", seg_buckets(g, 255 - np.arange(256), 300)))          # strictly descending low bytes
    c = M * S + 1
    cases.append(constructed("descending_%d" % c, seg_buckets(g, 255 - (np.arange(c) * 256) // c, 300)))   # ... and never ascending, over M + 1 blocks
    assert max(k.rows.shape[0] for k in cases) < 200000
    check(cases, tmp_path)


# ---------------------------------------------------------------- 2. chunk and group rows of k_msd_scatter

def every_digit_in_every_chunk(g, n):
    hi = np.concatenate([g.permutation(np.arange(min(CHUNK_S, n - o)) % 256) for o in range(0, n, CHUNK_S)])
    b = (hi << 8) | g.integers(0, 256, n)
    b[np.flatnonzero(hi == 0)[0]], b[np.flatnonzero(hi == 255)[0]] = 0, 65535
    for o in range(0, n - CHUNK_S + 1, CHUNK_S):
        assert (np.bincount(b[o:o + CHUNK_S] >> 8, minlength=256) > 0).all(), "a full chunk lacks a digit"
    return b


def each_digit_in_one_chunk(g, n):
    chunks = -(-n // CHUNK_S)
    assert chunks <= 256
    k = np.arange(n) // CHUNK_S
    hi = k + chunks * (g.integers(0, 1 << 30, n) % ((255 - k) // chunks + 1))     # a digit d with d mod chunks == k, d <= 255
    b = (hi << 8) | g.integers(0, 256, n)
    k255 = 255 % chunks
    b[0], b[k255 * CHUNK_S + (1 if k255 == 0 else 0)] = 0, 65535
    assert ((b >> 8) % chunks == k).all() and (b >> 8).max() == 255, "a digit lies outside its chunk"
    return b


def test_scatter_chunk_and_group_edges(tmp_path):
    """n on the edges of a chunk (GS_CHUNK_S items) and of a group row (G = GS_MSD_GROUP chunks), and ending one item into a new chunk
    of a new group: k_msd_scatter sums a chunk's offset from the rows of the groups before its own and of the chunks of its group
    before it, msd_column_sum clamps the rows that do not exist.  High bytes: every digit in every chunk (every row sum matters), and
    each digit d in chunk d mod chunks only (every other row holds 0 for it); low bytes random."""
    g = np.random.Generator(np.random.PCG64(2048))
    cases = []
    for n in (CHUNK_S - 1, CHUNK_S, CHUNK_S + 1, G - 1, G, G + 1, 2 * G + 1, 3 * G + CHUNK_S + 1):
        cases.append(constructed("scatter%d_every" % n, every_digit_in_every_chunk(g, n)))
        cases.append(constructed("scatter%d_one" % n, each_digit_in_one_chunk(g, n)))
    check(cases, tmp_path)


# ---------------------------------------------------------------- 3. the size switches of run_sort

class BigCloud:
    """GS_RADIX_LARGE_N + 1 buckets from a peaked distribution (a clipped normal around 0x8000, sigma 0x0800: the busiest segment holds
    ~12 % of the cloud) behind the two anchors, built once; a case is a slice, its references are computed once."""

    def __init__(self):
        g = np.random.Generator(np.random.PCG64(21))
        self.b = np.clip(np.rint(g.normal(0x8000, 0x0800, LARGE_N + 1)), 0, 65535).astype(np.int64)
        self.b[0], self.b[1] = 65535, 0
        self.cases = {}

    def case(self, n):
        if n not in self.cases:
            t0 = time.perf_counter()
            self.cases[n] = constructed("peaked_%d" % n, self.b[:n])
            print("references at n = %d: %.2f s" % (n, time.perf_counter() - t0))
        return self.cases[n]


@pytest.fixture(scope="module")
def big():
    return BigCloud()


@pytest.mark.parametrize("n", [MSD_MAX_N, MSD_MAX_N + 1, LARGE_N, LARGE_N + 1])
def test_size_switches(big, n):
    """n and n + 1 at GS_MSD_MAX_N (MSD | compact LSD, short geometry) and at GS_RADIX_LARGE_N (short | long geometry: 256-thread
    workgroups and 2048-item chunks | 512 and 4096), each on its default path and with wide records."""
    check([big.case(n)])


def test_dropped_buckets_where_the_compact_lsd_sort_begins(big):
    """GS_MSD_MAX_N + 1 splats with dropped buckets: the zero tail of the compact LSD sort's last pass (n_kept), and of the wide records'
    second pass, at the smallest size that takes that path without the environment switch -- on a context that has just sorted the
    peaked cloud of that size (all placed: the tail's slots hold its indices)."""
    case, Vp = dropped_case(MSD_MAX_N + 1)
    full = big.case(MSD_MAX_N + 1)
    bad = []
    for tag, wide in (("default", False), ("wide", True)):
        got = run_here(steps_of(case, tag, wide=wide, before=full))
        assert got[tag].size == case.want.size and not got[tag][Vp:].any(), tag
        bad += [differs("%s.%s" % (case.name, tag), got[tag], case.want), differs("%s.%s" % (full.name, tag), got[tag + ".before"], full.want)]
    assert not any(bad), bad


# ---------------------------------------------------------------- 4. dropped buckets and the zero tail

def test_dropped_buckets_and_zero_tail_every_path(tmp_path):
    """V' placed records and a zero tail [V', V) of 5 .. 50 % of V, at 40 000, 2049 and 4097 splats: filled by k_seg_sort (fill_to)
    on the MSD path, by the last radix pass (n_kept) on the compact LSD path, by GS_CULLED_KEY records on the wide path.  Every
    context first sorts as many splats that are all placed, so the tail's slots hold indices a fill that is skipped would leave."""
    cases, before = [], {}
    for n in (40000, CHUNK_S + 1, 2 * CHUNK_S + 1):
        case, Vp = dropped_case(n)
        print("%s: V = %d, V' = %d, zero tail %d" % (case.name, case.want.size, Vp, case.want.size - Vp))
        assert not case.want[Vp:].any() and case.want[:Vp].all()
        cases.append(case)
        before[case.name] = full_case(n)
    check(cases, tmp_path, before=before)


# ---------------------------------------------------------------- 5. culls, cutouts and IEEE specials

def cutout_window(zc, half, scale=1.0):
    """A cutout matrix (column-major, index.js:526-545) that keeps |z - zc| <= half (x = y = 0 lie inside); half a power of two.
    scale 1: affine (last row 0 0 0 1: gsm::in_cutout_affine); scale 2: every entry doubled, w = 1 / 2: the general form."""
    c = np.zeros(16, np.float32)
    c[0] = c[5] = c[15] = 1.0
    c[10] = 0.5 / half
    c[14] = -zc * 0.5 / half
    assert float(c[14]) == -zc * 0.5 / half and float(c[10]) * half == 0.5, "the window is not exact in f32"
    return c * np.float32(scale)


def test_culls_cutouts_and_specials(tmp_path):
    """The 12 seeds of test_sort_fuzz_specials_match_oracle (NaN / Inf / signed zeros / denormals / huge values in rows, view rows and
    cutout matrices; the oracle is the only reference) where they never ran: at their own sizes on the compact LSD sort with the short
    geometry (the child), and at n = GS_SEG_B + 1 and G + 1 on the MSD path and with wide records.  Constructed: a cutout that keeps
    exactly the splats of one segment (affine and general matrix), a cutout that keeps nothing (V = 0), and a cloud of which only the
    two anchors survive the size cull (V = 2)."""
    cases = [fuzz_case(seed, (SEG_B + 1, G + 1)[seed % 2]) for seed in range(12)]
    g = np.random.Generator(np.random.PCG64(5))
    c = SEG_MAXBLK * SEG_B + 1
    b = seg_buckets(g, g.integers(0, 256, c), 300)
    rows = rows_of(b)
    kept = np.flatnonzero(b >> 8 == SEG)
    assert kept.size == c
    order = kept[np.argsort(b[kept].astype(np.uint16), kind="stable")].astype(np.uint32)
    zc = (SEG << 8) + 127.5 - 65536.0                            # the segment's depths are zc -127.5 .. +127.5; its neighbours' begin at +-128.5
    for name, scale in (("cutout_one_segment_affine", 1.0), ("cutout_one_segment_general", 2.0)):
        cut = cutout_window(zc, 128.0, scale)
        want = oracle.sort(rows, VIEW, cut)
        assert want.size == c and np.array_equal(want, order), name    # (min / max are the segment's: 65535 / 255 = 257, bucket = 257 * low byte)
        cases.append(Case(name, rows, want, VIEW, cut))
    cut = cutout_window(1024.0, 128.0)                           # nothing lies at z > 0
    want = oracle.sort(rows, VIEW, cut)
    assert want.size == 0
    cases.append(Case("cutout_keeps_nothing", rows, want, VIEW, cut))
    two = rows.copy()
    two[:, 3] = 0.0                                              # size 0 is culled (0 > 1e-4 * |depth| fails) ...
    anchors = [int(np.flatnonzero(b == 0)[0]), int(np.flatnonzero(b == 65535)[0])]
    two[anchors, 3] = 100.0                                      # ... but for the anchors
    want = oracle.sort(two, VIEW)
    assert want.tolist() == anchors
    cases.append(Case("only_the_anchors", two, want))
    bad, t0 = [], time.perf_counter()
    for k in cases:
        for tag, wide in (("default", False), ("wide", True)):
            got = run_here(steps_of(k, tag, wide=wide, twice=not wide))
            bad += [differs("%s.%s" % (k.name, o), got[o], k.want) for o in sorted(got)]
    t1 = time.perf_counter()
    lsd = [fuzz_case(seed) for seed in range(12)] + cases[12:]
    got = run_child([steps_of(k, k.name + ".lsd", twice=True) for k in lsd], tmp_path)
    for k in lsd:
        bad += [differs(o, got[o], k.want) for o in (k.name + ".lsd", k.name + ".lsd.again")]
    print("%d + %d cases: %.2f s in this process, %.2f s in the child" % (len(cases), len(lsd), t1 - t0, time.perf_counter() - t1))
    bad = [x for x in bad if x]
    assert not bad, "\n".join(bad[:40])


# ---------------------------------------------------------------- 6. what one sort leaves for the next

def test_state_carried_from_sort_to_sort(big, tmp_path):
    """ONE context, every list checked: GS_MSD_MAX_N + 1 splats (compact LSD) -> clear, 65 splats -> pushed up to G + 1 (two group
    rows, which gs_msd_arm has the NEXT depth pass clear) -> wide records -> compact again -> the same view again (the list repeats)
    -> the mirrored cloud (z = b + 1, view row (0, 0, -1, 0): bucket 65535 - b, every segment's population changes).  The same in the
    child, where every sort is a compact LSD sort whose histogram rows are pre-filled by the bucket pass."""
    g = np.random.Generator(np.random.PCG64(6))
    b = np.minimum((g.random(G + 1) ** 3 * 65536).astype(np.int64), 65535)     # skewed: segment d and segment 255 - d differ in population
    b[0], b[1] = 65535, 0
    long_ = big.case(MSD_MAX_N + 1)
    c65, cG = constructed("first_65", b[:65]), constructed("up_to_G+1", b)
    pop = population(b)
    assert (pop != pop[::-1]).sum() >= 250 and pop.sum() == G + 1, "the mirrored cloud does not change the segments' populations"
    mirrored = np.zeros((G + 1, 4), np.float32)
    mirrored[:, 2] = (b + 1).astype(np.float32)
    mirrored[:, 3] = 100.0
    want_m = oracle.sort(mirrored, VIEW_BACK)
    assert np.array_equal(want_m, definition(65535 - b))
    steps = [["push", long_.rows], ["sort", VIEW, None, "1_long"], ["clear"], ["push", cG.rows[:65]], ["sort", VIEW, None, "2_short"],
             ["push", cG.rows[65:]], ["sort", VIEW, None, "3_pushed"], ["wide", 1], ["sort", VIEW, None, "4_wide"], ["wide", 0],
             ["sort", VIEW, None, "5_compact"], ["sort", VIEW, None, "6_again"], ["clear"], ["push", mirrored], ["sort", VIEW_BACK, None, "7_mirrored"]]
    want = {"1_long": long_.want, "2_short": c65.want, "3_pushed": cG.want, "4_wide": cG.want, "5_compact": cG.want, "6_again": cG.want,
            "7_mirrored": want_m}
    t0 = time.perf_counter()
    here = run_here(steps)
    t1 = time.perf_counter()
    child = run_child([[st[:3] + ["lsd_" + st[3]] if st[0] == "sort" else st for st in steps]], tmp_path)
    print("the sequence: %.2f s in this process, %.2f s in the child" % (t1 - t0, time.perf_counter() - t1))
    bad = [differs(k, here[k], want[k]) for k in sorted(want)] + [differs("lsd_" + k, child["lsd_" + k], want[k]) for k in sorted(want)]
    assert not any(bad), "\n".join(x for x in bad if x)


# ---------------------------------------------------------------- 7. the posted sort

def test_posted_sort_gives_the_list_sort_gives():
    """gs_sort_begin + gs_sort_poll(wait) run the same kernels on another lane's scratch: a segment of M S + 1 records, G + 1 splats
    over two group rows, and dropped buckets (after a full sort and a full posted sort on the same context: stale indices in both
    lanes' tails)."""
    g = np.random.Generator(np.random.PCG64(77))
    c = SEG_MAXBLK * SEG_B + 1
    seg = constructed("posted_segment", seg_buckets(g, g.integers(0, 256, c), 300))
    grp = constructed("posted_groups", every_digit_in_every_chunk(g, G + 1))
    drop, Vp = dropped_case(40000)
    full = full_case(40000)
    bad = []
    for k, before in ((seg, None), (grp, None), (drop, full)):
        steps = []
        if before is not None:
            steps += [["push", before.rows], ["sort", before.view, None, "b_sort"], ["posted", before.view, None, "b_posted"], ["clear"]]
        steps += [["push", k.rows], ["sort", k.view, k.cut, "sort"], ["posted", k.view, k.cut, "posted"], ["posted", k.view, k.cut, "posted_again"]]
        got = run_here(steps)
        for o in sorted(got):
            bad.append(differs("%s.%s" % (k.name, o), got[o], before.want if o.startswith("b_") else k.want))
        bad.append(differs("%s: posted against sort()" % k.name, got["posted"], got["sort"]))
    assert not got["posted"][Vp:].any() and got["posted"].size == drop.want.size
    assert not any(bad), "\n".join(x for x in bad if x)
