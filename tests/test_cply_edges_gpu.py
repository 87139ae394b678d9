"""GPU tier: the compressed .ply's kernels (csrc/gs_cply.hip) at the sizes and on the values where only the GPU has code of its own.

The arithmetic is shared with the host (gs_cply.h) and pinned there by test_cply_cpu.  What the device does alone: the Morton order by
four stable 8-bit radix passes over (code, staged index) on a private sorter whose histogram rows are one per CHUNK_S records; the box of
positions by wave reductions and atomics on a grid that ends at BOX_GRID workgroups; a chunk's bounds by wave reductions and one LDS step;
the grid stride of k_cply_decode and k_cply_keys beyond GRID workgroups; the SH store's growth (sh_reserve) and the decoder's SH strides.
So the sizes lie around one, three and many radix chunks and beyond each grid's end, and the values are the ones random data never has:
ties, NaN and inf, -0.0 against +0.0, zero extent, scales without a logarithm.

Every comparison is bit for bit against the host entry points (capi.splat_to_cply, capi.cply_to_splat, capi.cply_sh) over what the
context itself exports (test_cply_gpu.host_file); nothing is taken from the kernels.  Every size is an expression in the constants read
out of the sources, and the values the sizes rest on are asserted.  Where a case claims something about its own input, the claim is
asserted from the input, or from the host's answer, before the GPU's answer is looked at.

The tie clause of test_cply_gpu.test_export_cply_equals_the_host_writer lives on there; the cases in which it bites are section 2 here."""
import os
import re

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT, pkg
from test_cply_cpu import make_rows, split_file
from test_cply_gpu import host_file, morton_codes, resident, sh_rows_of
from test_sort_paths_gpu import _constant

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

HIDDEN = capi.STATE_HIDDEN
BLOCK = _constant("GS_BLOCK", "gs_internal.h")
CHUNK_S = _constant("GS_CHUNK_S", "gs_internal.h")
LARGE_N = _constant("GS_RADIX_LARGE_N", "gs_internal.h")
CHUNK = _constant("GS_CPLY_CHUNK", "gs_cply.h")
GRID = _constant("GS_CPLY_GRID", "gs_cply.hip")


def _cply_source():
    with open(os.path.join(ROOT, PKG_NAME, "csrc", "gs_cply.hip")) as f:
        return f.read()


def _box_grid():
    """the end of k_cply_bounds_pos' grid: a number in its launch, no #define"""
    m = re.search(r"hipLaunchKernelGGL\(k_cply_bounds_pos, dim3\(pass_grid\(n, (\d+)\)\), dim3\(GS_BLOCK\)", _cply_source())
    assert m, "the launch of k_cply_bounds_pos not found"
    return int(m.group(1))


def _sh_first_capacity():
    """sh_reserve starts at (size_t)1 << 16 rows and doubles: plain code, read from the text"""
    body = _cply_source().split("int sh_reserve(", 1)[1].split("\n}\n", 1)[0]
    m = re.search(r"size_t cap = ctx->sh_cap \? ctx->sh_cap : \(size_t\)1 << (\d+);\s*while \(cap < want\) cap \*= 2;", body)
    assert m, "sh_reserve's growth rule not found"
    return 1 << int(m.group(1))


BOX_GRID = _box_grid()
SH_CAP0 = _sh_first_capacity()
NBOX = BOX_GRID * BLOCK + 1                                          # the second trip of k_cply_bounds_pos
NDEC = GRID * BLOCK + 1                                              # the second trip of k_cply_decode
SORT_SIZES = [CHUNK_S - 1, CHUNK_S, CHUNK_S + 1, 3 * CHUNK_S + 1, NBOX]
NHARD = CHUNK_S + 1 + CHUNK + 4                                      # hard chunks before and behind the radix-chunk edge


def test_the_constants_the_sizes_rest_on():
    assert (BLOCK, CHUNK_S, CHUNK, GRID, BOX_GRID, SH_CAP0) == (256, 2048, 256, 16384, 1024, 65536)
    assert SORT_SIZES == [2047, 2048, 2049, 3 * 2048 + 1, 262145] and NDEC == 4194305 and NHARD == 2049 + 260
    assert CHUNK == BLOCK                                             # k_cply_encode: one workgroup per chunk
    assert NBOX <= LARGE_N                                            # every sort here runs on chunks of CHUNK_S: NBOX is 129 of them
    passes = re.search(r"for\s*\(\s*int\s+pass\s*=\s*0\s*;\s*pass\s*<\s*(\d+)\s*&&[^;]*;\s*pass\s*\+\+\s*\)", _cply_source())
    assert passes and int(passes.group(1)) == 4                       # four passes of 8 bits: 30-bit codes


# ---------------------------------------------------------------- inputs

def hidden_for(total, extra):
    """`extra` hidden splats spread over all of `total`: staged index != splat index from the second splat on"""
    hid = np.zeros(total, bool)
    hid[1 + np.arange(extra) * (total // extra)] = True
    assert hid.sum() == extra and hid[1] and not hid[0] and hid[total // 2:].any()
    return hid


EXTRA = 97


def context_of(rows, sh=None, sh_degree=0, hid=None):
    c = capi.Context(0)
    c.push_splat(rows)
    if sh is not None:
        c.push_sh(sh, sh_degree)
    if hid is not None:
        c.set_state(0, hid.astype(np.uint8) * HIDDEN)
    return c


def both_filters(m, rows_of):
    """(tag, rows, hidden set or None, filter): m passing splats through "all", and through "visible" of m + EXTRA splats"""
    return [("all", rows_of(m), None, "all"), ("visible", rows_of(m + EXTRA), hidden_for(m + EXTRA, EXTRA), "visible")]


def export_and_check(c, of, sh_degree, morton, passing, tag):
    """gs_export_cply against the host writer over what the context exports -> (file, out_index, the host's rows in file order)"""
    want, want_index, rows = host_file(c, of, sh_degree, morton)
    assert want_index.size == passing.size and np.array_equal(np.sort(want_index), passing), (tag, "the host's index")
    got, index = c.export_cply(of, sh_degree, morton=morton, want_index=True)
    assert np.array_equal(index, want_index), (tag, "out_index")
    assert np.array_equal(got, want), (tag, "the file")
    return got, index, rows


def positions(rows):
    return np.ascontiguousarray(rows[:, :12]).view(np.float32).reshape(-1, 3)


def set_positions(rows, pos, at=slice(None)):
    rows[at, 0:12] = np.ascontiguousarray(pos, "<f4").view(np.uint8).reshape(-1, 12)


# ---------------------------------------------------------------- 1. the Morton sort at the radix-chunk edges

@pytest.mark.parametrize("m", SORT_SIZES)
def test_morton_order_across_radix_chunks(m):
    """random positions, a partial SH store; NBOX is also the second trip of k_cply_bounds_pos"""
    for tag, rows, hid, of in both_filters(m, lambda n: make_rows(n, seed=8100 + m)[0]):
        n = len(rows)
        passing = np.flatnonzero(~hid).astype(np.uint32) if hid is not None else np.arange(n, dtype=np.uint32)
        assert passing.size == m and (hid is None or not np.array_equal(passing, np.arange(m)))
        with context_of(rows, sh_rows_of((2 * n) // 3, 1, seed=m), 1, hid) as c:
            got, index, in_order = export_and_check(c, of, 1, True, passing, (m, tag))
            assert capi.cply_info(got) == {"splats": m, "chunks": -(-m // CHUNK), "sh_degree": 1, "chunk_floats": 18}
            codes = morton_codes(c.export_splat(of), in_order).astype(np.int64)
            assert (np.diff(codes) >= 0).all() and (np.diff(index.astype(np.int64))[np.diff(codes) == 0] > 0).all()
            assert all(np.unique((codes >> s) & 255).size > 8 for s in (0, 8, 16, 24))             # no pass is idle (the last has 6 bits)
            if m == NBOX:
                assert not np.array_equal(index, passing)


# ---------------------------------------------------------------- 2. ties that mean something

def tie_rows(kind, n, seed):
    """-> rows of n splats whose positions make ties dominate (written in numpy: everything but the position is make_rows')"""
    rows = make_rows(n, seed)[0]
    g = np.random.Generator(np.random.PCG64([seed, n]))
    if kind == "one_code":
        pos = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (n, 1))
    elif kind == "two_codes":                                          # the even indices carry the HIGHER code: the order is odd, then even
        pos = np.where((np.arange(n) % 2 == 0)[:, None], np.array([[2.0, 3.0, 1.0]], np.float32), np.array([[-1.0, -4.0, -0.5]], np.float32))
    else:                                                              # 64 distinct positions, each n / 64 times, in shuffled index order
        pos = (g.normal(size=(64, 3)) * 3.0).astype(np.float32)[g.permutation(n) % 64]
    set_positions(rows, pos)
    return rows


TIE_MIN = {"one_code": lambda m: m - 1, "two_codes": lambda m: m - 2, "duplicated": lambda m: m - 64}


@pytest.mark.parametrize("kind", list(TIE_MIN))
@pytest.mark.parametrize("m", SORT_SIZES)
def test_morton_ties_keep_the_index_order(m, kind):
    for tag, rows, hid, of in both_filters(m, lambda n: tie_rows(kind, n, seed=8200 + m)):
        passing = np.flatnonzero(~hid).astype(np.uint32) if hid is not None else np.arange(m, dtype=np.uint32)
        with context_of(rows, hid=hid) as c:
            want, want_index, in_order = host_file(c, of, 0, True)
            staged = c.export_splat(of)
            codes = morton_codes(staged, in_order).astype(np.int64)
            ties = int((np.diff(codes) == 0).sum())
            # the data really has ties, and the host orders them by index (the host: std::stable_sort, pinned by test_cply_cpu)
            assert ties >= m - 64 and ties >= TIE_MIN[kind](m) and (np.diff(codes) >= 0).all()
            assert (np.diff(want_index.astype(np.int64))[np.diff(codes) == 0] > 0).all()
            if kind == "one_code":
                assert np.array_equal(want_index, passing)
            elif kind == "two_codes":
                high = morton_codes(staged, staged) == codes[-1]
                assert codes[0] < codes[-1] and high[0] and 0 < high.sum() < m and np.array_equal(high, (passing % 2) == 0)
                assert np.array_equal(want_index, np.concatenate([passing[~high], passing[high]]))
            else:
                assert np.unique(positions(staged), axis=0).shape[0] == 64 and not np.array_equal(want_index, passing)
            got, index = c.export_cply(of, 0, morton=True, want_index=True)
            assert np.array_equal(index, want_index), (kind, m, tag, "out_index")
            assert np.array_equal(got, want), (kind, m, tag, "the file")


# ---------------------------------------------------------------- 3. boxes and bounds on hard values

NAN, INF = np.float32(np.nan), np.float32(np.inf)
FAR = np.array([100.0, -50.0, 25.0], np.float32)                      # where the last chunk sits: a dead lane's 0 would be a new min or max
HARD = {"nan_wave_1": 1, "not_finite_x": 2, "zeros": 3, "zero_extent": 4, "scales": 5, "middle": 6, "nan_wave_3": 7, "not_finite_y": 8}
ZERO_EXTENT = np.array([1.5, -2.0, 0.25], np.float32)


def chunk_at(k):
    return slice(k * CHUNK, (k + 1) * CHUNK)


def hard_rows(n, seed=8300):
    """n > 9 chunks of splats; chunk k as HARD names it, the others random, the partial last one around FAR.  Chunks 1..7 lie before the
    radix-chunk edge at CHUNK_S, chunk 8 and the last one behind it."""
    assert 9 * CHUNK < n <= 10 * CHUNK and 8 * CHUNK == CHUNK_S
    rows = make_rows(n, seed)[0]
    pos = positions(rows).copy()
    pos[HARD["nan_wave_1"] * CHUNK + 64:HARD["nan_wave_1"] * CHUNK + 128, 0] = NAN        # one wave without a finite x; the other three have one
    pos[HARD["nan_wave_3"] * CHUNK + 192:HARD["nan_wave_3"] * CHUNK + 256, 0] = NAN
    pos[chunk_at(HARD["not_finite_x"])] = (INF, NAN, NAN)
    pos[chunk_at(HARD["not_finite_y"])] = (NAN, -INF, NAN)
    pos[chunk_at(HARD["zeros"])] = np.where((np.arange(CHUNK) % 2 == 0)[:, None], np.float32(-0.0), np.float32(0.0))
    pos[chunk_at(HARD["zero_extent"])] = ZERO_EXTENT
    pos[9 * CHUNK:] = FAR + pos[9 * CHUNK:] * np.float32(0.125)
    set_positions(rows, pos)
    # scales without a logarithm.  The packed record keeps scale * scale: a negative scale survives the pack only as -0.0, or next to a
    # NaN (which takes the whole record's scale factor with it) -- what reaches the encoder is asserted in the test.  Nothing is left
    # uncovered by that: cply_log_scale takes 0, -0.0, a negative scale and NaN by one comparison, !(scale > 0)
    sc = np.zeros((CHUNK, 3), np.float32)
    sc[1::4] = np.float32(-0.0)
    sc[2::4] = NAN
    sc[3::4] = (-1.0, NAN, -2.0)
    rows[chunk_at(HARD["scales"]), 12:24] = sc.astype("<f4").view(np.uint8).reshape(CHUNK, 12)
    return rows


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("tail", [5, 1, 63, 64, 65])
def test_bounds_on_hard_chunks(tail):
    """NHARD splats (tail 5), and a partial last chunk of 1, 63, 64 and 65 live splats: dead lanes against live ones in the LDS step"""
    n = 9 * CHUNK + tail
    assert tail != 5 or n == NHARD
    rows = hard_rows(n)
    passing = np.arange(n, dtype=np.uint32)
    with context_of(rows) as c:
        staged, wide = c.export_splat("all", want_wide=True)
        # what reaches the encoder: the positions as pushed, bit for bit; in the scales' chunk no scale with a logarithm
        assert np.array_equal(bits(positions(staged)), bits(positions(rows)))
        with np.errstate(invalid="ignore"):
            assert not (wide[chunk_at(HARD["scales"]), 0:3] > 0.0).any() and (wide[chunk_at(HARD["middle"]), 0:3] > 0.0).all()
        plain, index, _ = export_and_check(c, "all", 0, False, passing, (tail, "file order"))
        assert np.array_equal(index, passing)
        _, ch, packed, _, _ = split_file(plain)
        assert ch.shape == (10, 18) and np.isfinite(ch).all()
        for k, axis in ((HARD["nan_wave_1"], 0), (HARD["nan_wave_3"], 0)):         # the finite x of the other three waves, not the identities
            x = positions(rows)[chunk_at(k), 0]
            assert np.isnan(x).sum() == 64 and ch[k, 0] == np.nanmin(x) and ch[k, 3] == np.nanmax(x) and ch[k, 0] < ch[k, 3]
        for k in (HARD["not_finite_x"], HARD["not_finite_y"]):                     # nothing finite: 0, 0 by the bits, and words of 0
            assert not bits(ch[k, 0:6]).any() and not packed[chunk_at(k), 0].any()
        k = HARD["zeros"]
        assert list(bits(ch[k, 0:3])) == [0x80000000] * 3 and list(bits(ch[k, 3:6])) == [0] * 3 and not packed[chunk_at(k), 0].any()
        k = HARD["zero_extent"]
        assert np.array_equal(ch[k, 0:3], ZERO_EXTENT) and np.array_equal(ch[k, 3:6], ZERO_EXTENT) and not packed[chunk_at(k), 0].any()
        k = HARD["scales"]
        assert (ch[k, 6:12] == -20.0).all() and not packed[chunk_at(k), 2].any()
        last = positions(rows)[9 * CHUNK:]
        assert np.array_equal(ch[9, 0:3], last.min(axis=0)) and np.array_equal(ch[9, 3:6], last.max(axis=0)) and (np.abs(ch[9, 0:6]) > 20.0).all()
        # Morton: the box is of the finite positions alone, the hard splats sit on both sides of the radix-chunk edge
        got, index, in_order = export_and_check(c, "all", 0, True, passing, (tail, "morton"))
        codes = morton_codes(staged, in_order).astype(np.int64)
        assert (np.diff(codes) >= 0).all() and (np.diff(index.astype(np.int64))[np.diff(codes) == 0] > 0).all()
        assert not np.array_equal(index, passing) and np.isfinite(split_file(got)[1]).all()


def test_every_position_nan():
    """the box is (0, 0), every code is 0: the Morton order is the identity; every chunk's position bounds are 0, 0"""
    n = NHARD
    rows = make_rows(n, seed=8400)[0]
    set_positions(rows, np.full((n, 3), NAN))
    passing = np.arange(n, dtype=np.uint32)
    with context_of(rows) as c:
        assert np.isnan(positions(c.export_splat("all"))).all()
        for morton in (False, True):
            got, index, _ = export_and_check(c, "all", 0, morton, passing, morton)
            assert np.array_equal(index, passing)
            _, ch, packed, _, _ = split_file(got)
            assert not bits(ch[:, 0:6]).any() and not packed[:, 0].any() and packed[:, 2].any()


def test_a_filter_that_empties_the_middle_chunk():
    """chunks are over staged rows: hiding a whole chunk's index range makes the file one chunk shorter, and moves every later chunk"""
    n = NHARD
    rows = hard_rows(n)
    hid = np.zeros(n, bool); hid[chunk_at(HARD["middle"])] = True
    passing = np.flatnonzero(~hid).astype(np.uint32)
    with context_of(rows, hid=hid) as c:
        whole = c.export_cply("all", 0, morton=False)
        for morton in (False, True):
            got, index, _ = export_and_check(c, "visible", 0, morton, passing, morton)
            assert capi.cply_info(got)["splats"] == n - CHUNK and capi.cply_info(got)["chunks"] == 9
        got, index = c.export_cply("visible", 0, morton=False, want_index=True)
        assert np.array_equal(index, passing)
        a, b = split_file(whole), split_file(got)
        keep = np.delete(np.arange(10), HARD["middle"])
        assert np.array_equal(bits(b[1]), bits(a[1][keep])) and np.array_equal(b[2], a[2][~hid])


# ---------------------------------------------------------------- 4. decode beyond the grid's end, and the SH strides

def test_decode_beyond_the_grid():
    """the second trip of k_cply_decode: NDEC splats.  array_equal only: no message is built from arrays of this size"""
    rows, wide = make_rows(NDEC, seed=8500)
    data = capi.splat_to_cply(rows, wide)
    del rows, wide
    assert capi.cply_info(data)["splats"] == NDEC > GRID * BLOCK
    want_rows, want_wide = capi.cply_to_splat(data, want_wide=True)
    with capi.Context(0) as c:
        got_rows, got_wide = c.cply_to_splat_gpu(data, want_wide=True)
    assert got_rows.shape == (NDEC, 32) and want_rows[-1].any() and want_wide[-1].any()
    same_rows, same_wide = np.array_equal(got_rows, want_rows), np.array_equal(got_wide.view(np.uint32), want_wide.view(np.uint32))
    assert same_rows and same_wide


@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("option", [1, 2, 3])
def test_load_cply_sh_strides(option, degree):
    """`per` = 3, 8, 15 in the file against K kept and KS stored, nine pairs; a store behind the file's rows shows a stride that is too long"""
    n = CHUNK + 1
    rows, wide = make_rows(n, seed=8600 + degree)
    data = capi.splat_to_cply(rows, wide, sh_rows_of(n, degree, seed=8610 + option), degree)
    assert capi.cply_info(data)["sh_degree"] == degree
    sh, d = capi.cply_sh(data, option)
    D = min(option, degree)
    assert d == D and sh.shape == (n, 3 * (D + 1) ** 2) and sh.any(axis=0).all()
    with capi.Context(0) as a, capi.Context(0) as b:
        for c in (a, b):
            c.set_option(capi.OPT_SH_DEGREE, option)
        for _ in range(2):                                                        # the second load goes behind the first: sh_out is offset
            a.load_cply(data)
            b.push_splat(capi.cply_to_splat(data))
            b.push_sh(sh, D)
        assert a.count() == b.count() == 2 * n and a.sh_count() == b.sh_count() == (2 * n, D)
        for x, y in zip(resident(a, 2 * n), resident(b, 2 * n)):
            assert np.array_equal(x, y)
        got = a.download_sh()
        assert np.array_equal(got.view(np.uint32), b.download_sh().view(np.uint32))
        assert np.array_equal(got.view(np.uint32), np.concatenate([sh, sh]).view(np.uint32))


# ---------------------------------------------------------------- 5. the SH store's growth

class Member(capi.Context):
    """a context a gs_multi owns, seen through the single-context calls"""

    def __init__(self, multi, i):
        self._L = multi._L
        self._h = self._L.gs_multi_ctx(multi._h, int(i))
        assert self._h

    def close(self):
        self._h = None

    __del__ = close


def test_the_sh_store_grows_across_loads():
    sizes = (SH_CAP0 - 536, 1000, 70000)
    assert sizes[0] < SH_CAP0 < sizes[0] + sizes[1] and 2 * SH_CAP0 < sum(sizes) <= 4 * SH_CAP0 and sizes[0] == 65000
    files, hosts = [], []
    for k, n in enumerate(sizes):
        rows, wide = make_rows(n, seed=8700 + k)
        data = capi.splat_to_cply(rows, wide, sh_rows_of(n, 1, seed=8710 + k), 1, morton=(k == 1))
        sh, d = capi.cply_sh(data, 1)
        assert d == 1 and sh.shape == (n, 12) and sh.any(axis=1).all()
        files.append(data); hosts.append((capi.cply_to_splat(data), sh))
    after = []
    with capi.Context(0) as a, capi.Context(0) as b:
        for c in (a, b):
            c.set_option(capi.OPT_SH_DEGREE, 1)
        at = 0
        for data, (rows, sh) in zip(files, hosts):
            a.load_cply(data)
            b.push_splat(rows)
            b.push_sh(sh, 1)
            at += len(rows)
            assert a.count() == b.count() == at and a.sh_count() == b.sh_count() == (at, 1)
            rec, store = resident(a, at), a.download_sh().view(np.uint32)
            for x, y in zip(rec, resident(b, at)):
                assert np.array_equal(x, y)
            same = np.array_equal(store, b.download_sh().view(np.uint32))
            assert same, "the SH store after %d rows" % at
            assert np.array_equal(store, np.concatenate([h[1] for h in hosts])[:at].view(np.uint32))
            after.append((rec, store))
    with capi.Multi([0, 0]) as m:
        m.set_option(capi.OPT_SH_DEGREE, 1)
        at = 0
        for k in range(2):
            m.load_cply(files[k])
            at += sizes[k]
            assert m.count() == at
            for i in range(2):
                with Member(m, i) as c:
                    assert c.count() == at and c.sh_count() == (at, 1)
                    for x, y in zip(resident(c, at), after[k][0]):
                        assert np.array_equal(x, y)
                    same = np.array_equal(c.download_sh().view(np.uint32), after[k][1])
                    assert same, "member %d's SH store after %d rows" % (i, at)


# ---------------------------------------------------------------- 6. a Morton export while a sort is queued

def test_morton_export_between_sort_begin_and_poll():
    """the export's radix passes run on a sorter of their own: the posted sort's order and the frame are those of a context that never
    exported, and the file is the host's"""
    n = 2 * CHUNK_S + 1
    assert n == 4097
    cam = synth.index_html_camera(320, 180, 25.0, capi=capi)
    p = capi.make_params(cam["gs_mv"], cam["gs_proj"], 320, 180, focal_=cam["focal"])
    src = synth.make_splat_rows(n, seed=8800).reshape(n, 32).copy()
    with capi.Context(0) as a, capi.Context(0) as b:
        a.push_splat(src); b.push_splat(src)
        want_file, want_index, _ = host_file(a, "all", 0, True)
        a.sort_begin(cam["view"])
        got_file, index = a.export_cply("all", 0, morton=True, want_index=True)
        order = a.sort_poll(wait=True)
        frame = a.render(p)
        b.sort_begin(cam["view"])
        want_order = b.sort_poll(wait=True)
        want_frame = b.render(p)
    assert order is not None and want_order is not None and 0 < want_order.size <= n
    assert np.array_equal(order, want_order)
    assert want_frame.any() and np.array_equal(frame, want_frame)
    assert np.array_equal(index, want_index) and not np.array_equal(index, np.arange(n)) and np.array_equal(got_file, want_file)
