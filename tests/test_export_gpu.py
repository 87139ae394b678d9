"""GPU tier of the export (include/gs_splat.h: gs_export_splat, gs_export_sh, gs_export_ply).

The rows, wide parts and indices are exact: capi.export_row -- the kernel's own function on the host, pinned to the header's rule by
tests/test_export_cpu.py -- applied to the records the context holds (gs_download), for the splats the state filter passes, in order.
Sizes sit below, at and across the compaction chunk (GS_EDIT_CHUNK, read out of the source).  The picture of an exported cloud is held
against what the format itself costs a picture, measured on the CPU oracle."""
import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_export_cpu import covariance, quat_bytes
from test_sort_paths_gpu import _constant

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

CHUNK = _constant("GS_EDIT_IPT", "gs_cloud_pass.h") * _constant("GS_BLOCK", "gs_internal.h")
assert CHUNK == 2048
HIDDEN, SELECTED, CALLER = capi.STATE_HIDDEN, capi.STATE_SELECTED, 0x40
FILTERS = [(0, 0), (HIDDEN, 0), (3, SELECTED), (CALLER, CALLER)]
SIZES = [1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]


def make_rows(n, seed):
    return synth.make_splat_rows(n, seed=seed).reshape(n, 32).copy()


def records(c, n):
    return c.download(capi.BUF_CENTER_SCALE, n, np.float32, 4), c.download(capi.BUF_COV_COLOR, n, np.uint32, 4)


def passing_of(n, store, mask, value):
    st = np.zeros(n, np.uint8)
    st[:len(store)] = store
    return (st & np.uint8(mask)) == value


def random_store(g, length):
    st = g.integers(0, 4, length).astype(np.uint8)
    st[::3] |= CALLER
    return st


def check_export(c, want_rows, want_wide, store, mask, value):
    """one filter: the full call, the size query and the binding's variants against the host rows of the passing splats"""
    ok = np.flatnonzero(passing_of(len(want_rows), store, mask, value))
    rows, wide, index = c.export_splat((mask, value), want_wide=True, want_index=True)
    assert rows.shape == (ok.size, 32) and wide.shape == (ok.size, 7) and index.dtype == np.uint32
    assert np.array_equal(index, ok), (mask, value)
    assert np.array_equal(rows, want_rows[ok]), (mask, value, np.flatnonzero((rows != want_rows[ok]).any(axis=1))[:8])
    assert np.array_equal(wide.view(np.uint32), want_wide[ok].view(np.uint32)), (mask, value)
    import ctypes as C
    n = C.c_size_t(77)
    c._ck(c._L.gs_export_splat(c._h, mask, value, None, None, None, C.byref(n)))         # the size query
    assert n.value == ok.size
    assert np.array_equal(c.export_splat((mask, value)), rows)                            # rows alone: the same rows
    return ok


# ---------------------------------------------------------------- sizes x filters

@pytest.mark.parametrize("n", SIZES)
def test_rows_wide_parts_and_indices_equal_the_host_function(n):
    g = np.random.Generator(np.random.PCG64(7700 + n))
    src = make_rows(n, seed=500 + n)
    with capi.Context(0) as c:
        c.push_splat(src)
        cs, cc = records(c, n)
        want_rows, want_wide = capi.export_row(cs, cc, want_wide=True)
        assert np.array_equal(want_rows[:, :12], src[:, :12]) and np.array_equal(want_rows[:, 24:28], src[:, 24:28])
        check_export(c, want_rows, want_wide, np.zeros(0, np.uint8), 0, 0)                # no store at all
        check_export(c, want_rows, want_wide, np.zeros(0, np.uint8), HIDDEN, HIDDEN)      # ... nothing passes
        short = max(n - max(n // 3, 1), 0) if n > 1 else 0                                # a store shorter than N
        for length in sorted({short, n}):
            store = random_store(g, length)
            if length:
                c.set_state(0, store)
            for mask, value in FILTERS:
                check_export(c, want_rows, want_wide, store, mask, value)


def test_a_whole_chunk_fails_and_every_splat_fails():
    n = 3 * CHUNK + 5
    src = make_rows(n, seed=901)
    with capi.Context(0) as c:
        c.push_splat(src)
        want_rows, want_wide = capi.export_row(*records(c, n), want_wide=True)
        store = np.zeros(n, np.uint8)
        store[CHUNK:2 * CHUNK] = HIDDEN                                                   # the second chunk fails as a whole
        store[5] = HIDDEN; store[3 * CHUNK + 4] = HIDDEN
        c.set_state(0, store)
        ok = check_export(c, want_rows, want_wide, store, HIDDEN, 0)
        assert ok.size == n - CHUNK - 2
        ok = check_export(c, want_rows, want_wide, store, HIDDEN, HIDDEN)                 # ... and only that chunk (and two) pass
        assert ok.size == CHUNK + 2
        c.set_state(0, np.full(n, HIDDEN, np.uint8))                                      # every splat fails
        rows, wide, index = c.export_splat("visible", want_wide=True, want_index=True)
        assert rows.shape == (0, 32) and wide.shape == (0, 7) and index.size == 0
        ply = c.export_ply("visible")
        assert b"element vertex 0\n" in bytes(ply) and bytes(ply).endswith(b"end_header\n") and capi.ply_to_splat(ply).size == 0


def test_nothing_resident_and_matrices_only():
    import ctypes as C
    with capi.Context(0) as c:
        assert c.export_splat().shape == (0, 32)
        sh, d = c.export_sh()
        assert sh.shape[0] == 0 and d == 0
        ply = c.export_ply()
        assert bytes(ply).startswith(b"ply\n") and capi.ply_to_splat(ply).size == 0
        assert c._L.gs_export_splat(c._h, 0, 0, None, None, None, None) == capi.E_BADARG
        assert c._L.gs_export_sh(c._h, 0, 0, None, None, None) == capi.E_BADARG
        n = C.c_size_t(0)
        for bad in (-1, 4):
            assert c._L.gs_export_ply(c._h, 0, 0, bad, None, C.byref(n)) == capi.E_BADARG
        assert c._L.gs_export_ply(c._h, 0, 0, 0, None, None) == capi.E_BADARG
    with capi.Context(0) as c:
        c.push_matrices(np.zeros((4, 16), np.float32))
        for call in (c.export_splat, c.export_sh, c.export_ply):
            with pytest.raises(capi.GsError) as e:
                call()
            assert e.value.code == capi.E_STATE


# ---------------------------------------------------------------- the SH rows

def test_export_sh_returns_the_prefix():
    n, m, degree = CHUNK + 300, CHUNK + 10, 2
    g = np.random.Generator(np.random.PCG64(31))
    src = make_rows(n, seed=77)
    sh = g.normal(size=(m, 27)).astype(np.float32)
    store = random_store(g, n - 50)
    with capi.Context(0) as c:
        c.push_splat(src)
        c.push_sh(sh, degree)
        c.set_state(0, store)
        for mask, value in FILTERS:
            ok = passing_of(n, store, mask, value)
            got, d = c.export_sh((mask, value))
            assert d == degree and np.array_equal(got.view(np.uint32), sh[ok[:m]].view(np.uint32)), (mask, value)
            index = c.export_splat((mask, value), want_index=True)[1]
            assert (index[:len(got)] < m).all() and (index[len(got):] >= m).all()     # they belong to the first exported rows


# ---------------------------------------------------------------- read-only

def test_an_export_changes_no_frame_and_no_statistic():
    n = 3 * CHUNK + 5
    cam = synth.index_html_camera(320, 180, 25.0, capi=capi)
    p = capi.make_params(cam["gs_mv"], cam["gs_proj"], 320, 180, focal_=cam["focal"])
    src = make_rows(n, seed=1234)
    store = np.zeros(n, np.uint8); store[::5] = HIDDEN; store[1::7] |= SELECTED

    def two_frames(export):
        with capi.Context(0) as c:
            c.push_splat(src)
            c.set_state(0, store)
            c.sort(cam["view"])
            before, stats = c.render(p), c.stats()
            if export:
                assert len(c.export_splat("visible", want_wide=True, want_index=True)[0]) == int(((store & HIDDEN) == 0).sum())
                c.export_ply("selected")
                c.export_sh()
                assert c.stats() == stats                                                 # the calls themselves change no statistic
            after = c.render(p)                                                           # the same sort: no order was dropped
            return before, after, c.stats()

    before, after, stats = two_frames(True)
    assert np.array_equal(before, after) and before.any()
    b0, a0, s0 = two_frames(False)                                                        # ... and the second frame is the one drawn without them
    assert np.array_equal(b0, before) and np.array_equal(a0, after) and s0 == stats


# ---------------------------------------------------------------- compaction equivalence

def test_export_of_the_visible_equals_export_after_compact():
    n = 2 * CHUNK + 77
    g = np.random.Generator(np.random.PCG64(5))
    with capi.Context(0) as c:
        c.push_splat(make_rows(n, seed=66))
        store = (g.random(n - 9) < 0.3).astype(np.uint8) * HIDDEN
        store[::4] |= SELECTED
        c.set_state(0, store)
        rows, wide, index = c.export_splat("visible", want_wide=True, want_index=True)
        old = c.compact()
        assert np.array_equal(index, old)
        rows2, wide2, index2 = c.export_splat("all", want_wide=True, want_index=True)
        assert np.array_equal(rows, rows2) and np.array_equal(wide.view(np.uint32), wide2.view(np.uint32))
        assert np.array_equal(index2, np.arange(len(old), dtype=np.uint32))


# ---------------------------------------------------------------- closing the loop: the picture of an exported cloud

W, H, LOOP_N = 64, 48, 700


def loop_cloud():
    """-> (rows uint8[n, 32], unit quaternions f64[n, 4] as stored, scales f32[n, 3]): sizes far from sort_keep's threshold"""
    g = np.random.Generator(np.random.PCG64(424242))
    pos = (g.normal(size=(LOOP_N, 3)) * np.array([1.2, 0.6, 1.2])).astype(np.float32)
    scale = np.exp(g.uniform(np.log(0.03), np.log(0.3), size=(LOOP_N, 3))).astype(np.float32)
    q = g.normal(size=(LOOP_N, 4)); q /= np.sqrt((q * q).sum(axis=1))[:, None]
    rows = np.zeros((LOOP_N, 32), np.uint8)
    rows[:, 0:12] = pos.view(np.uint8).reshape(LOOP_N, 12)
    rows[:, 12:24] = scale.view(np.uint8).reshape(LOOP_N, 12)
    rows[:, 24:27] = g.integers(0, 256, (LOOP_N, 3))
    rows[:, 27] = g.integers(64, 256, LOOP_N)
    rows[:, 28:32] = quat_bytes(q)
    return rows, q, scale


def exact_records(cs, cc, q, scale):
    """the records pack would hold if the quaternion did not pass through bytes: the exact f64 covariance, quantised as pack quantises"""
    e = covariance(q, scale)
    mx = np.abs(e).max(axis=1)
    h = np.trunc(e * 32767.0 / mx[:, None]).astype(np.int64).astype(np.int16).view(np.uint16).astype(np.uint32)
    cs2, cc2 = cs.copy(), cc.copy()
    cs2[:, 3] = (mx / 32767.0).astype(np.float32)
    cc2[:, 0] = h[:, 0] | (h[:, 1] << np.uint32(16)); cc2[:, 1] = h[:, 2] | (h[:, 3] << np.uint32(16)); cc2[:, 2] = h[:, 4] | (h[:, 5] << np.uint32(16))
    return cs2, cc2


def test_the_picture_of_an_exported_cloud():
    """|picture of the exported rows - picture of the rows| <= 2 d_fmt + 1 LSB, d_fmt = what one pass through the format's 8-bit
    quaternion rounding costs the oracle's picture of the same rows (docs/LAB_NOTES.md 9n holds the measured figures)"""
    rows, q, scale = loop_cloud()
    cam = synth.index_html_camera(W, H, 20.0, capi=capi)
    mv, proj = cam["gs_mv"].astype(np.float32), cam["gs_proj"].astype(np.float32)
    p = capi.make_params(cam["gs_mv"], cam["gs_proj"], W, H, focal_=cam["focal"])
    # the format's own cost, on the oracle
    cs, cc, mats = oracle.pack(rows.reshape(-1))
    order = oracle.sort(mats, cam["view"])
    depth = mats[:, 12:15].astype(np.float64) @ np.asarray(cam["view"], np.float64)[:3] + float(cam["view"][3])
    size = mats[:, 15].astype(np.float64)
    assert (np.abs(size + 0.0001 * depth) > 0.2 * np.abs(0.0001 * depth)).all(), "a splat sits at sort_keep's size threshold"
    img_fmt, _, _ = oracle.render(cs, cc, order, mv, proj, cam["focal"], W, H, want_f32=False)
    xs, xc = exact_records(cs, cc, q, scale)
    img_exact, _, _ = oracle.render(xs, xc, order, mv, proj, cam["focal"], W, H, want_f32=False)
    d_fmt = int(np.abs(img_fmt.astype(int) - img_exact.astype(int)).max())
    assert d_fmt >= 1 and img_fmt.any(), "the scene does not show the format's rounding: the case proves nothing"
    with capi.Context(0) as a, capi.Context(0) as b:
        a.push_splat(rows)
        a.sort(cam["view"])
        img_a, stats_a = a.render(p), a.stats()
        out = a.export_splat()
        b.push_splat(out)
        b.sort(cam["view"])
        img_b, stats_b = b.render(p), b.stats()
    assert stats_a["n_sorted"] == stats_b["n_sorted"] == order.size
    d = int(np.abs(img_a.astype(int) - img_b.astype(int)).max())
    print("closing the loop: d_fmt = %d LSB, exported picture within %d LSB (bound %d)" % (d_fmt, d, 2 * d_fmt + 1))
    assert d <= 2 * d_fmt + 1


# ---------------------------------------------------------------- .ply loop

def test_ply_loop_keeps_count_and_sh_rows():
    n = CHUNK + 100
    src = make_rows(n, seed=2020)
    rest = np.random.default_rng(3).standard_normal((n, 45)).astype(np.float32) * np.float32(0.3)
    ply = synth.rows_to_inria_ply(src, rest)
    with capi.Context(0) as a, capi.Context(0) as b:
        a.set_option(capi.OPT_SH_DEGREE, 2)
        a.load_ply(ply)
        assert a.sh_count() == (n, 2)
        store = np.zeros(n, np.uint8); store[::6] = HIDDEN
        a.set_state(0, store)
        keep = np.flatnonzero(store == 0)
        out = a.export_ply("visible", sh_degree=2)
        b.set_option(capi.OPT_SH_DEGREE, 2)
        b.load_ply(out)
        assert b.count() == keep.size and b.sh_count() == (keep.size, 2)
        key = lambda c, m: [bytes(r) for r in np.ascontiguousarray(c.download(capi.BUF_CENTER_SCALE, m, np.float32, 4)[:, :3]).view(np.uint8).reshape(m, 12)]
        ka, kb = key(a, n), key(b, keep.size)
        assert len(set(ka)) == n
        sa, sb = a.download_sh(), b.download_sh()
        want = {ka[i]: sa[i].tobytes() for i in keep}
        got = {kb[j]: sb[j].tobytes() for j in range(keep.size)}
        assert got == want
        # the rows themselves: what export_splat gives, through the file, within the loader's rounding
        rows = a.export_splat("visible")
        back = capi.ply_to_splat(out).reshape(-1, 32)
        where = {bytes(r[:12]): j for j, r in enumerate(back)}
        gb = back[[where[bytes(r[:12])] for r in rows]]
        assert np.array_equal(gb[:, 27], rows[:, 27]) and np.abs(gb[:, 28:32].astype(int) - rows[:, 28:32].astype(int)).max() <= 1


# ---------------------------------------------------------------- two contexts of one GPU

def test_multi_export_equals_the_single_context():
    n = CHUNK + 33
    src = make_rows(n, seed=808)
    store = np.zeros(n - 5, np.uint8); store[::3] = HIDDEN; store[1::4] |= SELECTED
    with capi.Context(0) as c:
        c.push_splat(src)
        c.set_state(0, store)
        want = c.export_splat("selected", want_wide=True, want_index=True)
        want_ply = c.export_ply("visible", sh_degree=0)
    m = capi.Multi([0, 0])
    try:
        m.push_splat(src)
        m.set_state(0, store)
        got = m.export_splat("selected", want_wide=True, want_index=True)
        got_ply = m.export_ply("visible", sh_degree=0)
    finally:
        m.close()
    assert len(want[0]) == passing_of(n, store, 3, SELECTED).sum() > 0
    for w, g in zip(want, got):
        assert np.array_equal(w.view(np.uint8), g.view(np.uint8))
    assert np.array_equal(want_ply, got_ply)
