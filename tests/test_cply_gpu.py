"""GPU tier of the compressed .ply (include/gs_splat.h: gs_load_cply, gs_cply_to_splat_gpu, gs_export_cply and the multi forms).

Everything is exact: the kernels call the functions the host evaluators call, and tests/test_cply_cpu.py pins those to the header's rules.
Sizes sit below, at and across the 256-splat chunk; the SH store is shorter than the cloud."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
from test_cply_cpu import bounds, frac, make_file, make_rows, spread

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

HIDDEN, SELECTED = capi.STATE_HIDDEN, capi.STATE_SELECTED


def sh_rows_of(n, degree, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.normal(size=(n, 3 * (degree + 1) ** 2)) * 0.5).astype(np.float32)


def a_file(n, degree, seed, morton=False):
    rows, wide = make_rows(n, seed)
    return capi.splat_to_cply(rows, wide, sh_rows_of((2 * n) // 3, degree, seed + 1), degree, morton=morton)


# ---------------------------------------------------------------- decode

@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_the_decode_kernel_equals_the_host_decoder(n):
    with capi.Context(0) as c:
        for data in (a_file(n, 2, seed=300 + n), make_file(n, 12, 0, seed=n), make_file(n, 18, 15, seed=n + 1)):
            want_rows, want_wide = capi.cply_to_splat(data, want_wide=True)
            rows, wide = c.cply_to_splat_gpu(data, want_wide=True)
            assert rows.shape == (n, 32) and np.array_equal(rows, want_rows)
            assert np.array_equal(wide.view(np.uint32), want_wide.view(np.uint32))
            assert np.array_equal(c.cply_to_splat_gpu(data), want_rows)                    # rows alone
        assert c.count() == 0                                                              # a conversion loads nothing
        with pytest.raises(capi.GsError) as e:
            c.cply_to_splat_gpu(bytes(data)[:-1])
        assert e.value.code == capi.E_PLY_DATA


def resident(c, n):
    return [c.download(capi.BUF_CENTER_SCALE, n, np.float32, 4).view(np.uint32), c.download(capi.BUF_COV_COLOR, n, np.uint32, 4),
            c.download(capi.BUF_SORT_ROWS, n, np.float32, 4).view(np.uint32)]


@pytest.mark.parametrize("n,option", [(257, 2), (1000, 3), (256, 0)])
def test_load_cply_equals_pushing_the_host_rows(n, option):
    first, second = make_file(n, 18, 15, seed=40 + n), a_file(300, 3, seed=41 + n, morton=True)
    with capi.Context(0) as a, capi.Context(0) as b:
        for c in (a, b):
            c.set_option(capi.OPT_SH_DEGREE, option)
        for data in (first, second):                                                       # the second file goes behind the first
            a.load_cply(data)
            b.push_splat(capi.cply_to_splat(data))
            if option:
                sh, d = capi.cply_sh(data, option)
                assert d == option
                b.push_sh(sh, d)
        m = n + 300
        assert a.count() == b.count() == m and a.sh_count() == b.sh_count() == ((m, option) if option else (0, 0))
        for x, y in zip(resident(a, m), resident(b, m)):
            assert np.array_equal(x, y)
        if option:
            assert np.array_equal(a.download_sh().view(np.uint32), b.download_sh().view(np.uint32))


def test_load_cply_keeps_a_store_that_is_not_parallel_and_refuses_other_files():
    data = a_file(257, 2, seed=9)
    inria = synth.rows_to_inria_ply(make_rows(64, seed=3)[0])
    with capi.Context(0) as c:
        c.set_option(capi.OPT_SH_DEGREE, 2)
        c.push_splat(make_rows(10, seed=1)[0])                                             # ten splats without SH rows: the store is not parallel
        c.load_cply(data)
        assert c.count() == 267 and c.sh_count() == (0, 0)
        with pytest.raises(capi.GsError) as e:
            c.load_cply(inria)
        assert e.value.code == capi.E_PLY_HEADER and c.count() == 267
        c.load_ply(inria)                                                                  # ... which the existing loader reads as before
        assert c.count() == 267 + 64


# ---------------------------------------------------------------- encode

def host_file(c, of, sh_degree, morton):
    rows, wide, index = c.export_splat(of, want_wide=True, want_index=True)
    sh, stored = c.export_sh(of)
    D = min(sh_degree, stored)
    K, Ks = (D + 1) ** 2, (stored + 1) ** 2
    cut = np.ascontiguousarray(sh.reshape(-1, 3, Ks)[:, :, :K]).reshape(-1, 3 * K) if len(sh) else None
    data, order = capi.splat_to_cply(rows, wide, cut, D, morton=morton, want_index=True)
    return data, index[order], rows[order]


def morton_codes(rows_all, rows):
    """the header's rule for the codes of `rows` against the box of `rows_all` (test_cply_cpu.mirror_encode's expression: a position that
    is NaN or below the box takes 0 on its axis, +inf the last cell)"""
    pos_all = rows_all[:, :12].copy().view(np.float32).reshape(-1, 3)
    pos = rows[:, :12].copy().view(np.float32).reshape(-1, 3)
    lo, hi = bounds(pos_all)
    t = frac(pos, lo[None, :], hi[None, :])
    with np.errstate(invalid="ignore"):
        ax = np.where(np.isnan(t) | (t < 0.0), 0.0, np.minimum(1023.0, np.floor(t * 1024.0)))
    ax = np.nan_to_num(ax, nan=0.0).astype(np.uint32)
    return spread(ax[:, 0]) | (spread(ax[:, 1]) << np.uint32(1)) | (spread(ax[:, 2]) << np.uint32(2))


@pytest.mark.parametrize("n", [257, 1000])
def test_export_cply_equals_the_host_writer(n):
    src = synth.make_splat_rows(n, seed=70 + n).reshape(n, 32).copy()
    src[[101, 103, 104], 0:12] = src[100, 0:12]                                            # four visible splats at one position: one code
    store = np.zeros(n - 7, np.uint8); store[::3] = HIDDEN; store[1::5] |= SELECTED
    with capi.Context(0) as c:
        c.push_splat(src)
        c.push_sh(sh_rows_of((2 * n) // 3, 2, seed=n), 2)                                 # a partial SH store
        c.set_state(0, store)
        for of in ((0, 0), (HIDDEN, 0), (0x40, 0x40)):                                     # all, the visible, nothing
            for morton in (False, True):
                for sh_degree in (3, 1, 0):
                    want, want_index, rows = host_file(c, of, sh_degree, morton)
                    got, index = c.export_cply(of, sh_degree, morton=morton, want_index=True)
                    assert bytes(got) == bytes(want), (of, morton, sh_degree)
                    assert np.array_equal(index, want_index)
                    assert np.array_equal(c.export_cply(of, sh_degree, morton=morton), got)
                # out_index: a permutation of the passing indices; Morton codes ascend, ties ascend by index
                passing = c.export_splat(of, want_index=True)[1]
                assert np.array_equal(np.sort(index), passing)
                if morton and len(index):
                    codes = morton_codes(c.export_splat(of), rows).astype(np.int64)
                    assert (np.diff(codes) == 0).sum() >= 3                                    # the tie clause bites (more: test_cply_edges_gpu)
                    assert (np.diff(codes) >= 0).all() and (np.diff(index.astype(np.int64))[np.diff(codes) == 0] > 0).all()
                elif len(index):
                    assert np.array_equal(index, passing)
                info = capi.cply_info(got)
                assert info["splats"] == len(passing) and info["sh_degree"] == 0 and info["chunk_floats"] == 18   # (the last sh_degree asked for: 0)
        got = c.export_cply("all", 2)
        assert capi.cply_info(got)["sh_degree"] == 2
        nb = C.c_size_t(0)
        assert c._L.gs_export_cply(c._h, 0, 0, 0, 2, None, None, C.byref(nb)) == capi.E_BADARG        # an unknown flag
        assert c._L.gs_export_cply(c._h, 0, 0, 4, 0, None, None, C.byref(nb)) == capi.E_BADARG
        assert c._L.gs_export_cply(c._h, 0, 0, 0, 0, None, None, None) == capi.E_BADARG
    with capi.Context(0) as c:                                                             # nothing resident: the header alone
        assert capi.cply_info(c.export_cply())["splats"] == 0
        c.push_matrices(np.zeros((4, 16), np.float32))
        with pytest.raises(capi.GsError) as e:
            c.export_cply()
        assert e.value.code == capi.E_STATE


def test_an_exported_file_loads_back_within_the_format():
    n = 1000
    src = synth.make_splat_rows(n, seed=5).reshape(n, 32).copy()
    with capi.Context(0) as a, capi.Context(0) as b:
        a.push_splat(src)
        data, index = a.export_cply("all", 0, morton=True, want_index=True)
        b.load_cply(data)
        assert b.count() == n
        pa = a.download(capi.BUF_CENTER_SCALE, n, np.float32, 4)[index, :3].astype(np.float64)
        pb = b.download(capi.BUF_CENTER_SCALE, n, np.float32, 4)[:, :3].astype(np.float64)
        extent = pa.max(axis=0) - pa.min(axis=0)
        assert (np.abs(pa - pb) <= 0.5 * extent / 1023.0 * (1.0 + 2.0 ** -20) + 1e-6).all()


def test_an_export_changes_no_frame():
    n = 1000
    cam = synth.index_html_camera(320, 180, 25.0, capi=capi)
    p = capi.make_params(cam["gs_mv"], cam["gs_proj"], 320, 180, focal_=cam["focal"])
    src = synth.make_splat_rows(n, seed=1234).reshape(n, 32).copy()
    with capi.Context(0) as c:
        c.push_splat(src)
        c.sort(cam["view"])
        before, stats = c.render(p), c.stats()
        c.export_cply("all", 0, morton=True, want_index=True)
        c.export_cply("visible", 3, morton=False)
        assert c.stats() == stats
        after = c.render(p)                                                                # the same sort: no order was dropped
    assert before.any() and np.array_equal(before, after)


def test_multi_load_and_export_equal_the_single_context():
    data = a_file(600, 1, seed=17)
    with capi.Context(0) as c:
        c.set_option(capi.OPT_SH_DEGREE, 1)
        c.load_cply(data)
        want = c.export_cply("all", 1, morton=True, want_index=True)
        recs = resident(c, 600)
    m = capi.Multi([0, 0])
    try:
        m.set_option(capi.OPT_SH_DEGREE, 1)
        m.load_cply(data)
        assert m.count() == 600
        got = m.export_cply("all", 1, morton=True, want_index=True)
    finally:
        m.close()
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]) and len(recs[0]) == 600
