"""CPU tier of the per-splat properties (include/gs_splat.h: gs_prop_eval, gs_hist_bin): the kernels' own functions, compiled for the
host, against numpy mirrors of the rules the header states -- bit for bit -- every refusal that needs no GPU, and the constants of the
ctypes binding against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg
from oracle import oracle

capi = pkg("capi")
synth = pkg("synth")

NEW = ["gs_prop_eval", "gs_hist_bin", "gs_prop_range", "gs_histogram", "gs_select_range", "gs_multi_prop_range", "gs_multi_histogram",
       "gs_multi_select_range"]
PROPS = ["X", "Y", "Z", "RED", "GREEN", "BLUE", "ALPHA", "SIZE2"]


def _header():
    with open(os.path.join(ROOT, "include", "gs_splat.h")) as f:
        return f.read()


def _define(name):
    m = re.search(r"^#define\s+%s\s+(\d+)u?\b" % name, _header(), re.M)
    assert m, name
    return int(m.group(1))


def prop_mirror(cs, cc, prop):
    """the header's table, every operation f64 and in the stated order"""
    cs = np.asarray(cs, np.float32).reshape(-1, 4)
    cc = np.asarray(cc, np.uint32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        if prop == capi.PROP_X:
            return cs[:, 0].astype(np.float64)
        if prop == capi.PROP_Y:
            return cs[:, 1].astype(np.float64)
        if prop == capi.PROP_Z:
            return -(cs[:, 2].astype(np.float64))
        if capi.PROP_RED <= prop <= capi.PROP_ALPHA:
            return ((cc[:, 3] >> np.uint32(8 * (prop - capi.PROP_RED))) & np.uint32(255)).astype(np.float64)
        assert prop == capi.PROP_SIZE2
        q11 = (cc[:, 0] & np.uint32(0xFFFF)).astype(np.uint16).view(np.int16).astype(np.float64)
        q22 = (cc[:, 1] >> np.uint32(16)).astype(np.uint16).view(np.int16).astype(np.float64)
        q33 = (cc[:, 2] >> np.uint32(16)).astype(np.uint16).view(np.int16).astype(np.float64)
        return ((q11 + q22) + q33) * cs[:, 3].astype(np.float64)


def bin_mirror(v, lo, hi, nbins):
    """scale = (double)nbins / (hi - lo); bin = min((int64)floor((v - lo) * scale), nbins - 1); -1 below lo, -2 above hi, -3 NaN"""
    v = np.asarray(v, np.float64).reshape(-1)
    lo, hi = np.float64(lo), np.float64(hi)
    scale = np.float64(nbins) / (hi - lo)
    out = np.empty(v.size, np.int64)
    nan, below, above = np.isnan(v), v < lo, v > hi
    ok = ~(nan | below | above)
    out[nan], out[below], out[above] = -3, -1, -2
    out[ok] = np.minimum(np.floor((v[ok] - lo) * scale).astype(np.int64), nbins - 1)
    return out.astype(np.int32)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------- binding and header

def test_symbols_are_declared_exported_and_bound():
    hdr = _header()
    L = capi.load()
    for name in NEW:
        assert re.search(r"GS_API\s+int\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in capi.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name
    for name in ("prop_range", "histogram", "select_range"):
        assert hasattr(capi.Context, name) and hasattr(capi.Multi, name), name
    # appended: every declaration the header had keeps its place
    assert hdr.index("gs_prop_eval") > hdr.index("GS_API int gs_download(")


def test_constants_agree_with_the_header():
    for k, name in enumerate(PROPS):
        assert getattr(capi, "PROP_" + name) == _define("GS_PROP_" + name) == k
    assert capi.HIST_MAX_BINS == _define("GS_HIST_MAX_BINS") == 4096


# ---------------------------------------------------------------- gs_prop_eval

def hand_made_records():
    """covariance diagonals at -32768, -1, 0 and 32767 (the off-diagonal halves carry a pattern that must not leak in) x a cs[3] of 0, a
    denormal, Inf, NaN and ordinary values x positions of +-0, +-Inf, NaN"""
    diag = np.array([-32768, -1, 0, 32767], np.int16).view(np.uint16).astype(np.uint32)
    scales = np.array([0.0, -0.0, 1e-45, 1e-39, np.inf, -np.inf, np.nan, 1.0, 3.0517578e-05, 7.25], np.float32)
    pos = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.5, -2.75e-3], np.float32)
    cs, cc = [], []
    k = 0
    for a in diag:
        for b in diag:
            for c in diag:
                for s in scales:
                    cs.append((pos[k % 7], pos[(k // 7) % 7], pos[(k // 49) % 7], s))
                    cc.append((a | np.uint32(0x5A5A0000), (b << np.uint32(16)) | np.uint32(0x1234), (c << np.uint32(16)) | np.uint32(0xFEDC),
                               np.uint32((k * 2654435761) & 0xFFFFFFFF)))
                    k += 1
    # negative NaN and a NaN with a payload in the position and in the scale
    odd = np.array([0xFFC00000, 0x7FC12345, 0x7F800001], np.uint32).view(np.float32)
    for o in odd:
        cs.append((o, o, o, o)); cc.append((1, 1 << 16, 1 << 16, 0x80FF017F))
    return np.array(cs, np.float32), np.array(cc, np.uint32)


@pytest.mark.parametrize("prop", range(8))
def test_prop_eval_equals_the_mirror_on_packed_rows(prop):
    cs, cc, _ = oracle.pack(synth.make_splat_rows(4096))
    got = capi.prop_eval(cs, cc.view(np.uint32).reshape(-1, 4), prop)
    want = prop_mirror(cs, cc.view(np.uint32).reshape(-1, 4), prop)
    assert got.shape == (4096,) and np.array_equal(bits(got), bits(want))
    assert np.unique(got).size > (100 if prop != capi.PROP_ALPHA else 10), "the case proves nothing"


@pytest.mark.parametrize("prop", range(8))
def test_prop_eval_equals_the_mirror_on_hand_made_records(prop):
    cs, cc = hand_made_records()
    got, want = capi.prop_eval(cs, cc, prop), prop_mirror(cs, cc, prop)
    assert np.array_equal(bits(got), bits(want)), np.flatnonzero(bits(got) != bits(want))[:8]
    if prop == capi.PROP_SIZE2:
        assert np.isnan(got).any() and np.isinf(got).any() and (got == 0).any() and (got < 0).any()
        one = capi.prop_eval(np.array([0, 0, 0, 2.0], np.float32), np.array([32767, 32767 << 16, 32767 << 16, 0], np.uint32), prop)
        assert one == 3 * 32767 * 2.0
        low = capi.prop_eval(np.array([0, 0, 0, 0.5], np.float32), np.array([0x8000, 0x8000 << 16, 0x8000 << 16, 0], np.uint32), prop)
        assert low == -3 * 32768 * 0.5
    if prop == capi.PROP_Z:
        assert got[0] == 0 and np.signbit(capi.prop_eval(np.zeros(4, np.float32), np.zeros(4, np.uint32), prop))    # -(+0) = -0


def test_prop_eval_refuses():
    L = capi.load()
    cs, cc, out = (C.c_float * 4)(), (C.c_uint32 * 4)(), C.c_double(7.0)
    assert L.gs_prop_eval(cs, cc, 0, C.byref(out)) == capi.GS_OK and out.value == 0.0
    out.value = 7.0
    for bad in (-1, 8, 255, 1 << 30):
        assert L.gs_prop_eval(cs, cc, bad, C.byref(out)) == capi.E_BADARG
    assert L.gs_prop_eval(None, cc, 0, C.byref(out)) == capi.E_BADARG
    assert L.gs_prop_eval(cs, None, 0, C.byref(out)) == capi.E_BADARG
    assert L.gs_prop_eval(cs, cc, 0, None) == capi.E_BADARG
    assert out.value == 7.0


# ---------------------------------------------------------------- gs_hist_bin

RANGES = [(0.0, 255.0), (-1e-3, 1e30), (0.1, 0.3), (-8.0, 8.0), (-2.5e-7, -1.25e-7)]
DEGENERATE = [(5e-324, 1.5e-323), (-1.7e308, 1.7e308)]          # nbins / (hi - lo) is +inf, or hi - lo is: the product can be inf or NaN


def probe_values(lo, hi, nbins):
    lo, hi = np.float64(lo), np.float64(hi)
    v = [lo, hi, np.nextafter(lo, -np.inf), np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf),
         np.nan, np.inf, -np.inf, 0.0, -0.0, (lo + hi) / 2]
    with np.errstate(all="ignore"):
        edges = lo + np.arange(1, nbins, dtype=np.float64) * ((hi - lo) / np.float64(nbins))
    if edges.size > 300:
        edges = np.concatenate([edges[:100], edges[edges.size // 2 - 50:edges.size // 2 + 50], edges[-100:]])
    edges = edges[np.isfinite(edges)]
    return np.concatenate([np.array(v, np.float64), edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)])


@pytest.mark.parametrize("nbins", [1, 2, 3, 100, 256, 4096])
@pytest.mark.parametrize("rng", RANGES)
def test_hist_bin_equals_the_rule(rng, nbins):
    lo, hi = rng
    v = probe_values(lo, hi, nbins)
    with np.errstate(all="ignore"):
        want = bin_mirror(v, lo, hi, nbins)
    got = capi.hist_bin(v, lo, hi, nbins)
    assert np.array_equal(got, want), (rng, nbins, v[got != want][:5], got[got != want][:5], want[got != want][:5])
    assert got[0] == 0 and got[1] == nbins - 1 and got[2] == -1 and got[5] == -2 and got[6] == -3 and got[7] == -2 and got[8] == -1
    assert got.max() == nbins - 1 and got[got >= 0].min() == 0
    if nbins > 1:
        assert np.unique(got[got >= 0]).size >= min(nbins, 100) // 2, "the probes do not spread over the bins: the case proves nothing"


def test_hist_bin_bytes_land_in_their_own_bin():
    v = np.arange(256, dtype=np.float64)
    assert np.array_equal(capi.hist_bin(v, 0.0, 255.0, 256), np.minimum(np.floor(v * (256.0 / 255.0)), 255).astype(np.int32))
    assert np.array_equal(capi.hist_bin(v, 0.0, 256.0, 256), np.arange(256, dtype=np.int32))
    assert capi.hist_bin(255.0, 0.0, 255.0, 256) == 255 and capi.hist_bin(255.0, 0.0, 255.0, 1) == 0


def test_hist_bin_stays_inside_when_the_scale_overflows():
    """a range of two denormal steps, and one wider than the largest double: the product is inf or NaN for some values inside -- they
    land in the last bin, never at an index outside the table"""
    for lo, hi in DEGENERATE:
        for nbins in (1, 7, 4096):
            got = capi.hist_bin(np.array([lo, hi, (lo + hi) / 2], np.float64), lo, hi, nbins)
            assert ((got >= 0) & (got < nbins)).all()
            assert capi.hist_bin(np.nextafter(lo, -np.inf), lo, hi, nbins) == -1 and capi.hist_bin(np.nextafter(hi, np.inf), lo, hi, nbins) == -2


def test_hist_bin_refuses():
    L = capi.load()
    out = C.c_int32(77)
    ok = lambda *a: L.gs_hist_bin(*a)
    assert ok(0.5, 0.0, 1.0, 4, C.byref(out)) == capi.GS_OK and out.value == 2
    out.value = 77
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.nan), (-np.inf, 1.0), (0.0, np.inf), (np.nan, np.nan), (-np.inf, np.inf)):
        assert ok(0.5, lo, hi, 4, C.byref(out)) == capi.E_BADARG, (lo, hi)
    for nbins in (0, 4097, 0xFFFFFFFF):
        assert ok(0.5, 0.0, 1.0, nbins, C.byref(out)) == capi.E_BADARG, nbins
    assert ok(0.5, 0.0, 1.0, 4, None) == capi.E_BADARG
    assert ok(0.5, 0.0, 1.0, 1, C.byref(out)) == capi.GS_OK and ok(0.5, 0.0, 1.0, 4096, C.byref(out)) == capi.GS_OK
    with pytest.raises(capi.GsError):
        capi.hist_bin(0.5, 1.0, 0.0, 4)


def test_null_context_is_refused_without_a_gpu():
    L = capi.load()
    d, n, c = C.c_double(0), C.c_size_t(0), (C.c_uint32 * 4)()
    assert L.gs_prop_range(None, 0, 0, 0, C.byref(d), C.byref(d), C.byref(n)) == capi.E_BADARG
    assert L.gs_histogram(None, 0, 0.0, 1.0, 4, 0, 0, c, None) == capi.E_BADARG
    assert L.gs_select_range(None, 0, 0.0, 1.0, 0, 0, 0, C.byref(n)) == capi.E_BADARG
    assert L.gs_multi_prop_range(None, 0, 0, 0, C.byref(d), C.byref(d), C.byref(n)) == capi.E_BADARG
    assert L.gs_multi_histogram(None, 0, 0.0, 1.0, 4, 0, 0, c, None) == capi.E_BADARG
    assert L.gs_multi_select_range(None, 0, 0.0, 1.0, 0, 0, 0, C.byref(n)) == capi.E_BADARG
