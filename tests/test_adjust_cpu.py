"""CPU tier of the in-place colour adjustment (include/gs_splat.h: gs_colour_adjust, gs_adjust_word, gs_adjust_sh_row): the kernels' own
functions (csrc/gs_adjust.h), compiled for the host, against a numpy f64 mirror of the rule the header spells out -- bit for bit --, the
identity, the agreement of the adjusted SH row with the adjusted colour before the clamp, and the refused arguments.  No GPU anywhere."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg

capi = pkg("capi")

NEW = ["gs_adjust_colour", "gs_adjust_word", "gs_adjust_sh_row", "gs_replace_splat", "gs_replace_sh",
       "gs_multi_adjust_colour", "gs_multi_replace_splat", "gs_multi_replace_sh"]
SH_C0 = 0.28209479177387814
LUMA = np.array([0.2126, 0.7152, 0.0722])


def saturation(s):
    return s * np.eye(3) + (1.0 - s) * np.tile(LUMA, (3, 1))


# name -> (m, offset, alpha_scale, alpha_offset); everything is rounded to f32 by capi.colour_adjust, the mirror reads the f32 values back
PARAMS = {
    "identity": (np.eye(3), (0, 0, 0), 1.0, 0.0),
    "channel scale": (np.diag([0.5, 1.25, 2.0]), (0, 0, 0), 1.0, 0.0),
    "desaturate": (saturation(0.3), (0, 0, 0), 1.0, 0.0),
    "oversaturate": (saturation(1.75), (0, 0, 0), 0.5, 0.0),
    "negative": (np.array([[-1.0, 0, 0], [0.25, -1.5, 0.75], [0, 1.0, -0.5]]), (255.0, 64.0, 12.5), 1.0, 0.0),
    "offset clamps": (np.eye(3), (300.0, -300.0, 0.5), 1.0, -300.0),
    "alpha scale 0": (np.eye(3), (0, 0, 0), 0.0, 77.5),
    "alpha offset 255": (np.diag([1.0, 1.0, 0.5]), (0, 0, 0), 1.0, 255.0),
}


def adjust_of(name):
    m, off, a_s, a_o = PARAMS[name]
    return capi.colour_adjust(m, off, a_s, a_o)


def widened(a):
    """the struct's f32 members as f64, as the rule takes them"""
    return (np.array(list(a.m), np.float64).reshape(3, 3), np.array(list(a.offset), np.float64), float(a.alpha_scale), float(a.alpha_offset))


def clamped_u8(v):
    """clamp to [0, 255], round to nearest, ties to even, NaN -> 0 (gs_ply.h)"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, np.where(v >= 255, 255.0, np.rint(np.clip(v, 0, 255))), 0.0).astype(np.uint32)


def word_mirror(words, a):
    m, off, a_s, a_o = widened(a)
    w = np.asarray(words, np.uint32)
    R, G, B, A = [((w >> s) & 255).astype(np.float64) for s in (0, 8, 16, 24)]
    out = np.zeros(w.shape, np.uint32)
    for c in range(3):
        v = ((m[c, 0] * R + m[c, 1] * G) + m[c, 2] * B) + off[c]
        out |= clamped_u8(v) << np.uint32(8 * c)
    return out | (clamped_u8(a_s * A + a_o) << np.uint32(24))


def dc_mirror(a):
    """what band 0 of channel c gains"""
    m, off, _, _ = widened(a)
    return np.array([((0.5 * ((m[c, 0] + m[c, 1]) + m[c, 2]) + off[c] / 255) - 0.5) / SH_C0 for c in range(3)])


def sh_mirror(rows, degree, a):
    m, _, _, _ = widened(a)
    K = (degree + 1) ** 2
    s = np.asarray(rows, np.float32).reshape(-1, 3, K).astype(np.float64)
    out = np.zeros_like(s)
    dc = dc_mirror(a)
    for c in range(3):
        out[:, c, :] = (m[c, 0] * s[:, 0, :] + m[c, 1] * s[:, 1, :]) + m[c, 2] * s[:, 2, :]
        out[:, c, 0] = out[:, c, 0] + dc[c]
    return out.astype(np.float32).reshape(-1, 3 * K)


def rgba(r, g, b, a):
    return (r | g << 8 | b << 16 | a << 24) & 0xFFFFFFFF


# hand-made words: all-0, all-255, and bytes that land on x.5 under a 0.5 scale (1 -> 0.5, 3 -> 1.5, 5 -> 2.5, 253 -> 126.5, 255 -> 127.5)
HAND = np.array([0, 0xFFFFFFFF, rgba(1, 3, 5, 7), rgba(253, 255, 251, 1), rgba(5, 1, 3, 255), rgba(255, 0, 255, 0), rgba(0, 255, 0, 128),
                 rgba(127, 128, 129, 77), rgba(2, 4, 6, 8)], np.uint32)


def sample_words():
    g = np.random.Generator(np.random.PCG64(20261021))
    return np.concatenate([g.integers(0, 1 << 32, size=65536, dtype=np.uint64).astype(np.uint32), HAND])


WORDS = sample_words()


def random_rows(n, degree, seed, spread=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.normal(size=(n, 3 * (degree + 1) ** 2)) * spread).astype(np.float32)


def test_the_new_entry_points_are_exported():
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTS, name
    assert C.sizeof(capi.ColourAdjust) == 14 * 4


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_word_rule_against_the_mirror(name):
    a = adjust_of(name)
    got, want = capi.adjust_word(WORDS, a), word_mirror(WORDS, a)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d words differ, first %#x: %#x, mirror %#x" % (bad.size, WORDS[bad[0]], got[bad[0]], want[bad[0]])


def test_ties_round_to_even_and_the_clamps_hold():
    half = capi.colour_adjust(np.diag([0.5, 0.5, 0.5]), (0, 0, 0), 0.5, 0.0)
    # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4;  126.5 -> 126, 127.5 -> 128, 125.5 -> 126, 0.5 -> 0
    assert capi.adjust_word(rgba(1, 3, 5, 7), half) == rgba(0, 2, 2, 4)
    assert capi.adjust_word(rgba(253, 255, 251, 1), half) == rgba(126, 128, 126, 0)
    clamp = adjust_of("offset clamps")
    assert capi.adjust_word(rgba(10, 200, 7, 250), clamp) == rgba(255, 0, 8, 0)          # 310, -100, 7.5 -> 8, -50
    assert capi.adjust_word(rgba(10, 200, 8, 250), clamp) == rgba(255, 0, 8, 0)          # 8.5 -> 8
    assert capi.adjust_word(0x12345678, adjust_of("alpha scale 0")) >> 24 == 78          # 77.5 -> 78
    assert capi.adjust_word(0x00345678, adjust_of("alpha offset 255")) >> 24 == 255


def test_identity_gives_back_every_word_and_row():
    ident = capi.colour_adjust()
    assert np.array_equal(capi.adjust_word(WORDS, ident), WORDS)
    assert np.array_equal(word_mirror(WORDS, ident), WORDS)
    assert np.array_equal(dc_mirror(ident), np.zeros(3)) and not np.signbit(dc_mirror(ident)).any()   # the band-0 constant is exactly 0
    for degree in (1, 2, 3):
        rows = random_rows(257, degree, 40 + degree, spread=3.0)
        out = capi.adjust_sh_rows(rows, degree, ident)
        assert np.array_equal(out.view(np.uint32), rows.view(np.uint32)), degree


@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(PARAMS))
def test_sh_rule_against_the_mirror(name, degree):
    a = adjust_of(name)
    rows = random_rows(513, degree, 50 + degree, spread=2.0)
    rows[0] = 0.0
    rows[1, ::2] = 0.0
    want = sh_mirror(rows, degree, a)
    got = capi.adjust_sh_rows(rows, degree, a)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    aliased = rows.copy()
    assert capi.adjust_sh_rows(aliased, degree, a, in_place=True) is aliased                  # out_row == sh_row
    assert np.array_equal(aliased.view(np.uint32), want.view(np.uint32))


def basis_of(degree, cam, pos):
    """b_k(d) of gs_sh.h through the library: the row with sh[0][k] = 1 alone evaluates to (0.5 + b_k) * 255 in channel 0"""
    K = (degree + 1) ** 2
    b = np.zeros(K)
    for k in range(K):
        row = np.zeros(3 * K, np.float32)
        row[k] = 1.0
        b[k] = capi.sh_eval(row, degree, cam, pos, unrounded=True)[0] / 255 - 0.5
    return b


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_adjusted_row_and_adjusted_colour_agree_before_the_clamp(degree):
    """With u = gs_sh_eval_unrounded(row) = (0.5 + sum_k b_k sh[.][k]) * 255, the adjusted row evaluates -- in exact arithmetic -- to M u + offset:
    the matrix acts on every band, and band 0's constant dc_c carries b_0 dc_c * 255 = 127.5 sum_j m_cj + offset_c - 127.5 across.
    What separates the two in floating point, per channel c, relative to T = the sum of the absolute values of all terms that enter either side
        T = 255 (0.5 + sum_k sum_j |b_k m_cj sh[j][k]| + 0.5 sum_j |m_cj| + |offset_c| / 255 + 0.5):
      * ONE f32 rounding per adjusted coefficient, relative eps = 2^-24 of a value bounded by its terms' absolute sum: at most eps T (1 + eps);
      * f64 roundings, each at most 2^-53 of the absolute sum so far (<= T).  Counted generously: the two evaluations, K + 4 additions and as
        many multiplications each (2 (2 K + 8)); the adjustment of K coefficients, 3 products and 2 sums each and band 0's constant (6 K + 8);
        M u + offset (7): N = 10 K + 31 operations, i.e. N 2^-53 T = N 2^-29 eps T.
    So |difference| <= eps T ((1 + eps) + N 2^-29): a factor of 1.0000004 at K = 16, derived, not tuned."""
    K = (degree + 1) ** 2
    eps = 2.0 ** -24
    factor = (1 + eps) + (10 * K + 31) * 2.0 ** -29
    g = np.random.Generator(np.random.PCG64(60 + degree))
    rows = (g.normal(size=(64, 3, K)) * 0.15).astype(np.float32)
    rows[:, :, 0] = g.uniform(-0.6, 0.6, size=(64, 3)).astype(np.float32)
    pos = np.array([0.25, -0.5, 1.5], np.float32)
    cams = [np.array(c, np.float64) for c in ((0, 0, 0), (3, 1, -2), (-1.5, 4, 0.5), (0.25, -0.5, 7), (10, -10, 10))]
    checked = 0
    for name in ("desaturate", "channel scale", "negative", "oversaturate"):
        a = adjust_of(name)
        m, off, _, _ = widened(a)
        adjusted = capi.adjust_sh_rows(rows.reshape(64, 3 * K), degree, a)
        for cam in cams:
            b = basis_of(degree, cam, pos)
            for i in range(64):
                u = capi.sh_eval(rows[i].reshape(-1), degree, cam, pos, unrounded=True)
                want = np.array([((m[c, 0] * u[0] + m[c, 1] * u[1]) + m[c, 2] * u[2]) + off[c] for c in range(3)])
                if not (np.all(u > 0) and np.all(u < 255) and np.all(want > 0) and np.all(want < 255)):
                    continue                                   # (only colours that stay inside (0, 255) before and after)
                got = capi.sh_eval(adjusted[i], degree, cam, pos, unrounded=True)
                s = np.abs(rows[i].astype(np.float64))
                for c in range(3):
                    T = 255 * (0.5 + sum(abs(b[k]) * (abs(m[c]) * s[:, k]).sum() for k in range(K)) + 0.5 * abs(m[c]).sum() + abs(off[c]) / 255 + 0.5)
                    assert abs(got[c] - want[c]) <= eps * T * factor, (name, degree, i, c, got[c], want[c], eps * T * factor)
                checked += 1
    assert checked >= 200, checked


def test_bad_arguments():
    L = capi.load()
    out = C.c_uint32(0)
    good = capi.colour_adjust()
    row = np.zeros(48, np.float32)
    o = np.zeros(48, np.float32)
    p = capi._p
    assert L.gs_adjust_word(0, C.byref(good), C.byref(out)) == capi.GS_OK
    assert L.gs_adjust_word(0, None, C.byref(out)) == capi.E_BADARG
    assert L.gs_adjust_word(0, C.byref(good), None) == capi.E_BADARG
    assert L.gs_adjust_sh_row(None, 3, C.byref(good), p(o)) == capi.E_BADARG
    assert L.gs_adjust_sh_row(p(row), 3, None, p(o)) == capi.E_BADARG
    assert L.gs_adjust_sh_row(p(row), 3, C.byref(good), None) == capi.E_BADARG
    assert L.gs_adjust_sh_row(p(row), 4, C.byref(good), p(o)) == capi.E_BADARG
    assert L.gs_adjust_sh_row(p(row), -1, C.byref(good), p(o)) == capi.E_BADARG
    for bad in (np.nan, np.inf, -np.inf):
        for member in range(14):
            a = capi.colour_adjust()
            C.cast(C.byref(a), C.POINTER(C.c_float))[member] = bad
            assert L.gs_adjust_word(0x80808080, C.byref(a), C.byref(out)) == capi.E_BADARG, (bad, member)
            assert L.gs_adjust_sh_row(p(row), 3, C.byref(a), p(o)) == capi.E_BADARG, (bad, member)
    assert L.gs_adjust_colour(None, C.byref(good), 0, 0, None) == capi.E_BADARG
    assert L.gs_replace_splat(None, 0, None, 0) == capi.E_BADARG
    assert L.gs_replace_sh(None, 0, None, 0, 1) == capi.E_BADARG
