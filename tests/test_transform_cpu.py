"""CPU tier of gs_transform (include/gs_splat.h: gs_similarity, gs_transform_record, gs_transform_sh_row, gs_sh_rotation,
gs_similarity_about): the kernels' own functions (csrc/gs_transform.h), compiled for the host, against a numpy f64 mirror of the rule the
header spells out -- bit for bit --, the exact short cuts, the derived accuracy of the general case, the defining property of the SH
matrices, and the refused arguments.  No GPU anywhere.

A NaN is compared as a NaN: its sign and payload are not part of the rule (numpy and the compiled code may hand on another operand's)."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import pkg
from oracle import oracle

capi = pkg("capi")
synth = pkg("synth")

NEW = ["gs_transform", "gs_multi_transform", "gs_transform_record", "gs_transform_records", "gs_transform_sh_row", "gs_sh_rotation",
       "gs_similarity_about"]
F32, F64, U32 = np.float32, np.float64, np.uint32


# ---------------------------------------------------------------- the mirror

def widened(t):
    """(R [3, 3] rows' space, s, t [3]) as the rule takes them: steps 1 and 2, python floats are IEEE f64"""
    w, x, y, z = [float(v) for v in t.rotation]
    n = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    x2, y2, z2 = x + x, y + y, z + z
    xx, xy, xz = x * x2, x * y2, x * z2
    yy, yz, zz = y * y2, y * z2, z * z2
    wx, wy, wz = w * x2, w * y2, w * z2
    R = np.array([[1 - (yy + zz), xy - wz, xz + wy],
                  [xy + wz, 1 - (xx + zz), yz - wx],
                  [xz - wy, yz + wx, 1 - (xx + yy)]], F64)
    return R, float(t.scale), np.array([float(v) for v in t.translation], F64)


def halves(cc):
    """the six int16 of cc[0..2] as f64, pack_row's order: (0,0), (1,0), (2,0), (1,1), (2,1), (2,2)"""
    cc = np.asarray(cc, U32)
    h = [cc[:, 0] & 0xFFFF, cc[:, 0] >> 16, cc[:, 1] & 0xFFFF, cc[:, 1] >> 16, cc[:, 2] & 0xFFFF, cc[:, 2] >> 16]
    return [v.astype(np.uint16).view(np.int16).astype(F64) for v in h]


def record_mirror(cs_bits, cc, sr_bits, t):
    """steps 3..9 in the operation order of the header -> (cs', cc', sort row') as uint32 bits, bound f32"""
    R, s, tr = widened(t)
    ss = s * s
    cs = np.ascontiguousarray(cs_bits, U32).view(F32).reshape(-1, 4)
    sr = np.ascontiguousarray(sr_bits, U32).view(F32).reshape(-1, 4)
    cc = np.ascontiguousarray(cc, U32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        p0, p1, p2 = cs[:, 0].astype(F64), cs[:, 1].astype(F64), -cs[:, 2].astype(F64)
        n = [s * ((R[i, 0] * p0 + R[i, 1] * p1) + R[i, 2] * p2) + tr[i] for i in range(3)]
        c = [n[0].astype(F32), n[1].astype(F32), (-n[2]).astype(F32)]
        scl = cs[:, 3]
        finite = (scl.view(U32) & U32(0x7F800000)) != U32(0x7F800000)
        identity = bool(np.all(R == np.eye(3)))
        scl_out, words = scl.copy(), [cc[:, 0].copy(), cc[:, 1].copy(), cc[:, 2].copy()]
        if identity:
            if s != 1.0:
                scl_out = np.where(finite, (scl.astype(F64) * ss).astype(F32), scl)
        else:
            sd = scl.astype(F64)
            q = halves(cc)
            a00, a01, a02, a11, a12, a22 = [v * sd for v in q]
            m = R * np.array([[1, 1, -1], [1, 1, -1], [-1, -1, 1]], F64)      # Rm: negated where exactly one index is 2
            A = [[a00, a01, a02], [a01, a11, a12], [a02, a12, a22]]
            B = [[(m[i, 0] * A[0][k] + m[i, 1] * A[1][k]) + m[i, 2] * A[2][k] for k in range(3)] for i in range(3)]
            E = [((B[i][0] * m[j, 0] + B[i][1] * m[j, 1]) + B[i][2] * m[j, 2]) * ss for i, j in ((0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2))]
            mx = np.zeros(len(cs), F64)
            for e in E:
                mx = np.where(np.abs(e) > mx, np.abs(e), mx)
            h = []
            for e in E:
                v = np.rint(e * 32767.0 / mx)
                v = np.clip(np.where(np.isnan(v), 0.0, v), -32767.0, 32767.0)
                h.append(v.astype(np.int32).astype(U32) & U32(0xFFFF))
            new = [h[0] | (h[1] << U32(16)), h[2] | (h[3] << U32(16)), h[4] | (h[5] << U32(16))]
            words = [np.where(finite, new[k], words[k]) for k in range(3)]
            scl_out = np.where(finite, (mx / 32767.0).astype(F32), scl)
        size = (sr[:, 3].astype(F64) * s).astype(F32)
        cs2 = np.stack([c[0], c[1], c[2], scl_out.astype(F32)], axis=1)
        cc2 = np.stack(words + [cc[:, 3]], axis=1).astype(U32)
        sr2 = np.stack([c[0], c[1], c[2], size], axis=1)
        top = scl_out.astype(F32) * F32(32767.0)
        bound = np.where((top == top) & (top < F32(3.0e37)), np.sqrt(F32(3.0) * top) * F32(1.001), F32(np.inf)).astype(F32)
    out_cs = np.ascontiguousarray(cs2, F32).view(U32)
    out_cs[:, 3] = np.where(finite, out_cs[:, 3], cs_bits.reshape(-1, 4)[:, 3])                # (a kept word keeps its bits)
    return out_cs, cc2, np.ascontiguousarray(sr2, F32).view(U32), bound


def same_floats(a_bits, b_bits):
    """f32 words: equal bits, or a NaN on both sides"""
    a, b = np.asarray(a_bits, U32), np.asarray(b_bits, U32)
    nan = lambda w: (w & U32(0x7FFFFFFF)) > U32(0x7F800000)
    return bool(np.all((a == b) | (nan(a) & nan(b))))


# ---------------------------------------------------------------- the records

def quat(axis, deg):
    a = np.asarray(axis, F64) / np.linalg.norm(axis)
    h = math.radians(deg) / 2
    return (math.cos(h), *(math.sin(h) * a))


def packed(n=4096, seed=7):
    cs, cc, mats = oracle.pack(synth.make_splat_rows(n, seed=seed))
    return cs.view(U32).reshape(n, 4).copy(), cc.view(U32).reshape(n, 4).copy(), np.ascontiguousarray(mats[:, 12:16]).view(U32).copy()


def with_hard_records(cs, cc, sr):
    """... and, in front: a NaN position, cs[3] = 0, +inf, -inf, NaN, all six halves 0, the int16 extremes"""
    cs, cc, sr = cs.copy(), cc.copy(), sr.copy()
    f = lambda v: np.array([v], F32).view(U32)[0]
    cs[0, 0] = f(np.nan); sr[0, 0] = f(np.nan)
    cs[1, :3] = f(np.nan)
    cs[2, 3] = f(0.0)
    cs[3, 3] = f(np.inf)
    cs[4, 3] = f(-np.inf)
    cs[5, 3] = 0x7FC01234
    cc[6, :3] = 0
    cc[7, :3] = [0x7FFF8001, 0x80017FFF, 0x7FFF7FFF]
    cs[8, 3] = f(1.0e-42)                                        # a subnormal scale word
    cs[9, 3] = f(3.0e38); sr[9, 3] = f(3.0e38)
    return cs, cc, sr


SIMILARITIES = {
    "identity": capi.similarity(),
    "translation": capi.similarity(translation=(0.5, -1.25, 3.0)),
    "scale": capi.similarity(scale=1.75),
    "scale and translation": capi.similarity(scale=0.3, translation=(-2.0, 0.125, 0.7)),
    "quarter turn about z": capi.similarity(rotation=(1.0, 0.0, 0.0, 1.0)),
    "half turn about x": capi.similarity(rotation=(0.0, 2.0, 0.0, 0.0)),
    "general": capi.similarity(rotation=quat((0.3, -0.8, 0.52), 37.0), scale=1.75, translation=(0.5, -1.25, 3.0)),
    "unnormalised": capi.similarity(rotation=(3.0, -1.0, 2.5, 0.5), scale=0.6, translation=(0.0, 10.0, 0.0)),
    "tiny turn": capi.similarity(rotation=(1.0, 1.0e-4, 0.0, -2.0e-4)),
}


def test_the_new_entry_points_are_exported():
    L = capi.load()
    for name in NEW:
        assert hasattr(L, name) and name in capi.EXPORTS, name
    assert C.sizeof(capi.Similarity) == 8 * 4


@pytest.mark.parametrize("name", sorted(SIMILARITIES))
def test_record_rule_against_the_mirror(name):
    t = SIMILARITIES[name]
    cs, cc, sr = with_hard_records(*packed())
    got_cs, got_cc, got_sr, got_bound = capi.transform_records(cs, cc, sr, t, want_bound=True)
    want_cs, want_cc, want_sr, want_bound = record_mirror(cs, cc, sr, t)
    assert same_floats(got_cs, want_cs), np.flatnonzero((got_cs != want_cs).any(axis=1))[:8]
    assert np.array_equal(got_cc, want_cc), np.flatnonzero((got_cc != want_cc).any(axis=1))[:8]
    assert same_floats(got_sr, want_sr), np.flatnonzero((got_sr != want_sr).any(axis=1))[:8]
    assert same_floats(got_bound.view(U32), want_bound.view(U32)), np.flatnonzero(got_bound.view(U32) != want_bound.view(U32))[:8]
    # the hard records: the kept words keep their bits, the colour word always does
    for k in (3, 4, 5):
        assert got_cs[k, 3] == cs[k, 3] and np.array_equal(got_cc[k], cc[k])
    assert np.array_equal(got_cc[:, 3], cc[:, 3])


def test_one_record_at_a_time_and_in_place():
    t = SIMILARITIES["general"]
    cs, cc, sr = with_hard_records(*packed(300, 8))
    want = capi.transform_records(cs, cc, sr, t, want_bound=True)
    got = capi.transform_records(cs, cc, sr, t, want_bound=True, one_by_one=True)
    for a, b in zip(got, want):
        assert np.array_equal(a.view(U32), b.view(U32))
    L = capi.load()
    a, b, c = cs.copy(), cc.copy(), sr.copy()
    for i in range(len(a)):                                       # the outputs may be the inputs; bound_out is optional
        assert L.gs_transform_record(a.ctypes.data + 16 * i, b.ctypes.data + 16 * i, c.ctypes.data + 16 * i, C.byref(t),
                                     a.ctypes.data + 16 * i, b.ctypes.data + 16 * i, c.ctypes.data + 16 * i, None) == capi.GS_OK
    assert np.array_equal(a, want[0]) and np.array_equal(b, want[1]) and np.array_equal(c, want[2])


def test_exact_short_cuts():
    cs, cc, sr = packed()
    # the identity returns every input bit (finite positions)
    got = capi.transform_records(cs, cc, sr, SIMILARITIES["identity"])
    assert np.array_equal(got[0], cs) and np.array_equal(got[1], cc) and np.array_equal(got[2], sr)
    # a pure translation leaves cs[3], cc and sort_row[3] untouched
    got = capi.transform_records(cs, cc, sr, SIMILARITIES["translation"])
    assert np.array_equal(got[0][:, 3], cs[:, 3]) and np.array_equal(got[1], cc) and np.array_equal(got[2][:, 3], sr[:, 3])
    assert not np.array_equal(got[0][:, :3], cs[:, :3]) and np.array_equal(got[2][:, :3], got[0][:, :3])
    # a pure scale leaves cc untouched and gives cs'[3] = (float)(cs[3] * s^2)
    for name in ("scale", "scale and translation"):
        t = SIMILARITIES[name]
        s = float(t.scale)
        got = capi.transform_records(cs, cc, sr, t)
        assert np.array_equal(got[1], cc)
        assert np.array_equal(got[0][:, 3], (cs[:, 3].view(F32).astype(F64) * (s * s)).astype(F32).view(U32))
        assert np.array_equal(got[2][:, 3], (sr[:, 3].view(F32).astype(F64) * s).astype(F32).view(U32))


# ---------------------------------------------------------------- accuracy of the general case

def dequantised(cs, cc):
    """[n, 6] f64: the covariance entries a record stands for"""
    return np.stack(halves(cc), axis=1) * cs[:, 3].view(F32).astype(F64)[:, None]


def exact_cov(cs, cc, t):
    """[n, 6]: s^2 Rm A Rm^T in numpy f64 from the old record (matrix products, not the rule's order)"""
    R, s, _ = widened(t)
    m = R * np.array([[1, 1, -1], [1, 1, -1], [-1, -1, 1]], F64)
    d = dequantised(cs, cc)
    A = np.zeros((len(d), 3, 3))
    for k, (i, j) in enumerate(((0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2))):
        A[:, i, j] = A[:, j, i] = d[:, k]
    E = s * s * (m @ A @ m.T)
    return np.stack([E[:, i, j] for i, j in ((0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2))], axis=1)


@pytest.mark.parametrize("name", ["general", "unnormalised", "quarter turn about z", "tiny turn"])
def test_general_case_is_within_half_a_step(name):
    """Every dequantised entry of the new record lies within 0.51 cs'[3] of s^2 Rm A Rm^T: half a quantisation step of the rounding to
    nearest, plus 32767 * 2^-24 < 0.002 of a step for the f32 rounding of cs'[3] (an entry is at most 32767 steps), plus the f64
    roundings of the products (2^-50 of an entry: nothing)."""
    t = SIMILARITIES[name]
    cs, cc, sr = packed()
    got_cs, got_cc, _ = capi.transform_records(cs, cc, sr, t)
    step = got_cs[:, 3].view(F32).astype(F64)
    normal = np.isfinite(step) & (step >= float(np.finfo(F32).tiny))
    assert normal.sum() > 4000
    err = np.abs(dequantised(got_cs, got_cc) - exact_cov(cs, cc, t))[normal] / step[normal, None]
    assert err.max() <= 0.51, err.max()
    # ... and the rounding is to NEAREST: the signed error of the diagonal entries (positive numbers: a truncating quantiser leaves every one
    # of them short by half a step on average) averages to nothing.  Rounding errors are uniform in [-0.5, 0.5]: standard deviation
    # 1 / sqrt(12) each, 0.29 / sqrt(3 * 4000) = 0.0026 for the mean of these; 0.05 is nineteen of those, and a tenth of truncation's 0.5.
    signed = ((dequantised(got_cs, got_cc) - exact_cov(cs, cc, t))[normal] / step[normal, None])[:, [0, 3, 5]]
    largest = np.abs(np.stack(halves(got_cc), axis=1))[normal][:, [0, 3, 5]] == 32767     # (the entry that IS max_value has no error)
    assert abs(signed[~largest].mean()) < 0.05, signed[~largest].mean()


def test_five_hundred_rotations_do_not_drift():
    """500 successive random rotations of one record, then the inverse of their product: the trace of the covariance (a rotation leaves it
    alone) stays within 500 * 3 steps of cs[3] of its start."""
    g = np.random.Generator(np.random.PCG64(500))
    cs, cc, sr = packed(64, 11)
    k = int(np.argmax(np.abs(np.stack(halves(cc), axis=1)).min(axis=1)))       # a record with no zero entry
    cs, cc, sr = cs[k:k + 1].copy(), cc[k:k + 1].copy(), sr[k:k + 1].copy()
    step0 = float(cs[0, 3].view(F32))
    trace0 = dequantised(cs, cc)[0, [0, 3, 5]].sum()
    total = np.array([1.0, 0.0, 0.0, 0.0])

    def mul(a, b):
        return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                         a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])

    for _ in range(500):
        q = g.normal(size=4)
        q = (q / np.linalg.norm(q)).astype(F32).astype(F64)
        total = mul(q, total)
        total = total / np.linalg.norm(total)
        cs, cc, sr = capi.transform_records(cs, cc, sr, capi.similarity(rotation=q))
    back = capi.similarity(rotation=(total[0], -total[1], -total[2], -total[3]))
    cs, cc, sr = capi.transform_records(cs, cc, sr, back)
    trace = dequantised(cs, cc)[0, [0, 3, 5]].sum()
    assert abs(trace - trace0) <= 500 * 3 * step0, (trace, trace0, step0)


# ---------------------------------------------------------------- SH

def rotation_of(t):
    return widened(t)[0]


def random_similarity(g, scale=True):
    q = g.normal(size=4)
    return capi.similarity(rotation=q, scale=g.uniform(0.5, 2.0) if scale else 1.0, translation=g.uniform(-0.3, 0.3, size=3))


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_rotated_rows_show_the_rotated_camera_the_same_colour(degree):
    """THE property: gs_sh_eval_unrounded(sh', D, s R cam + t, s R pos + t) = gs_sh_eval_unrounded(sh, D, cam, pos) within 0.01 colour-byte
    units.  Each output coefficient is rounded to f32 (relative 2^-24), band norms are preserved (coefficients stay below sqrt(7) in size),
    at most 15 terms of |basis| < 1.5 are summed and the result is scaled by 255: below 1e-3.  The moved position is rounded to f32 as well
    (gs_sh_eval takes one): positions are kept within 0.5 of the origin and cameras at least 4 away, so that rounding turns the direction by
    less than 2^-24 / 4, another 1e-5 units."""
    K = (degree + 1) ** 2
    g = np.random.Generator(np.random.PCG64(700 + degree))
    rows = g.uniform(-1.0, 1.0, size=(24, 3 * K)).astype(F32)
    worst = 0.0
    for _ in range(12):
        t = random_similarity(g)
        R, s, tr = widened(t)
        moved = capi.transform_sh_rows(rows, degree, t)
        for i in range(len(rows)):
            pos = g.uniform(-0.25, 0.25, size=3).astype(F32)
            d = g.normal(size=3)
            cam = pos.astype(F64) + d / np.linalg.norm(d) * g.uniform(4.0, 9.0)
            pos2 = (s * (R @ pos.astype(F64)) + tr).astype(F32)
            cam2 = s * (R @ cam) + tr
            want = np.asarray(capi.sh_eval(rows[i], degree, cam, pos, unrounded=True))
            got = np.asarray(capi.sh_eval(moved[i], degree, cam2, pos2, unrounded=True))
            worst = max(worst, float(np.abs(got - want).max()))
    assert worst <= 0.01, worst


def test_band_matrices_are_orthogonal_and_compose():
    g = np.random.Generator(np.random.PCG64(710))
    for _ in range(20):
        for D in capi.sh_rotation(random_similarity(g)):
            assert np.abs(D @ D.T - np.eye(len(D))).max() <= 1e-10
    # D(R1 R2) = D(R1) D(R2): quaternions of small integers, whose product is exact in f32 (the rule normalises in f64)
    def mul(a, b):
        return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0])
    for _ in range(20):
        q1, q2 = [tuple(int(v) for v in g.integers(-9, 10, size=4)) for _ in range(2)]
        if not any(q1) or not any(q2):
            continue
        both = capi.sh_rotation(capi.similarity(rotation=mul(q1, q2)))
        for D12, D1, D2 in zip(both, capi.sh_rotation(capi.similarity(rotation=q1)), capi.sh_rotation(capi.similarity(rotation=q2))):
            assert np.abs(D12 - D1 @ D2).max() <= 1e-10
    # band 1 is the rotation itself in the basis (-y, z, -x)
    t = random_similarity(g)
    P = np.array([[0, -1.0, 0], [0, 0, 1.0], [-1.0, 0, 0]])
    assert np.abs(capi.sh_rotation(t)[0] - P @ rotation_of(t) @ P.T).max() <= 1e-12


def test_identity_rotation_is_exact():
    for t in (SIMILARITIES["identity"], SIMILARITIES["scale and translation"]):
        for D in capi.sh_rotation(t):
            assert np.array_equal(D, np.eye(len(D))) and not np.signbit(D).any()
        for degree in (0, 1, 2, 3):
            g = np.random.Generator(np.random.PCG64(720 + degree))
            rows = g.uniform(-1.0, 1.0, size=(65, 3 * (degree + 1) ** 2)).astype(F32)
            assert np.array_equal(capi.transform_sh_rows(rows, degree, t).view(U32), rows.view(U32))


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_sh_rule_against_the_mirror_and_in_place(degree):
    """sh'[c][k0 + i] = f32(sum_j D_l[i][j] sh[c][k0 + j]), ascending j, left to right, from the matrices gs_sh_rotation returns"""
    K = (degree + 1) ** 2
    g = np.random.Generator(np.random.PCG64(730 + degree))
    rows = g.uniform(-1.0, 1.0, size=(129, 3 * K)).astype(F32)
    t = SIMILARITIES["general"]
    Ds = capi.sh_rotation(t)
    src = rows.reshape(-1, 3, K).astype(F64)
    want = src.copy()
    for l in range(1, degree + 1):
        k0, w, D = l * l, 2 * l + 1, Ds[l - 1]
        for i in range(w):
            acc = D[i, 0] * src[:, :, k0]
            for j in range(1, w):
                acc = acc + D[i, j] * src[:, :, k0 + j]
            want[:, :, k0 + i] = acc
    want = want.astype(F32).reshape(-1, 3 * K)
    got = capi.transform_sh_rows(rows, degree, t)
    assert np.array_equal(got.view(U32), want.view(U32))
    assert np.array_equal(got[:, ::K].view(U32), rows[:, ::K].view(U32))              # k = 0 is unchanged
    aliased = rows.copy()
    assert capi.transform_sh_rows(aliased, degree, t, in_place=True) is aliased              # out_row == sh_row
    assert np.array_equal(aliased.view(U32), want.view(U32))


# ---------------------------------------------------------------- the other host entry points

def test_similarity_about_a_pivot():
    g = np.random.Generator(np.random.PCG64(740))
    for _ in range(50):
        pivot, q, s = g.uniform(-5, 5, size=3).astype(F32), g.normal(size=4).astype(F32), F32(g.uniform(0.25, 4.0))
        t = capi.similarity_about(pivot, q, s)
        assert np.array_equal(np.array(list(t.rotation), F32), q) and F32(t.scale) == s
        R, sd, _ = widened(capi.similarity(rotation=q, scale=s))
        p = pivot.astype(F64)
        want = [F32(p[i] - sd * ((R[i, 0] * p[0] + R[i, 1] * p[1]) + R[i, 2] * p[2])) for i in range(3)]
        assert np.array_equal(np.array(list(t.translation), F32).view(U32), np.array(want, F32).view(U32))
        # the pivot stays where it is, up to the f32 roundings of the translation (at most |pivot| + s |pivot| in size, |pivot| < 10) and of
        # the moved position: half an ulp each, 2^-24 relative
        cs = np.array([[pivot[0], pivot[1], -pivot[2], 0.0]], F32).view(U32)
        out = capi.transform_records(cs, np.zeros((1, 4), U32), cs, t)[0].view(F32)[0, :3] * np.array([1, 1, -1], F32)
        assert np.abs(out.astype(F64) - p).max() <= (2 + float(s)) * 10 * 2.0 ** -24


def test_bad_arguments():
    L = capi.load()
    p = capi._p
    good = capi.similarity()
    cs, cc, sr = np.zeros(4, F32), np.zeros(4, U32), np.zeros(4, F32)
    o1, o2, o3, b = np.zeros(4, F32), np.zeros(4, U32), np.zeros(4, F32), np.zeros(1, F32)
    row, out, mats = np.zeros(48, F32), np.zeros(48, F32), np.zeros(83, F64)
    piv, q = np.zeros(3, F32), np.array([1, 0, 0, 0], F32)
    sim = capi.Similarity()
    record = lambda t, a=(cs, cc, sr, o1, o2, o3): L.gs_transform_record(p(a[0]), p(a[1]), p(a[2]), t, p(a[3]), p(a[4]), p(a[5]), p(b))
    assert record(C.byref(good)) == capi.GS_OK
    assert L.gs_transform_record(p(cs), p(cc), p(sr), C.byref(good), p(o1), p(o2), p(o3), None) == capi.GS_OK      # bound_out is optional
    assert record(None) == capi.E_BADARG
    for k in range(6):
        a = [cs, cc, sr, o1, o2, o3]
        a[k] = None
        assert record(C.byref(good), a) == capi.E_BADARG, k
    assert L.gs_transform_records(p(cs), p(cc), p(sr), 1, None, p(o1), p(o2), p(o3), None) == capi.E_BADARG
    assert L.gs_transform_records(None, p(cc), p(sr), 1, C.byref(good), p(o1), p(o2), p(o3), None) == capi.E_BADARG
    assert L.gs_transform_records(None, None, None, 0, C.byref(good), None, None, None, None) == capi.GS_OK
    assert L.gs_transform_sh_row(p(row), 3, C.byref(good), p(out)) == capi.GS_OK
    assert L.gs_transform_sh_row(None, 3, C.byref(good), p(out)) == capi.E_BADARG
    assert L.gs_transform_sh_row(p(row), 3, None, p(out)) == capi.E_BADARG
    assert L.gs_transform_sh_row(p(row), 3, C.byref(good), None) == capi.E_BADARG
    assert L.gs_transform_sh_row(p(row), 4, C.byref(good), p(out)) == capi.E_BADARG
    assert L.gs_transform_sh_row(p(row), -1, C.byref(good), p(out)) == capi.E_BADARG
    assert L.gs_sh_rotation(C.byref(good), p(mats)) == capi.GS_OK
    assert L.gs_sh_rotation(None, p(mats)) == capi.E_BADARG
    assert L.gs_sh_rotation(C.byref(good), None) == capi.E_BADARG
    assert L.gs_similarity_about(p(piv), p(q), 1.0, C.byref(sim)) == capi.GS_OK
    assert L.gs_similarity_about(None, p(q), 1.0, C.byref(sim)) == capi.E_BADARG
    assert L.gs_similarity_about(p(piv), None, 1.0, C.byref(sim)) == capi.E_BADARG
    assert L.gs_similarity_about(p(piv), p(q), 1.0, None) == capi.E_BADARG
    assert L.gs_similarity_about(p(piv), p(q), 0.0, C.byref(sim)) == capi.E_BADARG
    assert L.gs_similarity_about(p(piv), p(np.zeros(4, F32)), 1.0, C.byref(sim)) == capi.E_BADARG
    assert L.gs_similarity_about(p(np.array([0, np.inf, 0], F32)), p(q), 1.0, C.byref(sim)) == capi.E_BADARG

    def refused(t):
        return (record(C.byref(t)) == capi.E_BADARG and L.gs_transform_sh_row(p(row), 3, C.byref(t), p(out)) == capi.E_BADARG and
                L.gs_sh_rotation(C.byref(t), p(mats)) == capi.E_BADARG and
                L.gs_transform_records(p(cs), p(cc), p(sr), 1, C.byref(t), p(o1), p(o2), p(o3), None) == capi.E_BADARG)

    for bad in (np.nan, np.inf, -np.inf):                         # a parameter that is not finite
        for member in range(8):
            t = capi.similarity()
            C.cast(C.byref(t), C.POINTER(C.c_float))[member] = bad
            assert refused(t), (bad, member)
    for scale in (0.0, -0.0, -1.0):                               # scale <= 0
        assert refused(capi.similarity(scale=scale)), scale
    assert refused(capi.similarity(rotation=(0.0, 0.0, 0.0, 0.0)))           # a quaternion of norm 0
    assert refused(capi.similarity(rotation=(-0.0, 0.0, -0.0, 0.0)))
    assert not refused(capi.similarity(rotation=(0.0, 0.0, 1.0e-45, 0.0)))   # the smallest subnormal is a direction
    assert L.gs_transform(None, C.byref(good), 0, 0, None) == capi.E_BADARG
    assert L.gs_multi_transform(None, C.byref(good), 0, 0, None) == capi.E_BADARG
