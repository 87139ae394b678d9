"""CPU tier of the export (include/gs_splat.h: gs_export_row, gs_splat_to_ply): the kernel's own function, compiled for the host, against a
numpy mirror of the rule the header spells out -- bit for bit --, what a row loses on its way through the packed record and back, measured
against what the reference's format loses by itself, and the .ply writer against the project's own loaders.  No GPU anywhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg
from test_host_check import _p, hc  # noqa: F401  (the host build of gs_device_math.h: pack_row, shared)

capi = pkg("capi")

NEW = ["gs_export_row", "gs_export_splat", "gs_export_sh", "gs_splat_to_ply", "gs_export_ply", "gs_multi_export_splat", "gs_multi_export_ply"]
N = 4096
# the degenerate rows of the cloud
ZERO, INF, TRIPLE, DOUBLE, IDENT = 5, 6, 7, 8, 9
DEGENERATE = [ZERO, INF]
SH_C0 = 0.28209479177387814


# ---------------------------------------------------------------- the cloud

def quat_bytes(q):
    """processPlyBuffer's rule (index.js:704-707): clamped_u8((q / |q|) * 128 + 128), ties to even"""
    q = np.asarray(q, np.float64)
    v = (q / np.sqrt((q * q).sum(axis=1))[:, None]) * 128 + 128
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def make_cloud():
    """-> (rows uint8[N, 32], unit quaternions f64[N, 4] as stored (w, x, y, z), scales f32[N, 3])"""
    g = np.random.Generator(np.random.PCG64(20261020))
    pos = (g.normal(size=(N, 3)) * 2.0).astype(np.float32)
    pos[:, 0] = (np.arange(N) * 0.001953125 - 4.0).astype(np.float32)         # unique positions (multiples of 2^-9: exact)
    base = np.exp(g.normal(size=(N, 1)) * 1.0 - 3.0)
    aniso = np.exp(g.uniform(np.log(0.005), 0.0, size=(N, 3)))                 # axis ratios down to 1 : 200 (asserted: beyond 1 : 100)
    scale = (base * aniso).astype(np.float32)
    q = g.normal(size=(N, 4))
    q /= np.sqrt((q * q).sum(axis=1))[:, None]
    rgba = np.stack([(np.arange(N) * 7) % 256, (np.arange(N) * 13 + 5) % 256, (np.arange(N) * 29 + 11) % 256, np.arange(N) % 256], axis=1).astype(np.uint8)
    scale[ZERO] = 0.0
    scale[INF] = (0.01, np.inf, 0.02)
    scale[TRIPLE] = 0.25
    scale[DOUBLE] = (0.5, 0.5, 0.03125)
    q[IDENT] = (1.0, 0.0, 0.0, 0.0)
    rows = np.zeros((N, 32), np.uint8)
    rows[:, 0:12] = pos.view(np.uint8).reshape(N, 12)
    rows[:, 12:24] = scale.view(np.uint8).reshape(N, 12)
    rows[:, 24:28] = rgba
    rows[:, 28:32] = quat_bytes(q)
    return rows, q, scale


def pack(hc, rows):
    rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, 32)
    n = len(rows)
    cs = np.zeros((n, 4), np.float32); cc = np.zeros((n, 4), np.uint32); sr = np.zeros((n, 4), np.float32)
    hc.hc_pack(_p(rows), n, _p(cs), _p(cc), _p(sr))
    return cs, cc, sr


@pytest.fixture(scope="module")
def cloud(hc):
    rows, q, scale = make_cloud()
    cs, cc, sr = pack(hc, rows)
    out, wide = capi.export_row(cs, cc, want_wide=True)
    return {"rows": rows, "q": q, "scale": scale, "cs": cs, "cc": cc, "sr": sr, "out": out, "wide": wide}


# ---------------------------------------------------------------- the header's rule in numpy

def _i16(half):
    return half.astype(np.uint16).view(np.int16).astype(np.float64)


def entries(cs, cc):
    """the six covariance entries of packed records (a00, a01, a02, a11, a12, a22), f64"""
    s = cs[:, 3].astype(np.float64)
    lo, hi = (lambda w: _i16(w & np.uint32(0xFFFF))), (lambda w: _i16(w >> np.uint32(16)))
    with np.errstate(all="ignore"):
        return [lo(cc[:, 0]) * s, hi(cc[:, 0]) * s, lo(cc[:, 1]) * s, hi(cc[:, 1]) * s, lo(cc[:, 2]) * s, hi(cc[:, 2]) * s]


def _jacobi(app, aqq, apq, arp, arq, vp, vq):
    """one rotation of the header's rule on arrays; vp, vq: lists of the three rows' entries of columns p and q"""
    m = apq != 0.0
    theta = (aqq - app) / (apq + apq)
    root = np.sqrt(theta * theta + 1.0)
    t = np.where(theta >= 0.0, 1.0 / (theta + root), -1.0 / (root - theta))
    c = 1.0 / np.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    w = lambda new, old: np.where(m, new, old)
    out_v = []
    for a, b in zip(vp, vq):
        out_v.append((w(c * a - s * b, a), w(s * a + c * b, b)))
    return (w(app - h, app), w(aqq + h, aqq), w(0.0, apq), w(c * arp - s * arq, arp), w(s * arp + c * arq, arq),
            [x[0] for x in out_v], [x[1] for x in out_v])


def _clamped_u8(v):
    return np.clip(np.rint(v), 0, 255).astype(np.uint32)


def export_mirror(cs, cc):
    """-> (rows uint8[n, 32], wide float32[n, 7]) by include/gs_splat.h's rule, every operation f64 and in the stated order"""
    cs = np.ascontiguousarray(cs, np.float32).reshape(-1, 4)
    cc = np.ascontiguousarray(cc, np.uint32).reshape(-1, 4)
    n = len(cs)
    w = np.zeros((n, 8), np.uint32)
    w[:, 0] = cs[:, 0].view(np.uint32); w[:, 1] = cs[:, 1].view(np.uint32); w[:, 2] = (-cs[:, 2]).view(np.uint32)
    w[:, 6] = cc[:, 3]
    sb = np.ascontiguousarray(cs[:, 3]).view(np.uint32)
    finite = (sb & np.uint32(0x7F800000)) != np.uint32(0x7F800000)
    empty = ((cc[:, 0] | cc[:, 1] | cc[:, 2]) == 0) | ((sb & np.uint32(0x7FFFFFFF)) == 0)
    live = finite & ~empty
    with np.errstate(all="ignore"):
        a00, a01, a02, a11, a12, a22 = entries(cs, cc)
        one, zero = np.ones(n), np.zeros(n)
        v = [[one.copy(), zero.copy(), zero.copy()], [zero.copy(), one.copy(), zero.copy()], [zero.copy(), zero.copy(), one.copy()]]   # v[row][col]
        col = lambda k: [v[0][k], v[1][k], v[2][k]]

        def put(k, c):
            v[0][k], v[1][k], v[2][k] = c

        for _ in range(8):
            a00, a11, a01, a02, a12, c0, c1 = _jacobi(a00, a11, a01, a02, a12, col(0), col(1)); put(0, c0); put(1, c1)
            a00, a22, a02, a01, a12, c0, c2 = _jacobi(a00, a22, a02, a01, a12, col(0), col(2)); put(0, c0); put(2, c2)
            a11, a22, a12, a01, a02, c1, c2 = _jacobi(a11, a22, a12, a01, a02, col(1), col(2)); put(1, c1); put(2, c2)
        l = [np.where(a00 > 0.0, a00, 0.0), np.where(a11 > 0.0, a11, 0.0), np.where(a22 > 0.0, a22, 0.0)]
        for p, q in ((0, 1), (1, 2), (0, 1)):
            sw = l[p] < l[q]
            l[p], l[q] = np.where(sw, l[q], l[p]), np.where(sw, l[p], l[q])
            cp, cq = col(p), col(q)
            put(p, [np.where(sw, b, a) for a, b in zip(cp, cq)])
            put(q, [np.where(sw, a, b) for a, b in zip(cp, cq)])
        (v00, v01, v02), (v10, v11, v12), (v20, v21, v22) = v
        det = (v00 * (v11 * v22 - v12 * v21) - v01 * (v10 * v22 - v12 * v20)) + v02 * (v10 * v21 - v11 * v20)
        ng = det < 0.0
        v02, v12, v22 = np.where(ng, -v02, v02), np.where(ng, -v12, v12), np.where(ng, -v22, v22)
        sc = [np.sqrt(x).astype(np.float32) for x in l]
        r00, r01, r02, r10, r11, r12, r20, r21, r22 = v00, v10, v20, v01, v11, v21, v02, v12, v22
        tr = (r00 + r11) + r22
        b0 = (tr >= r00) & (tr >= r11) & (tr >= r22)
        b1 = ~b0 & (r00 >= r11) & (r00 >= r22)
        b2 = ~b0 & ~b1 & (r11 >= r22)
        S0 = np.sqrt(tr + 1.0) * 2.0
        S1 = np.sqrt(((1.0 + r00) - r11) - r22) * 2.0
        S2 = np.sqrt(((1.0 + r11) - r00) - r22) * 2.0
        S3 = np.sqrt(((1.0 + r22) - r00) - r11) * 2.0
        pick = lambda x0, x1, x2, x3: np.where(b0, x0, np.where(b1, x1, np.where(b2, x2, x3)))
        qw = pick(S0 / 4.0, (r21 - r12) / S1, (r02 - r20) / S2, (r10 - r01) / S3)
        qx = pick((r21 - r12) / S0, S1 / 4.0, (r01 + r10) / S2, (r02 + r20) / S3)
        qy = pick((r02 - r20) / S0, (r01 + r10) / S1, S2 / 4.0, (r12 + r21) / S3)
        qz = pick((r10 - r01) / S0, (r02 + r20) / S1, (r12 + r21) / S2, S3 / 4.0)
        neg = (qw < 0.0) | ((qw == 0.0) & ((qx < 0.0) | ((qx == 0.0) & ((qy < 0.0) | ((qy == 0.0) & (qz < 0.0))))))
        qw, qx, qy, qz = [np.where(neg, -x, x) for x in (qw, qx, qy, qz)]
        qz = -qz
        # the degenerate records
        sc = [np.where(live, x, np.where(finite, np.float32(0.0), cs[:, 3])).astype(np.float32) for x in sc]
        qw, qx, qy, qz = np.where(live, qw, 1.0), np.where(live, qx, 0.0), np.where(live, qy, 0.0), np.where(live, qz, 0.0)
        for k in range(3):
            w[:, 3 + k] = np.ascontiguousarray(sc[k]).view(np.uint32)
        w[:, 7] = (_clamped_u8(qw * 128.0 + 128.0) | (_clamped_u8(qx * 128.0 + 128.0) << np.uint32(8)) |
                   (_clamped_u8(qy * 128.0 + 128.0) << np.uint32(16)) | (_clamped_u8(qz * 128.0 + 128.0) << np.uint32(24)))
        wide = np.stack(sc + [qw.astype(np.float32), qx.astype(np.float32), qy.astype(np.float32), qz.astype(np.float32)], axis=1)
    return np.ascontiguousarray(w).view(np.uint8).reshape(n, 32), np.ascontiguousarray(wide, np.float32)


def covariance(q, scale):
    """pack's construction (index.js:343-369) in exact-as-f64 arithmetic from a stored quaternion (w, x, y, z) and three scales:
    R^T diag(s^2) R, the six entries in the record's layout"""
    qw, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], -q[:, 3]
    x2, y2, z2 = qx + qx, qy + qy, qz + qz
    xx, xy, xz, yy, yz, zz, wx, wy, wz = qx * x2, qx * y2, qx * z2, qy * y2, qy * z2, qz * z2, qw * x2, qw * y2, qw * z2
    R = np.array([[1 - (yy + zz), xy - wz, xz + wy], [xy + wz, 1 - (xx + zz), yz - wx], [xz - wy, yz + wx, 1 - (xx + yy)]])   # R[row][col][n]
    M = np.einsum("kin,nk->ikn", R, scale.astype(np.float64))       # M = R^T diag(s)
    S = np.einsum("ikn,jkn->ijn", M, M)
    return np.stack([S[0, 0], S[1, 0], S[2, 0], S[1, 1], S[2, 1], S[2, 2]], axis=1)


def frob(e):
    """Frobenius norm of symmetric matrices given by their six entries (off-diagonal ones count twice)"""
    wgt = np.array([1.0, 2.0, 2.0, 1.0, 2.0, 1.0])
    return np.sqrt((e * e * wgt).sum(axis=1))


# ---------------------------------------------------------------- binding and header

def test_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "gs_splat.h")).read()
    L = capi.load()
    for name in NEW:
        assert re.search(r"GS_API\s+int\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in capi.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name
    for name in ("export_splat", "export_sh", "export_ply"):
        assert hasattr(capi.Context, name), name
    assert hasattr(capi.Multi, "export_splat") and hasattr(capi.Multi, "export_ply")
    assert hdr.index("gs_export_row") > hdr.index("GS_API int gs_contrib_info(")      # appended: every older declaration keeps its place
    assert capi.OF_FILTERS == {"all": (0, 0), "visible": (capi.STATE_HIDDEN, 0), "selected": (3, capi.STATE_SELECTED)}


def test_the_cloud_is_what_the_issue_asks_for(cloud):
    s = cloud["scale"][10:]
    assert (s.max(axis=1) / s.min(axis=1)).max() >= 100.0
    for k in range(4):
        assert np.unique(cloud["rows"][:, 24 + k]).size == 256
    assert np.unique(cloud["rows"][:, 0:12].view(np.float32), axis=0).shape[0] == N
    assert tuple(cloud["rows"][IDENT, 28:32]) == (255, 128, 128, 128)


# ---------------------------------------------------------------- gs_export_row against the rule

def test_export_row_equals_the_mirror_on_the_cloud(cloud):
    rows, wide = export_mirror(cloud["cs"], cloud["cc"])
    bad = np.flatnonzero((rows != cloud["out"]).any(axis=1))
    assert bad.size == 0, (bad[:8], rows[bad[:2]], cloud["out"][bad[:2]])
    assert np.array_equal(wide.view(np.uint32), cloud["wide"].view(np.uint32))


def hand_made_records():
    """entries at the int16 limits, diagonal and rank-one matrices, exact ties, negative-definite and indefinite ones, x a cs[3] of 0, -0,
    denormals, huge, Inf and NaN values"""
    q = lambda v: np.uint32(np.int16(v).view(np.uint16))
    mats = [(32767, 0, 0, 32767, 0, 32767), (32767, 0, 0, 1, 0, 0), (1, 1, 1, 1, 1, 1), (32767, 32767, 32767, 32767, 32767, 32767),
            (5, 0, 0, 7, 0, 7), (7, 0, 0, 7, 0, 5), (3, 0, 0, 9, 0, 6), (0, 32767, 0, 0, 0, 0), (0, 0, 0, 0, 0, 1), (-32768, 0, 0, -1, 0, -5),
            (100, -32768, 50, 200, -7, 300), (32767, 1, 0, 32767, 0, 32767), (1, 0, 32767, 2, 0, 1), (0, 0, 0, 0, 0, 0), (10, 3, 0, 10, 0, 2),
            (2, 0, 0, 2, 2, 2), (900, -30, 12, 1, 0, 32767)]
    scales = np.array([0.0, -0.0, 1e-45, 1e-39, 1e-20, 3.0517578e-05, 1.0, 7.25, 1e30, 3.4e38, np.inf, -np.inf, np.nan], np.float32)
    scales = np.concatenate([scales, np.array([0xFFC00000, 0x7FC12345, 0x7F800001], np.uint32).view(np.float32)])
    cs, cc = [], []
    k = 0
    for m in mats:
        for s in scales:
            cs.append((1.5 + k, -2.75e-3, -0.0 if k % 2 else 4.0, s))
            cc.append((q(m[0]) | (q(m[1]) << np.uint32(16)), q(m[2]) | (q(m[3]) << np.uint32(16)), q(m[4]) | (q(m[5]) << np.uint32(16)),
                       np.uint32((k * 2654435761) & 0xFFFFFFFF)))
            k += 1
    return np.array(cs, np.float32), np.array(cc, np.uint32)


def test_export_row_equals_the_mirror_on_hand_made_records():
    cs, cc = hand_made_records()
    got, gw = capi.export_row(cs, cc, want_wide=True)
    want, ww = export_mirror(cs, cc)
    bad = np.flatnonzero((got != want).any(axis=1) | (gw.view(np.uint32) != ww.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (bad[:8], cs[bad[:2]], cc[bad[:2]], got[bad[:2]], want[bad[:2]])
    sc = got[:, 12:24].view(np.float32)
    assert np.isnan(sc).any() and np.isinf(sc).any() and (sc == 0).any() and (sc[np.isfinite(sc)] > 1e15).any()
    assert (np.nan_to_num(sc[:, 0], nan=0.0) >= np.nan_to_num(sc[:, 1], nan=0.0)).all() and (np.nan_to_num(sc[:, 1], nan=0.0) >= np.nan_to_num(sc[:, 2], nan=0.0)).all()


def test_degenerate_records_come_out_as_specified(cloud):
    out = cloud["out"]
    ident = (255, 128, 128, 128)
    assert tuple(out[ZERO, 28:32]) == ident and (out[ZERO, 12:24].view(np.float32) == 0).all()
    assert cloud["cs"][ZERO, 3] == 0 and np.isinf(cloud["cs"][INF, 3])
    assert tuple(out[INF, 28:32]) == ident and np.isinf(out[INF, 12:24].view(np.float32)).all()
    assert np.array_equal(cloud["wide"][INF], np.array([np.inf, np.inf, np.inf, 1, 0, 0, 0], np.float32))
    # a NaN cs[3] of either sign comes back as the scale, bit for bit
    for bits in (0x7FC00000, 0xFFC00000, 0x7FC12345):
        cs = np.array([1, 2, 3, 0], np.float32); cs.view(np.uint32)[3] = bits
        row, wide = capi.export_row(cs, np.array([1, 2, 3, 4], np.uint32), want_wide=True)
        assert (row[0, 12:24].view(np.uint32) == bits).all() and tuple(row[0, 28:32]) == ident and (wide[0, :3].view(np.uint32) == bits).all()
    # equal scales: the matrix is a multiple of the identity up to the rounding of the quaternion bytes -- any rotation serves (the loss
    # test counts these rows like the others); the scales come back
    t = out[TRIPLE, 12:24].view(np.float32)
    assert np.allclose(t, 0.25, rtol=0.02)
    d = out[DOUBLE, 12:24].view(np.float32)
    assert np.allclose(d[:2], 0.5, rtol=0.02) and np.isclose(d[2], 0.03125, rtol=0.1)
    assert tuple(out[IDENT, 28:32]) == ident
    assert np.allclose(np.sort(out[IDENT, 12:24].view(np.float32)), np.sort(cloud["scale"][IDENT]), rtol=2e-3)


def test_export_row_refuses_null_pointers():
    L = capi.load()
    cs, cc, row = (C.c_float * 4)(), (C.c_uint32 * 4)(), (C.c_uint8 * 32)()
    assert L.gs_export_row(cs, cc, row, None) == capi.GS_OK and bytes(row)[28:32] == bytes([255, 128, 128, 128])
    assert L.gs_export_row(None, cc, row, None) == capi.E_BADARG
    assert L.gs_export_row(cs, None, row, None) == capi.E_BADARG
    assert L.gs_export_row(cs, cc, None, None) == capi.E_BADARG
    n = C.c_size_t(0)
    assert L.gs_export_splat(None, 0, 0, None, None, None, C.byref(n)) == capi.E_BADARG
    assert L.gs_export_sh(None, 0, 0, None, C.byref(n), None) == capi.E_BADARG
    assert L.gs_export_ply(None, 0, 0, 0, None, C.byref(n)) == capi.E_BADARG
    assert L.gs_multi_export_splat(None, 0, 0, None, None, None, C.byref(n)) == capi.E_BADARG
    assert L.gs_multi_export_ply(None, 0, 0, 0, None, C.byref(n)) == capi.E_BADARG


# ---------------------------------------------------------------- through the record and back

def test_repacking_gives_back_position_colour_and_sort_row(hc, cloud):
    cs, cc, sr = pack(hc, cloud["out"])
    assert np.array_equal(cs[:, :3].view(np.uint32), cloud["cs"][:, :3].view(np.uint32))
    assert np.array_equal(cc[:, 3], cloud["cc"][:, 3])
    assert np.array_equal(sr[:, :3].view(np.uint32), cloud["sr"][:, :3].view(np.uint32))
    assert np.array_equal(cloud["out"][:, :12], cloud["rows"][:, :12]) and np.array_equal(cloud["out"][:, 24:28], cloud["rows"][:, 24:28])


def test_loss_is_what_the_format_itself_loses(hc, cloud):
    """e = |Sigma_repacked - Sigma_resident|_F / |Sigma_resident|_F over the non-degenerate rows, against e_ref: the resident covariance
    against the exact f64 R^T diag(s^2) R of the unit quaternion and scales the cloud was generated from -- what the reference's own
    format (8-bit quaternion bytes, index.js:704-707, and int16 entries) costs the same splats.  Required: median(e) <= 1.5 median(e_ref)
    and max(e) <= 1.5 max(e_ref).  Measured: docs/LAB_NOTES.md 9n."""
    keep = np.ones(N, bool); keep[DEGENERATE] = False
    resident = np.stack(entries(cloud["cs"], cloud["cc"]), axis=1)[keep]
    cs2, cc2, _ = pack(hc, cloud["out"])
    repacked = np.stack(entries(cs2, cc2), axis=1)[keep]
    exact = covariance(cloud["q"], cloud["scale"])[keep]
    e = frob(repacked - resident) / frob(resident)
    e_ref = frob(resident - exact) / frob(exact)
    print("export loss: median %.4f %% p99 %.4f %% max %.4f %%   format loss: median %.4f %% p99 %.4f %% max %.4f %%" % (
        100 * np.median(e), 100 * np.percentile(e, 99), 100 * e.max(), 100 * np.median(e_ref), 100 * np.percentile(e_ref, 99), 100 * e_ref.max()))
    assert np.isfinite(e).all() and np.isfinite(e_ref).all()
    assert np.median(e) <= 1.5 * np.median(e_ref)
    assert e.max() <= 1.5 * e_ref.max()


# ---------------------------------------------------------------- gs_splat_to_ply -> the loaders

def by_position(rows):
    """row index by position bits (positions are unique in every cloud here)"""
    return {bytes(r[:12]): i for i, r in enumerate(np.asarray(rows, np.uint8).reshape(-1, 32))}


@pytest.mark.parametrize("with_wide", [True, False])
def test_ply_comes_back_through_the_loader(cloud, with_wide):
    rows = cloud["out"]
    ply = capi.splat_to_ply(rows, cloud["wide"] if with_wide else None)
    assert bytes(ply[:4]) == b"ply\n" and b"element vertex %d\n" % N in bytes(ply[:200])
    back = capi.ply_to_splat(ply).reshape(-1, 32)
    assert len(back) == N
    where = by_position(back)
    assert len(where) == N
    order = np.array([where[bytes(r[:12])] for r in rows])             # (a KeyError: position bits differ)
    got = back[order]
    assert np.array_equal(got[:, 24:28], rows[:, 24:28])
    for k in range(4):
        assert np.unique(got[:, 24 + k]).size == 256                   # every byte value 0..255, in every channel
    s0, s1 = rows[:, 12:24].view(np.float32).astype(np.float64), got[:, 12:24].view(np.float32).astype(np.float64)
    fin = np.isfinite(s0) & (s0 > 0)
    assert np.array_equal(s0[~fin], s1[~fin])                          # 0 and +inf come back as they are
    assert (s0[fin] >= np.exp(-16.0)).all() and (s0[fin] <= np.exp(16.0)).all()
    assert (np.abs(s1[fin] - s0[fin]) <= 1e-6 * s0[fin]).all(), np.abs(s1[fin] / s0[fin] - 1).max()
    assert np.abs(got[:, 28:32].astype(int) - rows[:, 28:32].astype(int)).max() <= 1


def test_every_colour_and_alpha_byte_comes_back():
    rows = np.zeros((256, 32), np.uint8)
    rows[:, 0:4] = np.arange(256, dtype=np.float32).view(np.uint8).reshape(256, 4)
    rows[:, 12:24] = np.full((256, 3), 0.125, np.float32).view(np.uint8).reshape(256, 12)
    for k in range(4):
        rows[:, 24 + k] = np.arange(256)
    rows[:, 28:32] = (255, 128, 128, 128)
    back = capi.ply_to_splat(capi.splat_to_ply(rows)).reshape(-1, 32)
    where = by_position(back)
    got = back[[where[bytes(r[:12])] for r in rows]]
    assert np.array_equal(got[:, 24:28], rows[:, 24:28])
    assert np.array_equal(got[:, 12:24], rows[:, 12:24]) and np.array_equal(got[:, 28:32], rows[:, 28:32])


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_sh_rows_come_back_bit_for_bit(cloud, degree):
    n, n_sh, K = 300, 200, (degree + 1) ** 2
    rows = cloud["out"][10:10 + n]
    g = np.random.Generator(np.random.PCG64(degree))
    sh = g.normal(size=(n_sh, 3 * K)).astype(np.float32)
    ply = capi.splat_to_ply(rows, cloud["wide"][10:10 + n], sh, degree)
    back = capi.ply_to_splat(ply).reshape(-1, 32)
    got, d = capi.ply_sh(ply, 3)
    assert d == degree and got.shape == (n, 3 * K)
    src = by_position(rows)
    idx = np.array([src[bytes(r[:12])] for r in back])                 # loader row j is input row idx[j]
    has = idx < n_sh
    assert has.sum() == n_sh
    assert np.array_equal(got[has].view(np.uint32), sh[idx[has]].view(np.uint32))
    # the rows without coefficients: the colour byte's own f_dc, zeros behind it
    rest = got[~has].reshape(-1, 3, K)
    assert (rest[:, :, 1:] == 0).all()
    want_dc = ((rows[idx[~has], 24:27].astype(np.float64) / 255.0 - 0.5) / SH_C0).astype(np.float32)
    assert np.array_equal(rest[:, :, 0], want_dc)
    # ... and a lower degree asked of the file gives the leading bands
    low, dl = capi.ply_sh(ply, degree - 1)
    Kl = degree ** 2
    assert dl == degree - 1 and np.array_equal(low.reshape(n, 3, Kl), got.reshape(n, 3, K)[:, :, :Kl])
    # the colour bytes of the rows with coefficients come from their f_dc
    dc = sh[idx[has]].reshape(-1, 3, K)[:, :, 0].astype(np.float64)
    assert np.array_equal(back[has, 24:27], np.clip(np.rint((0.5 + SH_C0 * dc) * 255), 0, 255).astype(np.uint8))


def test_an_empty_file_is_a_header_the_loader_accepts():
    for degree in (0, 2):
        ply = capi.splat_to_ply(np.zeros((0, 32), np.uint8), degree=degree)
        text = bytes(ply)
        assert text.startswith(b"ply\nformat binary_little_endian 1.0\nelement vertex 0\n") and text.endswith(b"end_header\n")
        assert capi.ply_to_splat(ply).size == 0
        got, d = capi.ply_sh(ply, 3)
        assert got.shape[0] == 0 and d == degree
        assert text.count(b"f_rest_") == 3 * ((degree + 1) ** 2 - 1)


def test_splat_to_ply_refuses():
    L = capi.load()
    rows = np.zeros((2, 32), np.uint8)
    sh = np.zeros((2, 12), np.float32)
    nb = C.c_size_t(7)
    ok = L.gs_splat_to_ply
    assert ok(_p(rows), None, None, 0, 0, 2, None, C.byref(nb)) == capi.GS_OK and nb.value > 2 * 17 * 4
    assert ok(None, None, None, 0, 0, 2, None, C.byref(nb)) == capi.GS_OK                      # the size query needs no rows
    out = np.zeros(nb.value, np.uint8)
    assert ok(None, None, None, 0, 0, 2, _p(out), C.byref(nb)) == capi.E_BADARG
    assert ok(_p(rows), None, None, 0, 0, 2, None, None) == capi.E_BADARG
    for degree in (-1, 4, 1 << 20):
        assert ok(_p(rows), None, None, 0, degree, 2, None, C.byref(nb)) == capi.E_BADARG
    assert ok(_p(rows), None, _p(sh), 3, 1, 2, None, C.byref(nb)) == capi.E_BADARG              # more SH rows than rows
    assert ok(_p(rows), None, None, 1, 1, 2, None, C.byref(nb)) == capi.E_BADARG               # SH rows promised, none given
    assert ok(_p(rows), None, _p(sh), 2, 1, 2, None, C.byref(nb)) == capi.GS_OK
    with pytest.raises(capi.GsError):
        capi.splat_to_ply(rows, degree=5)
