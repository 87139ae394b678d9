"""CPU tier of the parallel-projection cameras (GS_RENDER_PARALLEL): gs_project_record -- the kernels' own gsm::project_splat<PAR> on the
host -- against a numpy f32 MIRROR of the rule (include/gs_splat.h: "Parallel-projection cameras"), word for word, with and without the
flag; the closed form of an isotropic splat; gs_ortho_matrix against three.js' formula; the matrix check; and the scene the GPU tier
(test_parallel_gpu.py) draws: ~320 splats in a box around an orthographic view volume, a rotated entity, frames of 96x64 (square pixels)
and 100x70 (10 x 12.5 pixels per unit).

Nothing in the reference corresponds to the rule (its shader is perspective-only, index.js:127-131), so the mirror holds it, as
test_antialias_cpu.py's holds the opacity factor.  Pixels with a fragment within 1e-4 of the q = 4 discard boundary are left out of
frame comparisons (blend_mirror); at most 2 % of a frame, asserted here on the mirror alone."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_antialias_cpu import EXCLUDED_CAP, bits, blend_mirror, factor_of, project_mirror, record_words

capi = pkg("capi")
synth = pkg("synth")

f32 = np.float32
PAR = capi.RENDER_PARALLEL if hasattr(capi, "RENDER_PARALLEL") else 32


# ---------------------------------------------------------------- the rule, mirrored

def parallel_jacobian_mirror(mv, P, vw, vh):
    """gsm::parallel_jacobian: M[0..2] = row 0, M[3..5] = row 1, every operation f32 in the header's order"""
    mv, P = np.asarray(mv, f32).reshape(16), np.asarray(P, f32).reshape(16)
    hx, hy = f32(0.5) * f32(vw), f32(0.5) * f32(vh)
    j00, j01, j02 = hx * P[0], hx * P[4], hx * P[8]
    j10, j11, j12 = hy * P[1], hy * P[5], hy * P[9]
    M = np.zeros(6, f32)
    for k in range(3):
        M[k] = (j00 * mv[4 * k] + j01 * mv[4 * k + 1]) + j02 * mv[4 * k + 2]
        M[3 + k] = (j10 * mv[4 * k] + j11 * mv[4 * k + 1]) + j12 * mv[4 * k + 2]
    return M


def project_mirror_parallel(cs, cc, mv, P, vw, vh):
    """gsm::project_splat<true> for every row at once: test_antialias_cpu.project_mirror with the four j.. and six M.. lines replaced by
    the frame's constant M; the same dict comes back"""
    cs, cc = np.asarray(cs, f32), np.asarray(cc, np.uint32)
    mv, P = np.asarray(mv, f32).reshape(16), np.asarray(P, f32).reshape(16)
    vw, vh = f32(vw), f32(vh)
    with np.errstate(all="ignore"):
        cx, cy, cz, scl = cs[:, 0], cs[:, 1], cs[:, 2], cs[:, 3]
        cam = [((mv[i] * cx + mv[4 + i] * cy) + mv[8 + i] * cz) + mv[12 + i] for i in range(4)]
        camx, camy, camz, camw = cam
        px, py, pz, pw = [((P[i] * camx + P[4 + i] * camy) + P[8 + i] * camz) + P[12 + i] * camw for i in range(4)]
        bounds = f32(1.2) * pw
        vis = ~((pz < -pw) | (px < -bounds) | (px > bounds) | (py < -bounds) | (py > bounds)) & (pw > 0)

        def s16(w, hi):
            return ((w >> 16) if hi else (w & 0xFFFF)).astype(np.uint16).view(np.int16).astype(f32)
        m11, m12 = s16(cc[:, 0], 0) * scl, s16(cc[:, 0], 1) * scl
        m13, m22 = s16(cc[:, 1], 0) * scl, s16(cc[:, 1], 1) * scl
        m23, m33 = s16(cc[:, 2], 0) * scl, s16(cc[:, 2], 1) * scl
        M00, M01, M02, M10, M11, M12 = parallel_jacobian_mirror(mv, P, vw, vh)
        t0 = (m11 * M00 + m12 * M01) + m13 * M02
        t1 = (m12 * M00 + m22 * M01) + m23 * M02
        t2 = (m13 * M00 + m23 * M01) + m33 * M02
        u0 = (m11 * M10 + m12 * M11) + m13 * M12
        u1 = (m12 * M10 + m22 * M11) + m23 * M12
        u2 = (m13 * M10 + m23 * M11) + m33 * M12
        cov00 = (M00 * t0 + M01 * t1) + M02 * t2
        cov01 = (M10 * t0 + M11 * t1) + M12 * t2
        cov11 = (M10 * u0 + M11 * u1) + M12 * u2
        d1, od, d2 = cov00 + f32(0.3), cov01, cov11 + f32(0.3)
        mid = f32(0.5) * (d1 + d2)
        hd = (d1 - d2) / f32(2.0)
        radius = np.sqrt(hd * hd + od * od)
        l1 = mid + radius
        l2 = np.fmax(mid - radius, f32(0.1))
        dvx0, dvy0 = od, l1 - d1
        ln = np.sqrt(dvx0 * dvx0 + dvy0 * dvy0)
        fmax = f32(3.402823466e+38)
        vis &= (ln > 0) & (ln <= fmax) & (np.abs(l1) <= fmax)
        dvx, dvy = dvx0 / ln, dvy0 / ln
        s1 = np.fmin(np.sqrt(f32(2.0) * l1), f32(1024.0))
        s2 = np.fmin(np.sqrt(f32(2.0) * l2), f32(1024.0))
        v1x, v1y, v2x, v2y = s1 * dvx, s1 * dvy, s2 * dvy, s2 * -dvx
        ndcx, ndcy, zndc = px / pw, py / pw, pz / pw
        vis &= ~(zndc > f32(1.0))
        n1, n2 = v1x * v1x + v1y * v1y, v2x * v2x + v2y * v2y
        out = {"visible": vis, "cx": (ndcx * f32(0.5) + f32(0.5)) * vw, "cy": (ndcy * f32(0.5) + f32(0.5)) * vh,
               "ax": v2x / n2, "ay": v2y / n2, "bx": v1x / n1, "by": v1y / n1, "rgba": cc[:, 3].copy(),
               "alpha": (cc[:, 3] >> 24).astype(f32) / f32(255.0), "zndc": zndc, "cov": np.stack([cov00, cov01, cov11], 1),
               "c": factor_of(cov00, cov01, cov11, l1, l2), "v": (v1x, v1y, v2x, v2y),
               "culls": {"near": pz < -pw, "bounds": (px < -bounds) | (px > bounds) | (py < -bounds) | (py > bounds), "far": zndc > f32(1.0)}}
    return out


# ---------------------------------------------------------------- the scene

NEAR, FAR = 0.5, 12.0
VOLUMES = {(96, 64): (4.8, 3.2), (100, 70): (5.0, 2.8)}        # half width and height of the view volume: 10 x 10 and 10 x 12.5 pixels per unit


def ortho_camera(W, H):
    """an orthographic camera at the origin looking down -z, the entity 6 units ahead and turned by 25 degrees: the uniforms a host
    computes with gs_ortho_matrix, gs_projection_matrix, gs_model_view_matrix and gs_tick_uniforms"""
    a, b = VOLUMES[(W, H)]
    proj = capi.ortho_matrix(-a, a, b, -b, NEAR, FAR)
    return synth.uniforms(synth.compose((0.0, 0.0, 0.0)), synth.compose((0.3, -0.2, -6.0), 25.0), proj, W, H, capi=capi)


def _row(pos, sigma, rgba, quat):
    r = np.zeros(32, np.uint8)
    r[0:12] = np.asarray(pos, "<f4").view(np.uint8)
    r[12:24] = np.asarray(sigma, "<f4").view(np.uint8)
    r[24:28] = rgba
    r[28:32] = quat
    return r


class ParallelScene:
    """~320 splats: sub-pixel ones, thin tilted needles, mid-sized ones and a few that span several tiles, uniformly in a box that
    overhangs the view volume on every side (so the near plane, the far plane, the 1.2 bounds and the camera plane all cut through
    the population), plus four splats placed by hand on either side of each of those four culls."""

    def __init__(self, W=96, H=64, seed=11):
        g = np.random.default_rng(seed)
        cam = ortho_camera(W, H)
        mv64 = np.asarray(cam["gs_mv"], np.float64).reshape(4, 4).T
        inv = np.linalg.inv(mv64)
        a, b = VOLUMES[(W, H)]

        def at(camx, camy, camz):
            """the .splat position whose packed centre (x, y, -z) lands at that camera-space point"""
            p = inv @ np.array([camx, camy, camz, 1.0])
            return (p[0], p[1], -p[2])
        rows = []

        def put(n, sigma, alpha):
            for k in range(n):
                pos = at(g.uniform(-1.25 * a, 1.25 * a), g.uniform(-1.25 * b, 1.25 * b), -g.uniform(-0.6, FAR + 0.8))
                rows.append(_row(pos, sigma(k), (g.integers(0, 256), g.integers(0, 256), g.integers(0, 256), alpha(k)), g.integers(0, 256, 4)))
        put(90, lambda k: 10.0 ** g.uniform(-2.3, -1.5, 3), lambda k: int(g.integers(160, 256)))                        # sub-pixel: 0.05 .. 0.3 px
        put(70, lambda k: (g.uniform(0.5, 1.6), g.uniform(0.008, 0.03), g.uniform(0.008, 0.03)), lambda k: int(g.integers(20, 256)))   # needles
        put(90, lambda k: g.uniform(0.04, 0.25, 3), lambda k: int(g.integers(8, 256)))                                  # around a pixel
        put(40, lambda k: g.uniform(0.3, 0.9, 3), lambda k: int(g.integers(1, 256)))                                    # a tile and more
        put(6, lambda k: g.uniform(1.5, 2.5, 3), lambda k: int(g.integers(1, 40)))                                      # several tiles, faint
        quat = (255, 128, 128, 128)                                                                                      # (the identity rotation)
        for eps in (-2e-3, 2e-3):
            rows.append(_row(at(0.5, 0.5, -NEAR + eps), (0.2, 0.2, 0.2), (255, 0, 0, 200), quat))                        # the near plane
            rows.append(_row(at(-0.5, 0.5, -FAR + eps), (0.2, 0.2, 0.2), (0, 255, 0, 200), quat))                        # zndc > 1
            rows.append(_row(at(1.2 * a + eps, -0.5, -3.0), (0.3, 0.3, 0.3), (0, 0, 255, 200), quat))                    # the 1.2 bounds, x
            rows.append(_row(at(0.5, -1.2 * b + eps, -3.0), (0.3, 0.3, 0.3), (255, 255, 0, 200), quat))                  # the 1.2 bounds, y
            rows.append(_row(at(-0.5, -0.5, eps), (0.2, 0.2, 0.2), (255, 0, 255, 200), quat))                            # the camera plane (the sort's cull)
        order = g.permutation(len(rows))
        self.W, self.H, self.cam = W, H, cam
        self.rows = np.concatenate([rows[i] for i in order])
        self.hand = np.argsort(order)[-10:]                              # where the ten hand-placed splats went
        self.n = len(rows)
        self.cs, self.cc, self.mats = oracle.pack(self.rows)
        self.mv, self.pr = cam["gs_mv"].astype(f32), cam["gs_proj"].astype(f32)
        self.pm = project_mirror_parallel(self.cs, self.cc, self.mv, self.pr, W, H)
        self.pm_persp = project_mirror(self.cs, self.cc, self.mv, self.pr, cam["focal"], W, H)    # what the same params draw WITHOUT the flag
        self.idx = oracle.sort(self.mats, cam["view"])

    def params(self, x0=0, x1=None, flags=0, parallel=True, **kw):
        return capi.make_params(self.cam["gs_mv"], self.cam["gs_proj"], self.W, self.H, x0=x0, x1=x1, focal_=self.cam["focal"],
                                flags=flags | (PAR if parallel else 0), **kw)

    def blend(self, parallel=True, **kw):
        return blend_mirror(self.pm if parallel else self.pm_persp, self.idx, self.W, self.H, False, **kw)


_SCENES = {}
SCENE_SIZES = ((96, 64), (100, 70))


def scene(W=96, H=64, seed=11):
    if (W, H, seed) not in _SCENES:
        _SCENES[(W, H, seed)] = ParallelScene(W, H, seed)
    return _SCENES[(W, H, seed)]


def scene_inputs(sc, seed=3):
    """a scene depth (a checkerboard of far / the median splat depth) and colour for sc's frame"""
    yy, xx = np.mgrid[0:sc.H, 0:sc.W]
    zs = np.sort(sc.pm["zndc"][sc.pm["visible"]].astype(np.float64) * 0.5 + 0.5)
    depth = np.where(((yy // 12) + (xx // 12)) % 2 == 0, 1.0, zs[len(zs) // 2]).astype(f32)
    rgba = np.random.default_rng(seed).integers(0, 256, (sc.H, sc.W, 4), dtype=np.uint8)
    return depth, rgba


def sheared(P):
    """the same matrix with a shear in rows 0 and 1 (an oblique parallel projection): rows 0..2 are free"""
    Q = np.array(P, np.float64)
    Q[8], Q[9] = 0.031, -0.017
    return Q


# ---------------------------------------------------------------- tests

def test_symbols_and_flag():
    L = capi.load()
    for name in ("gs_project_record", "gs_ortho_matrix", "gs_projection_info"):
        assert hasattr(L, name) and name in capi.EXPORTS, name
    assert capi.RENDER_PARALLEL == 32
    assert capi.RENDER_PARALLEL & (capi.RENDER_FLIP_Y | capi.RENDER_COUNT_FRAGS | capi.RENDER_NO_EARLY_OUT | capi.RENDER_ASYNC | capi.RENDER_COUNT_EVALUATED) == 0
    assert capi.Stats._fields_[-3] == ("antialias", C.c_uint32)      # gs_stats is what it was: the feature reports through gs_projection_info
    assert L.gs_projection_info(None, None) == capi.E_BADARG


def test_ortho_matrix_is_threejs_make_orthographic():
    g = np.random.default_rng(2)
    for _ in range(50):
        l, b, n = g.uniform(-9, 0), g.uniform(-9, 0), g.uniform(-3, 3)
        r, t, f = l + g.uniform(0.1, 20), b + g.uniform(0.1, 20), n + g.uniform(0.1, 2000)
        got = capi.ortho_matrix(l, r, t, b, n, f)
        w, h, p = 1.0 / (r - l), 1.0 / (t - b), 1.0 / (f - n)
        want = np.array([2 * w, 0, 0, 0, 0, 2 * h, 0, 0, 0, 0, -2 * p, 0, -((r + l) * w), -((t + b) * h), -((f + n) * p), 1], np.float64)
        assert np.array_equal(got, want)
    m = capi.ortho_matrix(-2, 2, 1, -1, 0.5, 12).reshape(4, 4).T
    for corner, ndc in (((-2, -1, -0.5), (-1, -1, -1)), ((2, 1, -12), (1, 1, 1))):          # the box's corners land on the NDC cube's
        assert np.allclose(m @ np.array(corner + (1.0,)), np.array(ndc + (1.0,)), atol=1e-15)
    assert capi.load().gs_ortho_matrix(-1.0, 1.0, 1.0, -1.0, 0.1, 10.0, None) == capi.E_BADARG
    gp = capi.projection_matrix(m.T.reshape(16))
    assert gp[5] == -m[1, 1] and gp[3] == 0 and gp[7] == 0 and gp[11] == 0 and gp[15] == 1


def test_invalid_bottom_rows_are_refused_and_minus_zero_passes():
    sc = scene()
    L = capi.load()
    rec, z, v = (C.c_float * 8)(), C.c_float(0), C.c_int(0)
    cs, cc = np.ascontiguousarray(sc.cs[:1]), np.ascontiguousarray(sc.cc[:1])

    def call(p):
        return L.gs_project_record(cs.ctypes.data, cc.ctypes.data, C.byref(p), rec, C.byref(z), C.byref(v))
    good = sc.params()
    assert call(good) == 0
    for k, val in ((3, 1e-30), (7, -1e-30), (11, -1.0), (11, 1e-38), (15, 0.0), (15, 1.0000001), (15, np.nan), (3, np.nan)):
        p = sc.params()
        p.projection[k] = val
        assert call(p) == capi.E_BADARG, (k, val)
        p.flags = 0                                                  # without the flag any matrix is taken, as before
        assert call(p) == 0, (k, val)
    p = sc.params()
    for k in (3, 7, 11):
        p.projection[k] = -0.0
    assert call(p) == 0
    persp = capi.make_params(sc.cam["gs_mv"], synth.perspective(80.0, 1.5), sc.W, sc.H, flags=PAR)
    assert call(persp) == capi.E_BADARG
    # NULL pointers
    assert L.gs_project_record(None, cc.ctypes.data, C.byref(good), rec, C.byref(z), C.byref(v)) == capi.E_BADARG
    assert L.gs_project_record(cs.ctypes.data, None, C.byref(good), rec, C.byref(z), C.byref(v)) == capi.E_BADARG
    assert L.gs_project_record(cs.ctypes.data, cc.ctypes.data, None, rec, C.byref(z), C.byref(v)) == capi.E_BADARG
    assert L.gs_project_record(cs.ctypes.data, cc.ctypes.data, C.byref(good), None, C.byref(z), C.byref(v)) == capi.E_BADARG
    assert L.gs_project_record(cs.ctypes.data, cc.ctypes.data, C.byref(good), rec, None, C.byref(v)) == capi.E_BADARG
    assert L.gs_project_record(cs.ctypes.data, cc.ctypes.data, C.byref(good), rec, C.byref(z), None) == capi.E_BADARG


def _check_records(tag, cs, cc, params, pm):
    rec, zwin, vis = capi.project_record(cs, cc, params)
    assert np.array_equal(vis, pm["visible"]), tag
    want = record_words(pm, False)
    assert np.array_equal(rec[vis], want[vis]), (tag, int((rec[vis] != want[vis]).any(axis=1).sum()))
    assert np.array_equal(bits(zwin[vis]), bits((pm["zndc"] * f32(0.5) + f32(0.5))[vis])), tag
    assert not rec[~vis].any() and not zwin[~vis].any(), tag
    return vis


@pytest.mark.parametrize("size", SCENE_SIZES)
def test_project_record_equals_the_mirror_word_for_word(size):
    sc = scene(*size)
    vis = _check_records("parallel", sc.cs, sc.cc, sc.params(), sc.pm)
    _check_records("no flag", sc.cs, sc.cc, sc.params(parallel=False), sc.pm_persp)
    # focal is ignored with the flag; without it and focal <= 0 the rule is gs_render's: fb_height / 2 * |P[5]|
    p = sc.params()
    p.focal = 123.0
    assert np.array_equal(capi.project_record(sc.cs, sc.cc, p)[0], capi.project_record(sc.cs, sc.cc, sc.params())[0])
    p = sc.params(parallel=False)
    p.focal = 0.0
    f = f32((sc.H / 2.0) * abs(float(sc.pr[5])))
    _check_records("focal rule", sc.cs, sc.cc, p, project_mirror(sc.cs, sc.cc, sc.mv, sc.pr, f, sc.W, sc.H))
    # a sheared parallel projection, and another entity pose
    Q = sheared(sc.cam["gs_proj"])
    mv2 = capi.model_view_matrix(synth.compose((0.2, 0.1, 0.4)), synth.compose((0.3, -0.2, -6.0), -40.0, (1.3, 0.8, 1.1)))
    pq = capi.make_params(mv2, Q, sc.W, sc.H, flags=PAR)
    pmq = project_mirror_parallel(sc.cs, sc.cc, mv2.astype(f32), Q.astype(f32), sc.W, sc.H)
    assert _check_records("sheared", sc.cs, sc.cc, pq, pmq).sum() > 150
    # the two camera models really differ on these params
    a, b = record_words(sc.pm, False), record_words(sc.pm_persp, False)
    both = vis & sc.pm_persp["visible"]
    assert both.sum() > 150 and (a[both][:, 2:6] != b[both][:, 2:6]).any(axis=1).mean() > 0.95
    assert np.array_equal(a[both][:, :2], b[both][:, :2])            # the centre lands where the matrix puts it either way


def test_isotropic_closed_form_at_any_depth_and_position():
    """sigma s, identity rotation: the un-dilated covariance is diag((hx P0 s)^2, (hy P5 s)^2) wherever the splat is"""
    W, H = 100, 70
    a, b = VOLUMES[(W, H)]
    proj = capi.projection_matrix(capi.ortho_matrix(-a, a, b, -b, NEAR, FAR))
    eye = synth.compose((0.0, 0.0, 0.0))
    mv = capi.model_view_matrix(eye, eye)                              # identity poses: M is diag(hx P0, hy P5) and a zero column
    g = np.random.default_rng(5)
    n = 400
    s = (10.0 ** g.uniform(-2.0, 0.3, n))
    rows = np.concatenate([_row((g.uniform(-a, a), g.uniform(-b, b), g.uniform(NEAR + 0.1, FAR - 0.1)), (s[i],) * 3, (9, 9, 9, 255), (255, 128, 128, 128))
                           for i in range(n)])
    cs, cc, _ = oracle.pack(rows)
    p = capi.make_params(mv, proj, W, H, flags=PAR)
    pm = project_mirror_parallel(cs, cc, mv.astype(f32), proj.astype(f32), W, H)
    vis = _check_records("isotropic", cs, cc, p, pm)
    assert vis.all()
    sx, sy = 0.5 * W * float(f32(proj[0])), 0.5 * H * float(f32(proj[5]))
    assert abs(abs(sx) - 10.0) < 1e-6 and abs(abs(sy) - 12.5) < 1e-6  # pixels per unit: not square
    # the packed covariance: s^2 quantised to int16 steps of max / 32767 (relative 2^-15 at the diagonal, exactly 32767 steps) -- so the
    # reference value is taken from the record's own dequantised diagonal, in f64
    scl = cs[:, 3].astype(np.float64)
    m11 = (cc[:, 0] & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.float64) * scl
    m22 = (cc[:, 1] >> 16).astype(np.uint16).view(np.int16).astype(np.float64) * scl
    want00, want11 = sx * sx * m11, sy * sy * m22
    # f32 rounding: m = q * scl (1), M = j * mv summed (exact here: one non-zero term), t = m * M (1), cov = M * t (1), plus the
    # rounding of hx * P0 twice over (2): 6 ulp covers the chain
    eps = 6 * 2.0 ** -24
    assert (np.abs(pm["cov"][:, 0] - want00) <= eps * want00).all() and (np.abs(pm["cov"][:, 2] - want11) <= eps * want11).all()
    assert (np.abs(pm["cov"][:, 1]) <= eps * np.sqrt(want00 * want11)).all()
    assert (np.abs(m11 - s * s) <= 2.0 ** -14 * s * s).all()           # ... and that diagonal is s^2 up to the pack's quantisation


@pytest.mark.parametrize("size", SCENE_SIZES)
def test_scene_population_and_excluded_share(size):
    sc = scene(*size)
    live = sc.pm["visible"][sc.idx]
    print("%dx%d: %d rows, sorted %d, visible %d (perspective: %d)" % (sc.W, sc.H, sc.n, len(sc.idx), live.sum(), sc.pm_persp["visible"][sc.idx].sum()))
    assert 300 <= sc.n <= 340 and live.sum() >= 200
    square = abs(float(sc.pr[0]) * sc.W - abs(float(sc.pr[5])) * sc.H) < 1e-4    # (20 against 20, resp. 20 against 25)
    assert square == ((sc.W, sc.H) == (96, 64))                      # the ragged frame has a non-square pixel scale
    # every cull has splats on both sides, the hand-placed pairs among them
    culls = sc.pm["culls"]
    for name in ("near", "bounds", "far"):
        assert 3 <= culls[name].sum() <= sc.n - 3, name
    h = sc.hand
    assert [bool(culls["near"][h[k]]) for k in (0, 5)] == [False, True]           # camz = -near -+ eps
    assert [bool(culls["far"][h[k]]) for k in (1, 6)] == [True, False]            # camz = -far -+ eps
    assert [bool(culls["bounds"][h[k]]) for k in (2, 7)] == [False, True] and [bool(culls["bounds"][h[k]]) for k in (3, 8)] == [True, False]
    in_order = np.isin(h, sc.idx)
    assert bool(in_order[4]) and not bool(in_order[9])                           # behind the camera plane: dropped by the sort
    behind = (sc.mats[:, 12:15] * sc.cam["view"][:3]).sum(axis=1) + sc.cam["view"][3] >= 0
    assert behind.sum() >= 5 and not np.isin(np.nonzero(behind)[0], sc.idx).any()
    # sizes from sub-pixel to several tiles (half extent 2 |v1|), thin ones among them
    v1 = np.hypot(*sc.pm["v"][:2])[sc.idx][live]
    v2 = np.hypot(*sc.pm["v"][2:])[sc.idx][live]
    assert (2 * v1 < 2.0).sum() >= 30 and (2 * v1 > 32).sum() >= 5 and (v1 > 8 * v2).sum() >= 20
    on, ex = sc.blend()
    off, ex_off = sc.blend(parallel=False)
    print("excluded share %.4f (perspective %.4f); pixels that differ between the camera models %.3f" % (ex.mean(), ex_off.mean(), (on != off).any(axis=2).mean()))
    assert ex.mean() <= EXCLUDED_CAP and ex_off.mean() <= EXCLUDED_CAP
    assert (on != off).any(axis=2).mean() > 0.2
    depth, rgba = scene_inputs(sc)
    _, ex = sc.blend(scene_depth=depth, scene_rgba=rgba)
    assert ex.mean() <= EXCLUDED_CAP
