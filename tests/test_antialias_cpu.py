"""CPU tier of the anti-aliased splats (GS_OPT_ANTIALIAS): gs_antialias_factor against a numpy f32 MIRROR of its lines, bit for bit, and
everything the GPU tier (test_antialias_gpu.py) compares frames with -- the mirror of gsm::project_splat (every line an f32 numpy
operation in the header's order; pinned here against the oracle's C, record for record), the compensated alpha it yields, an f64
front-to-back blend over those records with frag_power in f32 and the discard at q > 4, and the scenes.

A pixel is LEFT OUT of a frame comparison where one of its fragments lies within 1e-4 of the q = 4 discard boundary (a one-ulp
difference decides up to 4.7 LSB there: test_gl_pin.py).  At most 2 % of the pixels of any scene may be left out: asserted here, on
the CPU, since the exclusion depends on the mirror alone."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_blend_paths_gpu import camera

capi = pkg("capi")
synth = pkg("synth")

f32 = np.float32
EXCLUDED_CAP = 0.02
Q_EDGE = 1e-4


# ---------------------------------------------------------------- the factor

def factor_mirror(cov00, cov01, cov11):
    """csrc/gs_device_math.h: dilated_eigenvalues + antialias_factor, f32, un-fused, in the header's order"""
    cov00, cov01, cov11 = (np.asarray(a, f32) for a in (cov00, cov01, cov11))
    with np.errstate(all="ignore"):
        d1, od, d2 = cov00 + f32(0.3), cov01, cov11 + f32(0.3)
        mid = f32(0.5) * (d1 + d2)
        hd = (d1 - d2) / f32(2.0)
        radius = np.sqrt(hd * hd + od * od)
        l1 = mid + radius
        l2 = np.fmax(mid - radius, f32(0.1))
        return factor_of(cov00, cov01, cov11, l1, l2)


def factor_of(cov00, cov01, cov11, l1, l2):
    with np.errstate(all="ignore"):
        p = cov00 * cov11
        q = cov01 * cov01
        det = p - q
        den = l1 * l2
        r = det / den
        r = np.fmin(np.fmax(r, f32(0.0)), f32(1.0))                # fmaxf(NaN, 0) = 0
        return np.sqrt(r).astype(f32)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def random_covariances(n, seed):
    """log-uniform variances over 1e-6 .. 1e4 px^2 and a correlation in (-1, 1)"""
    g = np.random.default_rng(seed)
    a = (10.0 ** g.uniform(-6, 4, n)).astype(f32)
    b = (10.0 ** g.uniform(-6, 4, n)).astype(f32)
    rho = g.uniform(-0.999, 0.999, n)
    return np.stack([a, (rho * np.sqrt(a.astype(np.float64) * b)).astype(f32), b], 1)


def test_factor_equals_the_mirror_bit_for_bit():
    cov = random_covariances(4000, 1)
    got = capi.antialias_factor(cov)
    want = factor_mirror(cov[:, 0], cov[:, 1], cov[:, 2])
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    assert 0.0 <= got.min() and got.max() <= 1.0 and got.min() < 1e-3 and got.max() > 0.9999
    assert len(np.unique(bits(got))) > 3000


def test_isotropic_closed_form():
    v = (10.0 ** np.linspace(-6, 4, 400)).astype(f32)
    got = capi.antialias_factor(np.stack([v, np.zeros_like(v), v], 1))
    assert np.array_equal(bits(got), bits(factor_mirror(v, f32(0) * v, v)))
    vd = v.astype(np.float64)
    # l2 = max(v + 0.3, 0.1) = v + 0.3 (f32), l1 the same: c = sqrt(v v / ((v + 0.3)(v + 0.3)))
    want = np.sqrt(vd * vd / ((vd + 0.3) * (vd + 0.3)))
    ulp = np.spacing(want.astype(f32)).astype(np.float64)
    # (v + 0.3 in f32, two products, a division and a root: each within half an ulp of its operands' -- 4 ulp of the result covers them)
    assert (np.abs(got.astype(np.float64) - want) <= 4 * ulp).all()
    assert bits(capi.antialias_factor([0.0, 0.0, 0.0])) == 0          # det = 0 exactly: c = +0
    assert capi.antialias_factor([1e8, 0.0, 1e8]) == f32(1.0)           # v + 0.3 == v in f32: nothing to compensate


def test_degenerate_covariances_draw_nothing():
    inf, nan = np.inf, np.nan
    zero = [[1.0, 2.0, 1.0], [0.5, -0.8, 1.0], [0.0, 1e-3, 0.0],       # cov01^2 > cov00 * cov11
            [nan, 0.0, 1.0], [1.0, nan, 1.0], [1.0, 0.0, nan], [nan, nan, nan],
            [3e38, 0.0, 3e38], [1e30, 0.0, 1e30], [inf, 0.0, 1.0], [inf, 0.0, inf],   # den = inf (det = inf or NaN)
            [-1.0, 0.0, 1.0], [-2.0, 0.0, -3.0]]                       # not positive semi-definite
    got = capi.antialias_factor(np.array(zero, f32))
    assert (got == 0.0).all(), got
    m = np.array(zero, f32)
    assert np.array_equal(bits(got), bits(factor_mirror(m[:, 0], m[:, 1], m[:, 2])))


def test_symbol_option_and_stats_field():
    L = capi.load()
    assert hasattr(L, "gs_antialias_factor") and "gs_antialias_factor" in capi.EXPORTS
    assert capi.OPT_ANTIALIAS == 20
    assert capi.Stats._fields_[-3] == ("antialias", C.c_uint32) and capi.Stats._fields_[-4][0] == "surface"    # (seg_count and n_runs follow)
    out = C.c_float(7.0)
    cov = (C.c_float * 3)(1.0, 0.0, 1.0)
    assert L.gs_antialias_factor(None, C.byref(out)) == capi.E_BADARG
    assert L.gs_antialias_factor(cov, None) == capi.E_BADARG and out.value == 7.0
    assert L.gs_antialias_factor(cov, C.byref(out)) == 0 and 0.0 < out.value < 1.0


# ---------------------------------------------------------------- project_splat, mirrored

def project_mirror(cs, cc, mv, P, focal, vw, vh):
    """gsm::project_splat (gs_device_math.h) for every row at once -> dict of f32 arrays: visible, the record (cx, cy, ax, ay, bx, by,
    rgba, alpha), zndc, the un-dilated covariance and the factor c."""
    cs, cc = np.asarray(cs, f32), np.asarray(cc, np.uint32)
    mv, P = np.asarray(mv, f32).reshape(16), np.asarray(P, f32).reshape(16)
    focal, vw, vh = f32(focal), f32(vw), f32(vh)
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
        j00, j02 = focal / camz, -(focal * camx) / (camz * camz)
        j11, j12 = -focal / camz, (focal * camy) / (camz * camz)
        M00, M01, M02 = j00 * mv[0] + j02 * mv[2], j00 * mv[4] + j02 * mv[6], j00 * mv[8] + j02 * mv[10]
        M10, M11, M12 = j11 * mv[1] + j12 * mv[2], j11 * mv[5] + j12 * mv[6], j11 * mv[9] + j12 * mv[10]
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
               "c": factor_of(cov00, cov01, cov11, l1, l2), "v": (v1x, v1y, v2x, v2y)}
    return out


def record_words(pm, antialias):
    """the 8 words of every row's projected record, as GS_BUF_PROJECTED holds them"""
    a = pm["alpha"] * pm["c"] if antialias else pm["alpha"]
    w = np.stack([bits(pm[k]) for k in ("cx", "cy", "ax", "ay", "bx", "by")] + [pm["rgba"], bits(a)], 1)
    return w


def blend_mirror(pm, idx, W, H, antialias, x0=0, x1=None, scene_depth=None, scene_rgba=None, bg=(0.0, 0.0, 0.0, 1.0), rgb=None):
    """f64 front-to-back blend of the mirrored records in the order idx (far -> near, as gs_sort returns it) -> (rgba8 [H, sw, 4],
    excluded [H, sw]).  frag_power in f32 (the fmaf steps through f64: products of f32 are exact there); discard at q > 4; with a scene
    depth a fragment survives iff its window depth is <= the buffer's (LEQUAL).  rgb: colour bytes per row instead of the packed ones."""
    x1 = W if x1 is None else x1
    sw = x1 - x0
    fx = (np.arange(x0, x1, dtype=f32) + f32(0.5))[None, :]
    fy = (f32(H - 1) - np.arange(H, dtype=f32) + f32(0.5))[:, None]
    T = np.ones((H, sw))
    Cc = np.zeros((H, sw, 3))
    excl = np.zeros((H, sw), bool)
    alpha = (pm["alpha"] * pm["c"] if antialias else pm["alpha"]).astype(f32)
    sd = None if scene_depth is None else np.asarray(scene_depth, f32)[:, x0:x1]
    v1x, v1y, v2x, v2y = pm["v"]
    for i in np.asarray(idx)[::-1]:
        if not pm["visible"][i]:
            continue
        hw = 2.0 * np.sqrt(float(v1x[i]) ** 2 + float(v2x[i]) ** 2) + 1.0
        hh = 2.0 * np.sqrt(float(v1y[i]) ** 2 + float(v2y[i]) ** 2) + 1.0
        if not (pm["cx"][i] + hw >= x0 and pm["cx"][i] - hw <= x1 and pm["cy"][i] + hh >= 0 and pm["cy"][i] - hh <= H):
            continue
        dx, dy = fx - pm["cx"][i], fy - pm["cy"][i]                       # f32
        ax, ay, bx, by = (np.float64(pm[k][i]) for k in ("ax", "ay", "bx", "by"))
        ppx = (dx.astype(np.float64) * ax + (dy * pm["ay"][i]).astype(np.float64)).astype(f32)
        ppy = (dx.astype(np.float64) * bx + (dy * pm["by"][i]).astype(np.float64)).astype(f32)
        q = (ppx.astype(np.float64) * ppx + (ppy * ppy).astype(np.float64)).astype(f32).astype(np.float64)
        keep = q <= 4.0
        excl |= np.abs(q - 4.0) < Q_EDGE
        if sd is not None:
            keep &= f32(pm["zndc"][i] * f32(0.5) + f32(0.5)) <= sd
        if not keep.any():
            continue
        e = np.where(keep, np.exp(-q) * T, 0.0)
        word = int(pm["rgba"][i])
        col = np.array([word & 0xFF, (word >> 8) & 0xFF, (word >> 16) & 0xFF] if rgb is None else rgb[i], np.float64)
        a = float(alpha[i])
        Cc += (col * (a / 255.0))[None, None, :] * e[:, :, None]
        T = T - a * e
    dst = np.broadcast_to(np.asarray(bg, np.float64), (H, sw, 4)) if scene_rgba is None else np.asarray(scene_rgba)[:, x0:x1].astype(np.float64) / 255.0
    out = np.empty((H, sw, 4))
    out[:, :, :3] = Cc + T[:, :, None] * dst[:, :, :3]
    out[:, :, 3] = (1.0 - T) + T * dst[:, :, 3]
    return np.floor(np.clip(out, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8), excl


# ---------------------------------------------------------------- the scenes

def _row(cam, cx, cy, depth, sigma_px, rgba, quat):
    """a .splat row centred at image pixel (cx, cy), `depth` away, with standard deviations of sigma_px pixels along its own axes"""
    W, H, gp, f = cam["vw"], cam["vh"], cam["gs_proj"], cam["focal"]
    X = (2.0 * cx / W - 1.0 + gp[8]) * depth / gp[0]
    Y = (2.0 * (H - cy) / H - 1.0 + gp[9]) * depth / gp[5]
    r = np.zeros(32, np.uint8)
    r[0:12] = np.array([X, Y, depth], "<f4").view(np.uint8)
    r[12:24] = (np.asarray(sigma_px, np.float64) * depth / f).astype("<f4").view(np.uint8)
    r[24:28] = rgba
    r[28:32] = quat
    return r


class AAScene:
    """~300 splats on a W x H frame: sub-pixel splats (variance << 0.3 px^2, c near 0), needles (one eigenvalue << 0.3, the other tens
    of px^2 and more), mid-sized ones (variance about 0.3), large ones, three giants whose c lies within a few ulp of 1, rows of rank one
    and rows of all-zero scale (det = 0: c = 0; the depth sort itself drops a splat of size zero, index.js:548), alpha bytes over the
    whole range, 255 and 1 included."""

    def __init__(self, W=96, H=64, seed=7):
        g = np.random.default_rng(seed)
        cam = camera(W, H)
        rows, d = [], [1.0]

        def put(n, sigma, alpha):
            for k in range(n):
                d[0] += 0.004 + 0.002 * g.random()
                s = sigma(k)
                need = int(np.ceil(2.6 / max(max(s), 1e-9)))             # (the sort keeps max(scale) * alpha / 255 > 1e-4 * depth)
                a = max(alpha(k), min(need, 255))
                rows.append(_row(cam, g.uniform(-4, W + 4), g.uniform(-4, H + 4), d[0], s,
                                 (g.integers(0, 256), g.integers(0, 256), g.integers(0, 256), a), g.integers(0, 256, 4)))
        put(80, lambda k: 10.0 ** g.uniform(-1.5, -0.5, 3), lambda k: int(g.integers(90, 256)))                     # sub-pixel
        put(60, lambda k: (g.uniform(6.0, 17.0), g.uniform(0.1, 0.3), g.uniform(0.1, 0.3)), lambda k: int(g.integers(20, 256)))   # needles
        put(50, lambda k: g.uniform(0.35, 1.5, 3), lambda k: int(g.integers(8, 256)))                                 # variance ~ 0.3
        put(96, lambda k: g.uniform(2.0, 9.0, 3), lambda k: (255, 1, 2, 128)[k] if k < 4 else int(g.integers(1, 256)))   # large
        put(3, lambda k: (2500.0, 2400.0, 2300.0), lambda k: 1 + k)                                                   # c within a few ulp of 1
        put(6, lambda k: (g.uniform(4.0, 12.0), 0.0, 0.0), lambda k: 200)                                             # rank one
        put(6, lambda k: (0.0, 0.0, 0.0), lambda k: 255)                                                              # all-zero scale
        order = g.permutation(len(rows))
        self.W, self.H, self.cam = W, H, cam
        self.rows = np.concatenate([rows[i] for i in order])
        self.n = len(rows)
        self.cs, self.cc, self.mats = oracle.pack(self.rows)
        self.mv, self.pr = cam["gs_mv"].astype(f32), cam["gs_proj"].astype(f32)
        self.pm = project_mirror(self.cs, self.cc, self.mv, self.pr, cam["focal"], W, H)
        self.idx = oracle.sort(self.mats, cam["view"])

    def params(self, x0=0, x1=None, **kw):
        return capi.make_params(self.cam["gs_mv"], self.cam["gs_proj"], self.W, self.H, x0=x0, x1=x1, focal_=self.cam["focal"], **kw)

    def blend(self, antialias, **kw):
        return blend_mirror(self.pm, self.idx, self.W, self.H, antialias, **kw)


_SCENES = {}


def scene(W=96, H=64, seed=7):
    if (W, H, seed) not in _SCENES:
        _SCENES[(W, H, seed)] = AAScene(W, H, seed)
    return _SCENES[(W, H, seed)]


def scene_inputs(sc, seed=3):
    """a scene depth (a checkerboard of near / far) and colour for sc's frame"""
    yy, xx = np.mgrid[0:sc.H, 0:sc.W]
    zs = np.sort(sc.pm["zndc"][sc.pm["visible"]].astype(np.float64) * 0.5 + 0.5)
    depth = np.where(((yy // 12) + (xx // 12)) % 2 == 0, 1.0, zs[len(zs) // 2]).astype(f32)
    rgba = np.random.default_rng(seed).integers(0, 256, (sc.H, sc.W, 4), dtype=np.uint8)
    return depth, rgba


SCENE_SIZES = ((96, 64), (100, 70))


@pytest.mark.parametrize("size", SCENE_SIZES)
def test_mirror_is_the_oracles_projection(size):
    sc = scene(*size)
    pm, n_vis = sc.pm, 0
    for i in range(sc.n):
        p = oracle.project(sc.cs, sc.cc, i, sc.mv, sc.pr, sc.cam["focal"], sc.W, sc.H)
        assert bool(p.visible) == bool(pm["visible"][i]), i
        if p.visible:
            n_vis += 1
            for k in ("cx", "cy", "ax", "ay", "bx", "by", "zndc", "alpha"):
                assert bits(f32(getattr(p, k))) == bits(pm[k][i]), (i, k)
    assert n_vis > 250
    # ... and its factor is gs_antialias_factor of its covariance
    assert np.array_equal(bits(capi.antialias_factor(pm["cov"])), bits(pm["c"]))


@pytest.mark.parametrize("size", SCENE_SIZES)
def test_scene_population_and_excluded_share(size):
    sc = scene(*size)
    live = sc.pm["visible"][sc.idx]
    c, ab = sc.pm["c"][sc.idx][live], (sc.pm["rgba"][sc.idx][live] >> 24)
    print("%dx%d: sorted %d, visible %d, c == 0: %d, c < 0.1: %d, c > 0.99: %d, c >= 1 - 4 ulp: %d" % (
        sc.W, sc.H, len(sc.idx), live.sum(), (c == 0).sum(), (c < 0.1).sum(), (c > 0.99).sum(), (c >= 1 - 2.4e-7).sum()))
    assert len(sc.idx) == sc.n - 6                                   # the rows of all-zero scale never leave the sort
    assert (c == 0).sum() >= 3 and (c < 0.1).sum() >= 40 and ((c > 0.3) & (c < 0.9)).sum() >= 40 and (c > 0.99).sum() >= 3
    assert (c >= 1 - 2.4e-7).sum() >= 1 and c.max() <= 1.0
    assert {1, 255} <= set(ab.tolist())
    on, ex_on = sc.blend(True)
    off, ex_off = sc.blend(False)
    assert np.array_equal(ex_on, ex_off)                             # (geometry only)
    print("excluded share %.4f; pixels that differ on/off %.3f" % (ex_on.mean(), (on != off).any(axis=2).mean()))
    assert ex_on.mean() <= EXCLUDED_CAP
    assert (on != off).any(axis=2).mean() > 0.2
    depth, rgba = scene_inputs(sc)
    _, ex = sc.blend(True, scene_depth=depth, scene_rgba=rgba)
    assert ex.mean() <= EXCLUDED_CAP
