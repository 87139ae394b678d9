"""CPU tier: the reach test of gs_sort_for (gsm::strip_may_touch, csrc/gs_device_math.h) and the norm bound its uniforms carry
(gs_norm_bound, csrc/gs_strip_uniforms.h), host build (tests/host_check/host_check.cpp: hc_reach_sweep, hc_norm_bound).

Norm.  hc_norm_bound(mv) against numpy's f64 SVD of the f32 matrix: 1 <= bound / true <= 1.03 over random matrices, the family with
the top right-singular vector orthogonal to a chosen direction and singular values (s, 1, 1), rotations times uniform scales, and
rank 1, rank 2 and zero.  old_norm() below keeps the parent commit's lines (64 power iterations from (1, 0.7, 0.4), + 2 %, capped at
Frobenius) as numpy.  Measured on the f32 matrices (rounding leaves the top vector orthogonal to the start to ~1e-8 only, which 64
iterations amplify by s^128 -- so from s = 1.2 up most draws converge after all): the parent's formula falls below the true norm in 494
of the 1 600 cases orthogonal to (1, 0.7, 0.4) -- 200, 200, 92 and 2 of 200 at s = 1.05, 1.1, 1.15 and 1.2; lowest ratios 0.9715,
0.9274, 0.8872 and 0.9124; none at s = 1.02 (1.0001: the 2 % just suffices) nor from s = 1.3 up -- in 2 of the 6 400 cases orthogonal
to a coordinate axis or to (1, 1, 1) (lowest 0.9737), and in 0 of 20 000 random matrices (lowest 1.0002).  The new bound: 1.0001 ..
1.0088 over all of them.

Reach.  A case is a pose (model-view, projection, focal length), a frame, a strip [x0, x1) and a 32-byte .splat row.  The row is packed
(gsm::pack_row), its bound_r taken as k_pack takes it, and projected (gsm::project_splat); the truth is "visible, and some pixel centre
of the strip has gsm::frag_power <= 4.0f", brute force over the strip's part of the ellipse's f64 bounding box widened by one pixel.  A
miss is truth with strip_may_touch == false; misses must be 0 with the reciprocal and the square root moved by -1, 0 and +1 ulp in all
nine combinations.  Poses (POSES): uniform scale 0.1, 1 and 10 under a yaw-only camera and the four pitched and rolled cameras of
test_gpu_parity._tilted_camera, one more turned 1e-3 rad off the axes (the row's quaternion bytes cannot say 1e-3 rad: the pose does),
model scales (1, 1, 3), (3, 1, 1), (1.15, 1, 1) and (1.2, 1, 1) axis-aligned, five poses of the family whose top right-singular vector
is orthogonal to (1, 0.7, 0.4) -- each the draw of 300 that the parent's formula underestimates most once rounded to f32 -- with the
stretched axis (1.15, 3) on the camera's x, (1.15) on its y, (3: the rotated (1, 1, 3)) on its view axis and (1.1) askew, a shear, and
the two XR eye matrices of synth.xr_eye_cameras (asymmetric frusta, canted 12 degrees; the focal length follows this test's frame height).
Frames 640 x 360 and 77 x 53, four strips each: the whole frame, the first 80 (16) columns, an interior strip, the last 16 columns.  Splats: isotropic with sigma 1e-4 .. 100 object units and with screen sizes 0.1 .. 300 px,
needles 1000 : 1 : 1 and discs 1000 : 1000 : 1 at 13 orientations, centres in 1.5 x the frustum, on the planes camz = -1e-3 .. -1e-6 and
behind the camera, on the |px| = 1.2 pw and |py| = 1.2 pw cull planes, and grazing: per strip edge and frame edge, the centre moved
along camera x (y) until the f64 ellipse ends 2 and 0.5 px inside and 0.5 px outside the edge, at half extents of 1 .. 400 px and at the
one that puts the centre on the principal point (where the reach has the least slack); the f32 result is kept whatever it is.

Measured (8 cores): 218 624 splat-cases, each swept twice (the new bound, the parent's norm), the file in 15 s of wall time.  Per pose,
cases that are truth and kept: 0.24 .. 0.33, neither truth nor kept: 0.27 .. 0.34 (asserted: each at least 0.10).  Tightness on the
rigid poses over the strips no wider than W / 4, kept / truth at the IEEE setting: 2.706 with the parent's norm, 2.703 with the new
bound (asserted: at most 1.1 x the parent's 2.706; the ratio is what a scene of needles, discs and splats at the 1024 clamp gives).  The
parent's norm fed into the same strip_may_touch misses 27 times (3 splats x nine settings) on the poses of the orthogonal family, all on
b_x_1.15: needles along the top vector that graze a strip's edge with their centre near the principal point.  b_y_1.15 shows none and
cannot: only the frame's top and bottom cull in y, and a splat grazing those has its centre outside the frame, where the Jacobian's
norm exceeds what a needle along y uses by 1.3 or more.  The new bound: 0 misses.  docs/LAB_NOTES.md 9j."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import pkg
from test_host_check import _p, hc  # noqa: F401  (the host build of the header, shared)

synth = pkg("synth")

START = np.array([1.0, 0.7, 0.4])
FRAMES = [((640, 360), [(0, 640), (0, 80), (272, 352), (624, 640)]),
          ((77, 53), [(0, 77), (0, 16), (21, 37), (61, 77)])]       # whole frame, the first columns, an interior strip, the last 16 columns
LIVE_SHARE = 0.10
PARENT_TIGHTNESS = 2.706                    # kept / truth with the parent's norm, rigid poses, strips <= W / 4 (measured: docstring)
N_BASE = 760                               # splats per (pose, frame) that every strip sees, plus the strip's grazing ones


# ---------------------------------------------------------------- the norm

def old_norm(mv):
    """The parent commit's fill_sort_uniforms, its lines as numpy (over a batch of matrices at once): power iteration on A^T A
    from (1, 0.7, 0.4), 2 % on top, never above Frobenius."""
    m = np.asarray(mv, np.float32).astype(np.float64).reshape(-1, 16)
    ata = np.zeros((m.shape[0], 3, 3))
    for i in range(3):
        for j in range(3):
            for r in range(3):
                ata[:, i, j] += m[:, 4 * i + r] * m[:, 4 * j + r]
    fro = ata[:, 0, 0] + ata[:, 1, 1] + ata[:, 2, 2]
    v, lam = np.tile([1.0, 0.7, 0.4], (m.shape[0], 1)), fro.copy()
    live = np.ones(m.shape[0], bool)                           # (the loop's `break`, per matrix)
    for _ in range(64):
        w = np.einsum("nij,nj->ni", ata, v)
        nn = np.sqrt((w * w).sum(1))
        live &= nn > 0.0
        v = np.where(live[:, None], w / np.where(nn > 0.0, nn, 1.0)[:, None], v)
        lam = np.where(live, nn, lam)
    na = np.sqrt(lam) * 1.02
    cap = np.sqrt(fro) * 1.0001
    na = np.where(na <= cap, na, cap)
    out = na.astype(np.float32) * np.float32(1.0001)
    return out if np.ndim(mv) > 1 else out[0]


def mv_of(A, t=(0.0, 0.0, 0.0)):
    """column-major 4x4 with mat3 = A (camera <- object) and translation t"""
    m = np.zeros(16, np.float32)
    for c in range(3):
        for r in range(3):
            m[4 * c + r] = A[r][c]
    m[12:15] = t
    m[15] = 1.0
    return m


def mat3_of(mv):
    return np.asarray(mv, np.float32).astype(np.float64).reshape(4, 4).T[:3, :3]


def true_norm(mv):
    return float(np.linalg.svd(mat3_of(mv), compute_uv=False)[0])


def rotation(g):
    q, r = np.linalg.qr(g.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def orthogonal_family(g, d, s, U=None, v1=None):
    """A = U diag(s, 1, 1) V^T with V's first column (v1, or a random one) orthogonal to d, its other axes random"""
    d = np.asarray(d, np.float64) / np.linalg.norm(d)
    v1 = np.cross(d, g.normal(size=3)) if v1 is None else np.asarray(v1, np.float64)
    assert abs(v1 @ d) < 1e-12 or v1 is None
    v1 = v1 / np.linalg.norm(v1)
    v2 = np.cross(d, v1)                                    # (d, v1, v2 orthonormal; turn v2, d about v1)
    a = g.uniform(0.0, 2.0 * math.pi)
    V = np.stack([v1, math.cos(a) * v2 + math.sin(a) * d, -math.sin(a) * v2 + math.cos(a) * d], 1)
    U = rotation(g) if U is None else U
    return U @ np.diag([s, 1.0, 1.0]) @ V.T


@pytest.fixture(scope="module")
def lib(hc):
    hc.hc_norm_bound.restype = C.c_float
    hc.hc_norm_bound.argtypes = [C.c_void_p]
    hc.hc_reach_sweep.restype = C.c_int64
    hc.hc_reach_sweep.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int,
                                  C.c_float, C.c_int, C.c_void_p, C.c_void_p]
    hc.hc_strip_uniforms.restype = C.c_int
    hc.hc_strip_uniforms.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p]
    return hc


def _ratios(lib, mats):
    mvs = np.stack([mv_of(A) for A in mats])
    t = np.linalg.svd(mvs.astype(np.float64).reshape(-1, 4, 4)[:, :3, :3], compute_uv=False)[:, 0]      # (the transpose has the same norm)
    new = np.array([float(lib.hc_norm_bound(_p(mv))) for mv in mvs])
    return new / t, old_norm(mvs).astype(np.float64) / t


S_FAMILY = (1.02, 1.05, 1.1, 1.15, 1.2, 1.3, 2.0, 10.0)


def test_norm_bound_brackets_the_spectral_norm(lib):
    """1 <= bound / ||A||_2 <= 1.03 on every family; the parent's formula (old_norm) fails 494 of the 1 600 cases of (b), 2 of the
    6 400 of (c) and none of (a), (d), (e): its numbers are printed and the failures of (b) asserted to exist."""
    g = np.random.Generator(np.random.PCG64(20261020))
    fam = {}
    fam["a random"] = [g.normal(size=(3, 3)) * np.exp(g.uniform(math.log(0.1), math.log(10.0), 3))[None, :] for _ in range(20000)]
    fam["b orthogonal to the start"] = [orthogonal_family(g, START, s) for s in S_FAMILY for _ in range(200)]
    fam["c orthogonal to axes and (1,1,1)"] = [orthogonal_family(g, d, s) for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1))
                                             for s in S_FAMILY for _ in range(200)]
    fam["d rotations times scales"] = [rotation(g) * k for k in (0.01, 1.0, 10.0, 1000.0) for _ in range(100)]
    u, v = g.normal(size=3), g.normal(size=3)
    fam["e rank 1, rank 2"] = [np.outer(u, v), np.outer(u, v) + np.outer(g.normal(size=3), g.normal(size=3)), np.outer(u, v) * 1e-20,
                               np.diag([0.0, 0.0, 5.0]), np.diag([2.0, 0.0, 2.0]), np.outer(u, v) * 1e15]
    old_fail = {}
    for name, mats in fam.items():
        new, old = _ratios(lib, mats)
        old_fail[name] = int((old < 1.0).sum())
        print("norm %-34s %6d cases: new %.5f .. %.5f, parent %.5f .. %.5f, parent below the norm in %d" % (
            name, len(mats), new.min(), new.max(), old.min(), old.max(), old_fail[name]))
        if name.startswith("b"):
            o = old.reshape(len(S_FAMILY), 200)
            print("   parent, lowest ratio by s:", {s: round(float(o[k].min()), 4) for k, s in enumerate(S_FAMILY)},
                  "failing by s:", {s: int((o[k] < 1.0).sum()) for k, s in enumerate(S_FAMILY)})
        assert new.min() >= 1.0 and new.max() <= 1.03, (name, new.min(), new.max())
    assert old_fail["b orthogonal to the start"] > 0, "the restated parent formula no longer shows the bug this test is for"
    # zero, and entries that are not finite
    z = np.zeros(16, np.float32)
    assert float(lib.hc_norm_bound(_p(z))) == 0.0
    su = np.zeros(31, np.float32)
    eye = mv_of(np.eye(3))
    P = synth.perspective(80.0, 16 / 9).astype(np.float32)
    assert lib.hc_strip_uniforms(_p(eye), _p(P), 100.0, 640.0, 360.0, 0, 80, _p(su)) == 1 and np.all(np.isfinite(su))
    assert lib.hc_strip_uniforms(_p(z), _p(P), 100.0, 640.0, 360.0, 0, 80, _p(su)) == 1 and np.all(np.isfinite(su))
    for bad in (np.nan, np.inf, -np.inf):
        for k in (0, 5, 10, 6):
            m = eye.copy(); m[k] = bad
            assert not np.isfinite(lib.hc_norm_bound(_p(m)))
            assert lib.hc_strip_uniforms(_p(m), _p(P), 100.0, 640.0, 360.0, 0, 80, _p(su)) == 0, (bad, k)
    big = mv_of(np.eye(3) * 3.0e38)                          # finite, and so is 1.0001 x 3e38
    assert np.isfinite(lib.hc_norm_bound(_p(big))) and float(lib.hc_norm_bound(_p(big))) >= 3.0e38


# ---------------------------------------------------------------- poses

def _cam_world(pitch, roll, yaw, pos):
    cy, sy = math.cos(math.radians(yaw)), math.sin(math.radians(yaw))
    cx, sx = math.cos(math.radians(pitch)), math.sin(math.radians(pitch))
    cz, sz = math.cos(math.radians(roll)), math.sin(math.radians(roll))
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    M = np.eye(4); M[:3, :3] = Ry @ Rx @ Rz; M[:3, 3] = pos
    return M.T.reshape(-1).copy()


# yaw-only, then the four of test_gpu_parity._tilted_camera: (pitch, roll, yaw, position)
CAMERAS = [(0.0, 0.0, 25.0, (0.0, 1.6, 0.0)), (35.0, 20.0, 0.0, (0.0, 1.6, 0.0)), (-50.0, -75.0, 160.0, (0.5, 3.0, -4.5)),
           (80.0, 5.0, 0.0, (0.0, -2.0, -2.0)), (0.0, 90.0, 30.0, (3.0, 1.5, 1.0))]
T_GENERIC = (0.1, -0.2, -3.0)


def _finish(u, kind):
    return {"mv": u["gs_mv"].astype(np.float32), "proj": u["gs_proj"].astype(np.float32), "focal": np.float32(u["focal"]), "kind": kind,
            "view": u["view"]}


def _generic(A, kind):
    def make(W, H):
        proj = synth.perspective(80.0, W / H)
        gp = (proj.reshape(4, 4).T @ np.diag([1.0, -1.0, 1.0, 1.0])).T.reshape(-1)
        mv = mv_of(A, T_GENERIC)
        return {"mv": mv, "proj": gp.astype(np.float32), "focal": np.float32((H / 2.0) * abs(gp[5])), "kind": kind,
                "view": np.array([mv[2], mv[6], mv[10], mv[14]], np.float32)}
    return make


def _rigid(scale, cam):
    def make(W, H):
        return _finish(synth.uniforms(_cam_world(*cam), synth.compose((0.0, 1.5, -2.0), 10.0, (scale,) * 3), synth.perspective(80.0, W / H), W, H), "rigid")
    return make


def _xr(eye):
    def make(W, H):
        # synth.xr_eye_cameras' own eye matrices (canted 12 degrees, object yaw 30); only the focal length follows this test's frame height
        eyes = synth.xr_eye_cameras(30.0, 0.25, cant_deg=12.0)
        u = dict(eyes[eye])
        u["focal"] = (H / 2.0) * abs(u["gs_proj"][5])
        p = _finish(u, "xr")
        p["view"] = eyes[2]["view"]                             # the sort of an XR frame uses the head camera's view row (index.js:441)
        return p
    return make


# orthogonal to START with components of nearly equal size: a needle along it has 3 max|Sigma_ij| = 1.097 lambda_max, so k_pack's bound_r
# is 4.7 % above its true sigma and hides little of the norm's error (a needle along an axis: 0 %; one along (0.9, 0.4, 0.1): 60 %)
V1_SPREAD = np.array([1.0, -6.0 / 7.0, -1.0])


def _worst_draw(g, s, U, tries=300):
    """of `tries` draws of the family orthogonal to START, the one the parent's formula underestimates most once rounded to f32 (the
    rounding leaves the top vector orthogonal to within 1e-8 or so, and 64 iterations amplify that by s^128: the test picks its pose)"""
    As = [orthogonal_family(g, START, s, U if U is not None else rotation(g), V1_SPREAD) for _ in range(tries)]
    mvs = np.stack([mv_of(A) for A in As])
    t = np.linalg.svd(mvs.astype(np.float64).reshape(-1, 4, 4)[:, :3, :3], compute_uv=False)[:, 0]
    return As[int(np.argmin(old_norm(mvs) / t))]


def _poses():
    g = np.random.Generator(np.random.PCG64(99))
    P = {}
    for sc in (0.1, 1.0, 10.0):
        for k, cam in enumerate(CAMERAS):
            P["rigid_%g_cam%d" % (sc, k)] = _rigid(sc, cam)
    P["rigid_1_off_axis_1e-3"] = _generic(np.array(_cam_world(math.degrees(1e-3), math.degrees(1e-3), 0.0, (0, 0, 0))).reshape(4, 4).T[:3, :3], "rigid")
    for name, s in (("113", (1.0, 1.0, 3.0)), ("311", (3.0, 1.0, 1.0)), ("1.15", (1.15, 1.0, 1.0)), ("1.2", (1.2, 1.0, 1.0))):
        P["scale_" + name] = _generic(np.diag(s), "scale")
    ex = np.eye(3)                                               # U e_1 = camera x
    ey = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])   # U e_1 = camera y (a rotation: det +1)
    P["b_x_1.15"] = _generic(_worst_draw(g, 1.15, ex), "b")
    P["b_y_1.15"] = _generic(_worst_draw(g, 1.15, ey), "b")
    P["b_x_3"] = _generic(_worst_draw(g, 3.0, ex), "b")
    P["b_skew_1.1"] = _generic(_worst_draw(g, 1.1, None), "b")          # askew to the camera
    P["shear"] = _generic(np.array([[1.0, 0.8, 0.0], [0.0, 1.0, 0.3], [0.0, 0.0, 1.0]]), "shear")
    P["xr_left"] = _xr(0)
    P["xr_right"] = _xr(1)
    # (1, 1, 3) in a rotated frame of the family: the stretched axis mapped onto the camera's view axis (the name sorts last: the seeds
    # of the other poses' rows follow the sorted names)
    ezu = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]])                     # U e_1 = -camera z (a rotation)
    P["zb_z_3"] = _generic(_worst_draw(g, 3.0, ezu), "b")
    return P


POSES = _poses()
GPU_POSES = ("rigid_1_cam1", "scale_113", "b_x_1.15", "b_y_1.15", "xr_left")


# ---------------------------------------------------------------- splats

def _quat_bytes():
    """13 orientations as the row's bytes (w, x, y, z at 128 + 128 q, clipped): the axes, 45 and 90 degrees about each, the smallest tilt
    the bytes can say (one step, 0.016 rad) about each, and three askew"""
    h = math.sqrt(0.5)
    qs = [(1, 0, 0, 0), (h, h, 0, 0), (h, 0, h, 0), (h, 0, 0, h), (0.92388, 0.38268, 0, 0), (0.92388, 0, 0.38268, 0), (0.92388, 0, 0, 0.38268)]
    out = [tuple(int(min(255, max(0, round(128 + 127 * c)))) for c in q) for q in qs]
    out += [(255, 129, 128, 128), (255, 128, 129, 128), (255, 128, 128, 127)]
    out += [(200, 60, 170, 110), (90, 210, 150, 40), (160, 100, 30, 220)]
    return np.array(out, np.uint8)


QUATS = _quat_bytes()


def make_rows(pos_obj, scales, quats, alpha=200):
    """.splat rows from object-space centres in the packed convention (cs = (x, y, z): the row stores (x, y, -z))"""
    n = pos_obj.shape[0]
    rows = np.zeros((n, 32), np.uint8)
    p = np.array(pos_obj, np.float64, order="C"); p[:, 2] = -p[:, 2]
    rows[:, 0:12] = p.astype("<f4").view(np.uint8).reshape(n, 12)
    rows[:, 12:24] = np.asarray(scales, np.float64).astype("<f4").view(np.uint8).reshape(n, 12)
    rows[:, 24:27] = (np.arange(n)[:, None] * np.array([37, 59, 83]) % 200 + 55).astype(np.uint8)
    rows[:, 27] = alpha
    rows[:, 28:32] = quats
    return rows


def cam_to_obj(pose, cam):
    m = pose["mv"].astype(np.float64).reshape(4, 4).T
    return (np.linalg.inv(m[:3, :3]) @ (np.asarray(cam, np.float64) - m[:3, 3]).T).T


def cam_from_ndc(pose, ndcx, ndcy, depth):
    gp = pose["proj"].astype(np.float64)
    return np.stack([(ndcx + gp[8]) * depth / gp[0], (ndcy + gp[9]) * depth / gp[5], -depth], 1)


def _shapes(g, pose, n, depth):
    """(scales, quaternion bytes): isotropic in object units, isotropic by screen size, needles and discs"""
    a = float(np.linalg.svd(mat3_of(pose["mv"]), compute_uv=False)[0])
    px = np.exp(g.uniform(math.log(0.1), math.log(300.0), n))                  # wanted screen sigma
    by_px = px * depth / (float(pose["focal"]) * a)
    sig = np.where(g.random(n) < 0.3, np.exp(g.uniform(math.log(1e-4), math.log(100.0), n)), by_px)
    kind = g.integers(0, 4, n)                                                 # 0, 1: isotropic; 2: needle; 3: disc
    sc = np.stack([sig, sig, sig], 1)
    sc[kind == 2, 1:] *= 1e-3
    sc[kind == 3, 2] *= 1e-3
    q = QUATS[g.integers(0, len(QUATS), n)]
    return sc, q


def base_rows(pose, W, H, seed, n=N_BASE):
    g = np.random.Generator(np.random.PCG64(seed))
    k = g.random(n)
    depth = np.exp(g.uniform(math.log(0.05), math.log(50.0), n))
    nx, ny = g.uniform(-1.5, 1.5, n), g.uniform(-1.5, 1.5, n)
    inside = k < 0.2
    nx[inside] *= 0.6; ny[inside] *= 0.6
    cull = (k >= 0.2) & (k < 0.32)                                           # on the |px| = 1.2 pw and |py| = 1.2 pw planes
    edge = g.choice([-1.2, 1.2], n) * (1.0 + g.choice([0.0, 1e-6, -1e-6, 1e-3, -1e-3], n))
    onx = g.random(n) < 0.5
    nx[cull & onx] = edge[cull & onx]; ny[cull & ~onx] = edge[cull & ~onx]
    nx[cull & ~onx] *= 0.6; ny[cull & onx] *= 0.6
    cam = cam_from_ndc(pose, nx, ny, depth)
    near = (k >= 0.32) & (k < 0.40)                                          # camz = -1e-3 .. -1e-6, and behind the camera
    z = g.choice([-1e-3, -1e-4, -1e-5, -1e-6, 1e-3, 0.5], n)
    cam[near, 2] = z[near]
    cam[near, 0] = g.uniform(-2e-3, 2e-3, n)[near]; cam[near, 1] = g.uniform(-2e-3, 2e-3, n)[near]
    sc, q = _shapes(g, pose, n, depth)
    big = cull & (g.random(n) < 0.7)                                          # wide enough to reach the frame from the cull plane
    a = float(np.linalg.svd(mat3_of(pose["mv"]), compute_uv=False)[0])
    sc[big] = (g.uniform(0.05, 0.5, n) * W * depth / (float(pose["focal"]) * a))[big, None] * (sc[big] / sc[big].max(1, keepdims=True))
    return make_rows(cam_to_obj(pose, cam), sc, q)


def pack(lib, rows):
    n = rows.shape[0]
    cs = np.zeros((n, 4), np.float32); cc = np.zeros((n, 4), np.uint32); sr = np.zeros((n, 4), np.float32)
    lib.hc_pack(_p(np.ascontiguousarray(rows)), n, _p(cs), _p(cc), _p(sr))
    return cs, cc


def project64(cs_pos, cc, scl, pose, W, H):
    """project_splat in f64, vectorised: centre (GL pixels) and the half extents of the |p| <= 2 ellipse in x and y"""
    mv = pose["mv"].astype(np.float64).reshape(4, 4).T; P = pose["proj"].astype(np.float64).reshape(4, 4).T
    f = float(pose["focal"])
    cam = cs_pos @ mv[:3, :3].T + mv[:3, 3]
    clip = np.concatenate([cam, np.ones((cam.shape[0], 1))], 1) @ P.T
    h = lambda w, hi: ((w >> (16 if hi else 0)) & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.float64) * scl
    m11, m12, m13, m22, m23, m33 = h(cc[:, 0], 0), h(cc[:, 0], 1), h(cc[:, 1], 0), h(cc[:, 1], 1), h(cc[:, 2], 0), h(cc[:, 2], 1)
    Sg = np.stack([np.stack([m11, m12, m13], 1), np.stack([m12, m22, m23], 1), np.stack([m13, m23, m33], 1)], 1)
    z = cam[:, 2]
    J = np.zeros((cam.shape[0], 2, 3))
    J[:, 0, 0] = f / z; J[:, 0, 2] = -(f * cam[:, 0]) / (z * z)
    J[:, 1, 1] = -f / z; J[:, 1, 2] = (f * cam[:, 1]) / (z * z)
    M = J @ mv[:3, :3]
    cov = M @ Sg @ np.transpose(M, (0, 2, 1))
    d1, od, d2 = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    mid, rad = 0.5 * (d1 + d2), np.sqrt(((d1 - d2) / 2.0) ** 2 + od * od)
    l1, l2 = mid + rad, np.maximum(mid - rad, 0.1)
    dv = np.stack([od, l1 - d1], 1)
    ln = np.linalg.norm(dv, axis=1); ln[ln == 0] = 1.0
    dv = dv / ln[:, None]
    s1, s2 = np.minimum(np.sqrt(2 * l1), 1024.0), np.minimum(np.sqrt(2 * l2), 1024.0)
    hw = 2.0 * np.sqrt((s1 * dv[:, 0]) ** 2 + (s2 * dv[:, 1]) ** 2)
    hh = 2.0 * np.sqrt((s1 * dv[:, 1]) ** 2 + (s2 * dv[:, 0]) ** 2)
    w = clip[:, 3]
    return (clip[:, 0] / w * 0.5 + 0.5) * W, (clip[:, 1] / w * 0.5 + 0.5) * H, hw, hh


def family_needle_quat(lib, pose):
    """the quaternion bytes whose needle (scale 1 : 1e-3 : 1e-3) lies closest to the top right-singular vector of the pose's mat3:
    found by packing 20 000 random byte quadruples and reading the covariance back"""
    g = np.random.Generator(np.random.PCG64(4242))
    q = g.integers(1, 256, (20000, 4)).astype(np.uint8)
    rows = make_rows(np.zeros((q.shape[0], 3)), np.tile([1.0, 1e-3, 1e-3], (q.shape[0], 1)), q)
    cs, cc = pack(lib, rows)
    h = lambda w, hi: ((w >> (16 if hi else 0)) & 0xFFFF).astype(np.uint16).view(np.int16).astype(np.float64)
    d = np.stack([h(cc[:, 0], 0), h(cc[:, 1], 1), h(cc[:, 2], 1)], 1)          # the diagonal: v_i^2 up to scale
    s01, s02 = np.sign(h(cc[:, 0], 1)), np.sign(h(cc[:, 1], 0))
    v = np.sqrt(np.maximum(d, 0.0)); v[:, 1] *= np.where(s01 < 0, -1, 1); v[:, 2] *= np.where(s02 < 0, -1, 1)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    top = np.linalg.svd(mat3_of(pose["mv"]))[2][0]
    return q[int(np.argmax(np.abs(v @ top)))]


def grazing_rows(lib, pose, W, H, x0, x1, seed):
    """Per edge (the strip's two, the frame's bottom and top), offset (2 and 0.5 px inside, 0.5 px outside) and shape: the centre
    moved along camera x (y) until the ellipse of the f64 projection ends there.  Solved by bisection on the shift; rows whose
    bracket holds no sign change (the 1024 clamp wider than the frame) stay at the bracket's end."""
    g = np.random.Generator(np.random.PCG64(seed))
    a = float(np.linalg.svd(mat3_of(pose["mv"]), compute_uv=False)[0])
    f = float(pose["focal"])
    qfam = family_needle_quat(lib, pose) if pose["kind"] in ("b", "scale", "shear") else QUATS[10]
    spec = []
    for edge in range(4):
        # ... and the size that puts the centre on the principal point, where the Jacobian's norm is attained by every direction and the
        # reach has the least slack: half extent = the edge's distance from the frame's centre
        princ = abs((x0, x1)[edge] - 0.5 * W) if edge < 2 else 0.5 * H
        for off in (2.0, 0.5, -0.5):
            for half_px in (1.0, 20.0, 150.0, 400.0, princ, princ):
                for shape in range(3):                                          # isotropic, needle along the pose's top vector, disc
                    spec.append((edge, off, max(half_px, 1.0), shape, float(np.exp(g.uniform(math.log(0.3), math.log(10.0)))), half_px == princ))
    n = len(spec)
    depth = np.array([s[4] for s in spec])
    want = np.array([s[2] for s in spec])
    edge = np.array([s[0] for s in spec]); off = np.array([s[1] for s in spec])
    along_x = edge < 2
    sig = want / (2.0 * math.sqrt(2.0)) * depth / (f * a)
    sc = np.stack([sig, sig, sig], 1)
    q = np.tile(QUATS[11], (n, 1))
    for k, s in enumerate(spec):
        if s[3] == 1:
            sc[k, 1:] *= 1e-3; q[k] = qfam
        elif s[3] == 2:
            sc[k, 2] *= 1e-3; q[k] = QUATS[g.integers(0, len(QUATS))]
    spread = np.where([s[5] for s in spec], 0.03, 0.5)
    c0 = cam_from_ndc(pose, g.uniform(-1.0, 1.0, n) * spread, g.uniform(-1.0, 1.0, n) * spread, depth)
    # the bytes' quaternion is not normalised and the pose stretches: one step of rescaling towards the half extent asked for
    cs, cc = pack(lib, make_rows(np.zeros((n, 3)), sc, q))
    _, _, hw0, hh0 = project64(cam_to_obj(pose, c0), cc, cs[:, 3].astype(np.float64), pose, W, H)
    ext0 = np.where(along_x, hw0, hh0)
    sc *= np.where((want >= 20.0) & (ext0 > 0.0), want / np.where(ext0 > 0.0, ext0, 1.0), 1.0)[:, None]
    rows = make_rows(np.zeros((n, 3)), sc, q)
    cs, cc = pack(lib, rows)
    gp = pose["proj"].astype(np.float64)
    span = 3.0 * depth / np.where(along_x, abs(gp[0]), abs(gp[5])) + 12.0 * sc.max(1) * a

    def fn(s):
        cam = c0.copy()
        cam[:, 0] += np.where(along_x, s, 0.0); cam[:, 1] += np.where(along_x, 0.0, s)
        cx, cy, hw, hh = project64(cam_to_obj(pose, cam), cc, cs[:, 3].astype(np.float64), pose, W, H)
        # edges 0, 1: the strip's left (splat on its left) and right; 2, 3: the frame's bottom (GL y = 0) and top
        return np.select([edge == 0, edge == 1, edge == 2, edge == 3],
                         [cx + hw - (x0 + off), (x1 - off) - (cx - hw), cy + hh - off, (H - off) - (cy - hh)]), cam
    # f > 0: the ellipse is past the target, into the strip.  Bracket: from the shift that puts it deepest to the one that takes it furthest out
    grid = np.linspace(-1.0, 1.0, 41)[:, None] * span[None, :]
    vals = np.stack([fn(s)[0] for s in grid])
    lo, hi = np.zeros(n), np.zeros(n)
    for k in range(n):
        v = vals[:, k]
        ch = np.nonzero((v[:-1] > 0) != (v[1:] > 0))[0]
        j = int(ch[len(ch) // 2]) if ch.size else 0
        lo[k], hi[k] = grid[j, k], grid[j + 1 if ch.size else j, k]
    flo = fn(lo)[0]
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        fm = fn(mid)[0]
        same = (fm > 0) == (flo > 0)
        lo, flo, hi = np.where(same, mid, lo), np.where(same, fm, flo), np.where(same, hi, mid)
    cam = fn(0.5 * (lo + hi))[1]
    return make_rows(cam_to_obj(pose, cam), sc, q)


def case_rows(lib, name, W, H, x0, x1):
    """the rows of one case: the (pose, frame)'s base rows, then the strip's grazing rows; deterministic in its arguments"""
    pose = POSES[name](W, H)
    seed = (sorted(POSES).index(name) * 1000 + W) * 1000
    rows = np.concatenate([base_rows(pose, W, H, seed), grazing_rows(lib, pose, W, H, x0, x1, seed + 1 + x0 * 7 + x1)])
    return pose, np.ascontiguousarray(rows)


def sweep(lib, pose, rows, W, H, x0, x1, norm=0.0, nine=1):
    out = np.zeros(10, np.int64)
    flags = np.zeros(rows.shape[0], np.uint8)
    rc = lib.hc_reach_sweep(_p(rows), rows.shape[0], _p(pose["mv"]), _p(pose["proj"]), float(pose["focal"]), W, H, x0, x1, float(norm), nine,
                            _p(out), _p(flags))
    assert rc == out[0] and rc >= 0, rc
    return dict(misses=int(out[0]), truth=int(out[1]), kept=int(out[2]), truth_kept=int(out[3]), neither=int(out[4]), n=rows.shape[0],
                first=dict(zip(("row", "px", "image_row", "ulp_rcp", "ulp_sqrt"), out[5:10].tolist())), flags=flags)


@pytest.fixture(scope="module")
def results(lib):
    """every case swept once: with the product's bound in nine settings, and with the parent's norm (same nine)"""
    res = {}
    for name in POSES:
        for (W, H), strips in FRAMES:
            for x0, x1 in strips:
                pose, rows = case_rows(lib, name, W, H, x0, x1)
                new = sweep(lib, pose, rows, W, H, x0, x1)
                old = sweep(lib, pose, rows, W, H, x0, x1, norm=float(old_norm(pose["mv"])))
                res[(name, W, H, x0, x1)] = (pose, rows, new, old)
    return res


def test_reach_is_a_superset_in_all_nine_ulp_settings(results):
    total = 0
    for key, (pose, rows, new, old) in results.items():
        f = new["first"]
        assert new["misses"] == 0, "%s: %d misses; first: row %d %s pixel (%d, image row %d) ulp(rcp, sqrt) = (%d, %d)" % (
            key, new["misses"], f["row"], rows[f["row"]].tobytes().hex() if f["row"] >= 0 else None, f["px"], f["image_row"], f["ulp_rcp"], f["ulp_sqrt"])
        total += new["n"]
    print("reach sweep: %d splat-cases, 0 misses" % total)
    assert total >= 150000


def test_every_pose_has_live_cases(results):
    """per pose, at least a tenth of the cases are truth and kept, and at least a tenth neither: a sweep of splats that all reach the
    strip, or none, proves nothing"""
    share = {}
    for (name, W, H, x0, x1), (_, _, new, _) in results.items():
        a = share.setdefault(name, [0, 0, 0])
        a[0] += new["truth_kept"]; a[1] += new["neither"]; a[2] += new["n"]
    for name, (tk, ne, n) in sorted(share.items()):
        print("live %-24s truth and kept %.3f, neither %.3f of %d" % (name, tk / n, ne / n, n))
    print("live: truth and kept %.3f .. %.3f, neither %.3f .. %.3f" % (min(v[0] / v[2] for v in share.values()), max(v[0] / v[2] for v in share.values()),
                                                                      min(v[1] / v[2] for v in share.values()), max(v[1] / v[2] for v in share.values())))
    for name, (tk, ne, n) in share.items():
        assert tk >= LIVE_SHARE * n and ne >= LIVE_SHARE * n, (name, tk, ne, n)


def test_the_new_bound_culls_as_tightly_as_the_parents_on_rigid_poses(results):
    """kept / truth over the rigid poses and the strips no wider than W / 4: at most 1.1 x what the parent's norm gives on the same
    cases (PARENT_TIGHTNESS, measured; recomputed here and compared with the constant).  A fix that keeps everything fails this."""
    kn = ko = tr = 0
    for (name, W, H, x0, x1), (pose, _, new, old) in results.items():
        if pose["kind"] == "rigid" and x1 - x0 <= W // 4:
            kn += new["kept"]; ko += old["kept"]; tr += new["truth"]
    print("tightness on rigid poses, strips <= W/4: truth %d, kept with the parent's norm %d (%.4f), with the new bound %d (%.4f)" % (
        tr, ko, ko / tr, kn, kn / tr))
    assert abs(ko / tr - PARENT_TIGHTNESS) <= 0.01 * PARENT_TIGHTNESS, (ko / tr, PARENT_TIGHTNESS)
    assert kn / tr <= 1.1 * PARENT_TIGHTNESS, (kn / tr, PARENT_TIGHTNESS)
    assert kn >= tr


def test_the_parents_norm_misses_on_the_orthogonal_family(results):
    """the demonstration: the same sweep, the same strip_may_touch, the parent's norm_a -- splats culled that cover pixels of the strip"""
    miss = {}
    for (name, W, H, x0, x1), (pose, _, new, old) in results.items():
        if pose["kind"] == "b":
            miss[name] = miss.get(name, 0) + old["misses"]
        else:
            assert old["misses"] == 0 or pose["kind"] != "rigid", (name, old["misses"])     # (rigid poses: the parent's norm was right)
    print("misses with the parent's norm on the orthogonal family:", miss, "total", sum(miss.values()))
    # (only a strip's edges can show it: at the frame's top and bottom a splat that grazes the edge has its centre outside the frame,
    # where the Jacobian's norm exceeds what a needle along y uses by 1.3 or more -- b_y_1.15 has no misses to show)
    assert miss["b_x_1.15"] > 0, miss


def test_the_sweep_counts_what_it_claims_to_count(lib):
    """known answers: a fat splat at the frame's centre is truth and kept in every strip; a small one far left of the frame is neither;
    a strip that cannot be tested (focal 0) is reported as such"""
    W, H = 77, 53
    pose = POSES["rigid_1_cam0"](W, H)
    cam = cam_from_ndc(pose, np.array([0.0, -3.0]), np.array([0.0, 0.0]), np.array([2.0, 2.0]))
    rows = make_rows(cam_to_obj(pose, cam), np.array([[3.0, 2.0, 1.0], [1e-3, 2e-3, 1e-3]]), QUATS[[10, 11]])
    for x0, x1 in FRAMES[1][1]:
        r = sweep(lib, pose, rows, W, H, x0, x1)
        assert r["misses"] == 0 and r["flags"].tolist() == [7, 0], (x0, x1, r["flags"].tolist())
    out = np.zeros(10, np.int64)
    assert lib.hc_reach_sweep(_p(rows), 2, _p(pose["mv"]), _p(pose["proj"]), 0.0, W, H, 0, 16, 0.0, 1, _p(out), None) == -2
    # and a miss is reported: a norm a hundred times too small culls the fat splat from a strip beside its centre
    r = sweep(lib, pose, rows[:1], W, H, 0, 16, norm=0.01 * true_norm(pose["mv"]))
    assert r["misses"] == 9 and r["first"]["row"] == 0 and 0 <= r["first"]["px"] < 16
