"""CPU tier: the exits of gsm::project_splat (csrc/gs_device_math.h; index.js:101-164) placed on their boundaries.  A crafted scene per
frame size -- 640 x 360 under a translation-only pose (so that head-on isotropic splats have cov01 == 0 exactly), 77 x 53 under a pitched
and rolled rigid pose -- whose centres are solved in f64 along a ray until a cull quantity crosses its threshold, then moved by single
ulps of one coordinate until the f32 expression tree (restated in numpy f32, un-fused, the header's order) puts the quantity 0, +-1 and
+-16 ulp from the threshold, or as near to that as f32 allows; what f32 gives is kept and counted per side.  The quantities, each
against its threshold as the header compares them: pz against -pw, px and py against -+(1.2f * pw), pw against 0, zndc against 1.
Then: isotropic splats seen head-on (cov01 == 0 and len == 0: the reference draws nothing), splats on the 1024 clamp, long needles
(whose 16-bit covariances put some short axes on the l2 = 0.1 clamp), scales that make l1 or the covariance scale infinite, NaN and
Inf positions, and plain visible splats.

hc_project (the header's host build) must equal oracle.project on EVERY row: the visible flag and the eight words of the record (cx, cy,
ax, ay, bx, by, the colour word, alpha).  Every exit must have at least 8 rows strictly on each side of its threshold (pw against 0:
on or below, and above -- with a projection whose last row is (0, 0, -1, 0) pw is -camz, whose neighbours of 0 are whole ulps of the
translation away).

Measured: 578 rows per frame (280 on thresholds); per exit 16 rows below, 8 on and 16 above (pz against -pw: 16 / 0 / 24 and 24 / 0 / 16:
one ulp of a coordinate is ~1000 ulps of that quantity; zndc lands exactly on 16 of its 40 targets: 1 + 16 ulp is beyond what the
projection can give); visible 377 and 394; on the 1024 clamp 46 and 54, on the l2 clamp 20 and 20; of the 24 head-on rows with
camy == 0 in the 640 x 360 frame 18 are invisible (len == 0) -- the others get an eigenvector out of one rounding of mid + radius, in the
oracle as in the header; no disagreement between header and oracle on any row; the file in 1.3 s."""
import numpy as np
import pytest

from oracle import oracle
from test_host_check import _p, hc  # noqa: F401
from test_reach_cpu import POSES, QUATS, _generic, cam_from_ndc, cam_to_obj, lib, make_rows  # noqa: F401

FRAMES = [(640, 360), (77, 53)]
TARGETS = (0, 1, -1, 16, -16)
EXITS = ("pz|-pw", "px|-b", "px|+b", "py|-b", "py|+b", "pw|0", "zndc|1")
MIN_SIDE = 8


def pose_of(W, H):
    return _generic(np.eye(3), "edges")(W, H) if W == 640 else POSES["rigid_1_cam1"](W, H)


def tree(xyz, mv, P):
    """the header's f32 expression tree for (px, py, pz, pw) and zndc, un-fused, in its order; xyz: float32 [n, 3]"""
    f = np.float32
    x, y, z = (np.asarray(xyz, f)[:, k] for k in range(3))
    mv, P = np.asarray(mv, f), np.asarray(P, f)
    with np.errstate(all="ignore"):
        cam = [((mv[r] * x + mv[4 + r] * y) + mv[8 + r] * z) + mv[12 + r] for r in range(4)]
        p = [((P[r] * cam[0] + P[4 + r] * cam[1]) + P[8 + r] * cam[2]) + P[12 + r] * cam[3] for r in range(4)]
        b = f(1.2) * p[3]
        return p[0], p[1], p[2], p[3], b, p[2] / p[3]


def ordered(a):
    i = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, -(i & 0x7FFFFFFF))


def from_ordered(o):
    o = np.asarray(o, np.int64)
    return np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32).view(np.float32)


def quantities(xyz, mv, P):
    """per exit: ulps of the quantity above its threshold (int64; meaningless where either is NaN)"""
    px, py, pz, pw, b, zn = tree(xyz, mv, P)
    one, zero = np.float32(1.0), np.float32(0.0)
    return {"pz|-pw": ordered(pz) - ordered(-pw), "px|-b": ordered(px) - ordered(-b), "px|+b": ordered(px) - ordered(b),
            "py|-b": ordered(py) - ordered(-b), "py|+b": ordered(py) - ordered(b), "pw|0": ordered(pw) - ordered(np.full_like(pw, zero)),
            "zndc|1": ordered(zn) - ordered(np.full_like(zn, one))}


def _threshold_rows(pose, W, H, g):
    """(object-space centres f32 [n, 3], scales [n, 3]) for every exit x target x 8 rays"""
    mv, P, f = pose["mv"], pose["proj"], float(pose["focal"])
    mv64, P64 = mv.astype(np.float64).reshape(4, 4).T, P.astype(np.float64).reshape(4, 4).T
    cen, scl = [], []

    def g64(exit_, cam):
        clip = P64 @ np.append(cam, 1.0)
        clip[3] = clip[3] if clip[3] != 0.0 else 1e-300
        return {"pz|-pw": clip[2] + clip[3], "px|-b": clip[0] + 1.2 * clip[3], "px|+b": clip[0] - 1.2 * clip[3], "py|-b": clip[1] + 1.2 * clip[3],
                "py|+b": clip[1] - 1.2 * clip[3], "pw|0": clip[3], "zndc|1": clip[2] / clip[3] - 1.0}[exit_]

    for e in EXITS:
        for tgt in TARGETS:
            for ray in range(8):
                u, v = g.uniform(-0.5, 0.5, 2)
                if e == "pz|-pw":
                    a, b_ = cam_from_ndc(pose, np.array([u]), np.array([v]), np.array([1e-3]))[0], cam_from_ndc(pose, np.array([u]), np.array([v]), np.array([1.0]))[0]
                elif e == "zndc|1":
                    a, b_ = cam_from_ndc(pose, np.array([u]), np.array([v]), np.array([3000.0]))[0], cam_from_ndc(pose, np.array([u]), np.array([v]), np.array([30000.0]))[0]
                elif e == "pw|0":
                    a, b_ = np.array([0.0, 0.0, -1e-3]), np.array([0.0, 0.0, 1e-3])
                else:
                    d = float(np.exp(g.uniform(np.log(1.0), np.log(8.0))))
                    s = -1.0 if e.endswith("-b") else 1.0
                    n0, n1 = ((0.0, v), (2.0 * s, v)) if e.startswith("px") else ((u, 0.0), (u, 2.0 * s))
                    a, b_ = (cam_from_ndc(pose, np.array([n[0]]), np.array([n[1]]), np.array([d]))[0] for n in (n0, n1))
                ga = g64(e, a)
                for _ in range(80):                                     # bisection in f64 along the ray
                    m = 0.5 * (a + b_)
                    if (g64(e, m) > 0) == (ga > 0):
                        a = m
                    else:
                        b_ = m
                obj = cam_to_obj(pose, a[None, :])[0].astype(np.float32)
                # single ulps of the coordinate the quantity depends on most: the f32 tree decides
                best = None
                for k in range(3):
                    cand = np.tile(obj, (513, 1))
                    steps = np.arange(-256, 257)
                    o = ordered(cand[:, k]) + steps * (32768 if e == "zndc|1" else 1)    # (zndc moves by one ulp per ~1000 units of depth at the far plane)
                    cand[:, k] = from_ordered(o)
                    q = quantities(cand, mv, P)[e]
                    # the nearest to the target ON THE TARGET'S SIDE of the threshold (a coordinate's ulp may be many ulps of the quantity)
                    cost = np.abs(q - tgt) * 1024 + np.abs(steps) + np.where((tgt != 0) & (np.sign(q) != np.sign(tgt)), 1 << 50, 0)
                    j = int(np.argmin(cost))
                    if best is None or cost[j] < best[0]:
                        best = (int(cost[j]), cand[j].copy())
                cen.append(best[1])
                cam = (mv64 @ np.append(best[1].astype(np.float64), 1.0))[:3]
                depth = max(abs(cam[2]), 1e-4)
                px = 0.08 * W if e[:2] in ("px", "py") else float(g.uniform(3.0, 12.0))
                scl.append(np.array([1.0, 0.6, 0.3]) * px * depth / f)
    return np.array(cen, np.float32), np.array(scl)


def edge_rows(W, H):
    """-> (pose, rows uint8 [n, 32], kinds: dict name -> slice)"""
    pose = pose_of(W, H)
    g = np.random.Generator(np.random.PCG64(W * 7919 + H))
    f = float(pose["focal"])
    parts, kinds, n = [], {}, 0

    def add(name, rows):
        nonlocal n
        parts.append(rows); kinds[name] = slice(n, n + rows.shape[0]); n += rows.shape[0]

    cen, scl = _threshold_rows(pose, W, H, g)
    r = make_rows(np.zeros((cen.shape[0], 3)), scl, QUATS[g.integers(10, 13, cen.shape[0])])
    pos = cen.copy(); pos[:, 2] = -pos[:, 2]                           # (the row stores -z: exact)
    r[:, 0:12] = np.ascontiguousarray(pos).view(np.uint8).reshape(-1, 12)
    add("thresholds", r)
    # head-on isotropic: identity quaternion, camy == 0 (24 rows; cov01 == 0 and len == 0 under the translation-only pose) or camx == 0 (8)
    k = 32
    nx, ny = g.uniform(-0.9, 0.9, k), g.uniform(-0.9, 0.9, k)
    cam = cam_from_ndc(pose, nx, ny, np.exp(g.uniform(np.log(0.5), np.log(20.0), k)))
    cam[:24, 1] = 0.0; cam[24:, 0] = 0.0; cam[:4, 0] = 0.0
    s = np.exp(g.uniform(np.log(0.01), np.log(0.3), k))
    add("head_on", make_rows(cam_to_obj(pose, cam), np.stack([s, s, s], 1), np.tile(np.array([255, 128, 128, 128], np.uint8), (k, 1))))

    def cloud(k, px_lo, px_hi, aniso):
        cam = cam_from_ndc(pose, g.uniform(-1.1, 1.1, k), g.uniform(-1.1, 1.1, k), np.exp(g.uniform(np.log(0.3), np.log(30.0), k)))
        s = np.exp(g.uniform(np.log(px_lo), np.log(px_hi), k)) * (-cam[:, 2]) / f
        return make_rows(cam_to_obj(pose, cam), s[:, None] * np.asarray(aniso)[None, :], QUATS[g.integers(0, len(QUATS), k)])
    add("clamp_1024", cloud(24, 800.0, 20000.0, (1.0, 0.7, 0.4)))
    add("needles", cloud(48, 300.0, 5000.0, (1.0, 1e-3, 1e-3)))
    add("plain", cloud(160, 0.3, 40.0, (1.0, 0.5, 0.25)))
    big = cloud(16, 1.0, 2.0, (1.0, 1.0, 0.5))
    big[:, 12:24] = (np.array([1e18, 3e18, 1e19, 1.8e19, 2e19, 1e20, 1e25, 3e38] * 2, "<f4")[:, None] * np.array([1.0, 0.5, 0.25], "<f4")).astype("<f4").view(np.uint8).reshape(16, 12)
    add("infinite", big)
    bad = cloud(18, 5.0, 20.0, (1.0, 0.5, 0.25))
    for i, (c, v) in enumerate((c, v) for c in range(3) for v in (np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)):
        bad[i, 4 * c:4 * c + 4] = np.array([v], "<f4").view(np.uint8)
    add("nan_inf", bad)
    return pose, np.ascontiguousarray(np.concatenate(parts)), kinds


def project_both(lib, pose, rows, W, H):
    """-> (visible per the oracle [n] bool, mismatching rows as text, oracle records, header bounds [n, 4])"""
    cs, cc, _ = oracle.pack(rows.reshape(-1))
    out = np.zeros(17, np.float32)
    vis, bad, recs, bounds = [], [], [], np.zeros((rows.shape[0], 4), np.float32)
    for i in range(rows.shape[0]):
        o = oracle.project(cs, cc, i, pose["mv"], pose["proj"], pose["focal"], W, H)
        v = lib.hc_project(_p(cs), _p(cc), i, _p(pose["mv"]), _p(pose["proj"]), pose["focal"], float(W), float(H), _p(out))
        vis.append(bool(o.visible)); recs.append(o)
        if v != o.visible:
            bad.append("row %d %s: visible header %d oracle %d" % (i, rows[i].tobytes().hex(), v, o.visible))
            continue
        if v:
            bounds[i] = out[13:17]
            want = np.array([o.cx, o.cy, o.ax, o.ay, o.bx, o.by, o.alpha], np.float32)
            got = np.concatenate([out[0:6], out[11:12]])
            w = int(out[12:13].view(np.uint32)[0])
            rgb = [np.float32(np.float32((w >> s) & 0xFF) / np.float32(255.0)) for s in (0, 8, 16)]
            if not np.array_equal(got.view(np.uint32), want.view(np.uint32)) or rgb != [np.float32(o.r), np.float32(o.g), np.float32(o.b)] or w != int(cc[i, 3]):
                bad.append("row %d %s: header %s oracle %s" % (i, rows[i].tobytes().hex(), got.tolist(), want.tolist()))
    return np.array(vis), bad, recs, bounds


@pytest.mark.parametrize("frame", range(len(FRAMES)))
def test_header_and_oracle_agree_on_every_row_and_every_exit_has_both_sides(lib, frame):
    W, H = FRAMES[frame]
    pose, rows, kinds = edge_rows(W, H)
    assert rows.shape[0] <= 2048
    vis, bad, recs, _ = project_both(lib, pose, rows, W, H)
    assert not bad, "%d rows differ; first: %s" % (len(bad), bad[0])
    cs, _, _ = oracle.pack(rows.reshape(-1))
    th = kinds["thresholds"]
    q = quantities(cs[th, :3], pose["mv"], pose["proj"])
    per = len(TARGETS) * 8
    for k, e in enumerate(EXITS):
        d = q[e][k * per:(k + 1) * per]
        v = vis[th][k * per:(k + 1) * per]
        below, on, above = int((d < 0).sum()), int((d == 0).sum()), int((d > 0).sum())
        print("%dx%d exit %-7s below %2d on %2d above %2d; exactly on a target %2d of %d; visible %2d" % (
            W, H, e, below, on, above, int(sum((d == t).sum() for t in TARGETS)), per, int(v.sum())))
        if e == "pw|0":
            assert below + on >= MIN_SIDE and above >= MIN_SIDE, (e, below, on, above)
        else:
            assert below >= MIN_SIDE and above >= MIN_SIDE, (e, below, on, above)
    # the cull decisions on the threshold rows are the comparisons' own: a row beyond a threshold is invisible
    culled = (q["pz|-pw"] < 0) | (q["px|-b"] < 0) | (q["px|+b"] > 0) | (q["py|-b"] < 0) | (q["py|+b"] > 0) | (q["pw|0"] <= 0) | (q["zndc|1"] > 0)
    assert not np.any(vis[th] & culled)
    assert int((vis[th] & ~culled).sum()) >= 5 * MIN_SIDE
    ho = vis[kinds["head_on"]]
    n_clamp = sum(1 for o in recs if o.visible and np.hypot(o.v1x, o.v1y) >= 1023.99)
    n_l2 = sum(1 for o in recs if o.visible and abs(np.hypot(o.v2x, o.v2y) - np.sqrt(0.2)) < 1e-4)
    print("%dx%d: %d rows, visible %d; head-on isotropic visible %d of %d; on the 1024 clamp %d, on the l2 clamp %d; infinite visible %d, NaN / Inf visible %d" % (
        W, H, rows.shape[0], int(vis.sum()), int(ho.sum()), ho.size, n_clamp, n_l2, int(vis[kinds["infinite"]].sum()), int(vis[kinds["nan_inf"]].sum())))
    if W == 640:
        # cov01 == 0 there; len == 0 too wherever mid + radius rounds back to d1 (the others get an eigenvector out of one rounding)
        assert int((~ho[:24]).sum()) >= 8 and np.any(ho[24:])
    assert n_clamp >= 16 and n_l2 >= 1
    assert not np.any(vis[kinds["nan_inf"]])
    assert int(vis[kinds["infinite"]].sum()) <= 6                      # (1e18 may still be finite at a far centre; the rest is not)
    assert int(vis[kinds["plain"]].sum()) >= 60
