"""CPU tier of the scene-compositing edges (include/gs_splat.h: gs_set_scene, GS_OPT_TERMINATION): the scenes and depth planes the GPU
tier (test_scene_edges_gpu.py) draws, a plain numpy MIRROR of blending over a scene, and the layout facts the GPU tier relies on.

The mirror blends back to front over the sorted order in f64 from oracle.project's records: a fragment is kept iff q <= 4 and
zwin <= plane, zwin = f32(zndc * 0.5f + 0.5f); the destination is the scene's bytes / 255, or the background.  The DECISION q <= 4 is
taken on the oracle's own f32 expression tree (fmaf(dx, ax, dy * ay), fmaf(px, px, py * py): each product of two f32 is exact in f64,
so one f64 addition and one rounding to f32 is the fused operation) -- a fragment count has no tolerance; the weights exp(-q) and the
sums are f64.

The stacks: W = 160, one tile row per case (K, m).  K runs cover tile column 4 at depths 1.0 + 0.002 k; with the near plane at 0.005
their window depths lie ~1e-5 (some 170 f32 ulps) apart.  Entry m (0 = nearest) and its neighbours m-1, m+1, m+2 are strong and
coloured, all others faint (alpha 3..6): nothing saturates, so a plane that cuts AT z_m and one that cuts one ulp below it differ by
entry m's pixels, in the picture and -- exactly -- in the fragment count."""
import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_blend_paths_gpu import Scene, camera, run, splat
from test_surface_cpu import synth_scene

capi = pkg("capi")

f32 = np.float32
TARGET = 4                                              # the tile column every stack covers
KS = (1, 2, 63, 64, 65, 128, 129)
CASES = [(K, m) for K in KS for m in sorted({0, K - 1, 62, 63, 64, 127, 128}) if 0 <= m < K]
SHAPES = [(4, 4), (2, 6), (4, 9), (0, 4), (3, 5)]       # tile columns a..b of a run; every one holds column 4
STRONG = [(255, 30, 0), (0, 255, 40), (30, 0, 255), (255, 255, 0)]   # entries m-1, m, m+1, m+2
SCENE_ALPHAS = (0, 1, 127, 128, 254, 255)
BACKGROUNDS = [(0.25, 0.5, 0.75, a) for a in (0.0, 0.5, 1.0)]
STRIP_X0, STRIP_W = (0, 4, 6, 13, 16), (1, 3, 4, 5, 17)
RAGGED = ((1, 1), (17, 17), (31, 47), (161, 33))
TERMINATIONS = (256, 257, 1024, 4096, 1 << 24)


def window_depths(scene):
    """f32(zndc * 0.5f + 0.5f) of every row, from oracle.project (what k_project writes to zwin); 2.0 for a row that is not visible"""
    c = scene.cam
    mv, pr = c["gs_mv"].astype(f32), c["gs_proj"].astype(f32)
    z = np.full(len(scene.rows) // 32, 2.0, f32)
    for i in range(z.size):
        p = oracle.project(scene.cs, scene.cc, i, mv, pr, c["focal"], scene.W, scene.H)
        if p.visible:
            z[i] = f32(f32(p.zndc) * f32(0.5) + f32(0.5))
    return z


class Stacks:
    """scene, cases, first[t] (the row of entry 0 of tile row t's stack), z[t] (its K window depths), rgba (the scene colour)"""

    def __init__(self, cases, strong_alpha=120, seed=3, alphas=None, W=160):
        g = np.random.Generator(np.random.PCG64(seed))
        self.cases, self.W, self.H = list(cases), W, 16 * len(cases)
        cam = camera(W, self.H)
        rows, self.first = [], []
        for ty, (K, m) in enumerate(self.cases):
            self.first.append(len(rows))
            for k in range(K):
                s = k - (m - 1)
                if alphas is not None:
                    col = tuple(int(v) for v in g.choice([0, 255], 3)) if k % 3 else (255, 255, 255)
                    rgba = col + (int(alphas[(k + ty) % len(alphas)]),)
                elif 0 <= s < 4:
                    rgba = STRONG[s] + (strong_alpha,)
                else:
                    rgba = (int(g.integers(0, 256)), int(g.integers(0, 256)), int(g.integers(0, 256)), 3 + k % 4)
                rows.append(run(cam, ty, *SHAPES[k % len(SHAPES)], 1.0 + 0.002 * k, rgba))
        self.scene = Scene(W, self.H, rows)
        zall = window_depths(self.scene)
        self.z = [zall[f:f + K] for f, (K, _) in zip(self.first, self.cases)]
        for z in self.z:
            assert z.dtype == f32 and (z < 1.0).all() and (np.diff(z) > 0).all(), "window depths of a stack must rise strictly"
        self.rgba = g.integers(0, 256, (self.H, W, 4)).astype(np.uint8)

    def rows_of(self, t):
        return range(self.first[t], self.first[t] + self.cases[t][0])

    def plane(self, fn):
        """[H, W] f32: tile row t holds fn(t, z_t, m_t, x[16, W], y[16, W]) (x, y: pixel column and row within the frame)"""
        z = np.ones((self.H, self.W), f32)
        x, y = np.meshgrid(np.arange(self.W), np.arange(16))
        for t, (K, m) in enumerate(self.cases):
            z[16 * t:16 * t + 16] = fn(t, self.z[t], m, x, y + 16 * t)
        return z

    # the planes of the GPU tier
    def exact(self):
        return self.plane(lambda t, z, m, x, y: z[m])

    def below(self):
        return self.plane(lambda t, z, m, x, y: np.nextafter(z[m], f32(-np.inf)))

    def alternating(self):
        """columns alternate between z_m and z_(m+1): m = 63 and 127 put the two on either side of a batch edge"""
        return self.plane(lambda t, z, m, x, y: np.where(x % 2 == 0, z[m], z[(m + 1) % len(z)]))

    def checker(self):
        return self.plane(lambda t, z, m, x, y: np.where((x // 4 + y // 4) % 2 == 0, z[m], z[(m + 1) % len(z)]))

    def one_pixel(self):
        """one pixel per tile at z_0 (only the nearest entry passes), the rest at 1.0"""
        def fn(t, z, m, x, y):
            tx = x // 16
            hit = (x % 16 == (5 * tx + 3 * t) % 16) & (y % 16 == 3 + (7 * tx + t) % 11)
            return np.where(hit, z[0], f32(1.0))
        return self.plane(fn)

    def planes(self):
        return {"exact": self.exact(), "below": self.below(), "alternating": self.alternating(), "checker": self.checker(),
                "one_pixel": self.one_pixel()}


def odd_values():
    """NaN of both signs and with a payload, the infinities, the zeros, 1, 2, -1, the smallest denormal, the float above 1"""
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFD54321], np.uint32).view(f32)
    rest = np.array([np.inf, -np.inf, -0.0, 0.0, 1.0, 2.0, -1.0], f32)
    return np.concatenate([nans, rest, np.array([1], np.uint32).view(f32), [np.nextafter(f32(1.0), f32(2.0))]]).astype(f32)


ODD_REJECTS = (0, 1, 2, 3, 5, 6, 7, 10, 11)            # of odd_values(): no window depth in (0, 1) is <= these


def odd_plane(st):
    v = odd_values()
    return np.broadcast_to(v[np.arange(st.W) % v.size], (st.H, st.W)).copy()


def destination_scene(seed=8):
    """160x32.  Tile row 0: runs over tile columns 5..9 only -- tiles 0..3 are covered by nothing; tile c of them holds all 256 byte
    values in channel c of the scene colour.  Tile row 1: 30 runs over every column; the scene's alpha bytes cycle through SCENE_ALPHAS
    by column.  The depth plane: 1.0, and every third column of tile row 1 cut at the 15th entry."""
    g = np.random.Generator(np.random.PCG64(seed))
    W, H = 160, 32
    cam = camera(W, H)
    rows = []
    for k in range(12):
        rows.append(run(cam, 0, *[(5, 9), (6, 8), (5, 5), (7, 9)][k % 4], 1.0 + 0.002 * k, (int(g.integers(0, 256)), 200, 40, 30 + 10 * k)))
    first = len(rows)
    for k in range(30):
        rows.append(run(cam, 1, *[(0, 9), (2, 6), (0, 4), (5, 9), (3, 3)][k % 5], 1.0 + 0.002 * k,
                        (int(g.integers(0, 256)), int(g.integers(0, 256)), 220, 20 + 3 * k)))
    scene = Scene(W, H, rows)
    rgba = g.integers(0, 256, (H, W, 4)).astype(np.uint8)
    for c in range(4):
        rgba[0:16, 16 * c:16 * c + 16, c] = np.arange(256).reshape(16, 16)
    rgba[16:, :, 3] = np.asarray(SCENE_ALPHAS, np.uint8)[np.arange(W) % len(SCENE_ALPHAS)]
    depth = np.ones((H, W), f32)
    depth[16:, ::3] = window_depths(scene)[first + 15]
    return scene, depth, rgba


def strips_scene(seed=12):
    """48x16, 48 runs over all three tile columns: six strong ones in front, then alpha 60 in alternating bright colours, so that a pixel
    that takes everything falls below the termination threshold after a dozen entries and what lies behind weighs up to the threshold.
    The plane carries a different cut in every column ((11 x) % 50: the entry whose depth the column holds; 48: 0.0, nothing passes --
    such a pixel keeps its lane in the list to the end --, 49: 1.0)."""
    W, H, K = 48, 16, 48
    cam = camera(W, H)
    cols = [(255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255)]
    rows = [run(cam, 0, *[(0, 2), (0, 1), (1, 2), (0, 2)][k % 4], 1.0 + 0.002 * k, cols[k % 6] + (200 if k < 6 else 60,)) for k in range(K)]
    scene = Scene(W, H, rows)
    z = window_depths(scene)
    assert (np.diff(z) > 0).all()
    cut = (11 * np.arange(W)) % 50
    assert len(set(cut.tolist())) == W
    col = np.where(cut == 48, f32(0.0), np.where(cut == 49, f32(1.0), z[np.minimum(cut, K - 1)])).astype(f32)
    g = np.random.Generator(np.random.PCG64(seed))
    return scene, np.broadcast_to(col, (H, W)).copy(), g.integers(0, 256, (H, W, 4)).astype(np.uint8)


def ragged_scene(w, h):
    """a few dozen large splats on a w x h frame; the plane holds, per pixel, the window depth of a random splat (equality is common) or 1.0"""
    sc = synth_scene(5 + w % 7, w, h, n=48)
    g = np.random.Generator(np.random.PCG64(w * 1000 + h))
    z = window_depths(sc)
    pool = np.concatenate([z[z < 1.5], [f32(1.0)] * 8]).astype(f32)
    return sc, pool[g.integers(0, pool.size, (h, w))], g.integers(0, 256, (h, w, 4)).astype(np.uint8)


def termination_stacks():
    """two tile rows of 129 runs, alphas 40..200, white and saturated colours; the scene colour is dark with white columns"""
    st = Stacks([(129, 64), (129, 128)], seed=21, alphas=(40, 200, 90, 150, 60, 120, 180))
    st.rgba[:, :, :3] = np.where((np.arange(st.W) % 5 == 0)[None, :, None], 255, np.array([0, 0, 64])[None, None, :])
    return st


# ---------------------------------------------------------------- the mirror

def geometry(scene, idx, x0=0, x1=None):
    """per visible splat of the order, back to front: (splat, rows r0:r1, columns c0:c1 of the strip, keep = q <= 4 there, q f64,
    window depth f32, (r, g, b, alpha))"""
    W, H, c = scene.W, scene.H, scene.cam
    x1 = W if x1 is None else x1
    mv, pr = c["gs_mv"].astype(f32), c["gs_proj"].astype(f32)
    out = []
    for i in np.asarray(idx):
        p = oracle.project(scene.cs, scene.cc, int(i), mv, pr, c["focal"], W, H)
        if not p.visible:
            continue
        hw = 2.0 * np.sqrt(p.v1x * p.v1x + p.v2x * p.v2x) + 2.0
        hh = 2.0 * np.sqrt(p.v1y * p.v1y + p.v2y * p.v2y) + 2.0
        c0, c1 = int(max(x0, np.floor(p.cx - hw))), int(min(x1 - 1, np.ceil(p.cx + hw))) + 1
        j0, j1 = int(max(0, np.floor(p.cy - hh))), int(min(H - 1, np.ceil(p.cy + hh))) + 1           # GL rows, 0 = bottom
        if c0 >= c1 or j0 >= j1:
            continue
        r0, r1 = H - j1, H - j0                                                                      # image rows
        dx = ((np.arange(c0, c1, dtype=f32) + f32(0.5)) - f32(p.cx))[None, :]
        dy = ((f32(H - 1) - np.arange(r0, r1, dtype=f32) + f32(0.5)) - f32(p.cy))[:, None]
        fma = lambda a, b, cc: (a.astype(np.float64) * np.float64(b) + cc.astype(np.float64)).astype(f32)
        ppx, ppy = fma(dx, f32(p.ax), dy * f32(p.ay)), fma(dx, f32(p.bx), dy * f32(p.by))
        q = (ppx.astype(np.float64) * ppx.astype(np.float64) + (ppy * ppy).astype(np.float64)).astype(f32)
        keep = q <= f32(4.0)
        if keep.any():
            out.append((int(i), r0, r1, c0 - x0, c1 - x0, keep, q.astype(np.float64), f32(f32(p.zndc) * f32(0.5) + f32(0.5)),
                        (p.r, p.g, p.b, p.alpha)))
    return out


def blend(geom, shape, x0=0, depth=None, rgba=None, bg=(0.0, 0.0, 0.0, 1.0)):
    """-> (image f64 [H, sw, 4] before rounding, fragments kept per pixel [H, sw], fragments kept per splat {splat: count})"""
    H, sw = shape
    img = np.empty((H, sw, 4))
    img[:] = np.asarray(bg, f32).astype(np.float64) if rgba is None else (np.asarray(rgba)[:, x0:x0 + sw].astype(f32) / f32(255.0)).astype(np.float64)
    n = np.zeros((H, sw), np.int64)
    per = {}
    for i, r0, r1, c0, c1, keep, q, zw, (r, g, b, a) in geom:
        k = keep if depth is None else keep & (zw <= np.asarray(depth, f32)[r0:r1, x0 + c0:x0 + c1])
        per[i] = per.get(i, 0) + int(k.sum())
        if not k.any():
            continue
        B = np.where(k, np.exp(-q) * a, 0.0)[:, :, None]
        d = img[r0:r1, c0:c1]
        d[:] = np.concatenate([np.array([r, g, b])[None, None, :] * B, B], axis=2) + d * (1.0 - B)
        n[r0:r1, c0:c1] += k
    return img, n, per


def to_u8(img):
    return np.floor(np.clip(img, 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


def order(scene):
    return oracle.sort(scene.mats, scene.cam["view"])


def oracle_frame(scene, idx, depth=None, rgba=None, bg=(0.0, 0.0, 0.0, 1.0), x0=0, x1=None):
    c = scene.cam
    u8, _, fr = oracle.render(scene.cs, scene.cc, idx, c["gs_mv"].astype(f32), c["gs_proj"].astype(f32), c["focal"], scene.W, scene.H,
                              x0=x0, x1=x1, bg=bg, want_f32=False, scene_depth=depth, scene_rgba=rgba)
    return u8, fr


def case_counts(st, idx, t, plane):
    """the oracle's fragment count of tile row t's stack alone (the order restricted to its splats) under a plane"""
    rows = st.rows_of(t)
    sub = np.asarray([i for i in idx if rows.start <= i < rows.stop], np.uint32)
    return oracle_frame(st.scene, sub, depth=plane)[1]


def count_condition(st, idx, exact, below):
    """for every case: the oracle's counts under the plane AT z_m and one ulp below differ by the pixels entry m covers, > 0"""
    geom = {g[0]: int(g[5].sum()) for g in geometry(st.scene, idx)}
    total = 0
    for t, (K, m) in enumerate(st.cases):
        covers = geom.get(st.first[t] + m, 0)
        a, b = case_counts(st, idx, t, exact), case_counts(st, idx, t, below)
        assert covers > 0 and a - b == covers, ("case", K, m, "counts", a, b, "entry m covers", covers)
        total += covers
    return total


# ---------------------------------------------------------------- fixtures and tests

@pytest.fixture(scope="module")
def stacks():
    return Stacks(CASES)


@pytest.fixture(scope="module")
def stacks_order(stacks):
    return order(stacks.scene)


def test_the_cases_are_the_issue_s():
    assert len(CASES) == 23 and all(0 <= m < K for K, m in CASES)
    assert {m for K, m in CASES if K == 129} == {0, 62, 63, 64, 127, 128} and (1, 0) in CASES and (2, 1) in CASES


def test_stack_layout(stacks, stacks_order):
    """window depths rise strictly (Stacks asserts it) some 170 ulps apart, every run survives the sort and covers pixels of tile
    column 4 of its own tile row only: the list of column 4 holds the K entries"""
    sc = stacks.scene
    assert set(stacks_order.tolist()) == set(range(len(sc.rows) // 32))
    rows_hit = {}
    for i, r0, r1, c0, c1, keep, *_ in geometry(sc, stacks_order, 16 * TARGET, 16 * TARGET + 16):
        rr = np.flatnonzero(keep.any(axis=1))
        rows_hit[i] = (r0 + int(rr[0]), r0 + int(rr[-1]) + 1)
    for t, (K, m) in enumerate(stacks.cases):
        ulps = np.diff(stacks.z[t].view(np.int32))
        assert K == 1 or 100 <= ulps.min() <= ulps.max() <= 250, (K, m, ulps.min(), ulps.max())
        for i in stacks.rows_of(t):
            assert i in rows_hit and 16 * t <= rows_hit[i][0] and rows_hit[i][1] <= 16 * t + 16, (K, m, i)
        pos = {int(i): k for k, i in enumerate(stacks_order)}
        at = [pos[i] for i in stacks.rows_of(t)]
        assert at == sorted(at, reverse=True), "the stack's entries are not drawn in their depth order"


def test_count_difference_between_the_cut_at_an_entry_and_one_ulp_below(stacks, stacks_order):
    exact, below = stacks.exact(), stacks.below()
    assert (exact.view(np.int32) - below.view(np.int32) == 1).all()
    total = count_condition(stacks, stacks_order, exact, below)
    assert oracle_frame(stacks.scene, stacks_order, depth=exact)[1] - oracle_frame(stacks.scene, stacks_order, depth=below)[1] == total


def _mirror_vs_oracle(scene, idx, depth, rgba, bg=(0.0, 0.0, 0.0, 1.0), x0=0, x1=None, geom=None):
    geom = geometry(scene, idx, x0, x1) if geom is None else geom
    sw = (scene.W if x1 is None else x1) - x0
    img, n, _ = blend(geom, (scene.H, sw), x0, depth, rgba, bg)
    want, frags = oracle_frame(scene, idx, depth, rgba, bg, x0, x1)
    assert int(n.sum()) == frags
    got = to_u8(img)
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
    none = n == 0
    dst = np.broadcast_to(to_u8(np.asarray(bg, f32).astype(np.float64)), want.shape) if rgba is None else rgba[:, x0:x0 + sw]
    assert np.array_equal(want[none], dst[none]) and np.array_equal(got[none], dst[none])
    return n


def test_mirror_equals_the_oracle_on_the_stacks(stacks, stacks_order):
    geom = geometry(stacks.scene, stacks_order)
    for name, plane in stacks.planes().items():
        n = _mirror_vs_oracle(stacks.scene, stacks_order, plane, stacks.rgba, geom=geom)
        assert n.any(), name


def test_mirror_equals_the_oracle_on_odd_depths():
    st = Stacks([(65, 32)], seed=4)
    idx, plane, v = order(st.scene), odd_plane(st), odd_values()
    assert np.isnan(v[:4]).all() and v[11] > 0 and v[11] < 1e-44 and v[12] > 1
    n = _mirror_vs_oracle(st.scene, idx, plane, st.rgba)
    cols = np.arange(st.W) % v.size
    assert not n[:, np.isin(cols, ODD_REJECTS)].any(), "a fragment passed a NaN, a zero, a negative or a denormal depth"
    assert n[:, ~np.isin(cols, ODD_REJECTS)].any()


def test_mirror_equals_the_oracle_on_the_destination_scene():
    scene, depth, rgba = destination_scene()
    idx = order(scene)
    for bg in BACKGROUNDS:
        for d, c in ((depth, rgba), (None, rgba), (depth, None)):
            n = _mirror_vs_oracle(scene, idx, d, c, bg)
            assert not n[0:16, 0:64].any() and n[16:].any()


def test_mirror_equals_the_oracle_on_strips_and_ragged_frames():
    scene, depth, rgba = strips_scene()
    idx = order(scene)
    for x0 in STRIP_X0:
        for w in STRIP_W:
            _mirror_vs_oracle(scene, idx, depth, rgba, x0=x0, x1=x0 + w)
    for w, h in RAGGED:
        sc, d, c = ragged_scene(w, h)
        _mirror_vs_oracle(sc, order(sc), d, c)


def test_termination_stacks_are_deep_enough_for_every_threshold():
    """every threshold of the GPU tier's bound test cuts something off somewhere: at the tile centres the transmittance behind all 129
    entries is below 2^-24, and the scene and the background contrast with the splats' colours"""
    st = termination_stacks()
    idx = order(st.scene)
    geom = geometry(st.scene, idx)
    T = np.ones((st.H, st.W))
    for i, r0, r1, c0, c1, keep, q, zw, (r, g, b, a) in geom:
        T[r0:r1, c0:c1] *= 1.0 - np.where(keep, np.exp(-q) * a, 0.0)
    assert (T < 2.0 ** -24).any() and (T < 1.0 / 256).mean() > 0.1
    _mirror_vs_oracle(st.scene, idx, None, st.rgba, geom=geom)
