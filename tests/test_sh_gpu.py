"""GPU tier of the view-dependent colour (GS_OPT_SH_DEGREE): k_project's SH instantiation against SUBSTITUTION.

The oracle is not taught spherical harmonics.  For a pose, the numpy mirror of csrc/gs_sh.h (test_sh_cpu.sh_mirror) computes every
splat's bytes for the camera gs_camera_in_object reports, and writes them into a copy of the plain .splat rows.  A frame drawn with
SH must then be BIT-IDENTICAL to the frame the same library draws from those rows with the option at 0 -- whatever way the frame
is drawn -- and within the standing 1 LSB of oracle.render on those rows, with equal fragment counts.

Scenes: synth.make_splat_rows through synth.rows_to_inria_ply with random f_rest (at most 200 k splats); frames of 640x360 and
smaller, one of 1920x1080."""
import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_gpu_parity import PIXEL_TOL_LSB, pix_check
from test_sh_cpu import sh_mirror

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")

W, H = 640, 360


class Scene:
    """A synthetic PLY with random f_rest, its converted rows (the converter's order) and its SH rows."""

    def __init__(self, n, seed, spread=0.35, alpha=None, zero_rest=False):
        rows = synth.make_splat_rows(n, seed=seed).reshape(-1, 32).copy()
        if alpha is not None:
            rows[:, 27] = alpha
        rest = np.random.default_rng(seed + 1).standard_normal((n, 45)).astype(np.float32) * np.float32(0.0 if zero_rest else spread)
        self.ply = synth.rows_to_inria_ply(rows, rest)
        self.rows = capi.ply_to_splat(self.ply).reshape(-1, 32)
        self.n = n
        self.pos = self.rows[:, 0:12].copy().view("<f4").reshape(n, 3)
        self.sh3, d = capi.ply_sh(self.ply, 3)
        assert d == 3 and self.sh3.shape == (n, 48)

    def sh(self, degree):
        K = (degree + 1) ** 2
        return np.ascontiguousarray(self.sh3.reshape(self.n, 3, 16)[:, :, :K]).reshape(self.n, 3 * K)

    def substituted(self, degree, mv, upto=None):
        """The plain rows with the colour bytes the mirror computes for the camera of `mv` (rows [0, upto) only)."""
        cam = capi.camera_in_object(np.asarray(mv, np.float32)) * np.array([1.0, 1.0, -1.0])   # model_view acts on (x, y, -z): rows' space
        out = self.rows.copy()
        m = self.n if upto is None else upto
        out[:m, 24:27] = sh_mirror(self.sh3.reshape(self.n, 3, 16)[:m], degree, cam, self.pos[:m])
        return out


@pytest.fixture(scope="module")
def scene():
    return Scene(60000, 4100)


def params(cam, **kw):
    return capi.make_params(cam["gs_mv"], cam["gs_proj"], cam["vw"], cam["vh"], focal_=cam["focal"], **kw)


def cams_for(yaws, w=W, h=H):
    return [synth.index_html_camera(w, h, y, capi=capi) for y in yaws]


def sh_context(scene, degree, how="load_ply", opts=()):
    c = capi.Context(0)
    for k, v in opts:
        c.set_option(k, v)
    c.set_option(capi.OPT_SH_DEGREE, degree)
    if how == "load_ply":
        c.load_ply(scene.ply)
    else:
        c.push_splat(scene.rows)
        c.push_sh(scene.sh(degree), degree)
    return c


def plain_context(rows, opts=()):
    c = capi.Context(0)
    for k, v in opts:
        c.set_option(k, v)
    c.push_splat(rows)
    return c


def draw(c, cam, cutout=None, **kw):
    c.sort(cam["view"], cutout)
    return c.render(params(cam, **kw))


def live_records(c):
    """The projected records the last frame wrote (sorted positions whose splat touched a tile) and where they are."""
    v = c.stats()["n_sorted"]
    live = c.download(capi.BUF_TILE_COUNT, v, np.uint32, 1)[:, 0] > 0
    return c.download(capi.BUF_PROJECTED, v, np.uint32, 8)[live], live


def check_substitution(scene, degree, cams, draw_all, opts=(), how="push", expect_stats=None):
    """draw_all(c, cams) -> one image per camera.  The SH context's images against those of plain contexts holding the rows
    substituted for each camera, drawn the same way with the same options."""
    with sh_context(scene, degree, how, opts) as c:
        got = draw_all(c, cams)
        st = c.stats()
    assert st["sh_degree"] == degree, st
    for k, v in (expect_stats or {}).items():
        assert st[k] == v, (k, st)
    for i, cam in enumerate(cams):
        with plain_context(scene.substituted(degree, cam["gs_mv"]), opts) as p:
            want = draw_all(p, cams)[i]
            assert p.stats()["sh_degree"] == 0
        assert got[i].shape == want.shape and np.array_equal(got[i], want), "frame %d differs in %d bytes" % (i, int((got[i] != want).sum()))
    return got, st


# ---------------------------------------------------------------- 7. substitution

@pytest.mark.parametrize("how", ["load_ply", "push"])
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_sh_frame_equals_frame_of_substituted_rows(scene, degree, how):
    cams = cams_for((0.0, 40.0, 200.0))
    one_round = [(capi.OPT_NEAR_PERMILLE, 1000)]                                # (every visible splat is projected and counted once)
    with sh_context(scene, degree, how, one_round) as c, plain_context(scene.rows, one_round) as orig:
        assert c.sh_count() == (scene.n, degree)
        assert np.array_equal(c.download_sh(), scene.sh(degree))
        for cam in cams:
            got = draw(c, cam)
            assert c.stats()["sh_degree"] == degree
            proj, live = live_records(c)
            sub = scene.substituted(degree, cam["gs_mv"])
            with plain_context(sub, one_round) as p:
                want = draw(p, cam)
                proj_sub, live_sub = live_records(p)
            assert np.array_equal(got, want)                                    # (a) bit-identical
            assert np.array_equal(live, live_sub) and np.array_equal(proj, proj_sub)   # ... down to every projected record
            plain = draw(orig, cam)                                             # (c) against the ORIGINAL rows at option 0:
            proj0, live0 = live_records(orig)
            assert np.array_equal(live, live0) and len(proj) > 1000
            diff = proj != proj0
            assert not diff[:, [0, 1, 2, 3, 4, 5, 7]].any() and diff[:, 6].any()      # the colour word only
            assert np.array_equal(proj[:, 6] >> 24, proj0[:, 6] >> 24)                # alpha stays the packed byte
            assert not np.array_equal(got, plain)


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_sh_frame_against_the_oracle_on_substituted_rows(degree):
    sc = Scene(20000, 4200 + degree)
    cam = synth.index_html_camera(320, 180, yaw_deg=25.0 * degree, capi=capi)
    sub = sc.substituted(degree, cam["gs_mv"])
    cs, cc, mats = oracle.pack(sub)
    idx = oracle.sort(mats, cam["view"])
    want, _, frags = oracle.render(cs, cc, idx, cam["gs_mv"].astype(np.float32), cam["gs_proj"].astype(np.float32), cam["focal"], 320, 180,
                                   want_f32=False)
    with sh_context(sc, degree, "load_ply") as c:
        got_idx = c.sort(cam["view"])
        assert np.array_equal(got_idx, idx)
        img = c.render(params(cam))
        pix_check("sh_degree%d_320x180" % degree, img, want, PIXEL_TOL_LSB)
        c.render(params(cam, flags=capi.RENDER_COUNT_FRAGS))
        st = c.stats()
        assert st["n_frags"] == frags and st["sh_degree"] == degree


# ---------------------------------------------------------------- 8. view dependence

def test_colour_changes_with_the_pose_and_zero_f_rest_changes_nothing(scene):
    cams = cams_for((0.0, 90.0))
    with sh_context(scene, 1, "push", [(capi.OPT_NEAR_PERMILLE, 1000)]) as c:
        words = {}
        for i, cam in enumerate(cams):
            idx = c.sort(cam["view"])
            c.render(params(cam))
            proj, live = live_records(c)
            words[i] = dict(zip(idx[live].tolist(), proj[:, 6].tolist()))
        common = set(words[0]) & set(words[1])
        assert len(common) > 100
        assert sum(words[0][k] != words[1][k] for k in common) > len(common) // 2     # the same splat, another colour word
    zero = Scene(30000, 4300, zero_rest=True)
    for degree in (1, 3):
        with sh_context(zero, degree, "load_ply") as c, plain_context(zero.rows) as p:
            for cam in cams_for((0.0, 77.0, 190.0)):
                assert np.array_equal(draw(c, cam), draw(p, cam))
                assert c.stats()["sh_degree"] == degree


# ---------------------------------------------------------------- 9. every way a frame is drawn

VARIANTS = {
    "lists": [(capi.OPT_BINNING, 0), (capi.OPT_ROW_WALK, 0), (capi.OPT_SUBTILE, 0)],
    "pairs": [(capi.OPT_BINNING, 1), (capi.OPT_ROW_WALK, 0), (capi.OPT_SUBTILE, 0)],
    "walk": [(capi.OPT_BINNING, 0), (capi.OPT_ROW_WALK, 2), (capi.OPT_SUBTILE, 0)],
    "subtile": [(capi.OPT_BINNING, 0), (capi.OPT_ROW_WALK, 0), (capi.OPT_SUBTILE, 2)],
    "split": [(capi.OPT_BINNING, 0), (capi.OPT_ROW_WALK, 0), (capi.OPT_SUBTILE, 0), (capi.OPT_BLEND_SPLIT, 1)],
}
VARIANT_STATS = {"lists": {"binning": 0, "row_walk": 0}, "pairs": {"binning": 1}, "walk": {"row_walk": 1}, "subtile": {"subtile": 1}, "split": {}}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_substitution_on_every_blend_path(scene, variant):
    opts = [(capi.OPT_NEAR_PERMILLE, 1000)] + VARIANTS[variant]
    check_substitution(scene, 3, cams_for((15.0, 130.0)), lambda c, cams: [draw(c, cam) for cam in cams], opts,
                       expect_stats=VARIANT_STATS[variant])


def test_substitution_in_paired_asynchronous_frames(scene):
    """GS_OPT_FRAME_BATCH 2: two queued frames of two poses share every launch (k_twin), each with its own camera."""
    opts = [(capi.OPT_NEAR_PERMILLE, 1000), (capi.OPT_FRAME_BATCH, 2)]

    def draw_all(c, cams):
        for cam in cams:                                                          # measure the share / warm the lanes synchronously
            draw(c, cam)
        frames = [capi.host_frame(H, W) for _ in cams]
        for rep in range(2):
            for cam, (fr, _) in zip(cams, frames):
                c.sort(cam["view"], want_indices=False)
                c.render_into(params(cam, flags=capi.RENDER_ASYNC), fr)
            c.sync()
        out = [fr.copy() for fr, _ in frames]
        for _, owner in frames:
            owner.free()
        return out

    cams = cams_for((10.0, 250.0))
    got, _ = check_substitution(scene, 2, cams, draw_all, opts)
    with sh_context(scene, 2, "push", [(capi.OPT_NEAR_PERMILLE, 1000)]) as c:    # ... and the pair equals the frames drawn alone
        for i, cam in enumerate(cams):
            assert np.array_equal(draw(c, cam), got[i])


def test_substitution_in_the_second_binning_round():
    sc = Scene(60000, 4400, alpha=12)                                            # low opacity: the nearest share saturates no tile
    opts = [(capi.OPT_NEAR_PERMILLE, 300)]
    _, st = check_substitution(sc, 3, cams_for((30.0,)), lambda c, cams: [draw(c, cam) for cam in cams], opts)
    assert st["unsat_tiles"] > 0, st                                            # round 0 left tiles unsaturated: round 1 had work to do


def test_substitution_in_strips_stereo_scene_depth_and_cutout(scene):
    one = lambda f: (lambda c, cams: [f(c, cam) for cam in cams])
    # a strip with x0 % 4 == 0: its camera is the frame's camera
    got, _ = check_substitution(scene, 3, cams_for((50.0,)), one(lambda c, cam: draw(c, cam, x0=64, x1=203)))
    with sh_context(scene, 3, "push") as c:
        full = draw(c, cams_for((50.0,))[0])
    assert np.array_equal(got[0], full[:, 64:203])
    # stereo: one sort from the head camera, one camera position per eye
    left, right, head = synth.xr_eye_cameras(yaw_deg=20.0, xr_pixel_ratio=0.125, capi=capi)

    def stereo(c, cams):
        c.sort(head["view"])
        return list(c.render_stereo(params(cams[0]), params(cams[1])))
    eyes, _ = check_substitution(scene, 3, [left, right], stereo)
    assert not np.array_equal(capi.camera_in_object(left["gs_mv"].astype(np.float32)), capi.camera_in_object(right["gs_mv"].astype(np.float32)))
    # scene depth + colour
    yy, xx = np.mgrid[0:H, 0:W]
    depth = np.where(((yy // 24) + (xx // 24)) % 2 == 0, 1.0, 0.0).astype(np.float32)
    rgba = np.random.default_rng(3).integers(0, 256, (H, W, 4), dtype=np.uint8)

    def with_scene(c, cam):
        c.set_scene(depth, rgba)
        return draw(c, cam)
    check_substitution(scene, 2, cams_for((300.0,)), one(with_scene))
    # a cutout sort
    cut = synth.cutout_demo_camera(W, H, 0.0, capi=capi)
    check_substitution(scene, 1, [cut], one(lambda c, cam: draw(c, cam, cutout=cam["cutout"])))


def test_substitution_through_two_contexts_of_one_process(scene):
    cam = cams_for((65.0,))[0]
    frames = [capi.host_frame(H, W) for _ in range(2)]
    with capi.Multi([0, 0]) as m:
        m.set_option(capi.OPT_SH_DEGREE, 3)                                      # through gs_multi_set_option
        m.load_ply(scene.ply)
        m.sort(cam["view"], None, params(cam)); m.render(params(cam), frames[0][0])
        assert [m.ctx_stats(i)["sh_degree"] for i in range(2)] == [3, 3]
    with capi.Multi([0, 0]) as m:
        m.push_splat(scene.substituted(3, cam["gs_mv"]))
        m.sort(cam["view"], None, params(cam)); m.render(params(cam), frames[1][0])
    assert np.array_equal(frames[0][0], frames[1][0])
    with capi.Multi([0, 0]) as m:                                                # push + push_sh on every device
        m.set_option(capi.OPT_SH_DEGREE, 3)
        m.push_splat(scene.rows); m.push_sh(scene.sh(3), 3)
        frames[1][0][:] = 0
        m.sort(cam["view"], None, params(cam)); m.render(params(cam), frames[1][0])
    assert np.array_equal(frames[0][0], frames[1][0])
    for _, owner in frames:
        owner.free()


def test_full_hd_frame_of_200k_splats():
    sc = Scene(200000, 4500)
    cams = cams_for((0.0,), 1920, 1080)
    check_substitution(sc, 3, cams, lambda c, cs: [draw(c, cam) for cam in cs], how="load_ply")


# ---------------------------------------------------------------- 10. partial stores and state

def test_partial_store_clear_degree_mismatch_and_lowered_option(scene):
    cam = cams_for((110.0,))[0]
    half = scene.n // 2
    with capi.Context(0) as c:
        c.set_option(capi.OPT_SH_DEGREE, 3)
        c.push_splat(scene.rows)
        c.push_sh(scene.sh(3)[:half], 3)                                         # SH rows for the first half only
        with plain_context(scene.substituted(3, cam["gs_mv"], upto=half)) as p:
            assert np.array_equal(draw(c, cam), draw(p, cam))
        with pytest.raises(capi.GsError) as ei:
            c.push_sh(scene.sh(2)[half:], 2)                                     # another degree behind stored rows
        assert ei.value.code == capi.E_BADARG
        with pytest.raises(capi.GsError):
            c.push_sh(np.zeros(75, np.float32), 4)                               # degrees above 3 are out of scope
        c.push_sh(scene.sh(3)[half:], 3)                                         # append-only: the rest
        assert c.sh_count() == (scene.n, 3)
        with plain_context(scene.substituted(3, cam["gs_mv"])) as p:
            assert np.array_equal(draw(c, cam), draw(p, cam))
        # the option lowered from 3 to 1 between frames = a store truncated to degree 1
        c.set_option(capi.OPT_SH_DEGREE, 1)
        low = draw(c, cam)
        assert c.stats()["sh_degree"] == 1
        with sh_context(scene, 1, "push") as t:
            assert np.array_equal(low, draw(t, cam))
        with plain_context(scene.substituted(1, cam["gs_mv"])) as p:
            assert np.array_equal(low, draw(p, cam))
        c.set_option(capi.OPT_SH_DEGREE, 0)                                      # off again: the packed bytes, the store kept
        with plain_context(scene.rows) as p:
            assert np.array_equal(draw(c, cam), draw(p, cam))
        assert c.stats()["sh_degree"] == 0 and c.sh_count() == (scene.n, 3)
        # gs_clear empties the store: a plain push afterwards draws plain colours, whatever the option
        c.set_option(capi.OPT_SH_DEGREE, 3)
        c.clear()
        assert c.sh_count() == (0, 0)
        c.push_splat(scene.rows)
        with plain_context(scene.rows) as p:
            assert np.array_equal(draw(c, cam), draw(p, cam))
        assert c.stats()["sh_degree"] == 0
        c.push_sh(scene.sh(2), 2)                                                # ... and accepts rows of another degree
        with plain_context(scene.substituted(2, cam["gs_mv"])) as p:
            assert np.array_equal(draw(c, cam), draw(p, cam))
        # a singular model_view is refused only while SH is active
        bad = params(cam)
        for i in (8, 9, 10):
            bad.model_view[i] = 0.0
        with pytest.raises(capi.GsError) as ei:
            c.render(bad)
        assert ei.value.code == capi.E_BADARG
        c.set_option(capi.OPT_SH_DEGREE, 0)
        c.render(bad)


# ---------------------------------------------------------------- 11. defaults untouched

def test_default_keeps_no_sh_store(scene):
    with capi.Context(0) as c:
        c.load_ply(scene.ply)                                                    # 45 coefficients per splat, option never set
        assert c.sh_count() == (0, 0) and c.download_sh().shape[0] == 0
        cam = cams_for((5.0,))[0]
        with plain_context(scene.rows) as p:
            assert np.array_equal(draw(c, cam), draw(p, cam))
        assert c.stats()["sh_degree"] == 0
        with pytest.raises(capi.GsError):
            c.set_option(capi.OPT_SH_DEGREE, 4)
