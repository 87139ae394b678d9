"""GPU tier of the highlighted selection (GS_OPT_HIGHLIGHT, include/gs_splat.h).

The claim: with the option on, a frame's projection replaces the RGB bytes of the colour word of every SELECTED splat it writes a record
for by the integer rule of the header -- and nothing else.  So context A (the rows, the states, the option) must draw, bit for bit, what
context B draws that was pushed rows whose RGB bytes the numpy mirror (test_highlight_cpu.highlight_mirror) replaced for the selected
splats and that has neither states nor the option -- on every way a frame is drawn.  The scene is test_edit_gpu's: 4096 splats at
256 x 144, the nearest quarter of the order selected; `dense` (large opaque splats) so that tiles saturate within the first binning
round and the row walk has long runs."""
import numpy as np
import pytest

from conftest import pkg
from test_edit_gpu import orbit_frames, scene
from test_gpu_parity import assert_path, force_path
from test_highlight_cpu import highlight_mirror

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")
HL = capi.OPT_HIGHLIGHT
SELECTED = capi.STATE_SELECTED
PINK = capi.highlight_option((255, 32, 200), 160)
CYAN = capi.highlight_option((0, 240, 255), 96)


def states_of(sc, rows=None):
    """the nearest quarter of the order selected (user bits set on others: they change nothing)"""
    st = np.where(sc.hid, SELECTED, 0).astype(np.uint8)
    st[~sc.hid] |= 0x40
    return st if rows is None else st[:rows]


def mirrored_rows(sc, value, rows=None, base=None):
    """the rows with the RGB bytes of the selected splats [0, rows) replaced by the rule"""
    out = (sc.rows if base is None else base).copy()
    sel = sc.hid.copy()
    if rows is not None:
        sel[rows:] = False
    word = np.ascontiguousarray(out[sel, 24:28]).view("<u4").reshape(-1)
    out[sel, 24:28] = highlight_mirror(word, value).astype("<u4").view(np.uint8).reshape(-1, 4)
    return out


def ctx_a(sc, value=PINK, opts=(), store=None, path=None, permille=1000):
    c = capi.Context(0)
    if path is not None:
        force_path(c, path, permille)
    for k, v in opts:
        c.set_option(k, v)
    c.push_splat(sc.rows)
    c.set_state(0, states_of(sc, store))
    c.set_option(HL, value)
    return c


def ctx_b(rows, opts=(), path=None, permille=1000):
    c = capi.Context(0)
    if path is not None:
        force_path(c, path, permille)
    for k, v in opts:
        c.set_option(k, v)
    c.push_splat(rows)
    return c


def draw(c, sc, params=None):
    c.sort(sc.cam["view"], want_indices=False)
    return c.render(sc.params if params is None else params)


# ---------------------------------------------------------------- the option

def test_option_values_and_a_fresh_context():
    sc = scene()
    with capi.Context(0) as c:
        for bad in (-1, 1 << 32, -(1 << 40)):
            with pytest.raises(capi.GsError) as e:
                c.set_option(HL, bad)
            assert e.value.code == capi.E_BADARG
        assert c.highlight_info() == (0, 0)
        c.push_splat(sc.rows)
        plain = draw(c, sc)
        assert c.highlight_info() == (0, 0)
        # option on, but no store: the plain kernels, the plain frame
        c.set_option(HL, 0xFFFFFFFF)
        assert np.array_equal(c.render(sc.params), plain) and c.highlight_info() == (0xFFFFFFFF, 0)
        # a store, W = 0: off whatever the colour bytes
        c.set_state(0, states_of(sc))
        c.set_option(HL, 0x00FFFFFF)
        assert np.array_equal(draw(c, sc), plain) and c.highlight_info() == (0x00FFFFFF, 0)
        c.set_option(HL, PINK)
        on = c.render(sc.params)
        assert c.highlight_info() == (PINK, 1) and not np.array_equal(on, plain)
        # the colour changes between two frames without a sort in between
        c.set_option(HL, CYAN)
        on2 = c.render(sc.params)
        c.set_option(HL, 0)
        assert np.array_equal(c.render(sc.params), plain) and c.highlight_info() == (0, 0)
    for value, img in ((PINK, on), (CYAN, on2)):
        with ctx_b(mirrored_rows(sc, value)) as b:
            assert np.array_equal(draw(b, sc), img), hex(value)
    assert not np.array_equal(on, on2)


# ---------------------------------------------------------------- every path

@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("permille", [1000, 200])
@pytest.mark.parametrize("path", ["lists", "walk", "subtile", "pairs"])
def test_frame_equals_frame_of_mirrored_rows(path, permille, dense):
    sc = scene(dense=dense)
    with ctx_a(sc, path=path, permille=permille) as a, ctx_b(mirrored_rows(sc, PINK), path=path, permille=permille) as b:
        fa, fb = draw(a, sc), draw(b, sc)
        sta, stb = assert_path(a, path), assert_path(b, path)
        assert a.highlight_info() == (PINK, 1) and b.highlight_info() == (0, 0)
        print("unsaturated tiles after round 0:", sta["unsat_tiles"], "pairs:", sta["n_pairs"])
        if permille < 1000 and not dense:
            assert sta["unsat_tiles"] > 0, "the second binning round did not run: the case proves nothing"
        for k in ("n_sorted", "n_visible", "n_pairs", "unsat_tiles"):
            assert sta[k] == stb[k], k
        assert fa.any() and np.array_equal(fa, fb)
        a.set_option(HL, 0)
        assert not np.array_equal(a.render(sc.params), fa), "the highlight did not change the picture"


def test_default_options_split_blend_and_antialias():
    sc = scene()
    for opts in ((), ((capi.OPT_BLEND_SPLIT, 1),), ((capi.OPT_ANTIALIAS, 1),)):
        with ctx_a(sc, opts=opts) as a, ctx_b(mirrored_rows(sc, PINK), opts=opts) as b:
            fa = draw(a, sc)
            assert a.highlight_info()[1] == 1
            assert np.array_equal(fa, draw(b, sc)), opts
            if opts and opts[0][0] == capi.OPT_ANTIALIAS:
                assert a.stats()["antialias"] == 1 and b.stats()["antialias"] == 1


def test_stereo_strip_and_surface():
    sc = scene()
    with ctx_a(sc) as a, ctx_b(mirrored_rows(sc, PINK)) as b:
        l, r, head = synth.xr_eye_cameras(yaw_deg=10.0, xr_pixel_ratio=0.1, capi=capi)
        eyes = [capi.make_params(e["gs_mv"], e["gs_proj"], e["vw"], e["vh"], focal_=e["focal"]) for e in (l, r)]
        a.sort(head["view"], want_indices=False); b.sort(head["view"], want_indices=False)
        for x, y in zip(a.render_stereo(*eyes), b.render_stereo(*eyes)):
            assert x.any() and np.array_equal(x, y)
        assert a.highlight_info()[1] == 1
        # a strip after its own sort, x0 a multiple of 16
        strip = capi.make_params(sc.cam["gs_mv"], sc.cam["gs_proj"], sc.W, sc.H, x0=64, x1=128, focal_=sc.cam["focal"])
        whole_b = draw(b, sc)
        for c in (a, b):
            c.sort_for(sc.cam["view"], None, strip, want_indices=False)
        sa, sb = a.render(strip), b.render(strip)
        assert sa.any() and np.array_equal(sa, sb) and np.array_equal(sa, whole_b[:, 64:128])
        # surface: the colour is B's, the planes are A's without the option
        a.sort(sc.cam["view"], want_indices=False); b.sort(sc.cam["view"], want_indices=False)
        ca, ida, da, aa = a.render_surface(sc.params)
        assert a.highlight_info()[1] == 1
        cb, _, _, _ = b.render_surface(sc.params)
        a.set_option(HL, 0)
        c0, id0, d0, a0 = a.render_surface(sc.params)
        assert np.array_equal(ca, cb) and not np.array_equal(ca, c0)
        assert (ida != capi.SURFACE_NONE).any()
        assert np.array_equal(ida, id0) and np.array_equal(da.view(np.uint32), d0.view(np.uint32)) and np.array_equal(aa.view(np.uint32), a0.view(np.uint32))
        pts = [(40, 30), (128, 72), (200, 100)]
        a.set_option(HL, PINK)
        for h, (x, y) in zip(a.pick(sc.params, pts), pts):
            assert h["id"] == id0[y, x]


def test_asynchronous_paired_orbit():
    sc = scene(dense=True)
    opts = [(capi.OPT_PIPELINE_DEPTH, 3), (capi.OPT_FRAME_BATCH, 2)]
    with ctx_a(sc, opts=opts) as a, ctx_b(mirrored_rows(sc, PINK), opts=opts) as b:
        fa, _ = orbit_frames(a, sc.W, sc.H)
        assert a.highlight_info() == (PINK, 1)
        fb, _ = orbit_frames(b, sc.W, sc.H)
        assert b.highlight_info() == (0, 0)
        a.set_option(HL, 0)
        f0, _ = orbit_frames(a, sc.W, sc.H)
        for k in range(len(fa)):
            assert fa[k].any() and np.array_equal(fa[k], fb[k]), k
        assert any(not np.array_equal(x, y) for x, y in zip(fa, f0))


def test_two_contexts_of_one_process():
    sc = scene()
    out = []
    for rows, edited in ((sc.rows, True), (mirrored_rows(sc, PINK), False)):
        with capi.Multi([0, 0]) as m:
            m.push_splat(rows)
            if edited:
                m.set_state(0, states_of(sc))
                m.set_option(HL, PINK)                                  # through gs_multi_set_option
            frame, owner = capi.host_frame(sc.H, sc.W)
            m.sort(sc.cam["view"], None, sc.params)
            m.render(sc.params, frame)
            m.sync()
            if edited:
                assert [m.ctx_highlight_info(i) for i in range(2)] == [(PINK, 1), (PINK, 1)]
            out.append(frame.copy()); owner.free()
    assert out[0].any() and np.array_equal(out[0], out[1])
    with ctx_b(sc.rows) as plain:
        assert not np.array_equal(draw(plain, sc), out[0])


# ---------------------------------------------------------------- combinations and edges

def test_with_view_dependent_colour():
    """order: SH, then highlight.  B's bytes are highlight(sh_eval) for the selected splats and sh_eval for the others; B has SH off"""
    sc = scene()
    n = sc.n
    sh = (np.random.default_rng(31).standard_normal((n, 48)) * 0.35).astype(np.float32)
    pos = sc.rows[:, 0:12].copy().view("<f4").reshape(n, 3)
    cam_obj = capi.camera_in_object(sc.cam["gs_mv"].astype(np.float32)) * np.array([1.0, 1.0, -1.0])
    base = sc.rows.copy()
    for i in range(n):
        base[i, 24:27] = capi.sh_eval(sh[i], 3, cam_obj, pos[i])
    assert (base[:, 24:27] != sc.rows[:, 24:27]).any()
    with ctx_a(sc, opts=[(capi.OPT_SH_DEGREE, 3)]) as a, ctx_b(mirrored_rows(sc, PINK, base=base)) as b, ctx_b(base) as sh_only:
        a.push_sh(sh, 3)
        fa = draw(a, sc)
        assert a.stats()["sh_degree"] == 3 and a.highlight_info()[1] == 1 and b.stats()["sh_degree"] == 0
        assert np.array_equal(fa, draw(b, sc))
        assert not np.array_equal(fa, draw(sh_only, sc))


def test_store_shorter_than_the_cloud():
    sc = scene()
    order_sel = np.flatnonzero(sc.hid)
    store = int(np.median(order_sel))                                  # about half of the selected splats lie beyond the store
    assert 0 < (order_sel < store).sum() < order_sel.size
    with ctx_a(sc, store=store) as a, ctx_b(mirrored_rows(sc, PINK, rows=store)) as b, ctx_b(mirrored_rows(sc, PINK)) as whole:
        assert a.state_count()[0] == store
        fa = draw(a, sc)
        assert np.array_equal(fa, draw(b, sc)) and not np.array_equal(fa, draw(whole, sc))


def test_after_compact_the_selected_bits_travel():
    sc = scene()
    g = np.random.default_rng(9)
    hide = g.random(sc.n) < 0.3
    assert (hide & sc.hid).any() and (~hide & sc.hid).any()
    kept = np.flatnonzero(~hide)
    st = states_of(sc) | np.where(hide, capi.STATE_HIDDEN, 0).astype(np.uint8)
    with capi.Context(0) as a, ctx_b(mirrored_rows(sc, PINK)[kept]) as b:
        a.push_splat(sc.rows)
        a.set_state(0, st)
        a.set_option(HL, PINK)
        assert np.array_equal(a.compact(), kept)
        assert np.array_equal(a.download_state(), states_of(sc)[kept])
        fa = draw(a, sc)
        assert a.highlight_info() == (PINK, 1)
        assert fa.any() and np.array_equal(fa, draw(b, sc))
