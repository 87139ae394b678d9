"""GPU tier of gs_select_mask (include/gs_splat.h): selection by a mask image over the last whole order, optionally limited by a plane of
window depths.  The construction is test_edit_gpu.test_select_rect's: n = 2048 at 320 x 180 (and 321 x 181, so that a stride or row-flip
mistake cannot cancel out), every seventh splat hidden; oracle.project gives visible, cx, cy and zndc (tests/test_host_check.py pins them
to the kernel's values), and the rule of the header is mirrored in numpy: hit counts and the downloaded store must be exact."""
import functools

import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_edit_gpu import want_order

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")
HIDDEN, SELECTED, INVERT = capi.STATE_HIDDEN, capi.STATE_SELECTED, capi.SELECT_INVERT
N = 2048


class Frame:
    def __init__(self, W, H):
        self.W, self.H, n = W, H, N
        self.rows = synth.make_splat_rows(n, seed=21).reshape(n, 32)
        self.cam = synth.index_html_camera(W, H, yaw_deg=25.0, capi=capi)
        self.p = capi.make_params(self.cam["gs_mv"], self.cam["gs_proj"], W, H, focal_=self.cam["focal"])
        cs, cc, mats = oracle.pack(self.rows.reshape(-1))
        self.hid = np.zeros(n, bool); self.hid[::7] = True
        self.order = want_order(mats[:, 12:16], self.hid, self.cam["view"])
        assert len(np.unique(self.order)) == self.order.size                  # (no zero tail in this scene: positions are splats)
        mv, P = self.cam["gs_mv"].astype(np.float32), self.cam["gs_proj"].astype(np.float32)
        self.col, self.row = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
        self.zwin = np.full(n, np.nan, np.float32)
        for i in self.order:
            o = oracle.project(cs, cc, int(i), mv, P, self.cam["focal"], W, H)
            if o.visible and np.isfinite(o.cx) and np.isfinite(o.cy):
                c, r = int(np.floor(o.cx)), H - 1 - int(np.floor(o.cy))
                if 0 <= c < W and 0 <= r < H:
                    self.col[i], self.row[i] = c, r
                    self.zwin[i] = np.float32(np.float32(o.zndc) * np.float32(0.5)) + np.float32(0.5)   # what k_project writes to zwin
        self.in_order = np.zeros(n, bool); self.in_order[self.order] = True
        self.on = np.flatnonzero(self.col >= 0)
        assert self.on.size > 100

    def want(self, mask, depth=None):
        """the splats the rule takes: in the order, accepted, centre pixel in the frame, mask set there, depth <= the plane there"""
        w = np.zeros(N, bool)
        on = self.on
        w[on] = mask[self.row[on], self.col[on]] != 0
        if depth is not None:
            with np.errstate(invalid="ignore"):
                w[on] &= self.zwin[on] <= depth[self.row[on], self.col[on]]       # (a NaN on either side: false)
        return w & self.in_order

    def state0(self):
        return self.hid.astype(np.uint8)

    def context(self):
        c = capi.Context(0)
        c.push_splat(self.rows); c.set_state(0, self.state0())
        return c


@functools.lru_cache(maxsize=None)
def frame(W, H):
    return Frame(W, H)


def masks_of(f):
    W, H = f.W, f.H
    one = np.zeros((H, W), np.uint8)
    k = f.on[3]
    one[f.row[k], f.col[k]] = 7
    yy, xx = np.mgrid[0:H, 0:W]
    lasso = capi.mask_polygon([(20.5, 10.0), (W - 30.0, 25.0), (W * 0.75, H - 12.0), (W * 0.5, H * 0.4), (35.0, H - 20.0)], W, H)
    assert 0.2 < lasso.mean() < 0.8
    padded = np.full((H, 323 if W <= 323 else W + 3), 255, np.uint8)            # not tight; the padding bytes are 255
    padded[:, :W] = ((xx // 16 + yy // 16) % 3 == 0) * 255
    return [("zero", np.zeros((H, W), np.uint8), 0), ("full", np.full((H, W), 255, np.uint8), None), ("one_pixel", one, None),
            ("checkerboard", (((xx + yy) & 1) * 200).astype(np.uint8), None), ("lasso", lasso, None), ("stride_323", padded[:, :W], None)]


def check(c, f, mask, depth, tag):
    want = f.want(np.asarray(mask), depth)
    for inv in (0, INVERT):
        w = (f.in_order & ~want) if inv else want
        c.set_state(0, f.state0())
        c.sort(f.cam["view"], want_indices=False)
        hit = c.select_mask(f.p, mask, depth, set_bits=SELECTED, flags=inv)
        assert hit == w.sum(), (tag, inv, hit, int(w.sum()))
        assert np.array_equal(c.download_state(), f.state0() | np.where(w, SELECTED, 0).astype(np.uint8)), (tag, inv)
    return want


@pytest.mark.parametrize("size", [(320, 180), (321, 181)])
def test_masks_with_and_without_invert(size):
    f = frame(*size)
    with f.context() as c:
        for name, mask, expect in masks_of(f):
            if name == "stride_323":
                assert mask.strides[0] != mask.shape[1] and not mask.flags.c_contiguous
            want = check(c, f, mask, None, name)
            assert want.sum() == expect if expect is not None else want.sum() >= 1, name
            if name in ("checkerboard", "lasso", "stride_323"):
                assert 0 < want.sum() < (f.in_order & (f.col >= 0)).sum(), name                        # neither nothing nor everything on screen
        assert not f.hid[np.flatnonzero(want)].any()


def test_depth_planes():
    f = frame(320, 180)
    full = np.full((f.H, f.W), 255, np.uint8)
    seen = f.in_order.copy(); seen[f.col < 0] = False
    med = np.sort(f.zwin[seen])[seen.sum() // 2]                              # the median, a depth that occurs: the LEQUAL edge is in the case
    with f.context() as c:
        plane = np.full((f.H, f.W), med, np.float32)
        want = check(c, f, full, plane, "median")
        assert 0 < want.sum() < seen.sum(), "both sides of the plane must be non-empty"
        assert want[f.zwin == med].all()
        g = np.random.default_rng(77)
        mixed = g.choice(np.array([np.nan, 0.0, 1.0, med], np.float32), size=(f.H, f.W)).astype(np.float32)
        want = check(c, f, full, mixed, "nan_and_zero")
        at = mixed[f.row[f.on], f.col[f.on]]
        assert np.isnan(at).any() and (at == 0).any() and 0 < want.sum() < seen.sum()
        assert not want[f.on][np.isnan(at) | (at == 0)].any()
        check(c, f, masks_of(f)[4][1], mixed, "lasso_and_depth")


def test_surface_depth_plane_selects_what_is_visible():
    """depth_max = the depth plane of gs_render_surface of the same frame.  The plane at a pixel is the window depth of that pixel's
    surface splat, so a splat that is the surface AT ITS OWN CENTRE PIXEL passes the LEQUAL test with equality and must be selected
    (a splat that is the surface elsewhere but lies behind the surface at its own centre is rightly not); the selection equals the
    mirror on the downloaded plane and is a subset of the selection without a plane."""
    f = frame(320, 180)
    mask = masks_of(f)[4][1]
    with f.context() as c:
        c.sort(f.cam["view"], want_indices=False)
        _, sid, depth, _ = c.render_surface(f.p)
        assert np.array_equal(c.download_state(), f.state0())                     # (drawing changes no state)
        want = check(c, f, mask, depth, "surface")
        no_depth = f.want(mask)
        assert 0 < want.sum() < no_depth.sum() and not (want & ~no_depth).any()
        ids = np.unique(sid[sid != capi.SURFACE_NONE])
        ids = ids[f.col[ids] >= 0]
        own = ids[(sid[f.row[ids], f.col[ids]] == ids) & (mask[f.row[ids], f.col[ids]] != 0)]
        centre_in_mask = ids[mask[f.row[ids], f.col[ids]] != 0]
        print("surface ids in the mask: %d, centre in the mask: %d, surface at their own centre: %d, of those selected: %d; "
              "selected among all with the centre in the mask: %d" % (ids.size, centre_in_mask.size, own.size, want[own].sum(), want[centre_in_mask].sum()))
        assert own.size > 10 and want[own].all()


def test_full_mask_is_select_rect_strip_sort_state_error_and_multi():
    f = frame(320, 180)
    full = np.full((f.H, f.W), 1, np.uint8)
    with f.context() as c:
        with pytest.raises(capi.GsError) as e:
            c.select_mask(f.p, full, set_bits=SELECTED)
        assert e.value.code == capi.E_STATE                                       # no completed order yet
        with pytest.raises(ValueError):
            c.select_mask(f.p, full[:, :-1], set_bits=SELECTED)
        c.sort(f.cam["view"], want_indices=False)
        n_rect = c.select_rect(f.p, (0, 0, f.W, f.H), set_bits=SELECTED)
        by_rect = c.download_state()
        c.set_state(0, f.state0()); c.sort(f.cam["view"], want_indices=False)
        assert c.select_mask(f.p, full, set_bits=SELECTED) == n_rect == f.want(full).sum()
        assert np.array_equal(c.download_state(), by_rect)
        # after a strip sort the mask still walks the WHOLE order
        strip = capi.make_params(f.cam["gs_mv"], f.cam["gs_proj"], f.W, f.H, x0=0, x1=64, focal_=f.cam["focal"])
        c.set_state(0, f.state0())
        c.sort_for(f.cam["view"], None, strip, want_indices=False)
        lasso = masks_of(f)[4][1]
        assert c.select_mask(f.p, lasso, set_bits=SELECTED) == f.want(lasso).sum()
        assert np.array_equal(c.download_state(), f.state0() | np.where(f.want(lasso), SELECTED, 0).astype(np.uint8))
        # hide instead of select: gone from the next order
        c.sort(f.cam["view"], want_indices=False)
        c.select_mask(f.p, lasso, set_bits=HIDDEN)
        assert c.state_count()[1] == (f.hid | f.want(lasso)).sum()
    with capi.Multi([0, 0]) as m:
        m.push_splat(f.rows); m.set_state(0, f.state0())
        m.sort(f.cam["view"], None, f.p)
        fr, owner = capi.host_frame(f.H, f.W)
        m.render(f.p, fr); m.sync()
        lib = capi.load()
        assert m.select_mask(f.p, lasso, set_bits=SELECTED) == f.want(lasso).sum()
        for i in range(2):
            st = np.zeros(N, np.uint8)
            assert lib.gs_download(lib.gs_multi_ctx(m._h, i), capi.BUF_STATE, st.ctypes.data, N) == capi.GS_OK
            assert np.array_equal(st, f.state0() | np.where(f.want(lasso), SELECTED, 0).astype(np.uint8)), i
        owner.free()
