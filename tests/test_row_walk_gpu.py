"""GPU tier: GS_OPT_ROW_WALK (round 7) -- round 0 of a span-list frame building no tile lists, its blend collecting each tile's
entries from the runs of the tile's row instead (64 runs per step: a ballot of the runs that cover the tile's column).  A tile's list
IS the runs of its row that cover its column, in run order, and the walk fills the blend's batches of 64 with the same entries in
the same slots, so the frames must be the SAME frames, bit for bit, as the list path's -- and so must everything the blend leaves
behind: the tiles left unsaturated for round 1, the need records the adaptive first-round share is set from, the completion words.

Compared here, the walk forced on (2) against off (0): the C1, C2 and C3 scenes and poses; the whole frame and two column strips;
one binning round and two (tiny, medium and adaptive first-round shares: round 1 keeps the lists and resumes per-pixel state);
the opaque scene's depth buffer and colour image; queued frames alone and in pairs (two frames per launch); and the automatic
setting (1): on at the headline pose, off where splats are small (the cloud seen from outside)."""
import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu
capi = pkg("capi")
synth = pkg("synth")
bc = pkg("bench_configs")


def _frame(c, cam, params, cutout):
    c.sort(cam["view"], cutout, want_indices=False)
    img = c.render(params)
    st = c.stats()
    return img, c.frame_status(), {k: st[k] for k in ("n_pairs", "n_visible", "need_splats", "near_permille", "unsat_tiles", "row_walk")}


@pytest.mark.parametrize("name", ["C1", "C2", "C3"])
def test_row_walk_changes_no_pixel_and_no_record(name):
    cfg = bc.ALL[name]
    rows = bc.make_rows(cfg, synth)
    cams, views, w, h = bc.poses(cfg, synth, capi, frames=[7])
    cam, base = cams[7], views[7][0]
    cutout = cam.get("cutout")
    tx, ty = (w + 15) // 16, (h + 15) // 16
    mw = (tx + 31) // 32
    x0 = (w // 3) & ~3
    strips = [(0, w), (x0, x0 + 16), (x0 + 4, min(w, x0 + 611))]
    depth = np.full((h, w), 0.9996, np.float32); depth[:, : w // 2] = 1.0
    rgba = np.zeros((h, w, 4), np.uint8); rgba[..., 2] = 70; rgba[..., 3] = 255

    def params(a, b):
        return capi.make_params(cam["gs_mv"], cam["gs_proj"], w, h, focal_=cam["focal"], x0=a, x1=b)

    out = {}
    for mode in (0, 2):
        res = []
        with capi.Context(0) as c:
            c.set_option(capi.OPT_ROW_WALK, mode)
            c.set_option(capi.OPT_SUBTILE, 0)                       # (the sub-tile lists keep the list path)
            bc.push_rows(c, rows)
            for permille in (1000, 3, 400, 0):
                c.set_option(capi.OPT_NEAR_PERMILLE, permille)
                for scene in (False, True):
                    if scene:
                        c.set_scene(depth, rgba)
                    for a, b in strips:
                        img, status, st = _frame(c, cam, params(a, b), cutout)
                        mask = c.download(capi.BUF_UNSAT_MASK, ty, np.uint32, mw)
                        res.append(((permille, scene, a, b), img, mask, status, st))
                        if mode == 2 and permille == 1000:
                            assert st["row_walk"] == 1, (name, a, b)
                    if scene:
                        c.set_scene(None, None)
            c.set_option(capi.OPT_NEAR_PERMILLE, 0)
            for batch in (1, 2):
                c.set_option(capi.OPT_FRAME_BATCH, batch)
                bufs = [capi.host_frame(h, w) for _ in range(5)]
                for b, _ in bufs:
                    c.sort(cam["view"], cutout, want_indices=False)
                    c.render_into(capi.make_params(cam["gs_mv"], cam["gs_proj"], w, h, focal_=cam["focal"], flags=capi.RENDER_ASYNC), b)
                c.sync()
                st = c.stats()
                for b, o in bufs:
                    res.append((("queued", batch), b.copy(), None, None, {k: st[k] for k in ("n_pairs", "n_visible", "need_splats", "near_permille")}))
                    o.free()
        out[mode] = res
    assert len(out[0]) == len(out[2])
    rounds1 = 0
    for a, b in zip(out[0], out[2]):
        tag = a[0]
        assert tag == b[0]
        assert np.array_equal(a[1], b[1]), (name, tag, int(np.abs(a[1].astype(np.int16) - b[1].astype(np.int16)).max()))
        if a[2] is not None:
            assert np.array_equal(a[2], b[2]), (name, tag, "unsaturated tiles")
            rounds1 += int(a[2].any())
        assert a[3] == b[3], (name, tag, "completion word", a[3], b[3])
        sa, sb = dict(a[4]), dict(b[4])
        sa.pop("row_walk", None); sb.pop("row_walk", None)
        assert sa == sb, (name, tag, sa, sb)
    assert rounds1 > 0, "no frame ran a second binning round"


def test_row_walk_chooses_itself_at_the_headline_and_not_outside_the_cloud():
    """GS_OPT_ROW_WALK = 1 (the default): decided from the last collected frame -- tiles per visible splat and runs per tile row.  At
    the headline pose (C2: dozens of tiles per splat) the second frame walks the rows; from outside the cloud (R_outside: 3-4 tiles per
    splat, rows of ~27 000 runs) it keeps the lists."""
    for name, want in (("C2", 1), ("R_outside", 0)):
        cfg = bc.ALL[name]
        rows = bc.make_rows(cfg, synth)
        cams, views, w, h = bc.poses(cfg, synth, capi, frames=[3])
        cam = cams[3]
        imgs = {}
        for mode in (1, 0):
            with capi.Context(0) as c:
                c.set_option(capi.OPT_ROW_WALK, mode)
                bc.push_rows(c, rows)
                got = []
                for _ in range(3):
                    img, _, st = _frame(c, cam, views[3][0], cam.get("cutout"))
                    got.append(st["row_walk"])
                imgs[mode] = img
            if mode == 1:
                print("%s: row walk per frame %s, %.1f tiles per visible splat" % (name, got, st["n_pairs"] / max(1, st["n_visible"])))
                assert got[0] == 0 and got[1:] == [want, want], (name, got)
        assert np.array_equal(imgs[0], imgs[1])
