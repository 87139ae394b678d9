"""GPU tier: k_project's culls on the crafted scenes of test_project_edges_cpu.py (every exit of gsm::project_splat with rows 0, +-1 and
+-16 ulp around its threshold, head-on isotropic splats, the 1024 and l2 = 0.1 clamps, infinite scales, NaN and Inf positions), one
pose per frame size (640 x 360, 77 x 53).  EVERY sorted position is compared, none skipped:
  * where the oracle says visible and the splat's pixel bounds (gsm::splat_pixel_bounds, clamped as k_project clamps them for a whole frame: columns
    [0, W), rows [0, H)) meet the frame, GS_BUF_PROJECTED words 0-5 and 7 equal the oracle's bit for bit;
  * GS_BUF_TILE_COUNT == 0 wherever the oracle says invisible or those bounds miss the frame, and > 0 wherever a pixel centre of the
    frame passes gsm::frag_power <= 4.0f (hc_reach_sweep's truth); between the two -- bounds that meet the frame, an ellipse that passes
    no pixel centre -- either is right;
  * the frame is within 1 LSB of oracle.render on the span lists and on the row walk, the counting frame counts the oracle's fragments.
test_gpu_parity.test_projected_records_bit_exact stays as it is."""
import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_gpu_parity import assert_path, force_path, pix_check
from test_host_check import hc  # noqa: F401
from test_project_edges_cpu import FRAMES, edge_rows, project_both
from test_reach_cpu import lib, sweep  # noqa: F401

pytestmark = pytest.mark.gpu
capi = pkg("capi")


@pytest.mark.parametrize("frame", range(len(FRAMES)))
def test_every_sorted_position_against_the_oracle(lib, frame):
    W, H = FRAMES[frame]
    pose, rows, kinds = edge_rows(W, H)
    cs, cc, mats = oracle.pack(rows.reshape(-1))
    vis, bad, recs, bounds = project_both(lib, pose, rows, W, H)
    assert not bad, bad[0]
    truth = (sweep(lib, pose, rows, W, H, 0, W, nine=0)["flags"] & 1) != 0
    on_frame = vis & (np.maximum(bounds[:, 0], 0.0) <= np.minimum(bounds[:, 1], W - 1.0)) & (np.maximum(bounds[:, 2], 0.0) <= np.minimum(bounds[:, 3], H - 1.0))
    want_idx = oracle.sort(np.ascontiguousarray(mats[:, 12:16]), pose["view"])
    par = lambda **kw: capi.make_params(pose["mv"].astype(np.float64), pose["proj"].astype(np.float64), W, H, focal_=float(pose["focal"]), **kw)
    want_img, _, want_frags = oracle.render(cs, cc, want_idx, pose["mv"], pose["proj"], pose["focal"], W, H, want_f32=False)
    assert want_frags > 0
    for path in ("lists", "walk"):
        with capi.Context(0) as c:
            force_path(c, path)
            c.push_splat(rows.reshape(-1))
            idx = c.sort(pose["view"])
            assert np.array_equal(idx, want_idx)
            got = c.render(par())
            assert_path(c, path, (W, H))
            pix_check("project_edges_%dx%d_%s" % (W, H, path), got, want_img)
            V = idx.size
            rec = c.download(capi.BUF_PROJECTED, V, np.float32, 8)
            cnt = c.download(capi.BUF_TILE_COUNT, V, np.uint32, 1).reshape(-1)
            n_rec = n_zero = n_touch = 0
            for j in range(V):
                i = int(idx[j])
                if not on_frame[i]:
                    assert cnt[j] == 0, "%s position %d row %d %s: the oracle says %s, tile count %d" % (
                        path, j, i, rows[i].tobytes().hex(), "visible but off the frame" if vis[i] else "invisible", int(cnt[j]))
                    n_zero += 1
                    continue
                o = recs[i]
                want = np.array([o.cx, o.cy, o.ax, o.ay, o.bx, o.by, o.alpha], np.float32)
                have = np.concatenate([rec[j, :6], rec[j, 7:8]])
                assert np.array_equal(have.view(np.uint32), want.view(np.uint32)), "%s position %d row %d %s: record %s, oracle %s" % (
                    path, j, i, rows[i].tobytes().hex(), have.tolist(), want.tolist())
                n_rec += 1
                if truth[i]:
                    assert cnt[j] > 0, "%s position %d row %d %s: covers a pixel centre, tile count 0" % (path, j, i, rows[i].tobytes().hex())
                    n_touch += 1
            print("project edges %dx%d %s: %d positions, %d records equal, %d with tile count 0 as the oracle says, %d touching" % (W, H, path, V, n_rec, n_zero, n_touch))
            assert n_rec >= 200 and n_zero >= 60 and n_touch >= 150
            assert c.stats()["n_visible"] == int((cnt > 0).sum())
            if path == "lists":
                c.render(par(flags=capi.RENDER_COUNT_FRAGS))
                assert c.stats()["n_frags"] == want_frags, (c.stats()["n_frags"], want_frags)
