"""GPU tier: gs_sort_for's reach test on the hardware's own v_rcp_f32 / v_sqrt_f32, on the scenes of the CPU tier (test_reach_cpu.py:
the same generators, a fixed subset of its poses -- one rigid, model scale (1, 1, 3), two of the family whose top right-singular
vector is orthogonal to the old power iteration's start, one XR eye sorted with the head camera's view row), 2 280 rows per scene in a
640 x 360 frame: the base rows plus the grazing rows of all four strips.

Per pose and strip: sort() equals oracle.sort; sort_for() is a subsequence of it; what it left out holds no splat the CPU tier's truth
(hc_reach_sweep: visible, and a pixel centre of the strip passes frag_power <= 4.0f) says touches the strip -- an offender is named by
its row, not by a pixel difference; the strip drawn from the sub-order equals the strip drawn from the whole order bit for bit; a
counting frame counts the oracle's fragments; and the sub-order is no longer than 1.1 x what the host tier keeps at its IEEE setting
(the hardware's 1-ulp operations may move borderline splats; both numbers are printed).  One pose runs a second time with one splat
hidden through gs_set_state, so that the <STRIP, HID> instantiation of the depth pass runs: the same assertions, the oracle sorting
the input without that splat.  The STRIP forms reached only through queued pairs of several contexts stay with test_multirank_gpu.py."""
import numpy as np
import pytest

from conftest import pkg
from oracle import oracle
from test_host_check import hc  # noqa: F401
from test_reach_cpu import FRAMES, GPU_POSES, N_BASE, POSES, base_rows, grazing_rows, lib, sweep  # noqa: F401

pytestmark = pytest.mark.gpu
capi = pkg("capi")

W, H = FRAMES[0][0]
STRIPS = FRAMES[0][1]


def scene_of(lib, name):
    pose = POSES[name](W, H)
    seed = 77000 + 100 * sorted(POSES).index(name)
    parts = [base_rows(pose, W, H, seed, 2 * N_BASE - 104)] + [grazing_rows(lib, pose, W, H, x0, x1, seed + 1 + k) for k, (x0, x1) in enumerate(STRIPS)]
    rows = np.ascontiguousarray(np.concatenate(parts))
    cs, cc, mats = oracle.pack(rows.reshape(-1))
    return pose, rows, cs, cc, mats


def params(pose, x0=0, x1=None, **kw):
    return capi.make_params(pose["mv"].astype(np.float64), pose["proj"].astype(np.float64), W, H, x0=x0, x1=x1, focal_=float(pose["focal"]), **kw)


def check_pose(lib, name, hide):
    pose, rows, cs, cc, mats = scene_of(lib, name)
    n = rows.shape[0]
    assert 2048 <= n <= 4096, n
    rows4 = np.ascontiguousarray(mats[:, 12:16]).copy()
    with capi.Context(0) as c:
        c.set_option(capi.OPT_NEAR_PERMILLE, 1000)
        c.push_splat(rows.reshape(-1))
        hidden = None
        if hide:
            # a splat that touches the interior strip and is in the order: hiding it changes that strip
            x0, x1 = STRIPS[2]
            f = sweep(lib, pose, rows, W, H, x0, x1, nine=0)["flags"]
            order = oracle.sort(rows4, pose["view"])
            hidden = int(next(i for i in order[::-1] if f[i] & 1))
            c.set_state(hidden, [capi.STATE_HIDDEN])
            rows4[hidden, 3] = 0.0                                   # size 0 fails the reference's keep test (index.js:548): out of the oracle's input
        want_full = oracle.sort(rows4, pose["view"])
        assert want_full.size > n // 3
        assert hidden is None or hidden not in set(want_full.tolist())
        for x0, x1 in STRIPS:
            full = c.sort(pose["view"])
            assert np.array_equal(full, want_full), (name, "whole order")
            from_full = c.render(params(pose, x0, x1))
            sub = c.sort_for(pose["view"], None, params(pose, x0, x1))
            pos = np.full(n, -1, np.int64); pos[full] = np.arange(full.size)
            p = pos[sub]
            assert np.all(p >= 0) and np.all(np.diff(p) > 0), (name, x0, x1, "not a sub-sequence of the whole order")
            r = sweep(lib, pose, rows, W, H, x0, x1, nine=0)
            assert r["misses"] == 0
            truth, kept_host = (r["flags"] & 1) != 0, (r["flags"] & 2) != 0
            left_out = np.setdiff1d(full, sub)
            bad = left_out[truth[left_out]]
            assert bad.size == 0, "%s strip (%d, %d): sort_for left out %d splats that touch it; first: row %d %s" % (
                name, x0, x1, bad.size, int(bad[0]), rows[int(bad[0])].tobytes().hex())
            got = c.render(params(pose, x0, x1))
            assert np.array_equal(got, from_full), (name, x0, x1)
            c.render(params(pose, x0, x1, flags=capi.RENDER_COUNT_FRAGS))
            frags = c.stats()["n_frags"]
            _, _, want_frags = oracle.render(cs, cc, want_full, pose["mv"], pose["proj"], pose["focal"], W, H, x0, x1, want_f32=False)
            predicted = int(kept_host[full].sum())
            print("reach %s%s strip (%d, %d): whole order %d, sort_for %d, host tier keeps %d, touching %d, fragments %d (oracle %d)" % (
                name, " hidden %d" % hidden if hide else "", x0, x1, full.size, sub.size, predicted, int(truth[full].sum()), frags, want_frags))
            assert frags == want_frags, (name, x0, x1, frags, want_frags)
            assert sub.size <= 1.1 * predicted, (name, x0, x1, sub.size, predicted)
            assert sub.size >= int(truth[full].sum())
            if x1 - x0 <= W // 4:
                assert sub.size < full.size, (name, x0, x1, "nothing culled")


@pytest.mark.parametrize("name", GPU_POSES)
def test_sort_for_leaves_out_no_splat_that_touches_the_strip(lib, name):
    check_pose(lib, name, hide=False)


def test_the_same_with_a_hidden_splat(lib):
    check_pose(lib, "b_x_1.15", hide=True)
