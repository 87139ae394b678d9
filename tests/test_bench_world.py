"""CPU tier: the python the driver launches for its scaling runs (`python -m torch.distributed.run ... bench.py --gpus N`) executed
with world_size 2 and 3 over gloo, the GPU replaced by a stand-in IN THE TEST'S PROCESS (tests/host_check/bench_world_driver.py;
bench.py and the package are not touched): rendezvous, the communicator id handed from rank 0 to the others, barriers, the
agreement of all ranks on a retry, the self-check of the assembled frame, exactly ONE JSON line from rank 0."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "host_check", "bench_world_driver.py")


def run(world, port, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    e.pop("GS_SPLAT_LIB", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(port), DRIVER, "--gpus", str(world)] + list(args)
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, "rank 0 prints ONE line, the other ranks nothing: %r" % lines
    return json.loads(lines[0]), p.stderr


@pytest.mark.parametrize("world", [2, 3])
def test_column_strips_over_ranks(world):
    d, err = run(world, 29620 + world, "--full", "--steps", "6", "--warmup", "2")
    assert d["n_gpus"] == world and d["steps"] == 6 and d["warmup"] == 2 and d["value"] > 0 and d["scaling"] == "strong"
    assert d["config"]["parallelism"].startswith("column strips x%d" % world) and "RCCL" in d["config"]["parallelism"]
    assert d["config"]["gathered_frame_equals_single_gpu_render"] is True
    x = d["config"]["pieces_of_rank0"]
    assert len(x) == 1 and x[0][0] == 0 and x[0][1] == 0 and x[0][2] % 16 == 0 and x[0][2] <= 1920 // world + 16
    assert "roofline" in d and d["roofline"]["traffic"] is None            # (PMC passes exist for the one-GPU form only)
    assert "cpu_baseline" not in d                                          # rank 0 at N = 1 only
    for r in range(world):
        assert "rank %d calls" % r in err                                   # every rank ran to the end


def test_xr_eyes_over_two_ranks_and_a_retry_agreed_by_all():
    # rank 1's 5th gs_sync (the one closing the timed region; the first is the feature ladder's probe) reports an incomplete frame: BOTH ranks measure the region again
    d, err = run(2, 29631, "--xr", "--steps", "4", "--warmup", "2", env={"BENCH_STANDIN_RETRY": "1:5"})
    assert d["n_gpus"] == 2 and "XR" in d["metric"] and d["config"]["parallelism"].startswith("XR eyes divided over 2 GPUs")
    assert d["occlusion_binning"]["timed_region_retries"] == 1
    assert d["config"]["pieces_of_rank0"] == [[0, 0, 1032]]


def test_sort_share_switched_on_for_long_scenes_only():
    d, _ = run(2, 29632, "--steps", "4", "--warmup", "2", env={"GS_BENCH_SORT_SHARE": "30"})
    assert d["config"]["sort_share_permille"] == 30
    d, _ = run(2, 29633, "--steps", "4", "--warmup", "2")
    assert d["config"]["sort_share_permille"] == 0


def test_fallback_when_the_librarys_communicator_cannot_be_set_up():
    # gs_comm_init fails on ONE rank.  The run still yields a line (VERDICT r4 "next" #8: the first real multi-GPU run must, whatever breaks):
    # the last rung of the ladder -- strips gathered by torch.distributed -- labelled as the FALLBACK it is, with what was tried before it
    d, _ = run(2, 29634, "--full", "--steps", "4", "--warmup", "2", env={"BENCH_STANDIN_COMM_FAIL": "1"})
    assert "FALLBACK" in d["config"]["parallelism"] and d["config"]["gathered_frame_equals_single_gpu_render"] is True and d["value"] > 0
    path = d["config"]["multi_gpu_path"]
    assert path[0][0].startswith("library gather") and "could not be set up" in path[0][1] and "torch.distributed" in path[-1][0] and path[-1][1] == "ok"
    # ... GS_BENCH_STRICT=1 refuses instead: a scaling line measured through torch.distributed measures PyTorch, not gs_comm.hip
    e = dict(os.environ)
    e.update({"BENCH_STANDIN_COMM_FAIL": "1", "GS_BENCH_STRICT": "1"})
    e.pop("GS_SPLAT_LIB", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29633", DRIVER, "--gpus", "2", "--steps", "4", "--warmup", "2"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=e, cwd=ROOT)
    assert p.returncode != 0 and not [l for l in p.stdout.splitlines() if l.strip().startswith("{")]
    assert "could not be set up" in p.stderr and "GS_BENCH_STRICT" in p.stderr


def test_feature_ladder_steps_down_when_a_probe_fails():
    # paired gathered frames assemble a WRONG image on this "node" (stand-in): the probe notices before anything is measured, the pairs
    # are switched off, the next rung's probe passes, and the line says which rung it was measured on
    d, _ = run(2, 29637, "--full", "--steps", "4", "--warmup", "2", env={"BENCH_STANDIN_PAIRS_BAD": "1"})
    path = d["config"]["multi_gpu_path"]
    assert path[0][0].startswith("gathered frames paired") and "differs" in path[0][1]
    assert path[-1] == ["gathered frames, one per launch", "ok"]
    assert d["config"]["frames_per_launch"] == 1 and d["config"]["gathered_frame_equals_single_gpu_render"] is True
    d, _ = run(2, 29638, "--steps", "4", "--warmup", "2")
    assert d["config"]["multi_gpu_path"] == [["gathered frames paired (GS_OPT_FRAME_BATCH = 2)", "ok"]] and d["config"]["frames_per_launch"] == 2


def test_first_contact_report_goes_to_stderr():
    # rank 0 prints what a failed scaling run is diagnosed from before anything is timed: devices, peer-access matrix, the pieces
    d, err = run(2, 29636, "--steps", "4", "--warmup", "2")
    assert "[bench] first contact: world 2" in err and "pieces of a mono" in err
