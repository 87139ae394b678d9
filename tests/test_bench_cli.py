"""CPU tier: bench.py's command line (the driver's contract: --gpus N --steps K --warmup W) and its refusal to run
without a GPU -- the product path has no CPU fallback, so the benchmark must fail loudly instead of measuring one."""
import os
import subprocess
import sys

from conftest import ROOT


def test_bench_help_lists_the_contract_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert flag in r.stdout


def test_bench_fails_loudly_without_a_gpu():
    if os.path.exists("/dev/kfd"):
        import pytest
        pytest.skip("a GPU is present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "0", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert r.stdout.strip() == ""                                  # no JSON line: nothing was measured
    assert "no CPU fallback" in r.stderr or "HIP" in r.stderr


def test_dumped_outputs_are_float32_and_within_the_budget(tmp_path):
    """--dump-outputs: an array that fits is written whole in float32; a 4K RGBA frame (132 MB in float32) becomes a fixed, seeded
    sample of its rows with the row indices beside it, and everything written stays within 64 MB"""
    import importlib
    import numpy as np
    bench = importlib.import_module("bench")
    rng = np.random.default_rng(7)
    small = rng.integers(0, 256, (1080, 1920, 4), dtype=np.uint8)
    big = rng.integers(0, 256, (2160, 3840, 4), dtype=np.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"frame": small})
        bench.dump_outputs(str(tmp_path / d / "big"), {"frame": big})
    got = np.load(tmp_path / "a" / "frame.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.astype(np.float32))
    rows = np.load(tmp_path / "a" / "big" / "frame_rows.npy")
    sample = np.load(tmp_path / "a" / "big" / "frame.npy")
    assert sample.dtype == np.float32 and sample.shape == (rows.size, 3840, 4) and 0 < rows.size < 2160
    assert np.array_equal(sample, big[rows.astype(np.int64)].astype(np.float32))
    assert np.array_equal(rows, np.load(tmp_path / "b" / "big" / "frame_rows.npy"))           # the same sample every run
    total = sum(os.path.getsize(tmp_path / "a" / "big" / f) for f in os.listdir(tmp_path / "a" / "big"))
    assert total <= 64_000_000
