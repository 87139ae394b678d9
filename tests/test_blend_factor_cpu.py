"""CPU tier: the blend's coverage factor on every float (tests/host_check/blend_factor.cpp).

csrc/gs_render.hip turns the coverage value q of a pixel and a list entry into a weight that is 1 where q <= qm and 0 elsewhere; since
GS_BLEND_FACTOR 2 it does so with one fused multiply-add, clamp(q * -1e30 + c), c a per-pixel constant.  The stand-alone program
compiled here finds the one float c that makes this exact, compares the three forms of the weight (compare, two roundings, one
rounding) on all 2^32 bit patterns for a pixel inside the strip and on every value a sum of squares can take for a pixel outside it, and
prints the constant.  This test runs it and holds the literal in gs_render.hip to what it printed."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_check", "blend_factor.cpp")
KERNELS = os.path.join(ROOT, "aframe-gaussian-splatting_amd", "csrc", "gs_render.hip")


def _compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def _defined(text, name):
    m = re.search(r"^#define\s+%s\s+(\S+)" % name, text, re.M)
    assert m, name + " is not defined in gs_render.hip"
    return m.group(1)


def test_one_fma_factor_equals_compare_on_every_float(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "blend_factor")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-pthread", SRC, "-o", exe], check=True, capture_output=True, timeout=120)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "disagreements: 0" in p.stdout and p.stdout.strip().endswith("OK")
    assert "inside: 4294967296 values" in p.stdout
    m = re.search(r"K = (\S+)\s+C_IN = (\S+)\s+C_OUT = (\S+)", p.stdout)
    assert m, p.stdout
    k, c_in, c_out = m.groups()
    text = open(KERNELS).read()
    # the constant, by its hex literal
    assert _defined(text, "GS_BLEND_W_C_IN") == c_in + "f", (_defined(text, "GS_BLEND_W_C_IN"), c_in)
    # K and the outside constant are written in decimal there: the same floats
    assert float.fromhex(k) == float(np.float32(_defined(text, "GS_BLEND_W_K").rstrip("f")))
    assert float(_defined(text, "GS_BLEND_W_C_OUT").rstrip("f")) == float.fromhex(c_out)
    assert re.search(r"^#define GS_BLEND_FACTOR 2\b", text, re.M), "the one-fma factor is not the default form"
