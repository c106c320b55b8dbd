"""
The index arithmetic of the subspace maps (csrc/submap_rank.h on csrc/subspace.h, pm_rank.h and perm_rank.h: the
configuration of a target row, the position and sign of the at most two source amplitudes that enter it, the complement
by mirror or by a second look-up, the bucketed search of an Explicit list) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/submap_rank_check.cpp is a plain C++ program that includes that header -- the very code
the kernel and dnm_subspace_map_indices run; no HIP runtime, no library, nothing loaded into Python.  It walks every
target row of SpinConserve(12, 6) <-> Full(12) with both XParity sectors on either side, of SpinConserve(12, 5) ->
Full(12), Parity(11, odd) <-> Full(11) plain and swizzled, Parity(12, even) <-> SpinConserve(12, 6), an unsorted Explicit
list of 40 states of 10 spins <-> Full(10) with and without its bucket table, the disjoint SpinConserve(10, 3) ->
(10, 4), and one set bit at 63 spins, against subspaces written out as lists and a std::map, with tables of exactly the
size the kernel is handed.  A wrong gather index on the device is a read out of bounds: this runs before any GPU test of
the pass.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_submap_rank_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")      # subspace.h includes the HIP headers
    if not os.path.exists(os.path.join(inc, "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers")
    exe = os.path.join(str(tmp_path), "submap_rank_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-D__HIP_PLATFORM_AMD__", "-I", inc, os.path.join(ROOT, "tests", "submap_rank_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("DNM_")}
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert "0 failure(s)" in run.stdout and "FAILED" not in run.stdout and run.stdout.count(": ok") == 31
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
