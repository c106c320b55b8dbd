"""
The host builder of the SpinConserve passes' tables (csrc/sc3_tables.cpp: the layout, the hops of a bond graph, the
partner tables of both passes, the split diagonal, the two dispatch orders, the blocks a rank reads) under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/sc3_tables_check.cpp is a plain C++ program linked with that one
source -- no HIP runtime, no library, nothing loaded into Python.  It builds the tables of dyadic operators in the (6, 4)
layout as dnm_mat_create does and checks every entry against its definition over all states of the subspace.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sc3_tables_host_builder_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")      # the sources include the HIP headers
    if not os.path.exists(os.path.join(inc, "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers")
    exe = os.path.join(str(tmp_path), "sc3_tables_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-D__HIP_PLATFORM_AMD__", "-I", inc, os.path.join(ROOT, "tests", "sc3_tables_check.cpp"),
           os.path.join(ROOT, "dynamite_amd", "csrc", "sc3_tables.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("DNM_")}
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout, run.stderr)
    # chain12, graph13, graph13 on ranks 0 1 2 of 3, xparity12, complex13, the operator with five Lo sign patterns
    # (cached diagonal), and chain12 / graph13 / xparity12 once more on real vectors; before them the block ranges as
    # places of the block sequence in the (22, 11) and (24, 12) layouts, which have empty blocks
    assert "0 failure(s)" in run.stdout and "FAILED" not in run.stdout and run.stdout.count(": ok") == 13
    assert run.stdout.count("blocks as places: ok") == 2
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
