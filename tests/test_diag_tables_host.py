"""
The host builder of the tiled kernel's records (csrc/passes.cpp with csrc/plan.cpp: generic form, flip-flop form, the
diagonal as tables) under AddressSanitizer and UndefinedBehaviorSanitizer: tests/diag_tables_check.cpp is a plain C++
program linked with those two sources -- no HIP runtime, no library, nothing loaded into Python.  It builds the passes of
three dyadic chains as dnm_mat_create does and checks every row of the tables bit for bit against the diagonal's terms.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_diag_tables_host_builder_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    inc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")      # the sources include the HIP headers
    if not os.path.exists(os.path.join(inc, "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers")
    exe = os.path.join(str(tmp_path), "diag_tables_check")
    csrc = os.path.join(ROOT, "dynamite_amd", "csrc")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-D__HIP_PLATFORM_AMD__", "-I", inc, os.path.join(ROOT, "tests", "diag_tables_check.cpp"),
           os.path.join(csrc, "passes.cpp"), os.path.join(csrc, "plan.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("DNM_")}
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert "0 failure(s)" in run.stdout and "FAILED" not in run.stdout and run.stdout.count(": ok") == 4
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
