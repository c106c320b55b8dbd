"""
The host arithmetic of the Krylov drivers (csrc/krylov_host.cpp: dense helpers, tridiagonal eigenpairs, expansion
coefficients, the choices made from a Lanczos probe) against known answers, under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/krylov_host_check.cpp is a plain C++ program linked with that one source -- no HIP,
no library, nothing loaded into Python.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_krylov_host_known_answers_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = os.path.join(str(tmp_path), "krylov_host_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "krylov_host_check.cpp"),
           os.path.join(ROOT, "dynamite_amd", "csrc", "krylov_host.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert "0 failure(s)" in run.stdout and "FAILED" not in run.stdout
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
