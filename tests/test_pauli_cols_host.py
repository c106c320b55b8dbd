"""
The column arithmetic of the two-spin Pauli pass (csrc/pauli_cols.h: the partner mask of a column, the configuration
whose bits it reads -- on a Parity sector the opposite sector's for a flipping column -- and its sign) under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/pauli_cols_check.cpp is a plain C++ program that includes that
header -- the very code the kernel and dnm_pauli_partner_indices run; no HIP runtime, no library, nothing loaded into
Python.  It walks every row and every column of Full(6) and of both sectors of Parity(7), and a handful of rows at 63
and 64 spins with sites 0 and L - 1, against a plain bit-by-bit loop of its own.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pauli_cols_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = os.path.join(str(tmp_path), "pauli_cols_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           os.path.join(ROOT, "tests", "pauli_cols_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("DNM_")}
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert "0 failure(s)" in run.stdout and "FAILED" not in run.stdout and run.stdout.count(": ok") == 9
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
