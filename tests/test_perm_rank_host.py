"""
The index arithmetic of the site-permutation pass (csrc/perm_rank.h on csrc/pm_rank.h: the source configuration of a
row under a permutation, built from the row's set bits through the inverse permutation; its colex rank; the complement's
index under XParity; the Full / Parity index; the step to the next configuration) under AddressSanitizer and
UndefinedBehaviorSanitizer: tests/perm_rank_check.cpp is a plain C++ program that includes that header -- the very code
the kernels and dnm_perm_partner_indices run; no HIP runtime, no library, nothing loaded into Python.  It walks every row
and every permutation of a fixed set -- identity, a transposition with site L - 1, the reversal, the shifts by 1 and by
L - 1, a three-cycle through L - 1, two seeded random ones -- of SpinConserve(16, 8) and (34, 2), of the edge sectors of 12
spins, of (12, 6) with its two XParity sectors and of one set bit at 63 and 64 spins, against a loop over all sites and a
plain re-ranking loop of its own, with a binomial table of exactly the size the kernel is handed; then Full(10),
Parity(11) and Parity(12) index by index.  A wrong gather index on the device is a read out of bounds: this runs before
any GPU test of the pass.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_perm_rank_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++")
    exe = os.path.join(str(tmp_path), "perm_rank_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           os.path.join(ROOT, "tests", "perm_rank_check.cpp"), "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("DNM_")}
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert "0 failure(s)" in run.stdout and "FAILED" not in run.stdout and run.stdout.count(": ok") == 12
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
