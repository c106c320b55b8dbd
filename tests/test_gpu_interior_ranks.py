"""The interior solver between rank PROCESSES: two ranks of a row-block partition (tests/interior_ranks_child.py, ctypes
alone, stand-in transport tests/fake_rccl) call dnm_eigsolve_interior through dnm_comm_hooks.  Reference: dense
diagonalisation on the host."""
import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

from dynamite_amd.subspaces import SpinConserve
from gpu_util import marshal
from test_gpu_interior import EPS, TOL, check_values, dense, heisenberg, nearest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_RCCL = os.path.join(ROOT, "tests", "fake_rccl", "libfake_rccl.so")


def fake_rccl():
    src = os.path.join(ROOT, "tests", "fake_rccl", "fake_rccl.cpp")
    if not os.path.exists(FAKE_RCCL) or os.path.getmtime(FAKE_RCCL) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-fPIC", "-shared", "-o", FAKE_RCCL, src])
    return FAKE_RCCL


def test_two_rank_processes(tmp_path):
    """Random-field Heisenberg chain, SpinConserve(12,6) split over 2 ranks (462 rows each, column windows), nev = 10
    at mid-band: (i) all nev nearest reference values within tol |H|_inf + n eps |H|_inf, (ii) ordered by
    |theta - sigma|; every rank returns the same numbers bit for bit; and the residuals and norms the ranks measured
    themselves with the partitioned multiply."""
    world, L, nev = 2, 12, 10
    H = heisenberg(L)
    sub = SpinConserve(L, L // 2)
    H.subspace = sub
    _, nrm, w, _ = dense(H, False)
    sigma = round(float(w[0] + 0.5 * (w[-1] - w[0])), 3)
    nearest(w, sigma, nev)                                   # the condition on the input
    masks, offs, signs, coeffs = marshal(H)
    fn = os.path.join(str(tmp_path), "case.npz")
    np.savez(fn, masks=masks, mask_offsets=offs, signs=signs, coeffs=coeffs, L=L, k=L // 2, nck=sub._nchoosek,
             dim=sub.get_dimension(), nev=nev, nev_max=2 * nev, sigma=sigma, tol=TOL)
    env = dict(os.environ, DNM_RCCL_LIB=fake_rccl(), DNM_FAKE_RCCL_TIMEOUT_S="300")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    idfile = os.path.join(str(tmp_path), "comm_id")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "interior_ranks_child.py"), fn, str(r),
                               str(world), idfile, os.path.join(str(tmp_path), "rep%d.json" % r)], env=env, cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
             for r in range(world)]
    errs = []
    try:
        for p in procs:
            errs.append(p.communicate(timeout=300)[1])
    finally:
        for p in procs:
            if p.poll() is None:
                os.killpg(p.pid, signal.SIGKILL)
    assert [p.returncode for p in procs] == [0] * world, "\n".join(e[-1500:] for e in errs)
    reps = [json.load(open(os.path.join(str(tmp_path), "rep%d.json" % r))) for r in range(world)]
    print(json.dumps(reps[0]))
    assert sum(r["nloc"] for r in reps) == sub.get_dimension()
    for r in reps:
        assert r["reason"] == 1 and r["nconv"] >= nev and r["matvecs"] > 0
        assert r["evals"] == reps[0]["evals"] and r["residuals"] == reps[0]["residuals"]
        check_values(r["evals"], w, sigma, nev, nrm)
        assert r["err_est"] <= TOL
        assert max(r["residuals"]) <= TOL * nrm + 100 * EPS * nrm
        assert max(abs(n - 1.0) for n in r["norms"]) <= 100 * r["nconv"] * EPS
