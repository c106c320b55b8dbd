#!/usr/bin/env python
"""Times the one-pass sigma-z moments (csrc/zz_kernels.hip, csrc/gram_tile.h, backend.zz_moments) against the route
they replace.

sigmaz_correlations_timing.py [STEP ...]    steps: full26 full30 sc32 sc30 (default: the first three; sc30 is the
                                            two-tile-row SpinConserve instance, L = 16 ... 31)

Every step runs in a process of its own under its own time limit; the first failure ends the run.  The output is
appended to profiles/sigmaz_correlations.txt as well.  Per shape, on a random state:
  - one call of backend.zz_moments: warm, device-synchronised, median of REPS calls, and the bytes/s of the state it
    streams (16 B per amplitude);
  - the two bounds of the kernel -- the read at HBM_BYTES_S and nb (nb + 1) / 2 MFMAs of 2048 flop per four amplitudes
    at MFMA_FLOP_S, nb = ceil((L + 1) / 16) -- which of them binds and the share of it the call reaches;
  - in the same process the route of today: (sigmaz(i) * sigmaz(j)).expectation(state) with the operator built
    beforehand and a temporary state at hand, per pair, and that time multiplied by L (L + 1) / 2.
A SpinConserve state in the internal layout is converted to reference order inside the call (one extra vector): the
sweep alone, on the converted vector, is timed beside it.
"""
import os
import statistics
import subprocess
import sys
import time

os.environ.setdefault("DNM_EXPERIMENTAL", "1")   # tools drive experiment knobs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"full26": 240, "full30": 420, "sc32": 480, "sc30": 480}
REPS = 11
HBM_BYTES_S = 8.0e12        # MI355X: HBM3E peak
MFMA_FLOP_S = 78.6e12       # MI355X: fp64 matrix peak


def median_time(fn, reps):
    import torch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts)


def run(sub):
    import numpy as np
    from dynamite_amd import backend
    from dynamite_amd.operators import sigmaz
    from dynamite_amd.states import State
    L = sub.L
    st = State(L=L, subspace=sub)
    st.set_random(seed=0, device_rng=True)
    rows = st.vec.rows
    sub_c = sub._to_c()
    tr, nwg, scratch = backend.zz_moments_plan(_plain(sub_c['data']), rows)
    print("%r: %d rows, layout %d, %d tile rows, %d workgroups, %.2f MB of partial tiles"
          % (sub, rows, st.vec.swz, tr, nwg, scratch / 1e6), flush=True)
    M = backend.zz_moments(st.vec, sub_c)                 # warm-up: scratch, tables
    assert np.array_equal(M, M.T) and abs(M[0, 0] - 1.0) < 1e-9
    med, best = median_time(lambda: backend.zz_moments(st.vec, sub_c), REPS)
    t_mem = 16.0 * rows / HBM_BYTES_S
    t_mfma = rows / 4.0 * (tr * (tr + 1) // 2) * 2048.0 / MFMA_FLOP_S
    bound, which = max((t_mem, "HBM read"), (t_mfma, "fp64 MFMA"))
    print("  zz_moments, one call: median of %d %9.3f ms (best %.3f)   %6.2f TB/s of state" % (REPS, med * 1e3, best * 1e3,
                                                                                             16.0 * rows / med / 1e12))
    print("  bounds: read %.3f ms at %.1f TB/s, MFMA %.3f ms at %.1f TFLOP/s -> %s binds; the call reaches %.1f %% of it"
          % (t_mem * 1e3, HBM_BYTES_S / 1e12, t_mfma * 1e3, MFMA_FLOP_S / 1e12, which, 100.0 * bound / med), flush=True)
    if st.vec.internal:
        x = st.vec.local_natural()
        plain = _plain(sub_c['data'])
        backend.zz_moments_block(x, plain, 0, rows)
        med2, best2 = median_time(lambda: backend.zz_moments_block(x, plain, 0, rows), REPS)
        print("  the sweep alone, on the state in reference order: median %9.3f ms (best %.3f), %.1f %% of the bound"
              % (med2 * 1e3, best2 * 1e3, 100.0 * bound / med2))
        del x
    # the route of today, one pair
    i, j = 0, L // 2
    op = sigmaz(i) * sigmaz(j)
    op.L = L
    op.add_subspace(sub)
    tmp = op.dot(st)                                       # builds the operator's handle; the temporary vector
    want = op.expectation(st, tmp_state=tmp)
    pair, _ = median_time(lambda: op.expectation(st, tmp_state=tmp), 5)
    npairs = L * (L + 1) // 2
    print("  (sigmaz(%d) * sigmaz(%d)).expectation, operator built: %9.3f ms per pair -> %.2f s for the %d moments "
          "(%.0f x the one call); values %.15f / %.15f"
          % (i, j, pair * 1e3, pair * npairs, npairs, pair * npairs / med, want, M[1 + i, 1 + j]), flush=True)
    if abs(want - M[1 + i, 1 + j]) > 1e-9:
        raise SystemExit("the two routes disagree")


def _plain(sub_c):
    """The descriptor for a state in reference order."""
    from dynamite_amd import _lib
    if int(sub_c.vec_swizzle) < 256:
        return sub_c
    d = _lib.Subspace.from_buffer_copy(sub_c)
    d.vec_swizzle = 0
    d.site_perm = None
    d._keep = sub_c
    return d


def step(name):
    from dynamite_amd.subspaces import Full, SpinConserve
    run({"full26": lambda: Full(L=26), "full30": lambda: Full(L=30), "sc32": lambda: SpinConserve(32, 16),
         "sc30": lambda: SpinConserve(30, 15)}[name]())


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        from dynamite_amd.config import config
        config._initialize()
        step(sys.argv[2])
        return
    steps = sys.argv[1:] or ["full26", "full30", "sc32"]
    log = os.path.join(ROOT, "profiles", "sigmaz_correlations.txt")
    for s in steps:
        cmd = ["timeout", "-k", "10", str(LIMITS[s]), sys.executable, os.path.abspath(__file__), "--step", s]
        with open(log, "a") as f, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                                   text=True) as p:
            def emit(line):
                sys.stdout.write(line)
                sys.stdout.flush()
                f.write(line)
            emit("== step %s ==\n" % s)
            for line in iter(p.stdout.readline, ""):
                emit(line)
            emit("== step %s: exit status %d ==\n\n" % (s, p.wait()))
        if p.returncode != 0:
            sys.exit(p.returncode)       # nothing more is started on the device after a failure
    return


if __name__ == "__main__":
    main()
