#!/usr/bin/env python
"""Times the one-pass sigma+ sigma- moments (csrc/pm_kernels.hip, csrc/gram_tile.h, csrc/observables.cpp,
backend.pm_moments) against the route they replace.

sigma_pm_correlations_timing.py [STEP ...]    steps: full26 full30 sc32 sc30 sc28 (default: full26 full30 sc32)

Every step runs in a process of its own under its own time limit; the first failure ends the run.  The output is
appended to profiles/sigma_pm_correlations.txt as well.  Per shape, on a random state:
  - one call of backend.pm_moments: warm, device-synchronised, median of REPS calls;
  - the MFMA bound of the kernel -- 2 NT + NB^2 MFMAs of 2048 flop per four rows of the operand matrix at MFMA_FLOP_S,
    NB = ceil(L / 16), NT = NB (NB + 1) / 2 -- and the share of it the call reaches;
  - the bytes per amplitude of the state that the time amounts to at HBM_BYTES_S, beside the 16 L bytes per amplitude
    the panel fill asks of the memory system (half of that for Full / Parity, where rows with a clear bit load nothing);
  - in the same process the route of today: Operator.expectation builds Hermitian operators only, so the pair (i, j)
    costs at least (sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j)).expectation(state) -- the real part alone; the
    imaginary part is a second call -- with the operator built beforehand and a temporary state at hand.  NPAIRS seeded
    pairs, their mean multiplied by L (L - 1) / 2.
A SpinConserve state in the internal layout is converted to reference order inside the call (one extra vector).
"""
import os
import statistics
import subprocess
import sys
import time

os.environ.setdefault("DNM_EXPERIMENTAL", "1")   # tools drive experiment knobs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"full26": 240, "full30": 480, "sc32": 540, "sc30": 420, "sc28": 300}
REPS = 7
NPAIRS = 8
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
    from math import comb
    from dynamite_amd import backend
    from dynamite_amd.operators import sigmax, sigmay
    from dynamite_amd.states import State
    from dynamite_amd.subspaces import SpinConserve
    L = sub.L
    st = State(L=L, subspace=sub)
    st.set_random(seed=0, device_rng=True)
    dim = st.vec.rows
    sub_c = sub._to_c()
    tr, pb, nwg, lds, scratch = backend.pm_moments_plan(_plain(sub_c['data']))
    rows = comb(L, sub.k + 1) if isinstance(sub, SpinConserve) else dim
    print("%r: %d amplitudes, %d rows, layout %d, %d tile rows, panels of 2^%d rows (%d bytes of LDS), %d workgroups, "
          "%.2f MB of partial tiles" % (sub, dim, rows, st.vec.swz, tr, pb, lds, nwg, scratch / 1e6), flush=True)
    P = backend.pm_moments(st.vec, sub_c)                 # warm-up: scratch, tables
    assert np.array_equal(P, P.conj().T)
    med, best = median_time(lambda: backend.pm_moments(st.vec, sub_c), REPS)
    nmfma = 2 * (tr * (tr + 1) // 2) + tr * tr
    t_mfma = rows / 4.0 * nmfma * 2048.0 / MFMA_FLOP_S
    asked = 16.0 * L * (1.0 if isinstance(sub, SpinConserve) else 0.5)
    print("  pm_moments, one call: median of %d %9.3f ms (best %.3f)" % (REPS, med * 1e3, best * 1e3))
    print("  MFMA bound: %d MFMAs per four rows, %.3f ms at %.1f TFLOP/s: the call reaches %.1f %% of it"
          % (nmfma, t_mfma * 1e3, MFMA_FLOP_S / 1e12, 100.0 * t_mfma / med))
    print("  the time amounts to %.0f B per amplitude at %.1f TB/s; the panel fill asks for %.0f B per amplitude "
          "(%.1f TB/s of loads, caches included)"
          % (med * HBM_BYTES_S / dim, HBM_BYTES_S / 1e12, asked * rows / dim, asked * rows / med / 1e12), flush=True)
    # the route of today: seeded pairs, the real part alone
    rng = np.random.default_rng(0)
    times, worst = [], 0.0
    tmp = None
    for _ in range(NPAIRS):
        i, j = sorted(int(v) for v in rng.choice(L, size=2, replace=False))
        op = sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j)
        op.L = L
        op.add_subspace(sub)
        tmp = op.dot(st, tmp) if tmp is not None else op.dot(st)      # builds the operator's handle; the temporary
        want = op.expectation(st, tmp_state=tmp)
        t, _ = median_time(lambda: op.expectation(st, tmp_state=tmp), 3)
        times.append(t)
        worst = max(worst, abs(want - 4.0 * P[i, j].real))
        print("    pair (%2d, %2d): %9.3f ms   %.15f / %.15f" % (i, j, t * 1e3, want, 4.0 * P[i, j].real), flush=True)
        op.destroy_mat()
    pair = statistics.mean(times)
    npairs = L * (L - 1) // 2
    print("  (sigmax sigmax + sigmay sigmay).expectation, operator built: %9.3f ms per pair (mean of %d) -> %.2f s for "
          "the %d pairs: %.1f x the one call" % (pair * 1e3, NPAIRS, pair * npairs, npairs, pair * npairs / med),
          flush=True)
    if worst > 1e-9:
        raise SystemExit("the two routes disagree by %.3e" % worst)


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
         "sc30": lambda: SpinConserve(30, 15), "sc28": lambda: SpinConserve(28, 14)}[name]())


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        from dynamite_amd.config import config
        config._initialize()
        step(sys.argv[2])
        return
    steps = sys.argv[1:] or ["full26", "full30", "sc32"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    log = os.path.join(ROOT, "profiles", "sigma_pm_correlations.txt")
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
