#!/usr/bin/env python
"""Times the one-pass Pauli moments (csrc/pauli_kernels.hip, csrc/gram_tile.h, csrc/observables.cpp,
backend.pauli_moments, computations.pauli_correlations) against the loop they replace.

pauli_correlations_timing.py [STEP ...]    steps: full26 full30 parity30 (default: all three)

  full26      all 78 columns of Full(L=26)
  full30      all 90 columns of Full(L=30)
  parity30    all 90 columns of Parity('even', L=30)

Every step runs in a process of its own under its own time limit; the first failure ends the run.  The output is
appended to profiles/pauli_correlations.txt as well.  Per shape, on a random state:
  - one call of backend.pauli_moments on the columns of the first pair of chunks of computations._pauli_chunks: warm,
    device-synchronised, median of REPS calls;
  - the MFMA bound of the kernel -- 2 NT + NB^2 MFMAs of 2048 flop per four rows of the operand matrix at MFMA_FLOP_S,
    NB = ceil((n + 1) / 16), NT = NB (NB + 1) / 2 -- and the share of it the call reaches;
  - the bytes per amplitude of the state that the time amounts to at HBM_BYTES_S, beside the 16 (1 + flipped sites) bytes
    per row the panel fill asks of the memory system (one load per row and flipped site, the row's own amplitude once);
  - computations.pauli_correlations(state) as a whole: every call of the kernel and the host arithmetic;
  - in the same process the loop of today, the only route to these correlators without the pass: (sigma^a_i *
    sigma^b_j).expectation(state) with the operator built beforehand and a temporary state at hand.  NPAIRS seeded
    correlators, their mean multiplied by the 9 L (L - 1) / 2 + 3 L correlators of the full set (on Parity the pairs are
    drawn among the operators that keep the sector: both factors flip or neither does).
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"full26": 240, "full30": 480, "parity30": 480}
REPS = 5
NPAIRS = 6
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
    from dynamite_amd import backend, computations
    from dynamite_amd.operators import sigmax, sigmay, sigmaz
    from dynamite_amd.states import State
    from dynamite_amd.subspaces import Parity
    L = sub.L
    st = State(L=L, subspace=sub)
    st.set_random(seed=0, device_rng=True)
    rows = st.vec.rows
    sub_c = sub._to_c()
    every = np.stack([np.repeat(np.arange(L), 3), np.tile([1, 2, 3], L)], axis=1)
    chunks = computations._pauli_chunks(every)
    cols = every[np.concatenate(chunks[:2])]
    n = len(cols)
    nsites = len(set(int(s) for s, k in cols if k != 3))
    tr, pb, _, lds, _ = backend.pauli_moments_plan(sub_c['data'], n)
    print("%r, %d of %d columns in %d chunks: %d rows, layout %d, %d tile rows, panels of 2^%d rows (%d bytes of LDS)"
          % (sub, n, len(every), len(chunks), rows, st.vec.swz, tr, pb, lds), flush=True)
    G = backend.pauli_moments(st.vec, sub_c, cols)        # warm-up: scratch
    assert np.array_equal(G, G.conj().T)
    med, best = median_time(lambda: backend.pauli_moments(st.vec, sub_c, cols), REPS)
    nmfma = 2 * (tr * (tr + 1) // 2) + tr * tr
    t_mfma = rows / 4.0 * nmfma * 2048.0 / MFMA_FLOP_S
    print("  pauli_moments, one call of %d columns (%d flipped sites): median of %d %9.3f ms (best %.3f)"
          % (n, nsites, REPS, med * 1e3, best * 1e3))
    print("  MFMA bound: %d MFMAs per four rows, %.3f ms at %.1f TFLOP/s: the call reaches %.1f %% of it"
          % (nmfma, t_mfma * 1e3, MFMA_FLOP_S / 1e12, 100.0 * t_mfma / med))
    print("  the time amounts to %.0f B per amplitude at %.1f TB/s; the panel fill asks for %d B per amplitude "
          "(%.1f TB/s of loads, caches included)"
          % (med * HBM_BYTES_S / rows, HBM_BYTES_S / 1e12, 16 * (nsites + 1), 16.0 * (nsites + 1) * rows / med / 1e12),
          flush=True)
    one, two = computations.pauli_correlations(st)
    whole, whole_best = median_time(lambda: computations.pauli_correlations(st), 3)
    ncalls = len(chunks) * (len(chunks) - 1) // 2 if len(chunks) > 1 else 1
    print("  pauli_correlations, all %d columns in %d calls: median of 3 %9.3f ms (best %.3f)"
          % (len(every), ncalls, whole * 1e3, whole_best * 1e3), flush=True)
    # the loop of today: seeded correlators at two different sites
    pauli = (sigmax, sigmay, sigmaz)
    rng = np.random.default_rng(0)
    times, worst = [], 0.0
    tmp = None
    while len(times) < NPAIRS:
        a, b = (int(v) for v in rng.integers(3, size=2))
        i, j = (int(v) for v in rng.choice(L, size=2, replace=False))
        if isinstance(sub, Parity) and (a == 2) != (b == 2):
            continue
        op = pauli[a](i) * pauli[b](j)
        op.L = L
        op.add_subspace(sub)
        tmp = op.dot(st, tmp) if tmp is not None else op.dot(st)      # builds the operator's handle; the temporary
        want = op.expectation(st, tmp_state=tmp)
        t, _ = median_time(lambda: op.expectation(st, tmp_state=tmp), 3)
        times.append(t)
        got = two[a, i, b, j]
        worst = max(worst, abs(want - got))
        print("    sigma^%s_%d sigma^%s_%d: %9.3f ms   %.15f / %.15f" % ("xyz"[a], i, "xyz"[b], j, t * 1e3, want, got.real),
              flush=True)
        op.destroy_mat()
    pair = statistics.mean(times)
    ncorr = 9 * L * (L - 1) // 2 + 3 * L
    print("  (sigma^a_i sigma^b_j).expectation, operator built: %9.3f ms per correlator (mean of %d) -> %.2f s for the %d "
          "correlators: %.1f x pauli_correlations" % (pair * 1e3, NPAIRS, pair * ncorr, ncorr, pair * ncorr / whole),
          flush=True)
    if worst > 1e-9:
        raise SystemExit("the two routes disagree by %.3e" % worst)


def step(name):
    from dynamite_amd.subspaces import Full, Parity
    run({"full26": lambda: Full(L=26), "full30": lambda: Full(L=30), "parity30": lambda: Parity('even', L=30)}[name]())


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        from dynamite_amd.config import config
        config._initialize()
        step(sys.argv[2])
        return
    steps = sys.argv[1:] or ["full26", "full30", "parity30"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    log = os.path.join(ROOT, "profiles", "pauli_correlations.txt")
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
