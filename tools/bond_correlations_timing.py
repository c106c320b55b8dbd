#!/usr/bin/env python
"""Times the one-pass bond-swap moments (csrc/swap_kernels.hip, csrc/gram_tile.h, csrc/observables.cpp,
backend.swap_moments) against the loop they replace.

bond_correlations_timing.py [STEP ...]    steps: kagome30 kagome30x full26 full30 (default: all four)

  kagome30    the 60 bonds of lattices.kagome('30') on SpinConserve(30, 15)
  kagome30x   the same bonds on XParity(SpinConserve(30, 15), '+'), the subspace benchmarking/run_kagome.py solves in
  full26      the 25 bonds of the open chain on Full(L=26)
  full30      the 29 bonds of the open chain on Full(L=30)

Every step runs in a process of its own under its own time limit; the first failure ends the run.  The output is
appended to profiles/bond_correlations.txt as well.  Per shape, on a random state:
  - one call of backend.swap_moments: warm, device-synchronised, median of REPS calls (a SpinConserve state in the
    internal layout is converted to reference order inside the call: one extra vector, counted);
  - the MFMA bound of the kernel -- 2 NT + NB^2 MFMAs of 2048 flop per four rows of the operand matrix at MFMA_FLOP_S,
    NB = ceil((n + 1) / 16), NT = NB (NB + 1) / 2 -- and the share of it the call reaches;
  - the bytes per amplitude of the state that the time amounts to at HBM_BYTES_S, beside the 16 (n + 1) bytes per row the
    panel fill asks of the memory system at the most (rows whose two bits are equal reuse the row's own amplitude);
  - in the same process the loop of today: (B_m * B_m').expectation(state) with B = sigma . sigma, taken in its Hermitian
    part (B_m B_m' + B_m' B_m) / 2 -- Operator.expectation builds Hermitian operators only; for bonds that share a site
    the other part is a second call -- with the operator built beforehand and a temporary state at hand.  NPAIRS seeded
    pairs of bonds, their mean multiplied by the n (n + 1) / 2 pairs.
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"kagome30": 300, "kagome30x": 300, "full26": 240, "full30": 480}
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


def heis(a, b):
    from dynamite_amd.operators import sigmax, sigmay, sigmaz
    return sigmax(a) * sigmax(b) + sigmay(a) * sigmay(b) + sigmaz(a) * sigmaz(b)


def run(sub, bonds):
    import numpy as np
    from dynamite_amd import backend, _lib
    from dynamite_amd.states import State
    from dynamite_amd.subspaces import XParity
    L, n = sub.L, len(bonds)
    sector = int(sub.sector) if isinstance(sub, XParity) else 0
    st = State(L=L, subspace=sub)
    st.set_random(seed=0, device_rng=True)
    rows = st.vec.rows
    sub_c = sub._to_c()
    plain = _lib.Subspace.from_buffer_copy(sub_c['data'])
    if int(plain.vec_swizzle) >= 256:        # the descriptor of the state in reference order
        plain.vec_swizzle = 0
        plain.site_perm = None
    tr, pb, _, lds, _ = backend.swap_moments_plan(plain, n)
    print("%r, %d bonds: %d rows, layout %d, %d tile rows, panels of 2^%d rows (%d bytes of LDS)"
          % (sub, n, rows, st.vec.swz, tr, pb, lds), flush=True)
    G = backend.swap_moments(st.vec, sub_c, bonds, sector)        # warm-up: scratch, tables
    assert np.array_equal(G, G.conj().T)
    med, best = median_time(lambda: backend.swap_moments(st.vec, sub_c, bonds, sector), REPS)
    nmfma = 2 * (tr * (tr + 1) // 2) + tr * tr
    t_mfma = rows / 4.0 * nmfma * 2048.0 / MFMA_FLOP_S
    print("  swap_moments, one call: median of %d %9.3f ms (best %.3f)" % (REPS, med * 1e3, best * 1e3))
    print("  MFMA bound: %d MFMAs per four rows, %.3f ms at %.1f TFLOP/s: the call reaches %.1f %% of it"
          % (nmfma, t_mfma * 1e3, MFMA_FLOP_S / 1e12, 100.0 * t_mfma / med))
    print("  the time amounts to %.0f B per amplitude at %.1f TB/s; the panel fill asks for at most %d B per amplitude "
          "(%.1f TB/s of loads, caches included)"
          % (med * HBM_BYTES_S / rows, HBM_BYTES_S / 1e12, 16 * (n + 1), 16.0 * (n + 1) * rows / med / 1e12), flush=True)
    # the loop of today: seeded pairs of bonds, the Hermitian part of the product
    rng = np.random.default_rng(0)
    times, worst = [], 0.0
    tmp = None
    for _ in range(NPAIRS):
        m, m2 = (int(v) for v in rng.choice(n, size=2, replace=False))
        Bm, Bm2 = heis(*bonds[m]), heis(*bonds[m2])
        op = 0.5 * (Bm * Bm2 + Bm2 * Bm)
        op.L = L
        op.add_subspace(sub)
        tmp = op.dot(st, tmp) if tmp is not None else op.dot(st)      # builds the operator's handle; the temporary
        want = op.expectation(st, tmp_state=tmp)
        t, _ = median_time(lambda: op.expectation(st, tmp_state=tmp), 3)
        times.append(t)
        got = (4.0 * G[1 + m, 1 + m2] - 2.0 * (G[1 + m, 0] + G[0, 1 + m2]) + G[0, 0]).real
        worst = max(worst, abs(want - got))
        print("    bonds %r %r: %9.3f ms   %.15f / %.15f" % (tuple(bonds[m]), tuple(bonds[m2]), t * 1e3, want, got),
              flush=True)
        op.destroy_mat()
    pair = statistics.mean(times)
    npairs = n * (n + 1) // 2
    print("  (B_m B_m' + B_m' B_m).expectation / 2, operator built: %9.3f ms per pair (mean of %d) -> %.2f s for the %d "
          "pairs: %.1f x the one call" % (pair * 1e3, NPAIRS, pair * npairs, npairs, pair * npairs / med), flush=True)
    if worst > 1e-9:
        raise SystemExit("the two routes disagree by %.3e" % worst)


def step(name):
    from dynamite_amd import lattices
    from dynamite_amd.subspaces import Full, SpinConserve, XParity
    if name in ("kagome30", "kagome30x"):
        nsites, bonds = lattices.kagome('30')
        assert nsites == 30 and len(bonds) == 60
        sub = SpinConserve(30, 15)
        run(XParity(sub, sector='+') if name == "kagome30x" else sub, bonds)
    else:
        L = {"full26": 26, "full30": 30}[name]
        run(Full(L=L), lattices.chain(L)[1])


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        from dynamite_amd.config import config
        config._initialize()
        step(sys.argv[2])
        return
    steps = sys.argv[1:] or ["kagome30", "kagome30x", "full26", "full30"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    log = os.path.join(ROOT, "profiles", "bond_correlations.txt")
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
