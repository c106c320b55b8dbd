#!/usr/bin/env python
"""Times the one-pass scalar-chirality moments (csrc/cyc_kernels.hip, csrc/cyc_rank.h, csrc/gram_tile.h,
csrc/observables.cpp, backend.cyc_moments) against the loop they replace.

chirality_correlations_timing.py [STEP ...]    steps: kagome30 kagome30x full26 full30 (default: all four)

  kagome30    the 20 triangles of lattices.kagome_triangles('30') on SpinConserve(30, 15)
  kagome30x   the same triangles on XParity(SpinConserve(30, 15), '+'), the subspace benchmarking/run_kagome.py solves in
  full26      the 24 triangles (i, i + 1, i + 2) of the open chain on Full(L=26)
  full30      the 28 triangles (i, i + 1, i + 2) of the open chain on Full(L=30)

Every step runs in a process of its own under its own time limit; the first failure ends the run.  The output is
appended to profiles/chirality_correlations.txt as well.  Per shape, on a random state:
  - one call of backend.cyc_moments on both senses of every triangle (2 n columns beside the state's own, what
    computations.chirality_correlations asks for): warm, device-synchronised, median of REPS calls (a SpinConserve state
    in the internal layout is converted to reference order inside the call: one extra vector, counted);
  - the MFMA bound of the kernel -- 2 NT + NB^2 MFMAs of 2048 flop per four rows of the operand matrix at MFMA_FLOP_S,
    NB = ceil((2 n + 1) / 16), NT = NB (NB + 1) / 2 -- and the share of it the call reaches;
  - the bytes per amplitude of the state that the time amounts to at HBM_BYTES_S, beside the 16 (2 n + 1) bytes per row
    the panel fill asks of the memory system at the most (rows whose three bits are equal reuse the row's own amplitude);
  - in the same process the loop of today: (X_t * X_t').expectation(state) with X = sigma_a . (sigma_b x sigma_c), six
    three-body terms, taken in its Hermitian part (X_t X_t' + X_t' X_t) / 2 -- Operator.expectation builds Hermitian
    operators only; for triangles that share one or two sites the other part is a second call -- with the operator
    built beforehand and a temporary state at hand.  NPAIRS seeded pairs of triangles, their mean multiplied by the
    n (n + 1) / 2 pairs.
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


def chi_op(a, b, c):
    from dynamite_amd.operators import op_sum, sigmax, sigmay, sigmaz
    s = (sigmax, sigmay, sigmaz)
    even, odd = ((0, 1, 2), (1, 2, 0), (2, 0, 1)), ((0, 2, 1), (2, 1, 0), (1, 0, 2))
    return op_sum([s[i](a) * s[j](b) * s[k](c) for i, j, k in even] + [-1 * s[i](a) * s[j](b) * s[k](c) for i, j, k in odd])


def run(sub, triangles):
    import numpy as np
    from dynamite_amd import backend, _lib
    from dynamite_amd.states import State
    from dynamite_amd.subspaces import XParity
    L, n = sub.L, len(triangles)
    cycles = [c for a, b, c3 in triangles for c in ((a, b, c3), (a, c3, b))]
    sector = int(sub.sector) if isinstance(sub, XParity) else 0
    st = State(L=L, subspace=sub)
    st.set_random(seed=0, device_rng=True)
    rows = st.vec.rows
    sub_c = sub._to_c()
    plain = _lib.Subspace.from_buffer_copy(sub_c['data'])
    if int(plain.vec_swizzle) >= 256:        # the descriptor of the state in reference order
        plain.vec_swizzle = 0
        plain.site_perm = None
    tr, pb, _, lds, _ = backend.cyc_moments_plan(plain, 2 * n)
    print("%r, %d triangles (%d columns): %d rows, layout %d, %d tile rows, panels of 2^%d rows (%d bytes of LDS)"
          % (sub, n, 2 * n + 1, rows, st.vec.swz, tr, pb, lds), flush=True)
    G = backend.cyc_moments(st.vec, sub_c, cycles, sector)        # warm-up: scratch, tables
    assert np.array_equal(G, G.conj().T)
    med, best = median_time(lambda: backend.cyc_moments(st.vec, sub_c, cycles, sector), REPS)
    nmfma = 2 * (tr * (tr + 1) // 2) + tr * tr
    t_mfma = rows / 4.0 * nmfma * 2048.0 / MFMA_FLOP_S
    print("  cyc_moments, one call: median of %d %9.3f ms (best %.3f)" % (REPS, med * 1e3, best * 1e3))
    print("  MFMA bound: %d MFMAs per four rows, %.3f ms at %.1f TFLOP/s: the call reaches %.1f %% of it"
          % (nmfma, t_mfma * 1e3, MFMA_FLOP_S / 1e12, 100.0 * t_mfma / med))
    print("  the time amounts to %.0f B per amplitude at %.1f TB/s; the panel fill asks for at most %d B per amplitude "
          "(%.1f TB/s of loads, caches included)"
          % (med * HBM_BYTES_S / rows, HBM_BYTES_S / 1e12, 16 * (2 * n + 1), 16.0 * (2 * n + 1) * rows / med / 1e12),
          flush=True)
    # the loop of today: seeded pairs of triangles, the Hermitian part of the product
    rng = np.random.default_rng(0)
    times, worst = [], 0.0
    tmp = None
    for _ in range(NPAIRS):
        t1, t2 = (int(v) for v in rng.choice(n, size=2, replace=False))
        X, Y = chi_op(*triangles[t1]), chi_op(*triangles[t2])
        op = 0.5 * (X * Y + Y * X)
        op.L = L
        op.add_subspace(sub)
        tmp = op.dot(st, tmp) if tmp is not None else op.dot(st)      # builds the operator's handle; the temporary
        want = op.expectation(st, tmp_state=tmp)
        t, _ = median_time(lambda: op.expectation(st, tmp_state=tmp), 3)
        times.append(t)
        f1, b1, f2, b2 = 1 + 2 * t1, 2 + 2 * t1, 1 + 2 * t2, 2 + 2 * t2
        got = (4.0 * ((G[f1, f2] + G[b1, b2]) - (G[f1, b2] + G[b1, f2]))).real
        worst = max(worst, abs(want - got))
        print("    triangles %r %r: %9.3f ms   %.15f / %.15f" % (tuple(triangles[t1]), tuple(triangles[t2]), t * 1e3,
                                                                want, got), flush=True)
        op.destroy_mat()
    pair = statistics.mean(times)
    npairs = n * (n + 1) // 2
    print("  (X_t X_t' + X_t' X_t).expectation / 2, operator built: %9.3f ms per pair (mean of %d) -> %.2f s for the %d "
          "pairs: %.1f x the one call" % (pair * 1e3, NPAIRS, pair * npairs, npairs, pair * npairs / med), flush=True)
    if worst > 1e-9:
        raise SystemExit("the two routes disagree by %.3e" % worst)


def step(name):
    from dynamite_amd import lattices
    from dynamite_amd.subspaces import Full, SpinConserve, XParity
    if name in ("kagome30", "kagome30x"):
        triangles = lattices.kagome_triangles('30')
        assert len(triangles) == 20
        sub = SpinConserve(30, 15)
        run(XParity(sub, sector='+') if name == "kagome30x" else sub, triangles)
    else:
        L = {"full26": 26, "full30": 30}[name]
        run(Full(L=L), [(i, i + 1, i + 2) for i in range(L - 2)])


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        from dynamite_amd.config import config
        config._initialize()
        step(sys.argv[2])
        return
    steps = sys.argv[1:] or ["kagome30", "kagome30x", "full26", "full30"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    log = os.path.join(ROOT, "profiles", "chirality_correlations.txt")
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
