#!/usr/bin/env python
"""Times the one-pass Gram matrix of many states (csrc/vgram_kernels.hip, csrc/gram_tile.h, csrc/observables.cpp,
backend.vec_gram, computations.overlap_matrix) against the two routes that exist without it.

state_gram_timing.py [STEP ...]    steps: full26_16 full26_32 full26_64 sc30_16 sc30_32 sc30_64 (default: all six)

  full26_N    N random states on Full(L=26)
  sc30_N      N random states on SpinConserve(30, 15)

Every step runs in a process of its own under its own time limit; the first failure ends the run.  The output is
appended to profiles/state_gram.txt as well.  Per shape the states are the rows of one contiguous basis, so that the
strided route needs no second copy of them (at 64 states of SpinConserve(30, 15) there is no room for one); the Gram
pass is handed their separate addresses and knows nothing of that.  Per shape:
  - one computations.overlap_matrix(states): warm, device-synchronised, median of REPS calls;
  - the rows per second of that call as a share of the MFMA bound of the kernel -- 2 NT + NB^2 MFMAs of 2048 flop per
    four rows at MFMA_FLOP_S, NB = ceil(N / 16), NT = NB (NB + 1) / 2 -- and its bytes per second, 16 N bytes per row
    read once, as a share of COPY_BYTES_S, the rate a copy reaches on this chip;
  - the loop of State.dot over all N^2 ordered pairs, one launch and one host synchronisation each: timed once;
  - N calls of dnm_vec_mdot on the contiguous basis, one per column of the matrix, each against all N vectors: median
    of REPS; the time of making a contiguous copy, which states of separate allocations would need first, is not in it.
The three routes are compared on their results as well (the largest difference is printed).
"""
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = {"full26": 240, "sc30": 600}       # time limit of a step, seconds
COUNTS = (16, 32, 64)
REPS = 5
MFMA_FLOP_S = 78.6e12       # MI355X: fp64 matrix peak
COPY_BYTES_S = 6.3e12       # what a copy reaches on this chip


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


def run(sub, nvec):
    import numpy as np
    import torch
    from dynamite_amd import _lib, backend, computations
    from dynamite_amd.backend import Vec, _stream
    from dynamite_amd.states import State
    probe = State(L=sub.L, subspace=sub).vec
    n, swz, sub_c = probe.alloc_size, probe.swz, probe.sub_c
    del probe
    basis = torch.zeros((nvec, n), dtype=torch.complex128, device="cuda")
    states = []
    for c in range(nvec):
        st = State(L=sub.L, subspace=sub)
        st._vec = Vec(sub.get_dimension(), array=basis[c], swz=swz, sub_c=sub_c)
        st.set_random(seed=c, device_rng=True)
        states.append(st)
    tr, pb, nwg, lds, _ = backend.vec_gram_plan(nvec, n)
    print("%r, %d states of %d elements (%d rows, layout %d; %.1f GB): %d tile rows, panels of 2^%d rows (%d bytes of "
          "LDS), %d workgroups" % (sub, nvec, n, states[0].vec.rows, swz, 16e-9 * n * nvec, tr, pb, lds, nwg),
          flush=True)
    S = computations.overlap_matrix(states)       # warm-up: scratch
    assert np.array_equal(S, S.conj().T)
    med, best = median_time(lambda: computations.overlap_matrix(states), REPS)
    nmfma = 2 * (tr * (tr + 1) // 2) + tr * tr
    t_mfma = n / 4.0 * nmfma * 2048.0 / MFMA_FLOP_S
    nbytes = 16.0 * n * nvec
    print("  overlap_matrix, one call: median of %d %9.3f ms (best %.3f)" % (REPS, med * 1e3, best * 1e3))
    print("  %.3f G rows/s; MFMA bound: %d MFMAs per four rows, %.3f ms at %.1f TFLOP/s: the call reaches %.1f %% of it"
          % (n / med / 1e9, nmfma, t_mfma * 1e3, MFMA_FLOP_S / 1e12, 100.0 * t_mfma / med))
    print("  %.3f TB/s of vector data read once: %.1f %% of the %.1f TB/s of a copy"
          % (nbytes / med / 1e12, 100.0 * nbytes / med / COPY_BYTES_S, COPY_BYTES_S / 1e12), flush=True)

    # the loop of State.dot: S[a, b] = <a|b> = b.dot(a) (VecDot conjugates its second argument)
    def dot_loop():
        return np.array([[states[b].dot(states[a]) for b in range(nvec)] for a in range(nvec)])
    dot_loop_warm = states[1].dot(states[0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    D = dot_loop()
    torch.cuda.synchronize()
    t_dot = time.perf_counter() - t0
    print("  State.dot over all %d pairs: %9.3f ms (once; %.3f ms per pair): %.1f x overlap_matrix"
          % (nvec * nvec, t_dot * 1e3, t_dot * 1e3 / nvec ** 2, t_dot / med), flush=True)

    # dnm_vec_mdot on the contiguous basis: h[j] = V_j^H w, column c of the matrix from w = vector c
    H = np.empty((nvec, nvec), dtype=np.complex128)

    def mdot_all():
        for c in range(nvec):
            col = np.empty(nvec, dtype=np.complex128)
            _lib.check(_lib.lib().dnm_vec_mdot(C.c_void_p(basis.data_ptr()), n, nvec, C.c_void_p(basis[c].data_ptr()),
                                               n, col.view(np.float64).ctypes.data_as(C.POINTER(C.c_double)),
                                               _stream()))
            H[:, c] = col
    mdot_all()
    t_mdot, mdot_best = median_time(mdot_all, REPS)
    print("  %d calls of dnm_vec_mdot on the contiguous basis: median of %d %9.3f ms (best %.3f): %.1f x overlap_matrix"
          % (nvec, REPS, t_mdot * 1e3, mdot_best * 1e3, t_mdot / med), flush=True)
    worst = max(np.abs(D - S).max(), np.abs(H - S).max())
    print("  largest difference between the routes: %.3e (first pair by State.dot: %r)" % (worst, dot_loop_warm))
    if worst > 1e-9:
        raise SystemExit("the routes disagree by %.3e" % worst)


def step(name):
    from dynamite_amd.subspaces import Full, SpinConserve
    shape, nvec = name.split("_")
    run({"full26": lambda: Full(L=26), "sc30": lambda: SpinConserve(30, 15)}[shape](), int(nvec))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        from dynamite_amd.config import config
        config._initialize()
        step(sys.argv[2])
        return
    steps = sys.argv[1:] or ["%s_%d" % (s, c) for s in SHAPES for c in COUNTS]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    log = os.path.join(ROOT, "profiles", "state_gram.txt")
    for s in steps:
        cmd = ["timeout", "-k", "10", str(SHAPES[s.split("_")[0]]), sys.executable, os.path.abspath(__file__),
               "--step", s]
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
