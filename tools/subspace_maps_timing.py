#!/usr/bin/env python
"""Times the subspace maps and the sector weights (csrc/submap_kernels.hip, csrc/submap_rank.h, csrc/observables.cpp,
backend.subspace_map, backend.sector_weights) beside the floor they can be held against and the host routes they
replace.

subspace_maps_timing.py [STEP ...]    steps: sc30 xsc30 full26 host26 (default: all four)

  sc30      SpinConserve(30, 15) <-> Full(30): to_subspace both ways, sector_weights of both states
  xsc30     XParity(SpinConserve(30, 15), '+') <-> its parent: to_subspace both ways, sector_weights of both states
  full26    Full(26) <-> Parity(26, even): to_subspace both ways, sector_weights of both states
  host26    at 26 spins, the host routes: XParity.convert_state for XParity(Full(26), '+') <-> Full(26), and State.to_numpy,
            a scatter in numpy and the upload for SpinConserve(26, 13) -> Full(26), each beside to_subspace

Every step runs in a process of its own under its own time limit; the first failure ends the run.  The output is
appended to profiles/subspace_maps.txt as well.  Per shape, on a random state, warm, device-synchronised, median of REPS
calls (a SpinConserve state in the internal layout is converted to reference order inside the call, and a result in that
layout brought home: the extra passes are counted; where a side is in that layout the two directions are timed once more
with both vectors in reference order, the kernel alone):
  - each call beside dnm_vec_copy (Vec.copy) of the larger of the two vectors, the floor of one read and one write of it;
  - the bytes per amplitude of the larger vector that the time amounts to at HBM_BYTES_S.
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"sc30": 420, "xsc30": 300, "full26": 240, "host26": 420}
REPS = 7
HBM_BYTES_S = 8.0e12        # MI355X: HBM3E peak


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


def report(what, med, best, floor, rows):
    print("  %-52s median of %d %9.3f ms (best %.3f): %.2f x dnm_vec_copy, %.0f B per amplitude at %.1f TB/s"
          % (what, REPS, med * 1e3, best * 1e3, med / floor, med * HBM_BYTES_S / rows, HBM_BYTES_S / 1e12), flush=True)


def random_state(sub, seed):
    from dynamite_amd.states import State
    st = State(L=sub.L, subspace=sub)
    st.set_random(seed=seed, device_rng=True)
    return st


def pair(small_sub, large_sub):
    """Both directions between a subspace and one that holds it, and the sector weights of both states."""
    from dynamite_amd import backend, computations
    from dynamite_amd.states import State
    small = random_state(small_sub, 0)
    large = State(L=large_sub.L, subspace=large_sub)
    rows = large.vec.rows
    print("%r (%d rows, layout %d) <-> %r (%d rows, layout %d)" % (small_sub, small.vec.rows, small.vec.swz, large_sub,
                                                                   rows, large.vec.swz), flush=True)
    computations.to_subspace(small, large_sub, result=large)        # warm-up: tables, scratch
    tmp = large.copy()
    copy, _ = median_time(lambda: large.vec.copy(tmp.vec), REPS)
    print("  dnm_vec_copy of the larger vector %9.3f ms (median of %d)" % (copy * 1e3, REPS), flush=True)
    del tmp
    med, best = median_time(lambda: computations.to_subspace(small, large_sub, result=large), REPS)
    report("to_subspace, embedding", med, best, copy, rows)
    back = State(L=small_sub.L, subspace=small_sub)
    computations.to_subspace(large, small_sub, result=back)
    med, best = median_time(lambda: computations.to_subspace(large, small_sub, result=back), REPS)
    report("to_subspace, restriction", med, best, copy, rows)
    n0, n1 = small.norm(), back.norm()
    if abs(n1 - n0) > 1e-9 * n0:
        raise SystemExit("embedding and restriction do not give the norm back: %r / %r" % (n0, n1))
    if small.vec.internal or large.vec.internal:
        # the kernel alone: both vectors in reference order, no copy to or from the internal layout inside the call
        (src, ssec), (dst, dsec) = computations._map_side(small_sub, ''), computations._map_side(large_sub, '')

        def plain(st):
            return backend.Vec(st.vec.size, array=st.vec.local_natural().clone(), swz=0) if st.vec.internal else st.vec
        s_ref, l_ref = plain(small), plain(large)
        up = lambda: backend.subspace_map(s_ref, src._to_c(), l_ref, dst._to_c(), ssec, dsec)
        down = lambda: backend.subspace_map(l_ref, dst._to_c(), s_ref, src._to_c(), dsec, ssec)
        for what, fn in (("embedding, both vectors in reference order", up),
                         ("restriction, both vectors in reference order", down)):
            fn()
            med, best = median_time(fn, REPS)
            report(what, med, best, copy, rows)
        del s_ref, l_ref
    for name, st in (("smaller", small), ("larger", large)):
        computations.sector_weights(st)
        med, best = median_time(lambda: computations.sector_weights(st), REPS)
        report("sector_weights of the %s state" % name, med, best, copy, rows)
    mag, flip = computations.sector_weights(large)
    print("  weights of the embedded state: sum %.15g, flip %r" % (mag.sum(), None if flip is None else flip.tolist()),
          flush=True)
    return small, large, copy


def host26():
    import numpy as np
    import torch
    from dynamite_amd import computations
    from dynamite_amd.states import State
    from dynamite_amd.subspaces import Full, SpinConserve, XParity
    L = 26
    full = Full(L=L)
    xp = XParity(full, sector='+')
    st = random_state(xp, 0)
    out = State(L=L, subspace=full)
    computations.to_subspace(st, full, result=out)
    med, _ = median_time(lambda: computations.to_subspace(st, full, result=out), REPS)
    t0 = time.perf_counter()
    ref = xp.convert_state(st)
    torch.cuda.synchronize()
    host = time.perf_counter() - t0
    err = (ref.vec.array - out.vec.array).abs().max().item()
    print("XParity(Full(26), '+') -> Full(26): to_subspace %.3f ms, XParity.convert_state %.3f s: %.0f x the pass "
          "(largest difference %.3g)" % (med * 1e3, host, host / med, err), flush=True)
    back = State(L=L, subspace=xp)
    computations.to_subspace(out, xp, result=back)
    med, _ = median_time(lambda: computations.to_subspace(out, xp, result=back), REPS)
    t0 = time.perf_counter()
    ref = xp.convert_state(out)
    torch.cuda.synchronize()
    host = time.perf_counter() - t0
    print("Full(26) -> XParity(Full(26), '+'): to_subspace %.3f ms, XParity.convert_state %.3f s: %.0f x the pass"
          % (med * 1e3, host, host / med), flush=True)
    del st, out, back, ref
    sc = SpinConserve(L, L // 2)
    st = random_state(sc, 1)
    out = State(L=L, subspace=full)
    computations.to_subspace(st, full, result=out)
    med, _ = median_time(lambda: computations.to_subspace(st, full, result=out), REPS)
    t0 = time.perf_counter()
    amps = st.to_numpy()
    t1 = time.perf_counter()
    wide = np.zeros(1 << L, dtype=np.complex128)
    wide[np.asarray(sc.idx_to_state(np.arange(amps.size)), dtype=np.int64)] = amps
    t2 = time.perf_counter()
    up = State(L=L, subspace=full)
    up.vec.set_local_from_numpy(wide)
    up.set_initialized()
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    if up.vec.array.ne(out.vec.array).any().item():
        raise SystemExit("the host route and the pass disagree")
    print("SpinConserve(26, 13) -> Full(26): to_subspace %.3f ms; host route: to_numpy %.3f s, numpy scatter %.3f s, "
          "back to the device %.3f s: %.3f s, %.0f x the pass"
          % (med * 1e3, t1 - t0, t2 - t1, t3 - t2, t3 - t0, (t3 - t0) / med), flush=True)


def step(name):
    from dynamite_amd.subspaces import Full, Parity, SpinConserve, XParity
    if name == "sc30":
        pair(SpinConserve(30, 15), Full(L=30))
    elif name == "xsc30":
        sub = SpinConserve(30, 15)
        pair(XParity(sub, sector='+'), sub)
    elif name == "full26":
        pair(Parity('even', L=26), Full(L=26))
    else:
        host26()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        from dynamite_amd.config import config
        config._initialize()
        step(sys.argv[2])
        return
    steps = sys.argv[1:] or ["sc30", "xsc30", "full26", "host26"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    log = os.path.join(ROOT, "profiles", "subspace_maps.txt")
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
