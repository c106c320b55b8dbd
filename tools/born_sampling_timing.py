#!/usr/bin/env python
"""Times Born sampling and the power sums of the participation entropies (csrc/born_kernels.hip, csrc/born.h,
csrc/observables.cpp, backend.born_sample, backend.power_sums) beside dnm_vec_norm2 of the same vector and the host
route they replace.

born_sampling_timing.py [STEP ...]    steps: full26 full30 sc30 sc30x (default: all four)

  full26   Full(L=26), and the host route: State.to_numpy, |psi|^2, numpy.cumsum, numpy.searchsorted
  full30   Full(L=30)
  sc30     SpinConserve(30, 15)
  sc30x    XParity(SpinConserve(30, 15), '+')

Every step runs in a process of its own under its own time limit; the first failure ends the run.  The output is
appended to profiles/born_sampling.txt as well.  Per shape, on a random state, warm, device-synchronised, median of REPS
calls:
  - dnm_vec_norm2 of the vector as it lies: it moves the same 16 bytes per row as the block-sum pass and the power-sum
    pass, which are to be read against it;
  - dnm_born_block_sums (the pass, the block sums to the host, the scan);
  - dnm_born_sample of SHOTS shots (that pass again, the scan to the device, the search, the rows to the host) and
    State.sample of as many (with the conversion to reference order of an internal-layout vector and idx_to_state);
  - dnm_vec_power_sums with q = (2, 3) -- q = 1 needs no exponent, H is part of every pass -- and
    State.participation_entropies((2, 3, 1)).
"""
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"full26": 300, "full30": 420, "sc30": 300, "sc30x": 300}
REPS = 7
SHOTS = 1 << 20
SEED = 12345


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


def report(what, med, best, norm2):
    print("  %-52s median of %d %9.3f ms (best %.3f): %6.2f x dnm_vec_norm2" % (what, REPS, med * 1e3, best * 1e3,
                                                                                  med / norm2), flush=True)


def host_route(st, shots):
    """What sampling replaces: the state to the host, the weights, their cumulative sum and a search per shot."""
    import numpy as np
    t0 = time.perf_counter()
    amps = st.to_numpy()
    t1 = time.perf_counter()
    w = amps.real ** 2 + amps.imag ** 2
    cum = np.cumsum(w)
    t2 = time.perf_counter()
    t = np.random.default_rng(SEED).random(shots) * cum[-1]
    rows = np.minimum(np.searchsorted(cum, t, side='right'), w.size - 1)
    t3 = time.perf_counter()
    p = w / cum[-1]
    ent = [-np.log(np.sum(p ** 2)), np.log(np.sum(p ** 3)) / -2, -np.sum(p * np.log(p))]
    t4 = time.perf_counter()
    return rows, ent, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)


def run(sub, host=False):
    import numpy as np
    from dynamite_amd import backend, _lib
    from dynamite_amd.states import State
    st = State(L=sub.L, subspace=sub)
    st.set_random(seed=0, device_rng=True)
    vec = st.vec
    x, sub_c = backend._reference_order(vec, sub._to_c()['data'])
    rows = vec.rows
    br, nb, sb = backend.born_plan(sub_c, rows)
    print("%r: %d rows, layout %d (%d elements), blocks of %d rows: %d block sums, %d bytes"
          % (sub, rows, vec.swz, vec.local_size, br, nb, sb), flush=True)
    out = (C.c_double * 1)()
    lib, stream = _lib.lib(), backend._stream()

    def norm2():
        _lib.check(lib.dnm_vec_norm2(vec.ptr, vec.local_size, out, stream))
    norm2()
    n2, n2best = median_time(norm2, REPS)
    print("  dnm_vec_norm2 %9.3f ms (best %.3f, median of %d): %.2f TB/s" % (n2 * 1e3, n2best * 1e3, REPS,
                                                                          16.0 * vec.local_size / n2 / 1e12), flush=True)
    sums, scan = backend.born_block_sums(x, sub_c, 0, rows)            # warm-up: scratch
    sums_med, best = median_time(lambda: backend.born_block_sums(x, sub_c, 0, rows), REPS)
    report("dnm_born_block_sums (reference-order vector)", sums_med, best, n2)
    if abs(scan[-1] - out[0] ** 2) > 1e-9 * scan[-1]:
        raise SystemExit("the total weight %r is not the squared norm %r" % (scan[-1], out[0] ** 2))
    r0, _ = backend.born_sample_block(x, sub_c, 0, rows, SEED, 0, SHOTS)
    med, best = median_time(lambda: backend.born_sample_block(x, sub_c, 0, rows, SEED, 0, SHOTS), REPS)
    report("dnm_born_sample, %d shots" % SHOTS, med, best, n2)
    print("    the shots' share (over the block-sum call): %.3f ms, %.1f ns a shot"
          % ((med - sums_med) * 1e3, (med - sums_med) / SHOTS * 1e9), flush=True)
    if r0.min() < 0 or r0.max() >= rows:
        raise SystemExit("a shot outside the state")
    st.sample(SHOTS, seed=SEED)                                        # warm-up: the copy to reference order
    med, best = median_time(lambda: st.sample(SHOTS, seed=SEED), REPS)
    report("State.sample, %d shots" % SHOTS, med, best, n2)
    backend.power_sums(vec, [2, 3])
    med, best = median_time(lambda: backend.power_sums(vec, [2, 3]), REPS)
    report("dnm_vec_power_sums, q = (2, 3) and H", med, best, n2)
    med, best = median_time(lambda: backend.power_sums(vec, [0.5, 2, 3]), REPS)
    report("dnm_vec_power_sums, q = (0.5, 2, 3) and H (one pow)", med, best, n2)
    ent = st.participation_entropies((2, 3, 1))
    med, best = median_time(lambda: st.participation_entropies((2, 3, 1)), REPS)
    report("State.participation_entropies((2, 3, 1))", med, best, n2)
    print("    S_2, S_3, S_1 = %.9f, %.9f, %.9f (ln of the product-basis dimension: %.9f)"
          % (ent[0], ent[1], ent[2], np.log(rows * (1 if st.subspace.product_state_basis else 2))), flush=True)
    if host:
        hrows, hent, (down, cum, search, entropy) = host_route(st, SHOTS)
        total = down + cum + search
        print("  host route: to_numpy %.3f s, weights and cumsum %.3f s, %d searches %.3f s: %.3f s; the three entropies "
              "from the weights %.3f s more" % (down, cum, SHOTS, search, total, entropy), flush=True)
        if np.max(np.abs(np.array(hent) - ent)) > 1e-9:
            raise SystemExit("the host route and the pass disagree on the entropies: %r / %r" % (hent, ent))
        # the two draws use different uniforms: compare the mean row, whose spread over 2^20 shots is rows / 2^10 / sqrt 12
        if abs(hrows.mean() - r0.mean()) > 6 * rows / 1024 / np.sqrt(12) * np.sqrt(2):
            raise SystemExit("the host route and the pass disagree on the mean row: %r / %r" % (hrows.mean(), r0.mean()))


def step(name):
    from dynamite_amd.subspaces import Full, SpinConserve, XParity
    if name == "sc30":
        run(SpinConserve(30, 15))
    elif name == "sc30x":
        run(XParity(SpinConserve(30, 15), sector='+'))
    else:
        run(Full(L={"full26": 26, "full30": 30}[name]), host=name == "full26")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        from dynamite_amd.config import config
        config._initialize()
        step(sys.argv[2])
        return
    steps = sys.argv[1:] or ["full26", "full30", "sc30", "sc30x"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    log = os.path.join(ROOT, "profiles", "born_sampling.txt")
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
