#!/usr/bin/env python
"""Times the site-operator product (csrc/site_ops_kernels.hip: dnm_site_ops_apply) and the exponential of a diagonal
operator (dnm_mat_expm_diagonal) on Full(L) beside dnm_vec_copy and beside the routes they replace.

site_ops_timing.py [--log FILE] [STEP ...]   steps: tiles26 tiles30 routes26 routes30 (default: all four)

  tilesL    at tile_bits 12 and at 13 (DNM_SITE_OPS_TILE_BITS, a process each): the product on all sites (the x-basis
            rotation), on one site (the top one), on the low 4 sites only, and an all-diagonal product, in place, each
            beside dnm_vec_copy of the same vector times the pass count
  routesL   dnm_mat_expm_diagonal of the nearest-neighbour ZZ chain and of an all-to-all ZZ coupling 1 / |i - j|^1.13,
            each beside default evolve of the same operator and t; evolve(algo='exact') of a global x field beside
            default evolve; the global X pulse beside Operator.dot of prod_j sigmax_j; at L = 26 sample(bases='x')
            beside the host route (to_numpy, the rotation in numpy, numpy's sampler)

Every step runs in a process of its own under its own time limit; the first failure ends the run.  The output is appended
to profiles/site_operators.txt (or FILE).  Timings: warm, device-synchronised, median of REPS calls on a random state.
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"tiles26": 240, "tiles30": 400, "routes26": 500, "routes30": 560}
REPS = 7


def median_time(fn, reps=REPS):
    import torch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts)


def once(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def random_state(L):
    from dynamite_amd.states import State
    from dynamite_amd.subspaces import Full
    st = State(L=L, subspace=Full(L=L))
    st.set_random(seed=0, device_rng=True)
    return st


def tiles(L):
    import numpy as np
    from dynamite_amd import backend
    from dynamite_amd.computations import apply_site_operators, basis_rotations
    st = random_state(L)
    tmp = st.copy()
    copy, _ = median_time(lambda: st.vec.copy(tmp.vec))
    del tmp
    sub_c = st.subspace._to_c()['data']
    eye = np.broadcast_to(np.eye(2, dtype=complex), (L, 2, 2))
    phases = np.array([np.diag([1, np.exp(0.1j * (j + 1))]) for j in range(L)])
    cases = [("all %d sites (x rotation)" % L, basis_rotations('x', L)),
             ("one site (the top one)", np.where(np.arange(L)[:, None, None] == L - 1, basis_rotations('x', L), eye)),
             ("the low 4 sites only", np.where(np.arange(L)[:, None, None] < 4, basis_rotations('x', L), eye)),
             ("all %d sites diagonal" % L, phases)]
    print("Full(L=%d), layout %d: dnm_vec_copy %.3f ms (median of %d)" % (L, st.vec.swz, copy * 1e3, REPS), flush=True)
    for what, mats in cases:
        tb, npasses, _, nwg, lds = backend.site_ops_plan(sub_c, mats)
        apply_site_operators(st, mats, result=st)
        med, best = median_time(lambda: apply_site_operators(st, mats, result=st))
        print("  tile_bits %d  %-28s %d pass(es), %6d workgroups, %6d B LDS: median %8.3f ms (best %.3f) = %.2f x "
              "(%d x dnm_vec_copy), %.0f GB/s of 32 B per amplitude and pass"
              % (tb, what, npasses, nwg, lds, med * 1e3, best * 1e3, med / (npasses * copy), npasses,
                 32.0 * npasses * (1 << L) / med / 1e9), flush=True)


def routes(L):
    import numpy as np
    from dynamite_amd.computations import apply_site_operators, evolve, sample
    from dynamite_amd.operators import index_sum, op_product, op_sum, sigmax, sigmaz
    st = random_state(L)
    st.normalize()
    out = st.copy()
    copy, _ = median_time(lambda: st.vec.copy(out.vec))
    print("Full(L=%d), layout %d: dnm_vec_copy %.3f ms (median of %d)" % (L, st.vec.swz, copy * 1e3, REPS), flush=True)
    sub = st.subspace
    chain = index_sum(sigmaz(0) * sigmaz(1), size=L)
    allpairs = op_sum(sigmaz(i) * sigmaz(j) * (1.0 / (j - i) ** 1.13) for i in range(L) for j in range(i + 1, L))
    field = index_sum(sigmax(0), size=L)
    for name, H, t in (("ZZ chain", chain, 1.0), ("all-to-all ZZ", allpairs, 1.0), ("global x field", field, 0.7)):
        H.L = L
        H.add_subspace(sub)
        first, _ = once(lambda: evolve(H, st, t, result=out, algo='exact'))       # builds the handle, caches the diagonal
        med, best = median_time(lambda: evolve(H, st, t, result=out, algo='exact'))
        print("  %-16s evolve(algo='exact', t=%.1f): first call %.3f s, then median %8.3f ms (best %.3f) = %.2f x "
              "dnm_vec_copy" % (name, t, first, med * 1e3, best * 1e3, med / copy), flush=True)
        ref = out.copy()
        evolve(H, st, t, result=out)                                                # warm: the probe of the norm, scratch
        took, _ = once(lambda: evolve(H, st, t, result=out))
        stats = dict(evolve.last_stats)
        ref.axpy(-1.0, out)
        print("  %-16s default evolve of the same: %.3f s, %d multiplies: %.0f x the exact route; the two differ by %.2e"
              % (name, took, stats['matvecs'], took / med, ref.norm()), flush=True)
        del ref
    pulse = op_product(sigmax(j) for j in range(L))
    pulse.L = L
    pulse.add_subspace(sub)
    X = np.array([[0, 1], [1, 0]], dtype=complex)
    pulse.dot(st, result=out)
    dot, _ = median_time(lambda: pulse.dot(st, result=out))
    ref = out.copy()
    apply_site_operators(st, X, result=out)
    med, best = median_time(lambda: apply_site_operators(st, X, result=out))
    same = not ref.vec.array.ne(out.vec.array).any().item()
    print("  global X pulse: apply_site_operators median %8.3f ms (best %.3f); Operator.dot of prod_j sigmax_j %8.3f ms; "
          "the same bits: %s" % (med * 1e3, best * 1e3, dot * 1e3, same), flush=True)
    del ref
    if L <= 26:
        shots = 1000
        sample(st, shots, seed=1, bases='x')
        med, best = median_time(lambda: sample(st, shots, seed=1, bases='x'), 3)
        t0 = time.perf_counter()
        amps = st.to_numpy()
        t1 = time.perf_counter()
        h = np.sqrt(0.5)
        for j in range(L):
            v = amps.reshape(1 << (L - 1 - j), 2, 1 << j)
            a, b = v[:, 0, :].copy(), v[:, 1, :]
            v[:, 0, :] = h * (a + b)
            v[:, 1, :] = h * (a - b)
        t2 = time.perf_counter()
        w = amps.real ** 2 + amps.imag ** 2
        np.random.default_rng(1).choice(w.size, size=shots, p=w / w.sum())
        t3 = time.perf_counter()
        print("  sample(bases='x'), %d shots: median %8.3f ms (copy, rotate, sample on the device); host route: to_numpy "
              "%.2f s, numpy rotation %.2f s, numpy sampler %.2f s = %.0f x"
              % (shots, med * 1e3, t1 - t0, t2 - t1, t3 - t2, (t3 - t0) / med), flush=True)


def step(name):
    L = int(name[-2:])
    if name.startswith("tiles"):
        tiles(L)
    else:
        routes(L)


def main():
    args = sys.argv[1:]
    if len(args) > 1 and args[0] == "--step":
        from dynamite_amd.config import config
        config._initialize()
        step(args[1])
        return
    log = os.path.join(ROOT, "profiles", "site_operators.txt")
    if len(args) > 1 and args[0] == "--log":
        log, args = os.path.abspath(args[1]), args[2:]
    steps = args or ["tiles26", "tiles30", "routes26", "routes30"]
    os.makedirs(os.path.dirname(log), exist_ok=True)
    for s in steps:
        for tb in (("12", "13") if s.startswith("tiles") else (None,)):
            env = dict(os.environ)
            if tb:
                env.update(DNM_EXPERIMENTAL="1", DNM_SITE_OPS_TILE_BITS=tb)
            cmd = ["timeout", "-k", "10", str(LIMITS[s]), sys.executable, os.path.abspath(__file__), "--step", s]
            with open(log, "a") as f, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                                                       env=env) as p:
                def emit(line):
                    sys.stdout.write(line)
                    sys.stdout.flush()
                    f.write(line)
                emit("== step %s%s ==\n" % (s, " tile_bits " + tb if tb else ""))
                for line in iter(p.stdout.readline, ""):
                    emit(line)
                emit("== step %s: exit status %d ==\n\n" % (s, p.wait()))
            if p.returncode != 0:
                sys.exit(p.returncode)       # nothing more is started on the device after a failure
    return


if __name__ == "__main__":
    main()
