#!/usr/bin/env python
"""Times the site-permutation pass (csrc/perm_kernels.hip, csrc/perm_rank.h, csrc/observables.cpp, backend.perm_apply,
backend.perm_dots) beside the floors it can be held against and the host route it replaces.

site_permutations_timing.py [STEP ...]    steps: full26 full30 kagome30 kagome30x (default: all four)

  full26      permute_sites with a seeded random permutation on Full(L=26), and the host route: State.to_numpy, the
              gather in numpy, the copy back
  full30      permute_sites with a seeded random permutation on Full(L=30)
  kagome30    on SpinConserve(30, 15): permute_sites with one translation of the kagome torus of 30 sites, and
              symmetry_expectations and symmetrize with its 20 space-group elements (10 translations x 2 point-group
              elements, lattices.kagome_translations / kagome_point_group)
  kagome30x   the same on XParity(SpinConserve(30, 15), '+'), the subspace benchmarking/run_kagome.py solves in

Every step runs in a process of its own under its own time limit; the first failure ends the run.  The output is
appended to profiles/site_permutations.txt as well.  Per shape, on a random state, warm, device-synchronised, median of
REPS calls (a SpinConserve state in the internal layout is converted to reference order inside the call and the result
brought home: the extra passes are counted):
  - each call beside dnm_vec_copy of the same vector (Vec.copy), the floor of one read and one write of it, and the
    dots beside dnm_vec_dot (Vec.dot), the floor of two reads;
  - the bytes per amplitude that the time amounts to at HBM_BYTES_S.
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"full26": 300, "full30": 420, "kagome30": 300, "kagome30x": 300}
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


def report(what, med, best, floor, floor_name, rows):
    print("  %-44s median of %d %9.3f ms (best %.3f): %.2f x %s, %.0f B per amplitude at %.1f TB/s"
          % (what, REPS, med * 1e3, best * 1e3, med / floor, floor_name, med * HBM_BYTES_S / rows, HBM_BYTES_S / 1e12),
          flush=True)


def floors(st, other):
    tmp = st.copy()
    copy, _ = median_time(lambda: st.vec.copy(tmp.vec), REPS)
    dot, _ = median_time(lambda: st.vec.dot(other.vec), REPS)
    print("  dnm_vec_copy %9.3f ms, dnm_vec_dot %9.3f ms (medians of %d)" % (copy * 1e3, dot * 1e3, REPS), flush=True)
    return copy, dot, tmp


def host_route(st, perm):
    """What the pass replaces: the state to the host, the gather in numpy, the copy back."""
    import numpy as np
    from dynamite_amd.states import State
    sub = st.subspace
    t0 = time.perf_counter()
    amps = st.to_numpy()
    t1 = time.perf_counter()
    cfg = np.asarray(sub.idx_to_state(np.arange(amps.size)), dtype=np.int64)
    src = np.zeros_like(cfg)
    for i, p in enumerate(perm):
        src |= ((cfg >> np.int64(p)) & 1) << np.int64(i)
    moved = amps[np.asarray(sub.state_to_idx(src), dtype=np.int64)]
    t2 = time.perf_counter()
    out = State(L=st.L, subspace=sub)
    out.vec.set_local_from_numpy(moved)
    out.set_initialized()
    import torch
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return out, (t1 - t0, t2 - t1, t3 - t2)


def run(sub, perm, group=None, host=False):
    import numpy as np
    from dynamite_amd import backend, computations, _lib
    from dynamite_amd.states import State
    L = sub.L
    st = State(L=L, subspace=sub)
    st.set_random(seed=0, device_rng=True)
    other = State(L=L, subspace=sub)
    other.set_random(seed=1, device_rng=True)
    rows = st.vec.rows
    plain = _lib.Subspace.from_buffer_copy(sub._to_c()['data'])
    if int(plain.vec_swizzle) >= 256:        # the descriptor of the state in reference order
        plain.vec_swizzle = 0
        plain.site_perm = None
    nw, lds, _ = backend.perm_plan(plain, 1 if group is None else len(group))
    print("%r: %d rows, layout %d, %d workgroups, %d bytes of LDS" % (sub, rows, st.vec.swz, nw, lds), flush=True)
    copy, dot, out = floors(st, other)
    computations.permute_sites(st, perm, result=out)        # warm-up: scratch, tables
    med, best = median_time(lambda: computations.permute_sites(st, perm, result=out), REPS)
    report("permute_sites, one permutation", med, best, copy, "dnm_vec_copy", rows)
    back = computations.permute_sites(out, np.argsort(perm))
    if back.vec.array.ne(st.vec.array).any().item():
        raise SystemExit("the inverse permutation does not give the state back bit for bit")
    if host:
        moved, (down, gather, up) = host_route(st, perm)
        total = down + gather + up
        print("  host route: to_numpy %.3f s, numpy gather %.3f s, back to the device %.3f s: %.3f s, %.0f x the pass"
              % (down, gather, up, total, total / med), flush=True)
        if moved.vec.array.ne(out.vec.array).any().item():
            raise SystemExit("the host route and the pass disagree")
    if group is None:
        return
    G = len(group)
    e = computations.symmetry_expectations(st, group, other=other)
    med, best = median_time(lambda: computations.symmetry_expectations(st, group, other=other), REPS)
    report("symmetry_expectations, %d permutations" % G, med, best, dot, "dnm_vec_dot", rows)
    print("    per permutation: %.2f x dnm_vec_dot" % (med / G / dot))
    if abs(e[0] - other.dot(st).conjugate()) > 1e-9 * abs(e[0]) + 1e-12:        # Vec.dot conjugates its argument
        raise SystemExit("the identity's expectation is not the overlap: %r / %r" % (e[0], other.dot(st).conjugate()))
    chi = np.exp(-2j * np.pi * np.arange(G) / G)
    computations.symmetrize(st, group, chi, result=out)
    med, best = median_time(lambda: computations.symmetrize(st, group, chi, result=out), REPS)
    report("symmetrize, %d permutations" % G, med, best, copy, "dnm_vec_copy", rows)
    print("    per permutation: %.2f x dnm_vec_copy" % (med / G / copy), flush=True)


def step(name):
    import numpy as np
    from dynamite_amd import lattices
    from dynamite_amd.subspaces import Full, SpinConserve, XParity
    if name in ("kagome30", "kagome30x"):
        trans = lattices.kagome_translations('30')
        point = lattices.kagome_point_group('30')
        group = [[t[g[i]] for i in range(30)] for _, t in trans for _, g in point]
        assert len(group) == 20 and group[0] == list(range(30)) and len({tuple(p) for p in group}) == 20
        sub = SpinConserve(30, 15)
        run(XParity(sub, sector='+') if name == "kagome30x" else sub, np.array(trans[1][1]), group)
    else:
        L = {"full26": 26, "full30": 30}[name]
        run(Full(L=L), np.random.default_rng(L).permutation(L), host=name == "full26")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        from dynamite_amd.config import config
        config._initialize()
        step(sys.argv[2])
        return
    steps = sys.argv[1:] or ["full26", "full30", "kagome30", "kagome30x"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    log = os.path.join(ROOT, "profiles", "site_permutations.txt")
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
