#!/usr/bin/env python
"""Times the sector-resolved reduced density matrix (csrc/rdm_sector_kernels.hip) against the dense form.

rdm_sectors_timing.py [STEP ...]    steps: 26 32 34 (default: 26 32)

Every step runs in a process of its own under its own time limit; the first failure ends the run.  The output is
appended to profiles/rdm_sectors.txt as well.
  26  SpinConserve(26, 13), 13 spins kept, random state: the blocks against the dense rdm_mfma_kernel route in one
      process -- the C call alone (kernels, synchronised) and the whole spectrum call (what entanglement_entropy pays)
  32  SpinConserve(32, 16), 16 spins kept: the XX chain's ground state from eigsolve, its half-chain entropy against
      Peschel's free-fermion formula; per block: kernel time, fp64 rate on the lower-triangle products, eigvalsh time
  34  SpinConserve(34, 17), 17 spins kept, random state: kernel and eigvalsh time of the largest block
"""
import os
import subprocess
import sys
import time

os.environ.setdefault("DNM_EXPERIMENTAL", "1")   # tools drive experiment knobs
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"26": 240, "32": 900, "34": 1100}


def timed(fn, reps=1):
    import torch
    best = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, out


def products(plan):
    """complex products of the lower triangles of the blocks"""
    return sum(d * (d + 1) // 2 * t for _, d, t in plan)


def random_state(sub):
    from dynamite_amd.states import State
    st = State(L=sub.L, subspace=sub)
    st.set_random(seed=0, device_rng=True)
    return st


def step26():
    import numpy as np
    import torch
    from dynamite_amd import backend, computations as cp
    from dynamite_amd.subspaces import SpinConserve
    L, k = 26, 13
    sub = SpinConserve(L, k)
    st = random_state(sub)
    keep = np.arange(13, dtype=np.int64)
    sub_c = sub._to_c()
    plan, scratch = backend.rdm_sector_plan(sub_c['data'], keep)
    ns = [n for n, _, _ in plan]
    print("SpinConserve(26,13), 13 kept: %d blocks, largest %d rows, %.3e lower-triangle products (dense: %.3e), "
          "scratch %.1f MB" % (len(plan), max(d for _, d, _ in plan), products(plan), (1 << 26) * (1 << 13) / 2,
                               scratch / 1e6))
    for name, fn in (("dense  C call (rdm_mfma_kernel + sum + mirror)",
                      lambda: backend.reduced_density_matrix(st.vec, sub_c, keep, on_device=True)),
                     ("blocks C call (all 14 blocks, one launch sequence)",
                      lambda: backend.rdm_sector_blocks(st.vec, sub_c, keep, 0, ns, plan=plan)),
                     ("dense  spectrum call (_rdm_spectrum: matrix, cut blocks, eigvalsh)",
                      lambda: cp._rdm_spectrum(st, keep)),
                     ("blocks spectrum call (_sector_spectrum: block, eigvalsh, free)",
                      lambda: cp._sector_spectrum(st, keep))):
        fn()                                     # warm-up: allocations, solver handles
        dt, out = timed(fn, reps=3)
        print("  %-72s %9.3f ms" % (name, dt * 1e3), flush=True)
        if "spectrum" in name:
            w = out
            print("  %-72s %.15f" % ("  entropy", cp._entropy_of_spectrum(w)))
        del out
    torch.cuda.empty_cache()


def peschel(L, k, nA):
    import numpy as np
    j = np.arange(1, L + 1)
    modes = np.argsort(np.cos(np.pi * j / (L + 1)))[:k] + 1
    phi = np.sqrt(2.0 / (L + 1)) * np.sin(np.pi * np.outer(j, modes) / (L + 1))
    nu = np.linalg.eigvalsh((phi @ phi.T)[:nA, :nA])
    nu = nu[(nu > 1e-15) & (nu < 1 - 1e-15)]
    return float(-(nu * np.log(nu) + (1 - nu) * np.log(1 - nu)).sum())


def per_block(st, sub, keep, only_largest=False):
    """kernel and eigvalsh time of every block, one at a time; returns the spectrum"""
    import numpy as np
    import torch
    from dynamite_amd import backend
    sub_c = sub._to_c()
    plan, scratch = backend.rdm_sector_plan(sub_c['data'], keep)
    print("  %d blocks, largest %d rows, %.3e lower-triangle products, blocks %.2f GB in all, scratch for all at once "
          "%.2f GB" % (len(plan), max(d for _, d, _ in plan), products(plan),
                       16 * sum(d * d for _, d, _ in plan) / 1e9, scratch / 1e9))
    if only_largest:
        plan = [max(plan, key=lambda b: b[1])]
    whole = backend._whole_state_on_rank0(st.vec, sub_c)
    free0 = torch.cuda.mem_get_info()[0]
    low = free0
    tk = te = 0.0
    out = []
    for n, d, t in plan:
        dk, blocks = timed(lambda: backend.rdm_sector_blocks(st.vec, sub_c, keep, 0, [n], whole=whole))
        low = min(low, torch.cuda.mem_get_info()[0])
        de, w = timed(lambda: torch.linalg.eigvalsh(blocks[n]))
        low = min(low, torch.cuda.mem_get_info()[0])
        flop = 8.0 * d * (d + 1) / 2 * t
        print("  block n=%2d  %6d rows x %6d traced   kernels %9.2f ms  %6.2f TFLOP/s   eigvalsh %9.2f ms"
              % (n, d, t, dk * 1e3, flop / dk / 1e12, de * 1e3), flush=True)
        tk += dk
        te += de
        out.append(w.cpu().numpy())
        del blocks, w
        torch.cuda.empty_cache()
    print("  kernels %.1f ms in all (%.2f TFLOP/s fp64 on the lower-triangle products), eigvalsh %.1f ms, device memory "
          "beyond the state at the peak: %.2f GB" % (tk * 1e3, 8.0 * products(plan) / tk / 1e12, te * 1e3,
                                                      (free0 - low) / 1e9))
    return np.sort(np.concatenate(out))


def step32():
    import numpy as np
    from dynamite_amd import computations as cp
    from dynamite_amd.config import config
    from dynamite_amd.operators import sigmax, sigmay, op_sum
    from dynamite_amd.subspaces import SpinConserve
    L, k = 32, 16
    config.L = L
    sub = SpinConserve(L, k)
    H = op_sum(0.25 * (sigmax(i) * sigmax(i + 1) + sigmay(i) * sigmay(i + 1)) for i in range(L - 1))
    H.L = L
    H.add_subspace(sub)
    t0 = time.perf_counter()
    ev, vecs = H.eigsolve(nev=1, tol=1e-11, getvecs=True, subspace=sub)
    j = np.arange(1, L + 1)
    exact = np.sort(np.cos(np.pi * j / (L + 1)))[:k].sum()
    print("SpinConserve(32,16) XX chain: eigsolve %.1f s, E0 = %.12f (exact %.12f)" % (time.perf_counter() - t0, ev[0], exact),
          flush=True)
    H.destroy_mat()
    keep = np.arange(16, dtype=np.int64)
    w = per_block(vecs[0], sub, keep)
    s, want = cp._entropy_of_spectrum(w), peschel(L, k, 16)
    print("  half-chain entropy %.10f, Peschel %.10f, difference %.2e (bar 1e-7)" % (s, want, abs(s - want)))
    dt, s2 = timed(lambda: cp.entanglement_entropy(vecs[0], keep))
    print("  entanglement_entropy, whole call: %.2f s (%.10f)" % (dt, s2))
    if abs(s - want) >= 1e-7 or abs(s2 - want) >= 1e-7:
        raise SystemExit("entropy off the free-fermion value")


def step34():
    import numpy as np
    from dynamite_amd.subspaces import SpinConserve
    sub = SpinConserve(34, 17)
    st = random_state(sub)
    print("SpinConserve(34,17), 17 kept, random state, largest block only", flush=True)
    per_block(st, sub, np.arange(17, dtype=np.int64), only_largest=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        from dynamite_amd.config import config
        config._initialize()
        {"26": step26, "32": step32, "34": step34}[sys.argv[2]]()
        return
    steps = sys.argv[1:] or ["26", "32"]
    log = os.path.join(ROOT, "profiles", "rdm_sectors.txt")
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


if __name__ == "__main__":
    main()
