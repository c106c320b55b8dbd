#!/usr/bin/env python
"""Bit-for-bit record of the Krylov drivers: a fixed list of small solves, one line each -- reason, its, matvecs, nconv,
err_est as a hex float, sha256 of the returned eigenvalues, sha256 of the eigenvectors / the evolved state.  No kernel
of the package adds atomically, so a solve is reproducible and two builds that launch the same kernels with the same
host arithmetic print the same file:

    DNM_EXPERIMENTAL=1 DNM_LIB=<other build>/libdynamite_amd.so python tools/solver_ab.py > a.txt
    python tools/solver_ab.py > b.txt && cmp a.txt b.txt

The cases are the smallest at which each branch of dnm_eigsolve (plain, filtered, basis-free, real-packed),
dnm_eigsolve_interior, dnm_expm_multiply and dnm_expm_chebyshev is still taken; the operators are those of
tests/test_gpu_interior.py and the goldens."""
import ctypes as C
import hashlib
import os
os.environ.setdefault("DNM_EXPERIMENTAL", "1")   # tools drive experiment knobs
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from dynamite_amd import _lib, backend, models  # noqa: E402
from dynamite_amd.computations import eigsolve, evolve  # noqa: E402
from dynamite_amd.config import config  # noqa: E402
from dynamite_amd.operators import sigmax, sigmay, sigmaz, index_sum, op_sum  # noqa: E402
from dynamite_amd.states import State  # noqa: E402
from dynamite_amd.subspaces import Full, SpinConserve  # noqa: E402

SMALL_TILES = {"DNM_TILE_BITS": "8", "DNM_LOG_ROWS": "2", "DNM_PLAN_MODE": "2", "DNM_GBITS": "3", "DNM_AMIN": "3"}
REAL = dict(SMALL_TILES, DNM_EIGS_REAL="1")      # the knobs of test_real_arithmetic


def heisenberg(L, seed=1234):
    """tests/test_gpu_interior.py: random-field Heisenberg chain"""
    rng = np.random.RandomState(seed)
    return (index_sum(op_sum(0.25 * s(0) * s(1) for s in (sigmax, sigmay, sigmaz)), size=L) +
            op_sum(0.5 * rng.uniform(-2, 2) * sigmaz(i) for i in range(L)))


def dm_chain(L, seed=1235):
    """... plus a Dzyaloshinskii-Moriya term: complex matrix elements"""
    return heisenberg(L, seed) + index_sum(0.1 * (sigmax(0) * sigmay(1) - sigmay(0) * sigmax(1)), size=L)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


CASE = [""]


def report(st, vals, vecs, note=""):
    name = CASE[0] + note
    print("%-28s reason %2d its %4d matvecs %6d nconv %3s err_est %-24s real %-5s vals %s vecs %s" % (
        name, st['reason'], st['its'], st['matvecs'], st.get('nconv', '-'),
        float(st.get('err_est', st.get('max_rel_residual', 0.0))).hex(), st.get('real_arithmetic', '-'),
        sha(vals) if vals is not None else '-',
        sha(np.concatenate(vecs)) if vecs else '-'), flush=True)


def eigs(mkH, mksub=None, getvecs=True, **kw):
    H = mkH()
    if mksub is not None:
        H.subspace = mksub()
    try:
        out = H.eigsolve(getvecs=getvecs, **kw)
    except Exception as e:       # a solve that raises must raise from both builds, with the same counts
        report(eigsolve.last_stats, None, None, " (" + type(e).__name__ + ")")
        return
    vals, vecs = out if getvecs else (out, None)
    report(eigsolve.last_stats, vals, [v.to_numpy() for v in vecs] if vecs else None)


def interior(mkH, mksub, frac, nev, getvecs=True):
    H = mkH()
    H.subspace = mksub()
    w = np.linalg.eigvalsh(H.to_numpy(sparse=False))
    sigma = round(float(w[0] + frac * (w[-1] - w[0])), 3)
    eigs(lambda: H, None, getvecs, nev=nev, target=sigma, interior='filter', tol=1e-9)


def expm(mkH, t, seed=4, **kw):
    H = mkH()
    H.establish_L()
    y = H.evolve(State(L=H.L, state='random', seed=seed), t=t, **kw)
    report(evolve.last_stats, None, [y.to_numpy()])


def hooked(which_interior):
    """the single-process hook arrangement of test_hook_path_single_process"""
    H = heisenberg(12)
    sub = SpinConserve(12, 6)
    H.subspace = sub
    w = np.linalg.eigvalsh(H.to_numpy(sparse=False))
    sigma = round(float(w[0] + 0.5 * (w[-1] - w[0])), 3)
    mat = H.get_mat(subspaces=(sub, sub))
    L = _lib.lib()

    def mult(ctx, x, y):
        return L.dnm_mat_mult(mat.handle, x, y, backend._stream())

    hooks = _lib.Hooks(None, _lib.MULT_FN(mult), _lib.REDUCE_FN(lambda ctx, buf, n: 0),
                       _lib.REDUCE_FN(lambda ctx, buf, n: 0))
    nev, nev_max = (10, 20) if which_interior else (3, 18)
    evals = np.zeros(nev_max)
    vecs = backend.device_zeros(nev_max * mat.n_local, empty=True)
    stats = _lib.SolverStats()
    tail = (0, 0, 0, C.byref(hooks), nev_max, _lib.pf64(evals), C.c_void_p(vecs.data_ptr()), C.byref(stats),
            backend._stream())
    if which_interior:
        _lib.check(L.dnm_eigsolve_interior(mat.handle, mat.n_local, nev, sigma, 1e-9, *tail))
    else:
        _lib.check(L.dnm_eigsolve(mat.handle, mat.n_local, nev, 0, 1e-10, *tail))
    st = {'reason': stats.reason, 'its': stats.its, 'matvecs': stats.matvecs, 'nconv': stats.nconv,
          'err_est': stats.err_est}
    report(st, evals[:stats.nconv], [vecs[:stats.nconv * mat.n_local].cpu().numpy()])


def cases():
    mbl12 = lambda: models.mbl(12)       # noqa: E731
    sc12 = lambda: SpinConserve(12, 6)   # noqa: E731
    # ---- dnm_eigsolve, the plain restarted scheme
    for which in ("lowest", "highest", "exterior"):
        for nev in (1, 5):
            yield "plain_%s_nev%d" % (which, nev), {}, lambda w=which, n=nev: eigs(mbl12, nev=n, which=w, tol=1e-10)
    yield "plain_sc12_nev3", {}, lambda: eigs(lambda: heisenberg(12), sc12, nev=3, tol=1e-10)
    yield "plain_ortho_full", {"DNM_EIGS_ORTHO": "full"}, lambda: eigs(mbl12, nev=5, tol=1e-10)
    yield "plain_beta_sweep", {"DNM_EIGS_BETA": "sweep"}, lambda: eigs(mbl12, nev=5, tol=1e-10)
    yield "plain_beta_rescale", {"DNM_EIGS_BETA": "rescale"}, lambda: eigs(mbl12, nev=5, tol=1e-10)
    yield "plain_known0", {"DNM_EIGS_KNOWN": "0"}, lambda: eigs(mbl12, nev=5, tol=1e-10)
    yield "plain_ncv8", {}, lambda: eigs(mbl12, nev=3, ncv=8, tol=1e-10)
    yield "plain_xsum8_breakdown", {}, lambda: eigs(lambda: models.xsum(8), nev=2, tol=1e-12)
    # ---- ... on the end filter
    for which in ("lowest", "highest"):
        yield "filtered_" + which, {"DNM_EIGS_FILTER": "1"}, lambda w=which: eigs(mbl12, nev=3, which=w, tol=1e-12)
        yield ("filtered_pro_" + which, {"DNM_EIGS_FILTER": "1", "DNM_EIGS_FILTER_PRO": "1"},
               lambda w=which: eigs(mbl12, nev=3, which=w, tol=1e-12))
    yield ("filtered_degree13", {"DNM_EIGS_FILTER": "1", "DNM_EIGS_FILTER_DEGREE": "13"},
           lambda: eigs(mbl12, nev=3, tol=1e-12))
    # ---- ... without a stored basis
    yield "basisfree_values", {"DNM_EIGS_BASISFREE": "1"}, lambda: eigs(mbl12, getvecs=False, nev=1, tol=1e-10)
    yield "basisfree_vectors", {"DNM_EIGS_BASISFREE": "1"}, lambda: eigs(mbl12, nev=1, tol=1e-10)
    yield "basisfree_deflated_nev3", {"DNM_EIGS_BASISFREE": "1"}, lambda: eigs(mbl12, nev=3, tol=1e-10)
    # ---- ... on the real-packed handle
    yield "real_plain", REAL, lambda: eigs(mbl12, lambda: Full(L=12), nev=3, tol=1e-11)
    yield "real_filtered", dict(REAL, DNM_EIGS_FILTER="1"), lambda: eigs(mbl12, lambda: Full(L=12), nev=3, tol=1e-11)
    # ---- dnm_eigsolve_interior
    yield "interior_sc12_mid", {}, lambda: interior(lambda: heisenberg(12), sc12, 0.5, 10)
    yield "interior_complex_sc12", {}, lambda: interior(lambda: dm_chain(12), sc12, 0.5, 10)
    yield "interior_full12_real", REAL, lambda: interior(lambda: heisenberg(12), lambda: Full(12), 0.6, 12)
    yield ("interior_widened", {"DNM_EIGS_INTERIOR_WINDOW": "0.2"},
           lambda: interior(lambda: heisenberg(12), sc12, 0.5, 10))
    yield "interior_values_only", {}, lambda: interior(lambda: heisenberg(12), sc12, 0.5, 10, getvecs=False)
    # ---- dnm_expm_multiply, dnm_expm_chebyshev
    yield "expm_default", {}, lambda: expm(mbl12, 5.0)
    yield "expm_krylov_pro", {"DNM_EXPM_HYBRID": "0"}, lambda: expm(mbl12, 5.0)
    yield "expm_ortho_full", {"DNM_EXPM_ORTHO": "full"}, lambda: expm(mbl12, 5.0)
    yield "expm_krylov_ortho_full", {"DNM_EXPM_HYBRID": "0", "DNM_EXPM_ORTHO": "full"}, lambda: expm(mbl12, 5.0)
    yield "expm_probe_mbl12", {"DNM_EXPM_PROBE": "1"}, lambda: expm(mbl12, 3.0)
    yield "expm_probe_syk8", {"DNM_EXPM_PROBE": "1"}, lambda: expm(lambda: models.BY_NAME["syk"](8), 0.3)
    yield "expm_imaginary_time", {}, lambda: expm(mbl12, -0.25j)
    yield "expm_ncv10", {}, lambda: expm(mbl12, 5.0, ncv=10)
    yield "expm_chebyshev", {}, lambda: expm(mbl12, 5.0, algo='chebyshev')
    # ---- through the hooks
    yield "hooks_plain", {}, lambda: hooked(False)
    yield "hooks_interior", {}, lambda: hooked(True)


def main():
    config._initialize()
    for name, env, run in cases():
        CASE[0] = name
        os.environ.update(env)
        try:
            run()
        finally:
            for k in env:
                del os.environ[k]


if __name__ == "__main__":
    main()
