"""Interior eigenpairs on the GPU: eigsolve(target=, interior='filter') -- thick-restart Lanczos on a Chebyshev filter
of the folded spectrum (csrc/krylov.cpp: dnm_eigsolve_interior) -- against dense diagonalisation on the host, and the
one-thread-per-row kernels with their fused epilogue (csrc/row_fused_kernels.hip) against the unfused composition.
The reference for every number is numpy.linalg.eigvalsh / eigh of H.to_numpy(), never the solver itself."""
import ctypes as C

import numpy as np
import pytest

from dynamite_amd import _lib, backend
from dynamite_amd.operators import sigmax, sigmay, sigmaz, index_sum, op_sum
from dynamite_amd.subspaces import Auto, Full, Parity, SpinConserve, XParity
from gpu_util import shell, vec_from

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
TOL = 1e-9


def heisenberg(L, seed=1234):
    """Random-field Heisenberg chain: couplings 0.25 (XX + YY + ZZ), fields 0.5 U(-2, 2) sigma_z."""
    rng = np.random.RandomState(seed)
    return (index_sum(op_sum(0.25 * s(0) * s(1) for s in (sigmax, sigmay, sigmaz)), size=L) +
            op_sum(0.5 * rng.uniform(-2, 2) * sigmaz(i) for i in range(L)))


def random_xxz(L, seed=1234):
    """Random-bond XXZ chain without fields: commutes with the global spin flip (XParity) and conserves S_z."""
    rng = np.random.RandomState(seed)
    return op_sum(0.25 * rng.uniform(0.5, 1.5) * (sigmax(i) * sigmax(i + 1) + sigmay(i) * sigmay(i + 1)) +
                  0.25 * rng.uniform(0.5, 1.5) * sigmaz(i) * sigmaz(i + 1) for i in range(L - 1))


def dm_chain(L, seed=1235):
    """The random-field chain plus a Dzyaloshinskii-Moriya term 0.1 (XY - YX): Hermitian with imaginary matrix
    elements in the product basis, so no real-packed form -- the complex128 path of the solver."""
    return heisenberg(L, seed) + index_sum(0.1 * (sigmax(0) * sigmay(1) - sigmay(0) * sigmax(1)), size=L)


def auto_half_filling(H):
    return Auto(H, 'U' * (H.get_length() // 2) + 'D' * (H.get_length() // 2))


# (name, operator, subspace, fraction of the band, nev, eigenvectors of the dense solve wanted)
CASES = {
    "sc12_mid": (lambda: heisenberg(12), lambda H: SpinConserve(12, 6), 0.5, 10, True),
    "sc14_mid": (lambda: heisenberg(14), lambda H: SpinConserve(14, 7), 0.5, 16, True),
    "sc14_low": (lambda: heisenberg(14), lambda H: SpinConserve(14, 7), 0.2, 16, False),
    "full12": (lambda: heisenberg(12), lambda H: Full(12), 0.6, 12, True),
    "parity12": (lambda: heisenberg(12), lambda H: Parity('even', L=12), 0.5, 12, False),
    "sc16_mid": (lambda: heisenberg(16), lambda H: SpinConserve(16, 8), 0.5, 24, False),
    "xparity_sc12": (lambda: random_xxz(12), lambda H: XParity(SpinConserve(12, 6), '+'), 0.5, 8, False),
    "auto12": (lambda: heisenberg(12), auto_half_filling, 0.5, 10, False),
    "complex_sc12": (lambda: dm_chain(12), lambda H: SpinConserve(12, 6), 0.5, 10, True),
}


def dense(H, want_vectors):
    A = H.to_numpy(sparse=False)
    assert np.abs(A - A.conj().T).max() == 0.0
    if np.abs(A.imag).max() == 0.0:
        A = np.ascontiguousarray(A.real)
    nrm = np.abs(A).sum(axis=1).max()
    if want_vectors:
        w, U = np.linalg.eigh(A)
        return A, nrm, w, U
    return A, nrm, np.linalg.eigvalsh(A), None


def nearest(w, sigma, nev):
    """The nev reference values nearest sigma, after asserting that "the nev nearest" is unambiguous: the (nev+1)-th
    distance exceeds the nev-th by >= 1e-4 (a condition on the INPUT, 10^5 tol -- a bad seed fails here, loudly)."""
    d = np.sort(np.abs(w - sigma))
    assert d[nev] - d[nev - 1] >= 1e-4, (d[nev - 1], d[nev])
    return np.sort(w[np.argsort(np.abs(w - sigma))[:nev]])


def check_values(vals, w, sigma, nev, nrm):
    vals = np.asarray(vals)
    assert vals.size >= nev
    # (ii) ordered by |theta - sigma|
    assert np.all(np.diff(np.abs(vals - sigma)) >= 0.0)
    # (i) as a multiset the returned values contain all nev reference values nearest sigma: tol |H|_inf of the
    # solver's contract plus n eps |H|_inf, the backward error of the dense reference itself
    bound = TOL * nrm + w.size * EPS * nrm
    got = sorted(vals)
    worst = 0.0
    for r in nearest(w, sigma, nev):
        j = int(np.argmin([abs(g - r) for g in got]))
        worst = max(worst, abs(got[j] - r))
        assert abs(got[j] - r) <= bound, (r, got[j], bound)
        got.pop(j)
    return worst


def half_chain_entropy_dense(sub, L, col):
    from dynamite_amd.computations import dm_entanglement_entropy
    full = np.zeros(1 << L, dtype=complex)
    full[sub.idx_to_state(np.arange(col.size))] = col
    m = full.reshape(1 << (L - L // 2), 1 << (L // 2))
    return dm_entanglement_entropy(m.T @ m.conj())


@pytest.mark.parametrize("name", sorted(CASES))
def test_interior_pairs_against_dense(name):
    st = solve_and_check(name)
    assert st['real_arithmetic'] is False          # (at these sizes; test_real_arithmetic forces the packed handle)


@pytest.mark.parametrize("name", ["full12", "parity12"])
def test_real_arithmetic(monkeypatch, name):
    """The same solves on the real-packed handle (what eigsolve picks for real-symmetric operators from 2^23
    amplitudes on; forced here, with tiles small enough for a 2^11-element vector): every inner product real, the
    Rayleigh-Ritz step in H real symmetric, eigenvectors handed back as complex states."""
    monkeypatch.setenv("DNM_EIGS_REAL", "1")
    for k, v in (("DNM_TILE_BITS", "8"), ("DNM_LOG_ROWS", "2"), ("DNM_PLAN_MODE", "2"), ("DNM_GBITS", "3"), ("DNM_AMIN", "3")):
        monkeypatch.setenv(k, v)
    st = solve_and_check(name)
    assert st['real_arithmetic'] is True


def test_window_too_narrow_is_widened(monkeypatch, capfd):
    """A first window with too few levels (the estimated half-width times 0.2: about 3 levels where 10 are wanted): the
    solver finds those, sees that fewer than nev lie inside, widens the window and goes on from the directions it
    has -- same assertions as every other case, and the trace shows that the branch ran."""
    monkeypatch.setenv("DNM_EIGS_INTERIOR_WINDOW", "0.2")
    monkeypatch.setenv("DNM_KRYLOV_DEBUG", "1")
    st = solve_and_check("sc12_mid")
    trace = capfd.readouterr().err
    assert "window widened" in trace, trace[-2000:]
    assert st['its'] >= 3
    print(trace[-1500:])


def solve_and_check(name):
    mkH, mksub, frac, nev, want_vectors = CASES[name]
    H = mkH()
    sub = mksub(H)
    H.subspace = sub
    L = H.get_length()
    A, nrm, w, U = dense(H, want_vectors)
    sigma = round(float(w[0] + frac * (w[-1] - w[0])), 3)
    nearest(w, sigma, nev)                                   # the condition on the input, before the solver runs
    vals, vecs = H.eigsolve(nev=nev, target=sigma, interior='filter', getvecs=True, tol=TOL)
    from dynamite_amd.computations import eigsolve as _es
    st = _es.last_stats
    worst = check_values(vals, w, sigma, nev, nrm)
    print("%s: dim %d, sigma %.3f, %d pairs, %d restarts, %d multiplies, residual/|H| %.2e, max |E - E_dense| %.2e, real "
          "arithmetic %s" % (name, w.size, sigma, len(vals), st['its'], st['matvecs'], st['max_rel_residual'], worst,
                             st['real_arithmetic']))
    assert st['max_rel_residual'] <= TOL
    # (iii) residuals recomputed here with H.dot, and orthonormality of the returned vectors
    k = len(vecs)
    V = np.stack([v.to_numpy() for v in vecs], axis=1)
    for i, v in enumerate(vecs):
        assert v.subspace == sub
        r = H.dot(v).to_numpy() - vals[i] * V[:, i]
        assert np.linalg.norm(r) <= TOL * nrm + 100 * EPS * nrm, (i, np.linalg.norm(r))
    G = V.conj().T @ V
    assert np.max(np.abs(G - np.eye(k))) <= 100 * k * EPS, np.max(np.abs(G - np.eye(k)))
    # (iv) half-chain entanglement entropy of a returned vector against the dense eigenvector's, for a level whose
    # neighbours are >= 1e-4 away (the bar of test_mbl_script_flow)
    if want_vectors:
        done = False
        for i in range(nev):
            j = int(np.argmin(np.abs(w - vals[i])))
            if min(w[j] - w[j - 1] if j > 0 else 1.0, w[j + 1] - w[j] if j + 1 < w.size else 1.0) < 1e-4:
                continue
            s_dense = half_chain_entropy_dense(sub, L, U[:, j])
            s_got = vecs[i].entanglement_entropy(keep=range(L // 2))
            assert abs(s_got - s_dense) < 1e-7, (i, s_got, s_dense)
            done = True
            break
        assert done, "no isolated level among the wanted ones"
    H.destroy_mat()
    return st


def test_values_only_and_which_is_forced():
    """getvecs=False returns the values alone; `which` is overridden by the target as in the reference."""
    H = heisenberg(12)
    H.subspace = SpinConserve(12, 6)
    _, nrm, w, _ = dense(H, False)
    sigma = round(float(w[0] + 0.5 * (w[-1] - w[0])), 3)
    vals = H.eigsolve(nev=10, which='highest', target=sigma, interior='filter', tol=TOL)
    assert isinstance(vals, np.ndarray)
    check_values(vals, w, sigma, 10, nrm)
    with pytest.raises(RuntimeError):
        H.eigsolve(nev=2, target=sigma)                      # the keyword is the opt-in


def test_hook_path_single_process():
    """hooks->mult set: every multiply of the filter goes through the hook and the recurrence's terms are separate
    sweeps (what a partitioned run does).  The hook here wraps dnm_mat_mult of the same handle and the reductions
    are those of one rank; assertions (i) and (ii).  (Real rank processes with real reductions:
    tests/test_gpu_interior_ranks.py.)"""
    H = heisenberg(12)
    sub = SpinConserve(12, 6)
    H.subspace = sub
    _, nrm, w, _ = dense(H, False)
    nev = 10
    sigma = round(float(w[0] + 0.5 * (w[-1] - w[0])), 3)
    mat = H.get_mat(subspaces=(sub, sub))
    L = _lib.lib()
    calls = [0]

    def mult(ctx, x, y):
        calls[0] += 1
        return L.dnm_mat_mult(mat.handle, x, y, backend._stream())

    hooks = _lib.Hooks(None, _lib.MULT_FN(mult), _lib.REDUCE_FN(lambda ctx, buf, n: 0),
                       _lib.REDUCE_FN(lambda ctx, buf, n: 0))
    nev_max = 2 * nev
    evals = np.zeros(nev_max)
    stats = _lib.SolverStats()
    _lib.check(L.dnm_eigsolve_interior(mat.handle, mat.n_local, nev, sigma, TOL, 0, 0, 0, C.byref(hooks), nev_max,
                                       _lib.pf64(evals), None, C.byref(stats), backend._stream()))
    assert stats.reason == 1 and stats.nconv >= nev
    assert calls[0] >= stats.matvecs > 0
    check_values(evals[:stats.nconv], w, sigma, nev, nrm)


# ---- the fused row kernels -----------------------------------------------------------------------------------------

def nnn_chain(L, complex_terms):
    """The random-field chain plus next-nearest-neighbour couplings: masks of two NON-adjacent spins take the general
    column search of the SpinConserve row kernel (adjacent bonds its table look-up)."""
    H = heisenberg(L) + index_sum(0.15 * (sigmax(0) * sigmax(2) + sigmay(0) * sigmay(2)) + 0.05 * sigmaz(0) * sigmaz(2), size=L)
    if complex_terms:
        H = H + index_sum(0.1 * (sigmax(0) * sigmay(2) - sigmay(0) * sigmax(2)), size=L)
    return H


def nnn_xxz(L):
    return random_xxz(L) + index_sum(0.15 * (sigmax(0) * sigmax(2) + sigmay(0) * sigmay(2)), size=L)


def _fuse_cases():
    Hr, Hc = heisenberg(12), dm_chain(12)
    return {
        # L = 18 with the block kernel off: the unranking walks the positions above 16, and the masks are of all three
        # kinds the SpinConserve row kernel knows (adjacent bonds, general pairs, XParity's complemented masks)
        "sc18_nnn_real": (nnn_chain(18, False), SpinConserve(18, 9), 0),
        "sc18_nnn_complex": (nnn_chain(18, True), SpinConserve(18, 9), 0),
        "xparity_sc18_nnn": (nnn_xxz(18), XParity(SpinConserve(18, 9), '-'), 0),
        "sc18_gather": (nnn_chain(18, True), SpinConserve(18, 9), _lib.MAT_FORCE_GATHER),
        "explicit_real": (Hr, auto_half_filling(Hr), 0),
        "explicit_complex": (Hc, auto_half_filling(Hc), 0),
        "xparity_sc": (random_xxz(12), XParity(SpinConserve(12, 6), '+'), 0),
        "sc_row_real": (Hr, SpinConserve(12, 6), 0),
        "sc_row_complex": (Hc, SpinConserve(12, 6), 0),
        "sc_gather_real": (Hr, SpinConserve(12, 6), _lib.MAT_FORCE_GATHER),
        "sc_gather_complex": (Hc, SpinConserve(12, 6), _lib.MAT_FORCE_GATHER),
        "full_gather": (Hc, Full(10), _lib.MAT_FORCE_GATHER),
        "parity_gather": (Hr, Parity('odd', L=12), _lib.MAT_FORCE_GATHER),
    }


@pytest.mark.parametrize("name", ["explicit_real", "explicit_complex", "xparity_sc", "sc_row_real", "sc_row_complex",
                                  "sc_gather_real", "sc_gather_complex", "full_gather", "parity_gather",
                                  "sc18_nnn_real", "sc18_nnn_complex", "xparity_sc18_nnn", "sc18_gather"])
@pytest.mark.parametrize("diag", [False, True])
def test_row_kernels_fuse_start_vectors_and_sums(monkeypatch, name, diag):
    """dnm_mat_fuses_init == 1 for the one-thread-per-row handles on one rank, and dnm_mat_mult_sub2 /
    dnm_mat_mult_lanczos equal the unfused composition (the multiply, then the sweeps in numpy) to
    nnz_per_row * eps * 100 relative -- the suite's bar for multiplies against the oracle; the sums to the same bar."""
    monkeypatch.setenv("DNM_SC_BLOCK", "0")       # SpinConserve pairs on the row kernel at every size
    H, sub, flags = _fuse_cases()[name]
    if name == "full_gather":
        H = dm_chain(10)
    if isinstance(sub, XParity):            # the operator is rewritten for the sector: through the Operator
        H.subspace = sub
        mat = H.get_mat(subspaces=(sub, sub))
    else:
        mat = shell(H, sub, flags=flags)
    if diag:
        mat.precompute_diagonal()
    L = _lib.lib()
    assert L.dnm_mat_fuses_init(mat.handle) == 1, mat.describe()
    assert "block form" not in mat.describe() and "tiled=1" not in mat.describe(), mat.describe()
    n = mat.N
    rs = np.random.RandomState(11)
    x, z, z2 = (rs.standard_normal(n) + 1j * rs.standard_normal(n) for _ in range(3))
    xv, yv = mat.createVecs()
    xv.set_local_from_numpy(x)
    zv, z2v = vec_from(z, mat.swz_left, mat._keep[0] if mat.swz_left >= 256 else None), \
        vec_from(z2, mat.swz_left, mat._keep[0] if mat.swz_left >= 256 else None)
    yv.set(777.0)
    mat.mult(xv, yv)
    Hx = yv.local_numpy()
    nnz = len(np.unique(H.msc['masks']))
    bar = nnz * EPS * 100
    st = backend._stream()
    b, c = 0.37, complex(-0.4, 0.9)
    # the fused kernel with nothing to add is the plain kernel's twin: the same sums in the same order, bit for bit
    # (-0 * z leaves a sum as it is) -- a drift between the two copies of the row loops shows here
    yv.set(777.0)
    _lib.check(L.dnm_mat_mult_sub2(mat.handle, xv.ptr, yv.ptr, zv.ptr, 0.0, None, 0.0, 0.0, st))
    assert np.array_equal(yv.local_numpy(), Hx)
    # y = A x - b z + c z2
    yv.set(777.0)
    _lib.check(L.dnm_mat_mult_sub2(mat.handle, xv.ptr, yv.ptr, zv.ptr, b, z2v.ptr, c.real, c.imag, st))
    want = Hx - b * z + c * z2
    assert np.max(np.abs(yv.local_numpy() - want)) <= bar * np.max(np.abs(want))
    # y = A x - b z (no second vector)
    yv.set(777.0)
    _lib.check(L.dnm_mat_mult_sub2(mat.handle, xv.ptr, yv.ptr, zv.ptr, b, None, 0.0, 0.0, st))
    want = Hx - b * z
    assert np.max(np.abs(yv.local_numpy() - want)) <= bar * np.max(np.abs(want))
    # the Lanczos multiply: the same vector and the three sums
    for zz, bb in ((zv, b), (None, 0.0)):
        yv.set(777.0)
        dot = (C.c_double * 3)()
        _lib.check(L.dnm_mat_mult_lanczos(mat.handle, xv.ptr, yv.ptr, zz.ptr if zz is not None else None, bb, dot, st))
        want = Hx - bb * z
        assert np.max(np.abs(yv.local_numpy() - want)) <= bar * np.max(np.abs(want))
        scale = np.linalg.norm(x) * np.linalg.norm(want)
        assert abs(complex(dot[0], dot[1]) - np.vdot(x, want)) <= bar * scale
        assert abs(dot[2] - np.vdot(want, want).real) <= bar * np.vdot(want, want).real
    if not isinstance(sub, XParity):
        mat.destroy()
