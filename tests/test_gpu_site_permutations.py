"""
Site permutations of a state in one pass (csrc/perm_kernels.hip, csrc/perm_rank.h, csrc/observables.cpp: dnm_perm_apply,
dnm_perm_dots; backend.perm_apply / perm_dots; computations.permute_sites, symmetrize, symmetry_expectations,
symmetry_representation).

P_pi moves the spin at site i to site pi(i): (P_pi psi)(c') = psi(c) where the source configuration c has bit i equal to
bit pi(i) of c'.  The reference is numpy on the host: the configurations of the subspace (idx_to_state), the source of
each by a loop over the sites, its index (state_to_idx) and a gather; for a state on an XParity sector the global flip is
written out -- a source with bit L - 1 set is the sector's sign times the amplitude of its complement -- and sums run
over the representatives, with no factor 2.

Bounds, with u = 2^-53.  A pure permutation rounds nothing: bits are compared.  States with integer amplitudes in
[-3, 3] + i [-3, 3] and coefficients in {+-1, +-i} (times a power of two) make every product and every partial sum an
integer (a multiple of that power) far below 2^53: kernel and reference agree to the last bit in any summation order.
For random states:
  dots        an entry is a complex sum of `rows` products with sum |conj(a) b| <= |phi| |psi| (Cauchy-Schwarz: P psi is a
              permutation of psi); each real sum takes about rows + 2 roundings, sqrt 2 for the modulus, once for the
              kernel and once for the reference: 4 rows u |phi| |psi| -- the derivation of
              test_gpu_chirality_correlations.py.
  symmetrize  entry r is a sum of G products c_g x[p_g(r)] with |c_g| = w: a complex product is two real sums of two
              rounded products (3 roundings), the G - 1 additions add G - 1 more, sqrt 2 for the modulus, once for the
              kernel and once for the reference, so 2 sqrt 2 (G + 2) u w S(r) <= 4 (G + 1) u w S(r) for G >= 2, with S(r) =
              sum_g |x[p_g(r)]|; symmetrize has w = 1 / G (the division of a unit-modulus character by G adds one
              rounding to each coefficient on both sides alike: the same numbers enter kernel and reference).
"""
import numpy as np
import pytest

from dynamite_amd import backend, lattices
from dynamite_amd.computations import permute_sites, symmetrize, symmetry_expectations, symmetry_representation
from dynamite_amd.config import config
from dynamite_amd.operators import op_sum, sigmax, sigmay, sigmaz
from dynamite_amd.states import State
from dynamite_amd.subspaces import Auto, Explicit, Full, Parity, SpinConserve, XParity

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


# ---- subspaces ----------------------------------------------------------------------------------------------------
def _x(make, sector):
    return lambda: XParity(make(), sector=sector)


CASES = [
    pytest.param((lambda: Full(L=10), False), id="full10_swizzled"),
    pytest.param((lambda: Full(L=10), False), id="full10", marks=pytest.mark.default_layout),
    pytest.param((lambda: Parity('odd', L=11), False), id="parity11_odd"),
    pytest.param((lambda: Parity('even', L=12), False), id="parity12_even"),
    pytest.param((lambda: SpinConserve(12, 6), False), id="sc12_6"),
    pytest.param((lambda: SpinConserve(13, 4), False), id="sc13_4"),
    pytest.param((lambda: SpinConserve(34, 2), False), id="sc34_2"),
    pytest.param((_x(lambda: Full(L=10), '+'), False), id="x_full10_plus"),
    pytest.param((_x(lambda: Full(L=10), '-'), False), id="x_full10_minus"),
    pytest.param((_x(lambda: Parity('even', L=12), '+'), False), id="x_parity12_plus"),
    pytest.param((_x(lambda: Parity('even', L=12), '-'), False), id="x_parity12_minus"),
    pytest.param((_x(lambda: SpinConserve(12, 6), '+'), False), id="x_sc12_6_plus"),
    pytest.param((_x(lambda: SpinConserve(12, 6), '-'), False), id="x_sc12_6_minus"),
    pytest.param((lambda: SpinConserve(12, 6), True), id="sc12_6_internal"),
]


@pytest.fixture(params=CASES)
def sub(request):
    """The subspace of a case; the last one with the (6, 4) field split, so that the state lies in the internal layout
    (test_gpu_layout_handles.py)."""
    make, internal = request.param
    old = (config.sc_layout, config.sc_layout_min_dim)
    if internal:
        config.sc_layout, config.sc_layout_min_dim = (6, 4), 0
    yield make()
    config.sc_layout, config.sc_layout_min_dim = old


def is_internal_case(request):
    return request.node.callspec.id.endswith("internal")


# ---- reference ----------------------------------------------------------------------------------------------------
def perm_set(L):
    """Identity, a transposition with site L - 1, the reversal, the shifts by 1 and by L - 1, a three-cycle through
    L - 1, two seeded random ones: the set of tests/perm_rank_check.cpp."""
    h = L // 2
    ident = np.arange(L)
    swap = ident.copy()
    swap[[h, L - 1]] = [L - 1, h]
    cyc = ident.copy()
    cyc[[1, L - 1, h + 1]] = [L - 1, h + 1, 1]
    rng = np.random.default_rng(100 + L)
    return np.array([ident, swap, ident[::-1], (ident + 1) % L, (ident + L - 1) % L, cyc, rng.permutation(L),
                     rng.permutation(L)], dtype=np.int64)


def parent_of(sub):
    return (sub.parent, int(sub.sector)) if isinstance(sub, XParity) else (sub, 0)


def source(cfg, perm):
    """bit i of the source = bit perm[i] of cfg"""
    src = np.zeros_like(cfg)
    for i, p in enumerate(perm):
        src |= ((cfg >> np.int64(p)) & 1) << np.int64(i)
    return src


_GATHERS = {}


def gather_of(sub, perm):
    """(index, factor) of the source amplitude of every row of the vector."""
    key = (repr(sub), tuple(int(p) for p in perm))
    if key not in _GATHERS:
        parent, s = parent_of(sub)
        L, rows = parent.L, sub.get_dimension()
        cfg = np.asarray(parent.idx_to_state(np.arange(rows)), dtype=np.int64)
        src = source(cfg, perm)
        top = (((src >> np.int64(L - 1)) & 1) == 1) if s else np.zeros(rows, dtype=bool)
        idx = np.asarray(parent.state_to_idx(np.where(top, src ^ ((np.int64(1) << np.int64(L)) - 1), src)),
                         dtype=np.int64)
        assert np.all((idx >= 0) & (idx < rows))
        _GATHERS[key] = (idx, np.where(top, s, 1).astype(np.float64))
    return _GATHERS[key]


def permuted(sub, amps, perm):
    idx, factor = gather_of(sub, perm)
    return factor * amps[idx]


def expanded(sub, amps):
    """The amplitudes on the parent's basis: as they are, or x on the representatives and s x on their complements."""
    parent, s = parent_of(sub)
    if s == 0:
        return parent, amps
    dim = parent.get_dimension()
    cfg = np.asarray(parent.idx_to_state(np.arange(dim // 2)), dtype=np.int64)
    other = np.asarray(parent.state_to_idx(cfg ^ ((np.int64(1) << parent.L) - 1)), dtype=np.int64)
    psi = np.zeros(dim, dtype=np.complex128)
    psi[:dim // 2] = amps
    psi[other] = s * amps
    return parent, psi


def int_amplitudes(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-3, 4, n) + 1j * rng.integers(-3, 4, n)).astype(np.complex128)


def state_from(sub, amps):
    st = State(subspace=sub)
    st.vec.set_local_from_numpy(amps)
    st.set_initialized()
    return st


def compose(second, first):
    """The spin at i goes to first[i], then to second[first[i]]: P_second P_first = P_compose."""
    return np.asarray(second)[np.asarray(first)]


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def expectation(op, st):
    op.L = st.subspace.L
    op.add_subspace(st.subspace)
    return op.expectation(st)


# ---- a. a pure permutation is bit-exact -----------------------------------------------------------------------------
def test_pure_permutation_bit_for_bit(sub, request):
    st = State(subspace=sub, state='random', seed=11)
    assert st.vec.internal == is_internal_case(request)
    amps = st.to_numpy()
    out = State(subspace=sub)
    for perm in perm_set(sub.L):
        got = permute_sites(st, perm, result=out)
        assert got is out
        assert same_bits(out.to_numpy(), permuted(sub, amps, perm)), perm
    assert same_bits(st.to_numpy(), amps)
    fresh = st.permute_sites(perm_set(sub.L)[6])
    assert fresh is not st and fresh.subspace == st.subspace
    assert same_bits(fresh.to_numpy(), permuted(sub, amps, perm_set(sub.L)[6]))
    assert not same_bits(fresh.to_numpy(), amps)


# ---- b. composition and inverse -------------------------------------------------------------------------------------
def test_composition_and_inverse(sub):
    st = State(subspace=sub, state='random', seed=12)
    perms = perm_set(sub.L)
    for p1, p2 in ((perms[6], perms[7]), (perms[3], perms[5]), (perms[1], perms[2])):
        one = permute_sites(st, p1)
        both = permute_sites(one, p2)
        direct = permute_sites(st, compose(p2, p1))
        assert same_bits(both.to_numpy(), direct.to_numpy())
        back = permute_sites(one, np.argsort(p1))
        assert same_bits(back.to_numpy(), st.to_numpy())
    assert same_bits(permute_sites(st, perms[0]).to_numpy(), st.to_numpy())


# ---- c. operator covariance -----------------------------------------------------------------------------------------
def covariance_operator(sub, site):
    """An operator the subspace carries, on the sites ``site(i)``: sigmax_0 sigmay_3 + sigmaz_1 where nothing forbids it;
    on SpinConserve its U(1)-symmetric kin; on XParity one that commutes with the global flip too."""
    parent, s = parent_of(sub)
    a, b, c, d = site(0), site(3), site(1), site(2)
    if s:
        return op_sum([sigmax(a) * sigmax(b), sigmay(a) * sigmay(b), sigmaz(c) * sigmaz(d), 2 * sigmaz(a) * sigmaz(d)])
    if isinstance(parent, SpinConserve):
        return op_sum([sigmax(a) * sigmax(b), sigmay(a) * sigmay(b), sigmaz(c)])
    return op_sum([sigmax(a) * sigmay(b), sigmaz(c)])


def test_operator_covariance(sub):
    """P sigma_i P^H = sigma_pi(i): <P psi|O(pi(sites))|P psi> = <psi|O(sites)|psi> to the last bit on integer
    amplitudes.  This pins the direction of pi: with the inverse the sites would not match."""
    st = state_from(sub, int_amplitudes(sub.get_dimension(), 13))
    want = expectation(covariance_operator(sub, lambda i: i), st)
    checked = 0
    for perm in perm_set(sub.L)[1:]:
        moved = permute_sites(st, perm)
        got = expectation(covariance_operator(sub, lambda i: int(perm[i])), moved)
        assert got == want, (perm, got, want)
        inverse = np.argsort(perm)
        if not np.array_equal(inverse, perm):
            checked += expectation(covariance_operator(sub, lambda i: int(inverse[i])), moved) != want
    assert want != 0 and float(want).is_integer()
    assert checked >= 1        # the other direction is another number


# ---- d. symmetrize and symmetry_expectations, exact on integers ------------------------------------------------------
UNITS = np.array([1, -1, 1j, -1j, 1, 1j, -1, -1j], dtype=np.complex128)


def test_integer_amplitudes_bit_for_bit(sub):
    dim = sub.get_dimension()
    amps, other = int_amplitudes(dim, 14), int_amplitudes(dim, 15)
    st, ot = state_from(sub, amps), state_from(sub, other)
    perms = perm_set(sub.L)
    images = np.array([permuted(sub, amps, p) for p in perms])
    # eight permutations: the division by G is exact
    got = symmetrize(st, perms, UNITS)
    want = (UNITS.conj()[:, None] * images).sum(axis=0) / 8
    assert np.array_equal(got.to_numpy(), want)
    assert same_bits(symmetrize(st, perms, UNITS).to_numpy(), got.to_numpy())
    plain = st.symmetrize(perms)
    assert np.array_equal(plain.to_numpy(), images.sum(axis=0) / 8)
    e = symmetry_expectations(st, perms, other=ot)
    assert e.shape == (8,) and e.dtype == np.complex128
    assert np.array_equal(e, np.array([np.vdot(other, im) for im in images]))
    assert same_bits(symmetry_expectations(st, perms, other=ot), e)
    own = st.symmetry_expectations(perms)
    assert np.array_equal(own, np.array([np.vdot(amps, im) for im in images]))
    assert own[0] == np.vdot(amps, amps) and own[0].imag == 0
    D = symmetry_representation([st, ot], perms[:3])
    assert D.shape == (3, 2, 2)
    for g in range(3):
        im_s, im_o = permuted(sub, amps, perms[g]), permuted(sub, other, perms[g])
        assert np.array_equal(D[g], np.array([[np.vdot(amps, im_s), np.vdot(amps, im_o)],
                                              [np.vdot(other, im_s), np.vdot(other, im_o)]]))


# ---- e. random states -----------------------------------------------------------------------------------------------
def symmetrize_bound(sub, amps, perms, weight):
    S = np.sum([np.abs(permuted(sub, amps, p)) for p in perms], axis=0)
    return 4.0 * (len(perms) + 1) * U * weight * S


def test_random_states(sub):
    st = State(subspace=sub, state='random', seed=16)
    ot = State(subspace=sub, state='random', seed=17)
    amps, other = st.to_numpy(), ot.to_numpy()
    perms = perm_set(sub.L)
    G = len(perms)
    images = np.array([permuted(sub, amps, p) for p in perms])
    rows = sub.get_dimension()
    tol = 4.0 * rows * U * np.linalg.norm(amps) * np.linalg.norm(other)
    e = symmetry_expectations(st, perms, other=ot)
    err = np.max(np.abs(e - np.array([np.vdot(other, im) for im in images])))
    print("dots, %d rows: largest error %.3e (bound %.3e)" % (rows, err, tol))
    assert err <= tol
    chi = np.exp(-2j * np.pi * np.arange(G) * 3 / G)
    got = symmetrize(st, perms, chi).to_numpy()
    want = ((chi.conj() / G)[:, None] * images).sum(axis=0)
    bound = symmetrize_bound(sub, amps, perms, 1.0 / G)
    worst = np.max((np.abs(got - want) - bound))
    print("symmetrize, %d permutations: largest error %.3e (bound there %.3e)"
          % (G, np.max(np.abs(got - want)), bound[np.argmax(np.abs(got - want))]))
    assert worst <= 0
    # unit-modulus coefficients as they stand, and accumulation on top of a vector
    out = State(subspace=sub, state='random', seed=18)
    before = out.to_numpy()
    backend.perm_apply(st.vec, sub._to_c(), perms.astype(np.int32), chi, out.vec, parent_of(sub)[1], accumulate=True)
    diff = np.abs(out.to_numpy() - (before + (chi[:, None] * images).sum(axis=0)))
    assert np.all(diff <= symmetrize_bound(sub, amps, perms, 1.0) + 4.0 * U * np.abs(before))


# ---- f. more permutations than one call takes ---------------------------------------------------------------------
@pytest.mark.parametrize("G", [65, 129])
def test_chunks(G):
    """Chunks of 64: the expectations are exact on integers whatever the cut; the sum over the chunks is held to the
    bound of a sum of G terms."""
    sub = Full(L=8)
    rng = np.random.default_rng(G)
    perms = np.array([rng.permutation(8) for _ in range(G)])
    amps, other = int_amplitudes(256, 19), int_amplitudes(256, 20)
    st, ot = state_from(sub, amps), state_from(sub, other)
    images = np.array([permuted(sub, amps, p) for p in perms])
    e = symmetry_expectations(st, perms, other=ot)
    assert e.shape == (G,)
    assert np.array_equal(e, np.array([np.vdot(other, im) for im in images]))
    chi = 1j ** rng.integers(0, 4, G)
    got = symmetrize(st, perms, chi).to_numpy()
    want = ((chi.conj() / G)[:, None] * images).sum(axis=0)
    assert np.all(np.abs(got - want) <= symmetrize_bound(sub, amps, perms, 1.0 / G))
    assert np.max(np.abs(want)) > 0.1


# ---- g. the three-site rotations of the chirality pass ---------------------------------------------------------------
@pytest.mark.parametrize("make", [pytest.param(lambda: SpinConserve(12, 6), id="sc12_6"),
                                  pytest.param(lambda: Full(L=12), id="full12"),
                                  pytest.param(lambda: XParity(SpinConserve(12, 6), sector='-'), id="x_sc12_6_minus")])
def test_three_cycles_are_the_rotations_of_the_chirality_pass(make):
    """<C_m> of backend.cyc_moments, row 0 of its matrix, is <psi|P_pi|psi> for pi(a) = b, pi(b) = c, pi(c) = a."""
    sub = make()
    triangles = lattices.kagome_triangles('12')
    perms = np.tile(np.arange(12), (len(triangles), 1))
    for m, (a, b, c) in enumerate(triangles):
        perms[m, [a, b, c]] = [b, c, a]
    st = state_from(sub, int_amplitudes(sub.get_dimension(), 21))
    G = backend.cyc_moments(st.vec, sub._to_c(), triangles, parent_of(sub)[1])
    e = symmetry_expectations(st, perms)
    assert np.array_equal(e, G[0, 1:])
    assert np.any(e.imag != 0)


# ---- h. projectors onto momenta -------------------------------------------------------------------------------------
def test_momentum_projectors():
    """P_k = (1 / 8) sum_g conj(chi_k(g)) T^g with chi_k(g) = exp(-2 pi i k g / 8) on a random normalised state of
    SpinConserve(8, 4), 70 rows.  By (e) a computed P_k psi differs from the exact one by d_k with |d_k| <= c |psi|, c = (4
    (G + 1) + 2) u: the bound of symmetrize, in the 2-norm ((1 / G) sum_g |psi o p_g| has the norm of psi at most), and 2 u
    for the characters, which are rounded cosines and sines.  ||P_k|| <= 1, T P_k = chi_k(1) P_k.  With N = |psi|:
      sum_k P_k psi = psi             | sum - psi |        <= 8 c N + 8 u sum_k |P_k psi| <= (8 c + 32 u) N  (summed in numpy)
      P_k P_k psi = P_k psi           | P_k f - f |        <= 2 |d_k| + c |f|            <= 4 c N            (f = computed P_k psi)
      <P_k psi|P_k' psi> = 0          | <f|f'> |           <= 2 c N^2 + c^2 N^2 + 4 rows u N^2
      <f|T|f> = chi_k(1) <f|f>        | difference |       <= |f| 2 |d_k| + 2 * 4 rows u |f|^2 + 4 u |f|^2
                                                           <= (2 c + 8 rows u + 4 u) N^2
    (the dots of numpy and of the pass to 4 rows u each, as in (e))."""
    sub = SpinConserve(8, 4)
    rows = sub.get_dimension()
    assert rows == 70
    T = lattices.chain_translations(8)
    G = 8
    st = State(subspace=sub, state='random', seed=22)
    psi = st.to_numpy()
    N = np.linalg.norm(psi)
    c = (4 * (G + 1) + 2) * U
    chi = [np.exp(-2j * np.pi * k * np.arange(G) / G) for k in range(G)]
    proj = [symmetrize(st, T, chi[k]) for k in range(G)]
    f = [p.to_numpy() for p in proj]
    total = np.linalg.norm(np.sum(f, axis=0) - psi)
    print("sum of the projections: %.3e (bound %.3e)" % (total, (8 * c + 32 * U) * N))
    assert total <= (8 * c + 32 * U) * N
    worst_idem = worst_orth = worst_eig = 0.0
    for k in range(G):
        twice = symmetrize(proj[k], T, chi[k]).to_numpy()
        worst_idem = max(worst_idem, np.linalg.norm(twice - f[k]))
        for k2 in range(k + 1, G):
            worst_orth = max(worst_orth, abs(np.vdot(f[k], f[k2])))
        t = symmetry_expectations(proj[k], [T[1]])[0]
        worst_eig = max(worst_eig, abs(t - chi[k][1] * np.vdot(f[k], f[k])))
    print("idempotent %.3e (bound %.3e), orthogonal %.3e (bound %.3e), eigenvalue %.3e (bound %.3e)"
          % (worst_idem, 4 * c * N, worst_orth, (2 * c + c * c + 4 * rows * U) * N * N, worst_eig,
             (2 * c + 8 * rows * U + 4 * U) * N * N))
    assert worst_idem <= 4 * c * N
    assert worst_orth <= (2 * c + c * c + 4 * rows * U) * N * N
    assert worst_eig <= (2 * c + 8 * rows * U + 4 * U) * N * N
    # the state has weight in more than one momentum
    assert sum(np.linalg.norm(v) > 1e-3 for v in f) >= 4


# ---- i. known answer: the Heisenberg ring ---------------------------------------------------------------------------
EIG_TOL = 1e-10
RING = {10: (-18.0617854, -1.0), 12: (-21.5495637, +1.0)}


def heisenberg_ring(L):
    return op_sum([s(i) * s((i + 1) % L) for i in range(L) for s in (sigmax, sigmay, sigmaz)])


@pytest.mark.parametrize("L", [10, 12])
def test_heisenberg_ring_ground_state(L):
    """The ground state of sum_i sigma_i . sigma_{i+1} on a ring of L sites in SpinConserve(L, L / 2) is non-degenerate
    (exact diagonalisation in numpy: E0 = -18.0617854 at L = 10 and -21.5495637 at L = 12, gaps 1.69 and 1.42) and an
    eigenstate of the translation by one site and of the reflection with eigenvalue -1 at L = 10 and +1 at L = 12 (a
    singlet of L / 2 odd resp. even).  With the vector's error |d| <= residual / gap and a normalised state, |<T> -+ 1|
    <= 2 |d|^2: 1e-8 is far inside what tol 1e-10 |E0| gives."""
    e0_want, sign = RING[L]
    saved = config.L
    try:
        config.L = L
        sub = SpinConserve(L, L // 2)
        H = heisenberg_ring(L)
        H.L = L
        H.add_subspace(sub)
        ev, vecs = H.eigsolve(nev=1, tol=EIG_TOL, getvecs=True, subspace=sub)
        H.destroy_mat()
        gs = vecs[0]
        n = gs.dot(gs).real
        t, r = symmetry_expectations(gs, [lattices.chain_translations(L)[1], lattices.chain_reflection(L)]) / n
    finally:
        config.L = saved
    assert abs(ev[0] - e0_want) < 1e-6
    print("L = %d: E0 = %.10f, <T> = %r, <R> = %r" % (L, ev[0], t, r))
    assert abs(t - sign) <= 1e-8 and abs(r - sign) <= 1e-8


@pytest.mark.parametrize("L", [10, 12])
def test_heisenberg_ring_xparity_multiplets(L):
    """The two lowest states of each XParity sector of the ring: D[g, m, n] = <m|P_g|n> for the translation by one site,
    that by three and the reflection, against numpy on the vectors expanded to the parent (x on the representatives, s x
    on their complements: sqrt 2 times the sector's state, so the parent's sums are halved, which is exact).  Bound: that
    of a dot of (e) for the 2 rows of the expanded sum, 4 (2 rows) u |m| |n|.  The lowest of the four is the ground state
    of the ring, with the eigenvalues of test_heisenberg_ring_ground_state."""
    perms = np.array([lattices.chain_translations(L)[1], lattices.chain_translations(L)[3], lattices.chain_reflection(L)])
    saved = config.L
    found = []
    try:
        config.L = L
        H = heisenberg_ring(L)
        H.L = L
        for sector in ('+', '-'):
            sub = XParity(SpinConserve(L, L // 2), sector=sector)
            H.add_subspace(sub)
            ev, vecs = H.eigsolve(nev=2, tol=EIG_TOL, getvecs=True, subspace=sub)
            D = symmetry_representation(vecs[:2], perms)
            found.append((sub, ev[:2], [v.to_numpy() for v in vecs[:2]], D))
        H.destroy_mat()
    finally:
        config.L = saved
    lowest = None
    for sub, ev, amps, D in found:
        assert D.shape == (3, 2, 2)
        rows = sub.get_dimension()
        parent, _ = parent_of(sub)
        big = [expanded(sub, a)[1] for a in amps]
        for g, perm in enumerate(perms):
            for m in range(2):
                for n in range(2):
                    want = np.vdot(big[m], permuted(parent, big[n], perm)) / 2
                    tol = 4.0 * 2 * rows * U * np.linalg.norm(amps[m]) * np.linalg.norm(amps[n])
                    assert abs(D[g, m, n] - want) <= tol, (sub, g, m, n, D[g, m, n], want, tol)
        if lowest is None or ev[0] < lowest[0]:
            lowest = (ev[0], D[:, 0, 0] / np.vdot(amps[0], amps[0]).real)
    e0_want, sign = RING[L]
    assert abs(lowest[0] - e0_want) < 1e-6
    # T, T^3, R on the ground state: sign, sign^3, sign
    assert np.all(np.abs(lowest[1] - sign) <= 1e-8)


# ---- j. refusals through Python -------------------------------------------------------------------------------------
def test_refusals():
    st = State(subspace=Full(L=8), state='random', seed=1)
    ident = np.arange(8)
    with pytest.raises(ValueError, match='another state'):
        permute_sites(st, ident, result=st)
    with pytest.raises(ValueError, match='another state'):
        symmetrize(st, [ident, ident[::-1]], result=st)
    with pytest.raises(ValueError, match='must match'):
        permute_sites(st, ident, result=State(subspace=Parity('even', L=8)))
    rng = np.random.default_rng(5)
    states = np.unique(rng.integers(0, 1 << 12, 300, dtype=np.int64))
    ex = State(subspace=Explicit(states, L=12), state='random', seed=1)
    for call in (lambda: permute_sites(ex, np.arange(12)), lambda: symmetrize(ex, [np.arange(12)]),
                 lambda: symmetry_expectations(ex, [np.arange(12)]), lambda: symmetry_representation([ex], [np.arange(12)])):
        with pytest.raises(ValueError, match='Explicit'):
            call()
    saved = config.L
    try:
        config.L = 8
        H = op_sum([sigmax(i) * sigmax(i + 1) + sigmay(i) * sigmay(i + 1) for i in range(7)])
        H.L = 8
        auto = State(subspace=Auto(H, 'UUUUDDDD'), state='random', seed=1)
    finally:
        config.L = saved
    with pytest.raises(ValueError, match='Auto|Explicit'):
        permute_sites(auto, ident)
    for bad in (np.arange(7), np.arange(9)):
        with pytest.raises(ValueError, match='length'):
            permute_sites(st, bad)
        with pytest.raises(ValueError, match='length'):
            symmetry_expectations(st, [bad])
    with pytest.raises(ValueError, match='one-dimensional'):
        permute_sites(st, [ident, ident])
    for bad in ([0, 1, 2, 3, 4, 5, 6, 6], [0, 1, 2, 3, 4, 5, 6, 8], [-1, 1, 2, 3, 4, 5, 6, 7]):
        with pytest.raises(ValueError, match='repeated site'):
            permute_sites(st, bad)
        with pytest.raises(ValueError, match='permutation 1 is not a bijection'):
            symmetrize(st, [ident, bad])
        with pytest.raises(ValueError, match='repeated site'):
            symmetry_expectations(st, [bad])
    with pytest.raises(ValueError, match='empty'):
        symmetry_expectations(st, [])
    with pytest.raises(ValueError, match='characters'):
        symmetrize(st, [ident, ident[::-1]], characters=[1, 1, 1])
    with pytest.raises(ValueError, match='same subspace'):
        symmetry_expectations(st, [ident], other=State(subspace=Parity('even', L=8), state='random', seed=2))
    # the C ABI below the Python checks
    with pytest.raises(RuntimeError, match='permutations'):
        backend.perm_dots(st.vec, st.vec, st.subspace._to_c(), np.tile(ident, (65, 1)))
    with pytest.raises(RuntimeError, match='bijection'):
        backend.perm_dots(st.vec, st.vec, st.subspace._to_c(), [[0, 0, 2, 3, 4, 5, 6, 7]])
    out = State(subspace=Full(L=8))
    with pytest.raises(ValueError, match='another vector'):
        backend.perm_apply(st.vec, st.subspace._to_c(), [ident], [1], st.vec)
    with pytest.raises(ValueError, match='coefficients'):
        backend.perm_apply(st.vec, st.subspace._to_c(), [ident], [1, 1], out.vec)
