"""
All scalar-chirality correlators of a list of triangles in one matrix-core pass (csrc/cyc_kernels.hip, csrc/cyc_rank.h,
csrc/gram_tile.h, csrc/observables.cpp: dnm_cyc_moments; backend.cyc_moments, computations.chirality_correlations).

The reference is numpy on the host, in the scheme of test_gpu_bond_correlations.py: the configurations of the subspace,
the operand matrix A[:, 0] = psi, A[:, 1 + m] = psi gathered through state_to_idx of the configurations with the bits of
the triple rotated (bit a from b, bit b from c, bit c from a), and G = A^H A.  For a state on an XParity sector the
reference does not use the kernel's flip logic: the amplitudes are expanded to the parent (x on the representatives, s x
on their complements), the parent's G of that vector is taken and halved -- the expanded vector is sqrt 2 times the
sector's state, and halving is exact.  States with integer amplitudes in [-3, 3] + i [-3, 3] make every product an
integer of modulus <= 18 and every sum an integer below 2^53: kernel and reference must then agree to the last bit in
any summation order.  Random states are held to e = 4 rows 2^-53 <psi|psi> per entry of G: an entry is a complex sum of
`rows` products with sum |conj(a) b| <= <psi|psi> (every column of A is a permutation of the state: Cauchy-Schwarz), each
real sum takes about rows + 2 roundings, sqrt 2 for the modulus, once for the kernel and once for the reference.  chi is
a combination of entries of G with moduli of the coefficients 2 + 2, cc with 4 + 4 + 4 + 4: their bounds are 4 e and 16 e.
"""
import numpy as np
import pytest

from dynamite_amd import backend, lattices
from dynamite_amd.computations import chirality_correlations
from dynamite_amd.config import config
from dynamite_amd.operators import op_sum, sigmax, sigmay, sigmaz
from dynamite_amd.states import State
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve, XParity

pytestmark = pytest.mark.gpu


# ---- reference ----------------------------------------------------------------------------------------------------
def rotated(cfg, a, b, c):
    """bit a <- bit b, bit b <- bit c, bit c <- bit a"""
    xa, xb, xc = (cfg >> a) & 1, (cfg >> b) & 1, (cfg >> c) & 1
    one = np.int64(1)
    return (cfg & ~((one << a) | (one << b) | (one << c))) | (xb << a) | (xc << b) | (xa << c)


def parent_of(sub):
    return (sub.parent, int(sub.sector)) if isinstance(sub, XParity) else (sub, 0)


def expanded(sub, amps):
    """The amplitudes on the parent's basis: as they are, or x on the representatives and s x on their complements."""
    parent, s = parent_of(sub)
    if s == 0:
        return parent, amps
    dim = parent.get_dimension()
    assert amps.size * 2 == dim
    cfg = np.asarray(parent.idx_to_state(np.arange(dim // 2)), dtype=np.int64)
    assert not np.any((cfg >> (parent.L - 1)) & 1)
    other = np.asarray(parent.state_to_idx(cfg ^ ((np.int64(1) << parent.L) - 1)), dtype=np.int64)
    assert np.array_equal(np.sort(other), np.arange(dim // 2, dim))
    psi = np.zeros(dim, dtype=np.complex128)
    psi[:dim // 2] = amps
    psi[other] = s * amps
    return parent, psi


def reference(sub, amps, cycles):
    """(G, rows of the sweep) for the amplitudes of the whole vector."""
    parent, psi = expanded(sub, np.asarray(amps, dtype=np.complex128))
    dim = parent.get_dimension()
    cfg = np.asarray(parent.idx_to_state(np.arange(dim)), dtype=np.int64)
    A = np.empty((dim, len(cycles) + 1), dtype=np.complex128)
    A[:, 0] = psi
    for m, (a, b, c) in enumerate(cycles):
        idx = np.asarray(parent.state_to_idx(rotated(cfg, int(a), int(b), int(c))), dtype=np.int64)
        assert np.all(idx >= 0)
        A[:, 1 + m] = psi[idx]
    G = A.conj().T @ A
    if parent is not sub:
        return G / 2, dim // 2
    return G, dim


def both_senses(triangles):
    """The columns chirality_correlations asks for: (a, b, c) at 1 + 2 t, (a, c, b) at 2 + 2 t."""
    out = []
    for a, b, c in triangles:
        out += [(a, b, c), (a, c, b)]
    return out


def from_gram(G):
    """(chi, cc) of chirality_correlations from the G of both_senses, the same formulas: exact on integers."""
    chi = -2.0 * (G[0, 1::2].imag - G[0, 2::2].imag)
    cc = 4.0 * ((G[1::2, 1::2] + G[2::2, 2::2]) - (G[1::2, 2::2] + G[2::2, 1::2]))
    return chi, cc


def int_amplitudes(n, seed, real=False):
    rng = np.random.default_rng(seed)
    re, im = rng.integers(-3, 4, n), rng.integers(-3, 4, n)
    return (re + (0 if real else 1j) * im).astype(np.complex128)


def state_from(sub, amps):
    st = State(subspace=sub)
    lo, hi = st.vec.getOwnershipRange()
    st.vec.set_local_from_numpy(amps[lo:hi])
    st.set_initialized()
    return st


def moments(st, cycles):
    return backend.cyc_moments(st.vec, st.subspace._to_c(), cycles, parent_of(st.subspace)[1])


def tolerance(rows, norm2):
    return 4.0 * rows * 2.0 ** -53 * norm2


def expectation(op, st):
    op.L = st.subspace.L
    op.add_subspace(st.subspace)
    return op.expectation(st)


def random_triples(L, n, seed, must=()):
    rng = np.random.default_rng(seed)
    out = [tuple(p) for p in must]
    while len(out) < n:
        out.append(tuple(int(v) for v in rng.choice(L, size=3, replace=False)))
    return out[:n]


@pytest.fixture
def small_layout():
    """(6, 4) field split for every SpinConserve subspace with L >= 11, whatever its dimension (test_gpu_sc3.py)."""
    old = (config.sc_layout, config.sc_layout_min_dim)
    config.sc_layout, config.sc_layout_min_dim = (6, 4), 0
    yield
    config.sc_layout, config.sc_layout_min_dim = old


def hermitian_to_the_last_bit(P):
    return np.array_equal(P, P.conj().T) and np.array_equal(np.diag(P).imag, np.zeros(P.shape[0]))


# ---- 1. convention ------------------------------------------------------------------------------------------------
def chi_op(a, b, c):
    """sigma_a . (sigma_b x sigma_c) = sum eps_{alpha beta gamma} sigma^alpha_a sigma^beta_b sigma^gamma_c"""
    s = (sigmax, sigmay, sigmaz)
    even, odd = ((0, 1, 2), (1, 2, 0), (2, 0, 1)), ((0, 2, 1), (2, 1, 0), (1, 0, 2))
    return op_sum([s[i](a) * s[j](b) * s[k](c) for i, j, k in even] + [-1 * s[i](a) * s[j](b) * s[k](c) for i, j, k in odd])


# share two sites, none, one; the last is the first in the other sense
FIVE = [(0, 1, 2), (2, 1, 3), (3, 4, 5), (5, 0, 3), (0, 2, 1)]


@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=6), id="full6"),
                                  pytest.param(lambda: SpinConserve(6, 3), id="sc6_3"),
                                  pytest.param(lambda: XParity(SpinConserve(6, 3), sector='+'), id="x_sc6_3")])
def test_convention_is_that_of_expectation(make):
    """chi[t] is <sigma_a . (sigma_b x sigma_c)> and cc[t, t'] is <chi_t chi_t'> as Operator.expectation defines them.
    expectation builds Hermitian operators only, so the product is taken in its two Hermitian parts, (X Y + Y X) / 2 and
    -i (X Y - Y X) / 2; where the two triangles have the same sites or share none they commute, the second part is the
    zero operator and its expectation value is 0 without a call.  The lower triangle is the conjugate of the upper to
    the last bit.  Bounds: 4 e for chi, 16 e for cc, the sums of the moduli of the coefficients."""
    sub = make()
    st = State(subspace=sub, state='random', seed=7)
    chi, cc = chirality_correlations(st, FIVE)
    n = len(FIVE)
    assert chi.shape == (n,) and chi.dtype == np.float64 and cc.shape == (n, n) and cc.dtype == np.complex128
    rows = sub.get_dimension()
    norm2 = st.dot(st).real
    tol = tolerance(rows, norm2)
    G = moments(st, both_senses(FIVE))
    N = G[0, 0].real                      # (<psi|psi> as the pass sums it)
    assert abs(N - norm2) <= tol
    worst_chi = worst_cc = worst_id = 0.0
    for t, tri in enumerate(FIVE):
        worst_chi = max(worst_chi, abs(chi[t] - expectation(chi_op(*tri), st)))
        # chi^2 = 12 on the two doublets, 0 on the quartet: 8 - 8 Re C
        worst_id = max(worst_id, abs(cc[t, t] - (8.0 * N - 8.0 * G[0, 1 + 2 * t].real)))
        for t2 in range(t, n):
            other = FIVE[t2]
            X, Y = chi_op(*tri), chi_op(*other)
            re = expectation(0.5 * (X * Y + Y * X), st)
            im = 0.0
            if 1 <= len(set(tri) & set(other)) <= 2:
                im = expectation(-0.5j * (X * Y - Y * X), st)
            worst_cc = max(worst_cc, abs(cc[t, t2] - (re + 1j * im)))
    print("convention: chi %.3e (bound %.3e), cc %.3e (bound %.3e), cc[t, t] = 8 N - 8 Re <C_t> %.3e"
          % (worst_chi, 4 * tol, worst_cc, 16 * tol, worst_id))
    assert worst_chi <= 4 * tol and worst_cc <= 16 * tol
    assert worst_id <= (16 + 8 + 8) * tol
    assert np.array_equal(cc, cc.conj().T)
    # the other sense of a triangle is minus its chirality, to the last bit
    assert chi[4] == -chi[0] and np.array_equal(cc[4], -cc[0]) and cc[4, 4] == cc[0, 0]
    chi2, cc2 = st.chirality_correlations(FIVE)
    assert np.array_equal(chi, chi2) and np.array_equal(cc, cc2)
    chic, ccc = chirality_correlations(st, FIVE, connected=True)
    assert np.array_equal(chic, chi) and np.array_equal(ccc, cc / N - np.outer(chi, chi) / N ** 2)
    wchi, wcc = from_gram(G)
    assert np.array_equal(chi, wchi) and np.array_equal(cc, wcc)


# ---- 2. exact arithmetic ------------------------------------------------------------------------------------------
def check_exact(sub, cycles, seed=3, real=False):
    dim = sub.get_dimension()
    amps = int_amplitudes(dim, seed, real)
    if dim == 1:
        amps[:] = 2 - 3j
    st = state_from(sub, amps)
    G = moments(st, cycles)
    want, _ = reference(sub, amps, cycles)
    n = len(cycles)
    assert G.shape == (n + 1, n + 1) and G.dtype == np.complex128
    assert np.array_equal(G, want), np.argwhere(G != want)[:8]
    assert hermitian_to_the_last_bit(G)
    assert np.array_equal(np.diag(G), np.full(n + 1, G[0, 0]))
    return st, G, amps


def check_exact_triangles(sub, triangles, seed=3, real=False):
    """The pass on both senses of the triangles, and chi, cc through the public function."""
    st, G, amps = check_exact(sub, both_senses(triangles), seed, real)
    chi, cc = chirality_correlations(st, triangles)
    wchi, wcc = from_gram(G)
    assert np.array_equal(chi, wchi) and np.array_equal(cc, wcc)
    assert np.array_equal(cc, cc.conj().T)
    assert np.array_equal(np.diag(cc), 8.0 * G[0, 0] - 8.0 * G[0, 1::2].real)
    return st, G, chi, cc


def test_integer_amplitudes_partial_panel():
    check_exact_triangles(Full(L=4), [(0, 1, 2), (1, 2, 3), (3, 0, 1), (2, 3, 0), (1, 3, 0)])


TILE_ROWS = [(15, 15), (15, 16), (15, 63), (16, 15), (16, 16), (16, 47), (16, 48), (16, 63), (17, 15), (17, 16), (17, 63)]


@pytest.mark.parametrize("L,n", TILE_ROWS, ids=["full%d_n%d" % c for c in TILE_ROWS])
def test_integer_amplitudes_tile_rows(L, n):
    """n + 1 = 16, 17, 48, 49, 64 columns: NB = 1, 2, 3, 4 with the last tile row full and with one column in it."""
    sub = Full(L=L)
    cycles = random_triples(L, n, 100 * L + n, must=[(0, L - 1, 1), (L - 1, 1, 0), (0, 1, 2), (5, 4, 3), (7, 6, L - 1),
                                                     (3, 9, 0)])
    assert backend.cyc_moments_plan(sub._to_c()['data'], n)[0] == -(-(n + 1) // 16)
    check_exact(sub, cycles)


@pytest.mark.default_layout
def test_integer_amplitudes_production_layout():
    """Full(20) as it lies in the default layout: triples inside the low bits, straddling bit 16 and above it."""
    st, _, _, _ = check_exact_triangles(Full(L=20), [(0, 1, 2), (2, 9, 5), (4, 15, 3), (3, 16, 8), (15, 16, 17),
                                                     (5, 19, 16), (16, 17, 18), (17, 19, 18), (19, 0, 16)])
    assert st.vec.swz == 16


EXACT = [
    pytest.param(lambda: Parity('even', L=17), id="parity17_even"),
    pytest.param(lambda: Parity('odd', L=17), id="parity17_odd"),
    pytest.param(lambda: SpinConserve(16, 8), id="sc16_8"),
    pytest.param(lambda: SpinConserve(34, 2), id="sc34_2"),
    pytest.param(lambda: SpinConserve(12, 12), id="sc12_12"),
    pytest.param(lambda: SpinConserve(12, 0), id="sc12_0"),
    pytest.param(lambda: XParity(Full(L=10), sector='+'), id="x_full10_plus"),
    pytest.param(lambda: XParity(Full(L=10), sector='-'), id="x_full10_minus"),
    pytest.param(lambda: XParity(Parity('even', L=12), sector='+'), id="x_parity12_plus"),
    pytest.param(lambda: XParity(Parity('even', L=12), sector='-'), id="x_parity12_minus"),
    pytest.param(lambda: XParity(SpinConserve(12, 6), sector='+'), id="x_sc12_6_plus"),
    pytest.param(lambda: XParity(SpinConserve(12, 6), sector='-'), id="x_sc12_6_minus"),
]


def triangles_at_the_edges(L, seed):
    """Site 0 (the spin Parity's index does not hold) and site L - 1 (the complement under XParity) in each place of a
    triple, above site 31 where there is one, adjacent and far, one repeat."""
    return random_triples(L, 10, seed, must=[(0, 1, 2), (5, 0, L - 1), (0, L - 1, 3), (L - 1, 3, 0), (L - 2, L - 1, L - 3),
                                            (L - 1, L // 2, 1), (L - 3, 2, L - 1), (0, 1, 2)])


@pytest.mark.parametrize("make", EXACT)
def test_integer_amplitudes_bit_for_bit(make):
    sub = make()
    st, G, _, _ = check_exact_triangles(sub, triangles_at_the_edges(sub.L, 7 * sub.L))
    if isinstance(sub, SpinConserve):
        assert not st.vec.internal
    if sub.get_dimension() == 1:
        assert np.array_equal(G, np.full((21, 21), 13.0 + 0j))


def test_integer_amplitudes_internal_layout(small_layout):
    """A SpinConserve state in the internal layout is converted to reference order on the way in."""
    st, _, _, _ = check_exact_triangles(SpinConserve(12, 6), triangles_at_the_edges(12, 5))
    assert st.vec.internal


@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=12), id="full12"),
                                  pytest.param(lambda: SpinConserve(12, 6), id="sc12_6"),
                                  pytest.param(lambda: XParity(SpinConserve(12, 6), sector='-'), id="x_sc12_6_minus")])
def test_a_real_state_has_no_chirality(make):
    """Real integer amplitudes: every <C_t> is real, chi is exactly 0 and cc exactly real."""
    sub = make()
    _, G, chi, cc = check_exact_triangles(sub, triangles_at_the_edges(12, 31), seed=17, real=True)
    assert np.array_equal(G.imag, np.zeros(G.shape))
    assert np.array_equal(chi, np.zeros(chi.shape))
    assert np.array_equal(cc.imag, np.zeros(cc.shape))
    assert np.any(cc.real != 0)


# ---- 3. random states ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=18), id="full18"),
                                  pytest.param(lambda: Parity('odd', L=18), id="parity18"),
                                  pytest.param(lambda: SpinConserve(18, 9), id="sc18_9"),
                                  pytest.param(lambda: XParity(SpinConserve(18, 9), sector='-'), id="x_sc18_9")])
def test_random_states(make):
    sub = make()
    triangles = random_triples(18, 30, 11, must=[(0, 17, 5), (17, 5, 0), (0, 1, 2), (15, 16, 17)])
    cycles = both_senses(triangles)
    st = State(subspace=sub, state='random', seed=9)
    G = moments(st, cycles)
    amps = st.to_numpy()
    want, rows = reference(sub, amps, cycles)
    tol = tolerance(rows, np.vdot(amps, amps).real)
    err = np.max(np.abs(G - want))
    print("random state, %d rows, 30 triangles: largest error %.3e (bound %.3e)" % (rows, err, tol))
    assert err <= tol
    assert hermitian_to_the_last_bit(G)


# ---- 4. determinism, a planted amplitude --------------------------------------------------------------------------
@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=17), id="full17"),
                                  pytest.param(lambda: SpinConserve(16, 8), id="sc16_8")])
def test_two_calls_and_a_planted_amplitude(make):
    sub = make()
    L, dim = sub.L, sub.get_dimension()
    cycles = random_triples(L, 20, 13, must=[(0, L - 1, 1), (L - 1, 1, 0), (L - 1, L - 2, L - 3), (0, 1, 2), (0, 1, 2),
                                             (0, 2, 1)])
    st = State(subspace=sub, state='random', seed=5)
    assert moments(st, cycles).tobytes() == moments(st, cycles).tobytes()
    # one amplitude 1 + 2i in the last panel of the sweep (Full: third from the end; SpinConserve: the last index):
    # column 1 + m of A then holds it in the row whose rotation is that configuration -- the configuration rotated the
    # other way round, (a, c, b)
    st = State(subspace=sub)
    st.set_initialized()
    idx = dim - 3 if isinstance(sub, Full) else dim - 1
    st.vec.set(0)
    st.vec.array[st.vec.positions(int(idx))] = 1 + 2j
    cfg = int(sub.idx_to_state(idx))
    lands = [cfg] + [int(rotated(np.int64(cfg), a, c, b)) for a, b, c in cycles]
    want = np.array([[5.0 if p == q else 0.0 for q in lands] for p in lands]).astype(np.complex128)
    assert 0 < np.count_nonzero(want) < want.size
    G = moments(st, cycles)
    assert np.array_equal(G, want)
    assert G.tobytes() == moments(st, cycles).tobytes()


# ---- 5. more than 31 triangles ------------------------------------------------------------------------------------
def test_more_triangles_than_one_call_takes():
    """35 triangles of 12 spins, four of them repeats: three chunks of 15, 15 and 5, one call per pair of chunks."""
    sub = Full(L=12)
    triangles = random_triples(12, 31, 77, must=[(0, 1, 2), (11, 0, 5), (9, 10, 11)])
    repeats = [0, 9, 17, 30]
    triangles += [triangles[i] for i in repeats]
    assert len(triangles) == 35
    amps = int_amplitudes(sub.get_dimension(), 21)
    st = state_from(sub, amps)
    chi, cc = chirality_correlations(st, triangles)
    want, _ = reference(sub, amps, both_senses(triangles))
    wchi, wcc = from_gram(want)
    assert chi.shape == (35,) and cc.shape == (35, 35)
    assert np.array_equal(chi, wchi) and np.array_equal(cc, wcc)
    assert np.array_equal(cc, cc.conj().T)
    assert np.any(chi != 0)
    for at, i in enumerate(repeats):
        assert chi[31 + at] == chi[i]
        assert np.array_equal(cc[31 + at], cc[i]) and np.array_equal(cc[:, 31 + at], cc[:, i])


# ---- 6. known answer ----------------------------------------------------------------------------------------------
EIG_TOL = 1e-10


@pytest.mark.parametrize("flip", [False, True], ids=["sc12_6", "xparity"])
def test_kagome_12_total_chirality_ground_state(flip):
    """The ground state of H = sum_t chi_t over the 8 triangles of the kagome torus of 12 sites (one sense:
    lattices.kagome_triangles), in SpinConserve(12, 6) and in the lower of its two XParity sectors.  The chiralities add
    up to the energy and the correlators to its square:
      |sum_t chi[t] / N - E0|    <= 10 tol + 8 * 4 e        (chi: |2| + |2| entries of G)
      |sum cc / N - E0^2|        <= 10 tol + 8^2 * 16 e     (cc: four entries of G with |4|)
    with e = 4 rows 2^-53, the bound of an entry of G at N = 1.  Every entry is also held against the numpy reference
    applied to the same vector, to 4 e and 16 e."""
    triangles = lattices.kagome_triangles('12')
    assert len(triangles) == 8
    saved = config.L
    try:
        config.L = 12
        H = op_sum(chi_op(*t) for t in triangles)
        H.L = 12
        if flip:
            found = []
            for sector in ('+', '-'):
                sub = XParity(SpinConserve(12, 6), sector=sector)
                H.add_subspace(sub)
                ev, vecs = H.eigsolve(nev=1, tol=EIG_TOL, getvecs=True, subspace=sub)
                found.append((sub, ev[0], vecs[0]))
            sub, e0, st = min(found, key=lambda f: f[1])
        else:
            sub = SpinConserve(12, 6)
            H.add_subspace(sub)
            ev, vecs = H.eigsolve(nev=1, tol=EIG_TOL, getvecs=True, subspace=sub)
            e0, st = ev[0], vecs[0]
        H.destroy_mat()
        N = st.dot(st).real
        chi, cc = chirality_correlations(st, triangles)
        amps = st.to_numpy()
    finally:
        config.L = saved
    assert abs(e0 - (-17.8772153)) < 1e-6       # (tests/test_kagome_triangles.py: the same number from numpy)
    rows = sub.get_dimension()
    e = tolerance(rows, 1.0)
    energy = abs(chi.sum() / N - e0)
    square = abs(cc.sum() / N - e0 ** 2)
    print("kagome-12 in %r: E0 = %.12f, energy from chi %.3e (bound %.3e), E0^2 from cc %.3e (bound %.3e)"
          % (sub, e0, energy, 10 * EIG_TOL + 8 * 4 * e, square, 10 * EIG_TOL + 64 * 16 * e))
    assert energy <= 10 * EIG_TOL + 8 * 4 * e
    assert square <= 10 * EIG_TOL + 64 * 16 * e
    want_chi, want_cc = from_gram(reference(sub, amps, both_senses(triangles))[0])
    norm2 = np.vdot(amps, amps).real
    err_chi = np.max(np.abs(chi - want_chi))
    err_cc = np.max(np.abs(cc - want_cc))
    print("  against the reference on the same vector: chi %.3e (bound %.3e), cc %.3e (bound %.3e)"
          % (err_chi, 4 * e * norm2, err_cc, 16 * e * norm2))
    assert err_chi <= 4 * e * norm2 and err_cc <= 16 * e * norm2
    # a chiral state: every triangle carries the same sign
    assert np.all(chi < 0)


# ---- 7. refusals through Python -----------------------------------------------------------------------------------
def test_refusals():
    rng = np.random.default_rng(5)
    states = np.unique(rng.integers(0, 1 << 12, 300, dtype=np.int64))
    st = State(subspace=Explicit(states, L=12), state='random', seed=1)
    with pytest.raises(ValueError, match='Explicit'):
        chirality_correlations(st, [(0, 1, 2)])
    st = State(subspace=Full(L=8), state='random', seed=1)
    for bad in ([(0, 1, 2), (3, 3, 4)], [(3, 4, 4)], [(4, 3, 4)]):
        with pytest.raises(ValueError, match='distinct'):
            chirality_correlations(st, bad)
    with pytest.raises(ValueError, match='outside'):
        chirality_correlations(st, [(0, 1, 2), (2, 8, 3)])
    with pytest.raises(ValueError, match='outside'):
        chirality_correlations(st, [(-1, 1, 2)])
    with pytest.raises(ValueError, match='empty'):
        chirality_correlations(st, [])
    with pytest.raises(ValueError, match='triples'):
        chirality_correlations(st, [(0, 1)])
    with pytest.raises(RuntimeError, match='cycles'):
        backend.cyc_moments(st.vec, st.subspace._to_c(), [(0, 1, 2)] * 64)
    with pytest.raises(RuntimeError, match='distinct'):
        backend.cyc_moments(st.vec, st.subspace._to_c(), [(0, 1, 1)])
