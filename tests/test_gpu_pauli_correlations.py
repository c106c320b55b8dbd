"""
All two-spin Pauli correlators of a state in one matrix-core pass (csrc/pauli_kernels.hip, csrc/pauli_cols.h,
csrc/gram_tile.h, csrc/observables.cpp: dnm_pauli_moments; backend.pauli_moments, computations.pauli_correlations,
two_site_density_matrices, mutual_information).

The reference is numpy on the host and does not use the pass's column arithmetic: the state is embedded in the full
space of 2^L configurations, column 1 + c of the operand matrix is the Pauli matrix applied there -- psi(r ^ e_j) for a
flip, times (-1)^(bit j of r) for a sign, without the phase -i of sigma-y -- and G = A^H A over all 2^L rows.  For a
state on a Parity sector the columns that flip then live on the rows of the opposite sector and the others on the
sector's own, so their products are zeros of themselves and every other entry is the sum the kernel takes, with zeros
added.  States with integer amplitudes in [-3, 3] + i [-3, 3] make every product an integer of modulus <= 18 and every
sum an integer below 2^53: kernel and reference must then agree to the last bit in any summation order.  Random states
are held to the bound tests/test_gpu_bond_correlations.py derives, 4 rows 2^-53 <psi|psi> per entry of G (an entry is a
complex sum of `rows` products with sum |conj(a) b| <= <psi|psi>, every column of A being a signed permutation of the
state), times the factor of the derived quantity: 1 for one and two (the phases are exact), 4 / <psi|psi> for an
entry of a two-site density matrix, a quarter of sixteen correlators.
"""
import numpy as np
import pytest

from dynamite_amd import backend
from dynamite_amd.computations import (_pauli_gram, entanglement_entropy, mutual_information, pauli_correlations,
                                       reduced_density_matrix, two_site_density_matrices)
from dynamite_amd.operators import sigmax, sigmay, sigmaz
from dynamite_amd.states import State
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve, XParity

pytestmark = pytest.mark.gpu

X, Y, Z = 1, 2, 3
PAULI = {X: sigmax, Y: sigmay, Z: sigmaz}
PHASE = np.array([1.0, -1j, 1.0])         # sigma^a psi = PHASE[a] * (column of kind a + 1)


# ---- reference ----------------------------------------------------------------------------------------------------
def embedded(sub, amps):
    full = np.zeros(1 << sub.L, dtype=np.complex128)
    full[np.asarray(sub.idx_to_state(np.arange(sub.get_dimension())), dtype=np.int64)] = amps
    return full


def column(full, site, kind):
    r = np.arange(full.size, dtype=np.int64)
    v = full[r ^ (np.int64(1) << site)] if kind in (X, Y) else full
    if kind in (Y, Z):
        v = v * (1.0 - 2.0 * ((r >> site) & 1))
    return v


def reference(sub, amps, cols):
    full = embedded(sub, np.asarray(amps, dtype=np.complex128))
    A = np.empty((full.size, len(cols) + 1), dtype=np.complex128)
    A[:, 0] = full
    for c, (site, kind) in enumerate(cols):
        A[:, 1 + c] = column(full, int(site), int(kind))
    return A.conj().T @ A


def site_cols(sites):
    return [(int(s), k) for s in sites for k in (X, Y, Z)]


def from_gram(G, n):
    """(one, two) of pauli_correlations from the G of site_cols, the same formulas: exact on integers."""
    phase = np.tile(PHASE, n)
    one = (G[0, 1:] * phase).real.reshape(n, 3).T
    two = np.conj(phase)[:, None] * G[1:, 1:] * phase[None, :]
    return one, two.reshape(n, 3, n, 3).transpose(1, 0, 3, 2)


def int_amplitudes(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-3, 4, n) + 1j * rng.integers(-3, 4, n)).astype(np.complex128)


def state_from(sub, amps):
    st = State(subspace=sub)
    lo, hi = st.vec.getOwnershipRange()
    st.vec.set_local_from_numpy(amps[lo:hi])
    st.set_initialized()
    return st


def moments(st, cols):
    return backend.pauli_moments(st.vec, st.subspace._to_c(), cols)


def tolerance(rows, norm2):
    return 4.0 * rows * 2.0 ** -53 * norm2


def expectation(op, st):
    op.L = st.subspace.L
    op.allow_projection = True       # (a single flip leaves a SpinConserve sector: the projected operator is meant)
    op.add_subspace(st.subspace)
    return op.expectation(st)


def random_cols(L, n, seed, must=()):
    rng = np.random.default_rng(seed)
    out = [tuple(c) for c in must]
    while len(out) < n:
        out.append((int(rng.integers(L)), int(rng.integers(1, 4))))
    return out[:n]


def hermitian_to_the_last_bit(P):
    return np.array_equal(P, P.conj().T) and np.array_equal(np.diag(P).imag, np.zeros(P.shape[0]))


def two_is_hermitian(two):
    n = two.shape[1]
    return hermitian_to_the_last_bit(two.reshape(3 * n, 3 * n))


# ---- 1. convention ------------------------------------------------------------------------------------------------
def check_against_expectation(st, rows):
    """one[a, i] and two[a, i, b, j], i != j, are what Operator.expectation gives for the operator and the product (two
    Paulis at different sites commute: the product is Hermitian and its expectation value real); at the same site the
    entries follow from sigma^a sigma^a = 1 and sigmax sigmay = i sigmaz and its cyclic partners.  Bound: that of one
    entry of G, twice that where two entries are compared with each other."""
    L = st.subspace.L
    one, two = pauli_correlations(st)
    assert one.shape == (3, L) and one.dtype == np.float64
    assert two.shape == (3, L, 3, L) and two.dtype == np.complex128
    norm2 = st.dot(st).real
    tol = tolerance(rows, norm2)
    worst_one = worst_two = worst_same = 0.0
    for a in range(3):
        for i in range(L):
            worst_one = max(worst_one, abs(one[a, i] - expectation(PAULI[a + 1](i), st)))
            worst_same = max(worst_same, abs(two[a, i, a, i] - norm2))
            nxt, last = (a + 1) % 3, (a + 2) % 3
            worst_same = max(worst_same, abs(two[a, i, nxt, i] - 1j * one[last, i]) / 2,
                             abs(two[nxt, i, a, i] + 1j * one[last, i]) / 2)
            for b in range(3):
                for j in range(i + 1, L):
                    # (the two operators commute: sigma^b_j sigma^a_i is the same operator, one call serves both entries)
                    want = expectation(PAULI[a + 1](i) * PAULI[b + 1](j), st)
                    worst_two = max(worst_two, abs(two[a, i, b, j] - want), abs(two[b, j, a, i] - want))
    print("convention on %r: one %.3e, two %.3e, same site %.3e (bound %.3e)"
          % (st.subspace, worst_one, worst_two, worst_same, tol))
    assert worst_one <= tol and worst_two <= tol and worst_same <= tol
    assert two_is_hermitian(two)
    one2, two2 = st.pauli_correlations()
    assert np.array_equal(one, one2) and np.array_equal(two, two2)
    return one, two


def test_convention_is_that_of_expectation():
    st = State(subspace=Full(L=5), state='random', seed=7)
    check_against_expectation(st, 32)


# ---- 2. - 5. exact arithmetic --------------------------------------------------------------------------------------
def check_exact(sub, cols, seed=3):
    dim = sub.get_dimension()
    amps = int_amplitudes(dim, seed)
    st = state_from(sub, amps)
    G = moments(st, cols)
    want = reference(sub, amps, cols)
    n = len(cols)
    assert G.shape == (n + 1, n + 1) and G.dtype == np.complex128
    assert np.array_equal(G, want), np.argwhere(G != want)[:8]
    assert hermitian_to_the_last_bit(G)
    assert np.array_equal(np.diag(G), np.full(n + 1, G[0, 0]))
    return st, amps, G


def test_integer_amplitudes_partial_panel():
    """Full(4) has 16 rows, less than the smallest panel: all 12 columns, and the public function on them."""
    sub = Full(L=4)
    st, amps, G = check_exact(sub, site_cols(range(4)))
    one, two = pauli_correlations(st)
    want_one, want_two = from_gram(G, 4)
    assert np.array_equal(one, want_one) and np.array_equal(two, want_two)
    assert two_is_hermitian(two)


TILE_ROWS = [(L, n) for L in (15, 16, 17) for n in (15, 16, 47, 48, 63)]


@pytest.mark.parametrize("L,n", TILE_ROWS, ids=["full%d_n%d" % c for c in TILE_ROWS])
def test_integer_amplitudes_tile_rows(L, n):
    """n + 1 = 16, 17, 48, 49, 64 columns: NB = 1, 2, 3, 4 with the last tile row full and with one column in it.  Site 0,
    site L - 1, all three kinds at one site, a repeated column, sites below and above the log2 of the panel's rows (9 at
    one tile row, 7 from two on)."""
    sub = Full(L=L)
    must = [(0, X), (L - 1, Y), (5, X), (5, Y), (5, Z), (5, X), (3, Z), (12, X), (L - 1, Z), (0, Y), (8, Y), (6, X)]
    cols = random_cols(L, n, 100 * L + n, must=must)
    tr, pb = backend.pauli_moments_plan(sub._to_c()['data'], n)[:2]
    assert tr == -(-(n + 1) // 16) and 3 < pb < 12
    check_exact(sub, cols)


@pytest.mark.default_layout
def test_integer_amplitudes_production_layout():
    """Full(20) as it lies in the default layout: flips below, at and above the swizzle shift."""
    cols = [(s, k) for s in (0, 4, 15, 16, 19) for k in (X, Y)] + [(16, Z), (3, Z)]
    st, _, _ = check_exact(Full(L=20), cols)
    assert st.vec.swz == 16


@pytest.mark.parametrize("make", [pytest.param(lambda: Parity('even', L=17), id="parity17_even"),
                                  pytest.param(lambda: Parity('odd', L=17), id="parity17_odd")])
def test_integer_amplitudes_parity(make):
    """Site 0 (the spin the index does not hold: its flip pairs a row with its own amplitude, its sign is read from the
    parity) in all three kinds, site L - 1, and a mixed list.  The entries between a flipping and a non-flipping column
    are exact zeros."""
    sub = make()
    L = sub.L
    must = [(0, X), (0, Y), (0, Z), (L - 1, X), (L - 1, Y), (L - 1, Z), (1, Y), (1, Z), (0, Y), (7, X)]
    cols = random_cols(L, 30, 7 * L, must=must)
    st, amps, G = check_exact(sub, cols)
    flips = np.array([False] + [k != Z for _, k in cols])
    cross = flips[:, None] != flips[None, :]
    assert np.array_equal(G[cross], np.zeros(np.count_nonzero(cross)))
    assert np.count_nonzero(G[~cross]) > 0.9 * np.count_nonzero(~cross)
    sites = [0, 1, L - 1]
    one, two = pauli_correlations(st, sites)
    want_one, want_two = from_gram(reference(sub, amps, site_cols(sites)), 3)
    assert np.array_equal(one, want_one) and np.array_equal(two, want_two)
    assert np.array_equal(one[:2], np.zeros((2, 3)))


# ---- 6. random states ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=18), id="full18"),
                                  pytest.param(lambda: Parity('odd', L=18), id="parity18")])
def test_random_states(make):
    sub = make()
    rows = sub.get_dimension()
    cols = random_cols(18, 40, 11, must=[(0, X), (0, Y), (0, Z), (17, Y), (17, Z), (16, X)])
    st = State(subspace=sub, state='random', seed=9)
    G = moments(st, cols)
    amps = st.to_numpy()
    tol = tolerance(rows, np.vdot(amps, amps).real)
    err = np.max(np.abs(G - reference(sub, amps, cols)))
    print("random state, %d rows, 40 columns: largest error %.3e (bound %.3e)" % (rows, err, tol))
    assert err <= tol
    assert hermitian_to_the_last_bit(G)
    sites = [0, 3, 9, 16, 17]
    one, two = pauli_correlations(st, sites)
    want_one, want_two = from_gram(reference(sub, amps, site_cols(sites)), len(sites))
    err_one, err_two = np.max(np.abs(one - want_one)), np.max(np.abs(two - want_two))
    print("  one %.3e, two %.3e (bound %.3e)" % (err_one, err_two, tol))
    assert err_one <= tol and err_two <= tol
    assert two_is_hermitian(two)


# ---- 7. determinism, a planted amplitude --------------------------------------------------------------------------
def test_two_calls_and_a_planted_amplitude():
    sub = Full(L=17)
    L, dim = 17, 1 << 17
    cols = random_cols(L, 20, 13, must=[(0, X), (L - 1, Y), (L - 1, Z), (0, Y), (0, Y), (16, X), (1, Z)])
    st = State(subspace=sub, state='random', seed=5)
    assert moments(st, cols).tobytes() == moments(st, cols).tobytes()
    # one amplitude 1 + 2i in the last panel of the sweep, third from the end: column 1 + c of A holds it in the row
    # with the site flipped (or in its own row), with the sign read there
    st = State(subspace=sub)
    st.set_initialized()
    idx = dim - 3
    st.vec.set(0)
    st.vec.array[st.vec.positions(int(idx))] = 1 + 2j
    lands, signs = [idx], [1.0]
    for site, kind in cols:
        r = idx ^ (1 << site) if kind in (X, Y) else idx
        lands.append(r)
        signs.append(-1.0 if kind in (Y, Z) and (r >> site) & 1 else 1.0)
    want = np.array([[5.0 * s * t if p == q else 0.0 for q, t in zip(lands, signs)]
                     for p, s in zip(lands, signs)]).astype(np.complex128)
    assert 0 < np.count_nonzero(want) < want.size and np.any(want.real < 0)
    G = moments(st, cols)
    assert np.array_equal(G, want)
    assert G.tobytes() == moments(st, cols).tobytes()


# ---- 8. more columns than one call takes --------------------------------------------------------------------------
def test_more_columns_than_one_call_takes():
    """All 36 columns of 12 spins and 34 repeats: 70 columns, three chunks, one call per pair of chunks."""
    sub = Full(L=12)
    cols = site_cols(range(12))
    cols += cols[:34]
    assert len(cols) == 70
    amps = int_amplitudes(sub.get_dimension(), 21)
    st = state_from(sub, amps)
    G = _pauli_gram(st, np.array(cols))
    want = reference(sub, amps, cols)
    assert G.shape == (71, 71)
    assert np.array_equal(G, want), np.argwhere(G != want)[:8]
    assert hermitian_to_the_last_bit(G)


def test_all_sites_of_22_spins():
    """sites=None on Full(22) is 66 columns: the chunked route through the public function, against numpy on sampled
    entries (no dense operators)."""
    L = 22
    sub = Full(L=L)
    amps = int_amplitudes(sub.get_dimension(), 23)
    st = state_from(sub, amps)
    one, two = pauli_correlations(st)
    assert one.shape == (3, L) and two.shape == (3, L, 3, L)
    assert two_is_hermitian(two)
    rng = np.random.default_rng(4)
    samples = [(0, 0, 1, 0), (0, 0, 1, 21), (1, 21, 2, 21), (2, 15, 0, 16), (1, 14, 1, 15), (0, 21, 0, 20)]
    samples += [tuple(int(v) for v in (rng.integers(3), rng.integers(L), rng.integers(3), rng.integers(L)))
                for _ in range(14)]
    for a, i, b, j in samples:
        left, right = PHASE[a] * column(amps, i, a + 1), PHASE[b] * column(amps, j, b + 1)
        assert two[a, i, b, j] == np.vdot(left, right), (a, i, b, j)
        assert one[a, i] == np.vdot(amps, left).real, (a, i)


# ---- 9. SpinConserve: assembled from the sigma-z and the sigma+ sigma- pass ---------------------------------------
@pytest.mark.parametrize("k", [4, 3])
def test_spin_conserve_assembly(k):
    sub = SpinConserve(8, k)
    st = State(subspace=sub, state='random', seed=3)
    one, two = check_against_expectation(st, sub.get_dimension())
    assert np.array_equal(one[:2], np.zeros((2, 8)))
    for a, b in ((0, 2), (1, 2), (2, 0), (2, 1)):
        assert np.array_equal(two[a, :, b, :], np.zeros((8, 8)))


# ---- 10. two-site density matrices and mutual information ---------------------------------------------------------
# the largest deviation of I_ij from the three entanglement entropies measured on an MI355X for the state below (four
# units in the last place of entropies of about ln 2 and ln 4)
MI_MEASURED = 8.882e-16


def test_two_site_density_matrices_and_mutual_information():
    """Full(10), random state.  Every rho_ij against reduced_density_matrix(state, [i, j]) to 4 times the bound of an
    entry of G over <psi|psi>: an entry of rho is a quarter of sixteen correlators.  I_ij against the three entanglement
    entropies: no bound is derived for the logarithm -- the spectra of a random state of 10 spins are far from zero, so
    only rounding contributes; the largest deviation measured over the 45 pairs is MI_MEASURED = 8.882e-16 and ten times
    that, 8.882e-15, is asserted."""
    L = 10
    st = State(subspace=Full(L=L), state='random', seed=12)
    norm2 = st.dot(st).real
    pairs = [(i, j) for i in range(L) for j in range(i + 1, L)]
    rho = two_site_density_matrices(st)
    assert rho.shape == (len(pairs), 4, 4) and rho.dtype == np.complex128
    tol = 4.0 * tolerance(1 << L, norm2) / norm2
    worst = max(np.max(np.abs(rho[n] - reduced_density_matrix(st, [i, j]) / norm2)) for n, (i, j) in enumerate(pairs))
    print("rho_ij of %d pairs: largest error %.3e (bound %.3e)" % (len(pairs), worst, tol))
    assert worst <= tol
    some = [(0, 9), (3, 4), (2, 7)]
    assert np.array_equal(st.two_site_density_matrices(some), rho[[pairs.index(p) for p in some]])
    mi = mutual_information(st)
    assert mi.shape == (L, L) and mi.dtype == np.float64
    assert np.array_equal(mi, mi.T) and np.array_equal(np.diag(mi), np.zeros(L))
    single = [entanglement_entropy(st, [i]) for i in range(L)]
    dev = max(abs(mi[i, j] - (single[i] + single[j] - entanglement_entropy(st, [i, j]))) for i, j in pairs)
    print("I_ij: largest deviation from the entanglement entropies %.3e (asserted: %.3e)" % (dev, 10 * MI_MEASURED))
    assert dev <= 10 * MI_MEASURED
    assert np.array_equal(st.mutual_information(), mi)
    sub_mi = mutual_information(st, [7, 2, 5])
    assert np.max(np.abs(sub_mi - mi[np.ix_([7, 2, 5], [7, 2, 5])])) <= 10 * MI_MEASURED


def test_known_answers():
    """A product state has I = 0.  The GHZ state of 6 spins has I_ij = ln 2 for every pair (S_i = S_ij = ln 2),
    <sigmaz_i sigmaz_j> = 1 and <sigmax_i sigmax_j> = 0.  Sums of one or two products each: a few roundings."""
    st = State(subspace=Full(L=6), state='UDDUDU')
    assert np.max(np.abs(mutual_information(st))) <= 1e-14
    ghz = np.zeros(64, dtype=np.complex128)
    ghz[0] = ghz[63] = np.sqrt(0.5)
    st = state_from(Full(L=6), ghz)
    one, two = pauli_correlations(st)
    off = ~np.eye(6, dtype=bool)
    assert np.max(np.abs(two[2, :, 2, :] - 1.0)) <= 1e-15
    assert np.array_equal(two[0, :, 0, :][off], np.zeros(30))
    assert np.max(np.abs(one)) == 0.0
    mi = mutual_information(st)
    assert np.max(np.abs(mi[off] - np.log(2.0))) <= 1e-14
    rho = two_site_density_matrices(st, [(1, 4)])[0]
    assert np.max(np.abs(rho - np.diag([0.5, 0, 0, 0.5]))) <= 1e-15


# ---- 11. refusals through Python ----------------------------------------------------------------------------------
def test_refusals():
    st = State(subspace=XParity(Full(L=8), sector='+'), state='random', seed=1)
    for call in (pauli_correlations, two_site_density_matrices, mutual_information):
        with pytest.raises(ValueError, match='global spin flip'):
            call(st)
    rng = np.random.default_rng(5)
    states = np.unique(rng.integers(0, 1 << 12, 300, dtype=np.int64))
    st = State(subspace=Explicit(states, L=12), state='random', seed=1)
    for call in (pauli_correlations, two_site_density_matrices, mutual_information):
        with pytest.raises(ValueError, match='Explicit'):
            call(st)
    st = State(subspace=Full(L=8), state='random', seed=1)
    for sites in ([0, 8], [-1, 2]):
        with pytest.raises(ValueError, match='outside'):
            pauli_correlations(st, sites)
        with pytest.raises(ValueError, match='outside'):
            mutual_information(st, sites)
    with pytest.raises(ValueError, match='empty'):
        pauli_correlations(st, [])
    with pytest.raises(ValueError, match='empty'):
        two_site_density_matrices(st, [])
    with pytest.raises(ValueError, match='outside'):
        two_site_density_matrices(st, [(0, 8)])
    with pytest.raises(ValueError, match='i < j'):
        two_site_density_matrices(st, [(3, 3)])
    with pytest.raises(ValueError, match='i < j'):
        two_site_density_matrices(st, [(4, 2)])
    with pytest.raises(ValueError, match='pairs of sites'):
        two_site_density_matrices(st, [0, 1, 2])
