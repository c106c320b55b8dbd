"""
All bond-swap (dimer-dimer) correlators of a state in one matrix-core pass (csrc/swap_kernels.hip, csrc/gram_tile.h,
csrc/observables.cpp: dnm_swap_moments; backend.swap_moments, computations.bond_correlations).

The reference is numpy on the host: the configurations of the subspace, the operand matrix A[:, 0] = psi, A[:, 1 + m] =
psi gathered through state_to_idx of the configurations with bits a_m and b_m exchanged, and G = A^H A.  For a state on
an XParity sector the reference does not use the kernel's flip logic: the amplitudes are expanded to the parent (x on
the representatives, s x on their complements), the parent's G of that vector is taken and halved -- the expanded vector
is sqrt 2 times the sector's state, and halving is exact.  States with integer amplitudes in [-3, 3] + i [-3, 3] make
every product an integer of modulus <= 18 and every sum an integer below 2^53: kernel and reference must then agree to
the last bit in any summation order.  Random states are held to 4 rows 2^-53 <psi|psi> per entry of G: an entry is a
complex sum of `rows` products with sum |conj(a) b| <= <psi|psi> (every column of A is a permutation of the state:
Cauchy-Schwarz), each real sum takes about rows + 2 roundings, sqrt 2 for the modulus, once for the kernel and once for
the reference.
"""
import numpy as np
import pytest

from dynamite_amd import backend, lattices
from dynamite_amd.computations import bond_correlations
from dynamite_amd.config import config
from dynamite_amd.operators import op_sum, sigmax, sigmay, sigmaz
from dynamite_amd.states import State
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve, XParity

pytestmark = pytest.mark.gpu


# ---- reference ----------------------------------------------------------------------------------------------------
def exchanged(cfg, a, b):
    differ = ((cfg >> a) ^ (cfg >> b)) & 1
    return cfg ^ (differ << a) ^ (differ << b)


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


def reference(sub, amps, bonds):
    """(G, rows of the sweep) for the amplitudes of the whole vector."""
    parent, psi = expanded(sub, np.asarray(amps, dtype=np.complex128))
    dim = parent.get_dimension()
    cfg = np.asarray(parent.idx_to_state(np.arange(dim)), dtype=np.int64)
    A = np.empty((dim, len(bonds) + 1), dtype=np.complex128)
    A[:, 0] = psi
    for m, (a, b) in enumerate(bonds):
        idx = np.asarray(parent.state_to_idx(exchanged(cfg, int(a), int(b))), dtype=np.int64)
        assert np.all(idx >= 0)
        A[:, 1 + m] = psi[idx]
    G = A.conj().T @ A
    if parent is not sub:
        return G / 2, dim // 2
    return G, dim


def from_gram(G):
    """(b, bb) of bond_correlations from G, the same formulas: exact on integers."""
    b = 2.0 * G[0, 1:].real - G[0, 0].real
    bb = 4.0 * G[1:, 1:] - 2.0 * (G[1:, :1] + G[:1, 1:]) + G[0, 0]
    return b, bb


def int_amplitudes(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-3, 4, n) + 1j * rng.integers(-3, 4, n)).astype(np.complex128)


def state_from(sub, amps):
    st = State(subspace=sub)
    lo, hi = st.vec.getOwnershipRange()
    st.vec.set_local_from_numpy(amps[lo:hi])
    st.set_initialized()
    return st


def moments(st, bonds):
    return backend.swap_moments(st.vec, st.subspace._to_c(), bonds, parent_of(st.subspace)[1])


def tolerance(rows, norm2):
    return 4.0 * rows * 2.0 ** -53 * norm2


def expectation(op, st):
    op.L = st.subspace.L
    op.add_subspace(st.subspace)
    return op.expectation(st)


def random_bonds(L, n, seed, must=()):
    rng = np.random.default_rng(seed)
    out = [tuple(p) for p in must]
    while len(out) < n:
        a, b = (int(v) for v in rng.choice(L, size=2, replace=False))
        out.append((a, b))
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
def heis(a, b):
    return sigmax(a) * sigmax(b) + sigmay(a) * sigmay(b) + sigmaz(a) * sigmaz(b)


RING = [(i, (i + 1) % 6) for i in range(6)] + [(0, 3)]


@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=6), id="full6"),
                                  pytest.param(lambda: SpinConserve(6, 3), id="sc6_3"),
                                  pytest.param(lambda: XParity(SpinConserve(6, 3), sector='+'), id="x_sc6_3")])
def test_convention_is_that_of_expectation(make):
    """b[m] is <sigma_a . sigma_b> and bb[m, m'] is <B_m B_m'> as Operator.expectation defines them.  expectation builds
    Hermitian operators only, so the product is taken in its two Hermitian parts, (B_m B_m' + B_m' B_m) / 2 and
    -i (B_m B_m' - B_m' B_m) / 2; where the two bonds are equal or share no site they commute, the second part is the
    zero operator and its expectation value is 0 without a call.  Bound: 9 times the per-entry bound of G for bb (|4| +
    |2| + |2| + |1|), 3 times for b."""
    sub = make()
    st = State(subspace=sub, state='random', seed=7)
    b, bb = bond_correlations(st, RING)
    n = len(RING)
    assert b.shape == (n,) and b.dtype == np.float64 and bb.shape == (n, n) and bb.dtype == np.complex128
    rows = sub.get_dimension()
    norm2 = st.dot(st).real
    tol = tolerance(rows, norm2)
    worst_b = worst_bb = worst_id = 0.0
    for m, (a, c) in enumerate(RING):
        worst_b = max(worst_b, abs(b[m] - expectation(heis(a, c), st)))
        worst_id = max(worst_id, abs(bb[m, m] - (3.0 * norm2 - 2.0 * b[m])))
        for m2, (d, e) in enumerate(RING):
            re = expectation(0.5 * (heis(a, c) * heis(d, e) + heis(d, e) * heis(a, c)), st)
            im = 0.0
            if len({a, c} & {d, e}) == 1:
                im = expectation(-0.5j * (heis(a, c) * heis(d, e) - heis(d, e) * heis(a, c)), st)
            worst_bb = max(worst_bb, abs(bb[m, m2] - (re + 1j * im)))
    print("convention: b %.3e (bound %.3e), bb %.3e (bound %.3e), bb[m, m] = 3 N - 2 b[m] %.3e"
          % (worst_b, 3 * tol, worst_bb, 9 * tol, worst_id))
    assert worst_b <= 3 * tol and worst_bb <= 9 * tol
    assert worst_id <= (9 + 2 * 3) * tol
    assert np.array_equal(bb, bb.conj().T)
    b2, bb2 = st.bond_correlations(RING)
    assert np.array_equal(b, b2) and np.array_equal(bb, bb2)
    bc, bbc = bond_correlations(st, RING, connected=True)
    N = moments(st, RING)[0, 0].real          # (<psi|psi> as the pass sums it)
    assert abs(N - norm2) <= tol
    assert np.array_equal(bc, b) and np.array_equal(bbc, bb / N - np.outer(b, b) / N ** 2)


# ---- 2. exact arithmetic ------------------------------------------------------------------------------------------
def check_exact(sub, bonds, seed=3):
    dim = sub.get_dimension()
    amps = int_amplitudes(dim, seed)
    if dim == 1:
        amps[:] = 2 - 3j
    st = state_from(sub, amps)
    G = moments(st, bonds)
    want, _ = reference(sub, amps, bonds)
    n = len(bonds)
    assert G.shape == (n + 1, n + 1) and G.dtype == np.complex128
    assert np.array_equal(G, want), np.argwhere(G != want)[:8]
    assert hermitian_to_the_last_bit(G)
    assert np.array_equal(np.diag(G), np.full(n + 1, G[0, 0]))
    b, bb = bond_correlations(st, bonds)
    wb, wbb = from_gram(want)
    assert np.array_equal(b, wb) and np.array_equal(bb, wbb)
    assert np.array_equal(np.diag(bb), 3.0 * G[0, 0] - 2.0 * b)      # (sigma . sigma)^2 = 3 - 2 sigma . sigma
    return st, G


def test_integer_amplitudes_partial_panel():
    check_exact(Full(L=4), [(0, 1), (1, 2), (3, 0), (2, 3), (1, 3)])


TILE_ROWS = [(15, 15), (15, 16), (15, 63), (16, 15), (16, 16), (16, 47), (16, 48), (16, 63), (17, 15), (17, 16), (17, 63)]


@pytest.mark.parametrize("L,n", TILE_ROWS, ids=["full%d_n%d" % c for c in TILE_ROWS])
def test_integer_amplitudes_tile_rows(L, n):
    """n + 1 = 16, 17, 48, 49, 64 columns: NB = 1, 2, 3, 4 with the last tile row full and with one column in it."""
    sub = Full(L=L)
    bonds = random_bonds(L, n, 100 * L + n, must=[(0, L - 1), (L - 1, 1), (0, 1), (5, 4), (7, 6), (3, 9)])
    assert backend.swap_moments_plan(sub._to_c()['data'], n)[0] == -(-(n + 1) // 16)
    check_exact(sub, bonds)


@pytest.mark.default_layout
def test_integer_amplitudes_production_layout():
    """Full(20) as it lies in the default layout: bonds inside the low bits, straddling bit 16 and both above it."""
    st, _ = check_exact(Full(L=20), [(0, 1), (2, 9), (4, 15), (3, 16), (15, 16), (5, 19), (16, 17), (17, 19), (19, 18)])
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


@pytest.mark.parametrize("make", EXACT)
def test_integer_amplitudes_bit_for_bit(make):
    """Bonds at site 0 (the spin Parity's index does not hold), at site L - 1 (the complement under XParity), above
    site 31 where there is one, adjacent and far, in both orders, one repeat."""
    sub = make()
    L = sub.L
    bonds = random_bonds(L, 20, 7 * L, must=[(0, 1), (5, 0), (0, L - 1), (L - 1, 3), (L - 2, L - 1), (L - 1, L // 2),
                                             (L - 3, 2), (0, 1)])
    st, G = check_exact(sub, bonds)
    if isinstance(sub, SpinConserve):
        assert not st.vec.internal
    if sub.get_dimension() == 1:
        assert np.array_equal(G, np.full((21, 21), 13.0 + 0j))


def test_integer_amplitudes_internal_layout(small_layout):
    """A SpinConserve state in the internal layout is converted to reference order on the way in."""
    st, _ = check_exact(SpinConserve(12, 6), random_bonds(12, 20, 5, must=[(0, 11), (11, 4), (0, 1)]))
    assert st.vec.internal


# ---- 3. random states ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=18), id="full18"),
                                  pytest.param(lambda: Parity('odd', L=18), id="parity18"),
                                  pytest.param(lambda: SpinConserve(18, 9), id="sc18_9"),
                                  pytest.param(lambda: XParity(SpinConserve(18, 9), sector='-'), id="x_sc18_9")])
def test_random_states(make):
    sub = make()
    bonds = random_bonds(18, 40, 11, must=[(0, 17), (17, 5), (0, 1), (16, 17)])
    st = State(subspace=sub, state='random', seed=9)
    G = moments(st, bonds)
    amps = st.to_numpy()
    want, rows = reference(sub, amps, bonds)
    tol = tolerance(rows, np.vdot(amps, amps).real)
    err = np.max(np.abs(G - want))
    print("random state, %d rows, 40 bonds: largest error %.3e (bound %.3e)" % (rows, err, tol))
    assert err <= tol
    assert hermitian_to_the_last_bit(G)


# ---- 4. determinism, a planted amplitude --------------------------------------------------------------------------
@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=17), id="full17"),
                                  pytest.param(lambda: SpinConserve(16, 8), id="sc16_8")])
def test_two_calls_and_a_planted_amplitude(make):
    sub = make()
    L, dim = sub.L, sub.get_dimension()
    bonds = random_bonds(L, 20, 13, must=[(0, L - 1), (L - 1, 0), (L - 1, L - 2), (0, 1), (0, 1)])
    st = State(subspace=sub, state='random', seed=5)
    assert moments(st, bonds).tobytes() == moments(st, bonds).tobytes()
    # one amplitude 1 + 2i in the last panel of the sweep (Full: third from the end; SpinConserve: the last index):
    # column 1 + m of A then holds it in the row swap_m of that configuration
    st = State(subspace=sub)
    st.set_initialized()
    idx = dim - 3 if isinstance(sub, Full) else dim - 1
    st.vec.set(0)
    st.vec.array[st.vec.positions(int(idx))] = 1 + 2j
    cfg = int(sub.idx_to_state(idx))
    lands = [cfg] + [int(exchanged(np.int64(cfg), a, b)) for a, b in bonds]
    want = np.array([[5.0 if p == q else 0.0 for q in lands] for p in lands]).astype(np.complex128)
    assert 0 < np.count_nonzero(want) < want.size
    G = moments(st, bonds)
    assert np.array_equal(G, want)
    assert G.tobytes() == moments(st, bonds).tobytes()


# ---- 5. more than 63 bonds ----------------------------------------------------------------------------------------
def test_more_bonds_than_one_call_takes():
    """All 66 pairs of 12 spins and four repeats: 70 bonds, three chunks, one call per pair of chunks."""
    sub = Full(L=12)
    bonds = [(a, b) for a in range(12) for b in range(a + 1, 12)]
    repeats = [0, 17, 40, 65]
    bonds += [bonds[i] for i in repeats]
    assert len(bonds) == 70
    amps = int_amplitudes(sub.get_dimension(), 21)
    st = state_from(sub, amps)
    b, bb = bond_correlations(st, bonds)
    want, _ = reference(sub, amps, bonds)
    wb, wbb = from_gram(want)
    assert b.shape == (70,) and bb.shape == (70, 70)
    assert np.array_equal(b, wb) and np.array_equal(bb, wbb)
    assert np.array_equal(bb, bb.conj().T)
    for at, i in enumerate(repeats):
        assert b[66 + at] == b[i]
        assert np.array_equal(bb[66 + at], bb[i]) and np.array_equal(bb[:, 66 + at], bb[:, i])


# ---- 6. known answer ----------------------------------------------------------------------------------------------
EIG_TOL = 1e-10


def solve(H, sub):
    ev, vecs = H.eigsolve(nev=1, tol=EIG_TOL, getvecs=True, subspace=sub)
    dense = np.asarray(H.to_numpy(subspaces=(sub, sub), sparse=False))
    return ev[0], vecs[0], dense


@pytest.mark.parametrize("flip", [False, True], ids=["sc12_6", "xparity"])
def test_kagome_12_ground_state(flip):
    """The Heisenberg ground state on the kagome torus of 12 sites, H = 0.25 sum of sigma . sigma over its 24 bonds, in
    SpinConserve(12, 6) and in the XParity sector that holds it -- the subspace benchmarking/run_kagome.py solves in.
    The bond energies add up to the energy and the bond-bond correlators to its square:
      |0.25 sum_m b[m] / N - E0|   <= 10 tol + (24 / 4) 3 e       (b: |2| + |1| entries of G)
      |sum bb / (16 N) - E0^2|      <= 10 tol + (24^2 / 16) 9 e    (bb: |4| + |2| + |2| + |1|)
    with e = 4 rows 2^-53, the bound of an entry of G at N = 1.  Every entry is also held against the ground vector of
    a dense diagonalisation put through the numpy reference: eigsolve's vector has a residual below tol |H|, so it is
    within tol |H| / gap of the true one, and an expectation value of an operator of norm w moves by at most twice
    that times w (w = 3 for b, 9 for bb), beside the rounding of the two sums."""
    nsites, edges = lattices.kagome('12')
    assert nsites == 12 and len(edges) == 24
    saved = config.L
    try:
        config.L = 12
        H = op_sum(0.25 * heis(a, b) for a, b in edges)
        H.L = 12
        parent = SpinConserve(12, 6)
        if flip:
            found = []
            for sector in ('+', '-'):
                sub = XParity(SpinConserve(12, 6), sector=sector)
                H.add_subspace(sub)
                found.append((sub,) + solve(H, sub))
            sub, e0, st, dense = min(found, key=lambda f: f[1])
        else:
            sub = parent
            H.add_subspace(sub)
            e0, st, dense = solve(H, sub)
        H.destroy_mat()
        N = st.dot(st).real
        b, bb = bond_correlations(st, edges)
    finally:
        config.L = saved
    rows = sub.get_dimension()
    e = tolerance(rows, 1.0)
    energy = abs(0.25 * b.sum() / N - e0)
    variance = abs(bb.sum() / (16.0 * N) - e0 ** 2)
    print("kagome-12 in %r: E0 = %.12f, energy from b %.3e (bound %.3e), E0^2 from bb %.3e (bound %.3e)"
          % (sub, e0, energy, 10 * EIG_TOL + 6 * 3 * e, variance, 10 * EIG_TOL + 36 * 9 * e))
    assert energy <= 10 * EIG_TOL + 6 * 3 * e
    assert variance <= 10 * EIG_TOL + 36 * 9 * e
    w, v = np.linalg.eigh(dense)
    assert abs(w[0] - e0) <= 10 * EIG_TOL
    gap = w[1] - w[0]
    assert gap > 1e-3                       # (a degenerate ground state would leave the vector undetermined)
    moved = 2.0 * EIG_TOL * max(abs(w[0]), abs(w[-1])) / gap
    want_b, want_bb = from_gram(reference(sub, v[:, 0].astype(np.complex128), edges)[0])
    err_b = np.max(np.abs(b / N - want_b))
    err_bb = np.max(np.abs(bb / N - want_bb))
    print("  against the dense ground vector (gap %.4f): b %.3e (bound %.3e), bb %.3e (bound %.3e)"
          % (gap, err_b, 3 * (moved + 2 * e), err_bb, 9 * (moved + 2 * e)))
    assert err_b <= 3 * (moved + 2 * e) and err_bb <= 9 * (moved + 2 * e)


# ---- 7. refusals through Python -----------------------------------------------------------------------------------
def test_refusals():
    rng = np.random.default_rng(5)
    states = np.unique(rng.integers(0, 1 << 12, 300, dtype=np.int64))
    st = State(subspace=Explicit(states, L=12), state='random', seed=1)
    with pytest.raises(ValueError, match='Explicit'):
        bond_correlations(st, [(0, 1)])
    st = State(subspace=Full(L=8), state='random', seed=1)
    with pytest.raises(ValueError, match='itself'):
        bond_correlations(st, [(0, 1), (3, 3)])
    with pytest.raises(ValueError, match='outside'):
        bond_correlations(st, [(0, 1), (2, 8)])
    with pytest.raises(ValueError, match='outside'):
        bond_correlations(st, [(-1, 1)])
    with pytest.raises(ValueError, match='empty'):
        bond_correlations(st, [])
