"""
All <sigma+_i sigma-_j> of a state in one matrix-core pass (csrc/pm_kernels.hip, csrc/gram_tile.h,
csrc/observables.cpp: dnm_pm_moments; backend.pm_moments, computations.sigma_pm_correlations / spin_correlations).

The reference is numpy on the host: the configurations of the subspace and of the row sector (sigma_minus(j) sets bit
j: every configuration for Full, the opposite parity for Parity, k + 1 set bits for SpinConserve(L, k)), the operand
matrix A[:, j] = psi(r ^ e_j) gathered through state_to_idx where bit j of the row r is set, and P = A^H A.  States with
integer amplitudes in [-3, 3] + i [-3, 3] make every product an integer of modulus <= 18 and every sum an integer below
2^53: kernel and reference must then agree to the last bit in any summation order.  Random states are held to
4 rows 2^-53 <psi|psi> per entry: an entry is a complex sum of `rows` products with sum |conj(a) b| <= <psi|psi>
(Cauchy-Schwarz), each real sum takes about rows + 2 roundings, sqrt 2 for the modulus, once for the kernel and once
for the reference.
"""
import numpy as np
import pytest

from dynamite_amd import backend
from dynamite_amd.computations import sigma_pm_correlations, sigmaz_correlations, spin_correlations
from dynamite_amd.config import config
from dynamite_amd.operators import op_sum, sigma_minus, sigma_plus, sigmax, sigmay, sigmaz
from dynamite_amd.states import State
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve, XParity

pytestmark = pytest.mark.gpu


# ---- reference ----------------------------------------------------------------------------------------------------
def row_configurations(sub):
    """The configurations sigma_minus maps the subspace into, in the order the kernel enumerates them."""
    L = sub.L
    if isinstance(sub, SpinConserve):
        if sub.k + 1 > L:
            return np.zeros(0, dtype=np.int64)
        other = SpinConserve(L, sub.k + 1)
    elif isinstance(sub, Parity):
        other = Parity(1 - sub.space, L=L)
    else:
        other = sub
    return np.asarray(other.idx_to_state(np.arange(other.get_dimension())), dtype=np.int64)


def reference(sub, psi):
    """(P, rows of A) for the amplitudes psi of the whole subspace."""
    L = sub.L
    rows = row_configurations(sub)
    A = np.zeros((rows.size, L), dtype=np.complex128)
    for j in range(L):
        has = ((rows >> j) & 1) == 1
        idx = np.asarray(sub.state_to_idx(rows[has] ^ (np.int64(1) << j)), dtype=np.int64)
        assert np.all(idx >= 0)
        A[has, j] = psi[idx]
    return A.conj().T @ A, rows.size


def int_amplitudes(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-3, 4, n) + 1j * rng.integers(-3, 4, n)).astype(np.complex128)


def state_from(sub, amps):
    st = State(subspace=sub)
    lo, hi = st.vec.getOwnershipRange()
    st.vec.set_local_from_numpy(amps[lo:hi])
    st.set_initialized()
    return st


def moments(st):
    return backend.pm_moments(st.vec, st.subspace._to_c())


def tolerance(rows, norm2):
    return 4.0 * rows * 2.0 ** -53 * norm2


def expectation(op, st):
    op.L = st.subspace.L
    op.add_subspace(st.subspace)
    return op.expectation(st)


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
@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=6), id="full6"),
                                  pytest.param(lambda: SpinConserve(6, 3), id="sc6_3")])
def test_convention_is_that_of_expectation(make):
    """pm[i, j] is <sigma_plus(i) sigma_minus(j)> as Operator.expectation defines it.  expectation builds Hermitian
    operators only, so the product is taken in its two Hermitian parts, sigma+_i sigma-_j = (sigmax_i sigmax_j +
    sigmay_i sigmay_j) + i (sigmay_i sigmax_j - sigmax_i sigmay_j); the diagonal, Hermitian as it stands, directly."""
    sub = make()
    L = sub.L
    st = State(subspace=sub, state='random', seed=7)
    pm = sigma_pm_correlations(st)
    assert pm.shape == (L, L) and pm.dtype == np.complex128
    _, rows = reference(sub, st.to_numpy())
    tol = 4.0 * tolerance(rows, st.dot(st).real)          # (pm = 4 P)
    worst = 0.0
    for i in range(L):
        for j in range(L):
            if i == j:
                want = expectation(sigma_plus(i) * sigma_minus(i), st)
            else:
                want = (expectation(sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j), st) +
                        1j * expectation(sigmay(i) * sigmax(j) - sigmax(i) * sigmay(j), st))
            worst = max(worst, abs(pm[i, j] - want))
    print("convention: largest deviation %.3e (bound %.3e)" % (worst, tol))
    assert worst <= tol
    assert np.array_equal(pm, st.sigma_pm_correlations())


def test_product_state():
    """A spin that is up ('U', bit clear) can be lowered: sigma_plus sigma_minus = 2 (1 + sigmaz) is 4 there, 0 on a
    down spin, and a product state has no transverse correlations."""
    up = State(subspace=Full(L=6), state='UDUUDU')
    pm = up.sigma_pm_correlations()
    assert np.array_equal(pm, np.diag([4, 0, 4, 4, 0, 4]).astype(np.complex128))
    ss = up.spin_correlations()
    mz = np.array([1, -1, 1, 1, -1, 1.0])
    want = np.outer(mz, mz)
    np.fill_diagonal(want, 3.0)
    assert np.array_equal(ss, want)


# ---- 2. exact arithmetic ------------------------------------------------------------------------------------------
EXACT = [
    pytest.param(lambda: Full(L=4), 16, id="full4"),
    pytest.param(lambda: Full(L=15), 1 << 15, id="full15"),
    pytest.param(lambda: Full(L=16), 1 << 16, id="full16"),
    pytest.param(lambda: Full(L=17), 1 << 17, id="full17"),
    pytest.param(lambda: Full(L=20), 1 << 20, id="full20_swizzle16", marks=pytest.mark.default_layout),
    pytest.param(lambda: Parity('even', L=17), 1 << 16, id="parity17_even"),
    pytest.param(lambda: Parity('odd', L=17), 1 << 16, id="parity17_odd"),
    pytest.param(lambda: SpinConserve(16, 8), 12870, id="sc16_8"),
    pytest.param(lambda: SpinConserve(34, 2), 561, id="sc34_2"),
    pytest.param(lambda: SpinConserve(50, 2), 1225, id="sc50_2"),       # four tile rows, 19 600 rows
    pytest.param(lambda: SpinConserve(12, 12), 1, id="sc12_12"),
    pytest.param(lambda: SpinConserve(12, 0), 1, id="sc12_0"),
]


def check_exact(sub, dim, seed=3):
    assert sub.get_dimension() == dim
    amps = int_amplitudes(dim, seed)
    if dim == 1:
        amps[:] = 2 - 3j
    st = state_from(sub, amps)
    P = moments(st)
    want, _ = reference(sub, amps)
    assert P.shape == (sub.L, sub.L) and P.dtype == np.complex128
    assert np.array_equal(P, want), np.argwhere(P != want)[:8]
    assert hermitian_to_the_last_bit(P)
    # the diagonal is the weight of the configurations whose bit i is clear: the sums of the sigma-z pass
    M = backend.zz_moments(st.vec, sub._to_c())
    assert np.array_equal(np.diag(P).real, (M[0, 0] + M[0, 1:]) / 2)
    return st, P


@pytest.mark.parametrize("make,dim", EXACT)
def test_integer_amplitudes_bit_for_bit(make, dim):
    sub = make()
    st, P = check_exact(sub, dim)
    if isinstance(sub, Full) and sub.L == 20:
        assert st.vec.swz == 16          # the production layout: partners across the swizzle's XOR
    if isinstance(sub, SpinConserve):
        assert not st.vec.internal
        if sub.k == sub.L:
            assert np.array_equal(P, np.zeros((sub.L, sub.L)))
        if sub.k == 0:
            assert np.array_equal(P, 13.0 * np.eye(sub.L))
    assert np.array_equal(sigma_pm_correlations(st), 4.0 * P)


def test_integer_amplitudes_internal_layout(small_layout):
    """A SpinConserve state in the internal layout is converted to reference order on the way in."""
    st, _ = check_exact(SpinConserve(12, 6), 924)
    assert st.vec.internal


# ---- 3. random states ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=18), id="full18"),
                                  pytest.param(lambda: Parity('odd', L=18), id="parity18"),
                                  pytest.param(lambda: SpinConserve(18, 9), id="sc18_9")])
def test_random_states(make):
    sub = make()
    st = State(subspace=sub, state='random', seed=9)
    P = moments(st)
    amps = st.to_numpy()
    want, rows = reference(sub, amps)
    tol = tolerance(rows, np.vdot(amps, amps).real)
    err = np.max(np.abs(P - want))
    print("random state, %d rows: largest error %.3e (bound %.3e)" % (rows, err, tol))
    assert err <= tol
    assert hermitian_to_the_last_bit(P)


# ---- 4. determinism, planted rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=17), id="full17"),
                                  pytest.param(lambda: SpinConserve(16, 8), id="sc16_8")])
def test_two_calls_and_a_planted_amplitude(make):
    sub = make()
    dim = sub.get_dimension()
    st = State(subspace=sub, state='random', seed=5)
    assert moments(st).tobytes() == moments(st).tobytes()
    # one amplitude 1 + 2i, in the last panel of the sweep (Full: third from the end; SpinConserve: the last index):
    # weight 5 on the diagonal for every spin of that configuration that can be lowered, exact zeros elsewhere
    st = State(subspace=sub)
    st.set_initialized()
    idx = dim - 3 if isinstance(sub, Full) else dim - 1
    st.vec.set(0)
    st.vec.array[st.vec.positions(int(idx))] = 1 + 2j
    cfg = int(sub.idx_to_state(idx))
    want = np.diag([5.0 * (1 - ((cfg >> i) & 1)) for i in range(sub.L)]).astype(np.complex128)
    P = moments(st)
    assert np.array_equal(P, want)
    assert P.tobytes() == moments(st).tobytes()


# ---- 5. known answers ---------------------------------------------------------------------------------------------
EIG_TOL = 1e-10
# eigsolve returns a vector whose residual is below EIG_TOL (relative to the norm of H); an expectation value of an
# operator of norm 4 in it is held to ten times that
KNOWN_TOL = 10 * EIG_TOL


def ground_state(terms, sub):
    L = sub.L
    H = op_sum(terms)
    H.L = L
    H.add_subspace(sub)
    ev, vecs = H.eigsolve(nev=1, tol=EIG_TOL, getvecs=True, subspace=sub)
    dense = H.to_numpy(subspaces=(sub, sub), sparse=False)
    H.destroy_mat()
    return ev[0], vecs[0], np.asarray(dense)


def test_free_fermion_ground_state():
    """The ground state of 0.25 sum (sigmax sigmax + sigmay sigmay) on an open chain, SpinConserve(12, 6): hopping
    fermions.  Between neighbours there is no Jordan-Wigner string, <sigma+_i sigma-_{i+1}> = 4 <c+_i c_{i+1}> from the
    filled orbitals of the hopping matrix; all pairs against a dense diagonalisation of the 924-dimensional block."""
    L, k = 12, 6
    saved = config.L
    try:
        config.L = L
        sub = SpinConserve(L, k)
        e0, st, dense = ground_state((0.25 * (sigmax(i) * sigmax(i + 1) + sigmay(i) * sigmay(i + 1))
                                      for i in range(L - 1)), sub)
        n = st.dot(st).real
        pm = sigma_pm_correlations(st) / n
    finally:
        config.L = saved
    T = np.zeros((L, L))
    for i in range(L - 1):
        T[i, i + 1] = T[i + 1, i] = 0.5
    w, phi = np.linalg.eigh(T)
    Cm = phi[:, :k] @ phi[:, :k].T
    assert abs(e0 - w[:k].sum()) <= KNOWN_TOL
    nn = max(abs(pm.real[i, i + 1] / 2 - 2 * Cm[i, i + 1]) for i in range(L - 1))
    wd, vd = np.linalg.eigh(dense)
    want, _ = reference(sub, vd[:, 0].astype(np.complex128))
    allp = max(abs(pm[i, j] / 2 - 2 * want[i, j]) for i in range(L) for j in range(L))
    print("free fermions: neighbours %.3e, all pairs %.3e (bound %.3e)" % (nn, allp, KNOWN_TOL))
    assert nn <= KNOWN_TOL and allp <= KNOWN_TOL


def test_spin_correlations_of_a_singlet():
    """The Heisenberg ground state on an open chain of 12 spins is a total-spin singlet: sum_j <sigma_i . sigma_j> = 0
    for every i, and <sigma_i . sigma_j> = 3 <sigmaz_i sigmaz_j> off the diagonal."""
    L = 12
    saved = config.L
    try:
        config.L = L
        sub = SpinConserve(L, 6)
        _, st, _ = ground_state((0.25 * (sigmax(i) * sigmax(i + 1) + sigmay(i) * sigmay(i + 1) +
                                         sigmaz(i) * sigmaz(i + 1)) for i in range(L - 1)), sub)
        n = st.dot(st).real
        ss = spin_correlations(st) / n
        _, zz = sigmaz_correlations(st)
        assert np.array_equal(ss * n, st.spin_correlations())
    finally:
        config.L = saved
    zz = zz / n
    off = ~np.eye(L, dtype=bool)
    rowsum = np.max(np.abs(ss.sum(axis=1)))
    su2 = np.max(np.abs(ss[off] - 3 * zz[off]))
    print("singlet: row sums %.3e, ss - 3 zz %.3e (bound %.3e)" % (rowsum, su2, KNOWN_TOL))
    assert np.allclose(np.diag(ss), 3.0, rtol=0, atol=1e-14)
    assert rowsum <= KNOWN_TOL and su2 <= KNOWN_TOL


# ---- 6. refusals through Python -----------------------------------------------------------------------------------
def test_refusals():
    rng = np.random.default_rng(5)
    states = np.unique(rng.integers(0, 1 << 12, 300, dtype=np.int64))
    for sub, word in ((XParity(Full(L=10), sector='+'), 'global spin flip'), (Explicit(states, L=12), 'Full, Parity or SpinConserve')):
        st = State(subspace=sub, state='random', seed=1)
        for f in (sigma_pm_correlations, spin_correlations):
            with pytest.raises(ValueError, match=word):
                f(st)
