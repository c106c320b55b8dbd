"""
Overlaps and operator matrix elements of many states in one pass (computations.overlap_matrix,
Operator.matrix_elements on backend.vec_gram / csrc/vgram_kernels.hip).

The reference is numpy on the states' to_numpy(): B.conj().T @ K.  States with integer amplitudes in [-3, 3] + i [-3, 3]
make every sum an exact integer, so the pass and numpy agree to the last bit -- for a SpinConserve state in the internal
layout that also proves the padding contributes nothing.  Random states are held to the derived bound of
tests/test_gpu_bond_correlations.py, 4 rows 2^-53 |bra| |ket| per entry.  For matrix elements the images of the
reference are the to_numpy() of Operator.dot -- the same device multiply -- so that only the Gram pass is under test.
"""
import numpy as np
import pytest

from dynamite_amd import models
from dynamite_amd.computations import overlap_matrix
from dynamite_amd.extras import majorana
from dynamite_amd.operators import sigmaz
from dynamite_amd.states import State, UninitializedError
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve, XParity

from test_gpu_pauli_correlations import hermitian_to_the_last_bit, int_amplitudes, state_from
from test_gpu_sc3_graph import small_layout        # noqa: F401  (the internal layout for small SpinConserve subspaces)

pytestmark = pytest.mark.gpu

SUBSPACES = {
    "full10": lambda: Full(L=10),
    "parity10": lambda: Parity('even', L=10),
    "sc12_6": lambda: SpinConserve(12, 6),
    "xparity_sc12_6": lambda: XParity(SpinConserve(12, 6), sector='+'),
    "explicit": lambda: Explicit([3, 5, 6, 9, 10, 12, 17, 40, 65, 130, 257, 300, 511], L=10),
}


def int_states(sub, n, seed):
    dim = sub.get_dimension()
    return [state_from(sub, int_amplitudes(dim, seed + i)) for i in range(n)]


def random_states(sub, n, seed):
    rng = np.random.default_rng(seed)
    dim = sub.get_dimension()
    return [state_from(sub, rng.standard_normal(dim) + 1j * rng.standard_normal(dim)) for _ in range(n)]


def columns(states):
    return np.stack([s.to_numpy() for s in states], axis=1)


def bound(B, K):
    """4 rows 2^-53 |bra| |ket| for every pair of a column of B and a column of K"""
    return 4.0 * B.shape[0] * 2.0 ** -53 * np.outer(np.linalg.norm(B, axis=0), np.linalg.norm(K, axis=0))


@pytest.mark.parametrize("name", sorted(SUBSPACES))
def test_overlap_matrix(small_layout, name):     # noqa: F811
    sub = SUBSPACES[name]()
    states = int_states(sub, 6, 20)
    if name == "sc12_6":
        assert states[0].vec.internal and states[0].vec.alloc_size > sub.get_dimension()
    A = columns(states)
    S = overlap_matrix(states)
    assert S.dtype == np.complex128 and np.array_equal(S, A.conj().T @ A)
    assert hermitian_to_the_last_bit(S)
    assert np.array_equal(State.overlap_matrix(states), S)
    # the rectangular form
    others = int_states(sub, 3, 40)
    R = overlap_matrix(states, others)
    assert R.shape == (6, 3) and np.array_equal(R, A.conj().T @ columns(others))
    # random amplitudes: the derived bound
    states = random_states(sub, 6, 21)
    A = columns(states)
    S = overlap_matrix(states)
    assert np.all(np.abs(S - A.conj().T @ A) <= bound(A, A))
    assert hermitian_to_the_last_bit(S)


def test_mixed_layouts(small_layout):     # noqa: F811
    """One state has been through an operator on a bond graph and sits in its relabelled layout: the list of mixed
    layouts gives the same matrix, whichever layout comes first."""
    H = models.kagome("15")
    sub = SpinConserve(15, 7)
    H.add_subspace(sub)
    states = int_states(sub, 6, 60)
    A = columns(states)
    want = A.conj().T @ A
    assert np.array_equal(overlap_matrix(states), want)
    H.dot(states[2])                           # states[2] adopts the operator's layout (Operator.dot)
    assert states[2].vec.perm is not None and states[0].vec.perm is None
    assert np.array_equal(columns(states), A)
    assert np.array_equal(overlap_matrix(states), want)
    order = [2, 0, 1, 3, 4, 5]
    assert np.array_equal(overlap_matrix([states[i] for i in order]), want[np.ix_(order, order)])
    H.destroy_mat()


def test_chunking():
    """70 states: more than 64 columns, so chunks of 32, 32 and 6 and one call per pair of chunks."""
    sub = Full(L=8)
    states = int_states(sub, 70, 100)
    A = columns(states)
    S = overlap_matrix(states)
    assert np.array_equal(S, A.conj().T @ A)
    assert hermitian_to_the_last_bit(S)
    R = overlap_matrix(states[:40], states[30:])
    assert np.array_equal(R, A[:, :40].conj().T @ A[:, 30:])


@pytest.mark.parametrize("which", ("mbl", "sigmaz3"))
def test_matrix_elements(small_layout, which):     # noqa: F811
    L = 10
    sub = SpinConserve(L, 5)
    O = models.mbl(L) if which == "mbl" else sigmaz(3)      # (mbl: the Heisenberg chain in a random field)
    O.L = L
    O.add_subspace(sub)
    kets = random_states(sub, 8, 30)
    bras = random_states(sub, 8, 31)
    images = columns([O.dot(k) for k in kets])
    B = columns(bras)
    M = O.matrix_elements(kets, bras)
    assert M.shape == (8, 8) and M.dtype == np.complex128
    assert np.all(np.abs(M - B.conj().T @ images) <= bound(B, images))
    # batches of three images: the same entries summed in the same order
    M3 = O.matrix_elements(kets, bras, batch=3)
    assert np.array_equal(M3.view(np.float64), M.view(np.float64))
    # bras = kets and a Hermitian operator: M = M^H within twice the bound
    K = columns(kets)
    D = O.matrix_elements(kets)
    assert np.all(np.abs(D - K.conj().T @ images) <= bound(K, images))
    assert np.all(np.abs(D - D.conj().T) <= 2.0 * np.maximum(bound(K, images), bound(K, images).T))
    O.destroy_mat()


def test_matrix_elements_rectangular():
    """majorana(0) takes the even parity sector to the odd one: four even kets, three odd bras."""
    L = 8
    even, odd = Parity('even', L=L), Parity('odd', L=L)
    O = majorana(0)
    O.L = L
    O.add_subspace(even, odd)
    O.add_subspace(odd, even)                  # (left, right): the pair that takes even kets to odd bras
    kets = random_states(even, 4, 50)
    bras = random_states(odd, 3, 51)
    images = columns([O.dot(k) for k in kets])
    B = columns(bras)
    M = O.matrix_elements(kets, bras)
    assert M.shape == (3, 4)
    assert np.all(np.abs(M - B.conj().T @ images) <= bound(B, images))
    assert np.abs(M).max() > 0.1
    O.destroy_mat()


def test_errors():
    sub, other = Full(L=6), Parity('even', L=6)
    O = sigmaz(3)
    O.L = 6
    O.add_subspace(sub)
    good = random_states(sub, 2, 70)
    elsewhere = random_states(other, 2, 71)
    with pytest.raises(ValueError, match="No operator subspace found"):
        O.dot(elsewhere[0])
    with pytest.raises(ValueError, match="No operator subspace found"):
        O.matrix_elements(elsewhere)
    with pytest.raises(ValueError, match="Subspaces of matrix and result vector do not match"):
        O.matrix_elements(good, elsewhere)
    with pytest.raises(ValueError, match="one subspace"):
        O.matrix_elements([good[0], elsewhere[0]])
    with pytest.raises(ValueError, match="empty"):
        O.matrix_elements([])
    blank = State(subspace=sub)
    with pytest.raises(UninitializedError):
        O.matrix_elements([good[0], blank])
    with pytest.raises(UninitializedError):
        overlap_matrix([good[0], blank])
    with pytest.raises(UninitializedError):
        overlap_matrix(good, [blank])
    with pytest.raises(ValueError, match="same subspace"):
        overlap_matrix([good[0], elsewhere[0]])
    with pytest.raises(ValueError, match="same subspace"):
        overlap_matrix(good, elsewhere)
    with pytest.raises(ValueError, match="empty"):
        overlap_matrix([])
    O.destroy_mat()
