"""
The numpy reference of the site-operator product (tests/site_ops_ref.py) against the dense Kronecker product, and under a
swizzle against the positions of the layout.  No GPU, no library.
"""
import numpy as np
import pytest

import site_ops_ref as ref


@pytest.mark.parametrize("L", [1, 2, 3, 5, 8])
def test_against_kronecker_product(L):
    rng = np.random.default_rng(L)
    mats = rng.normal(size=(L, 2, 2)) + 1j * rng.normal(size=(L, 2, 2))
    x = rng.normal(size=1 << L) + 1j * rng.normal(size=1 << L)
    want = ref.dense(mats) @ x
    got = ref.apply_product(x, mats)
    assert np.max(np.abs(got - want)) <= 64 * L * np.finfo(float).eps * np.max(np.abs(want))


@pytest.mark.parametrize("L", [1, 4, 7])
def test_exact_inputs_are_exact(L):
    mats = ref.exact_matrices(L, 3 * L, classes=[2] * L)
    x = ref.gaussian_integers(1 << L, L)
    assert np.array_equal(ref.apply_product(x, mats), ref.dense(mats) @ x)


def test_spin_is_index_bit():
    """The non-symmetric M = [[1, 2], [3i, 4]] on site j alone: (M x)(c') = sum_c M[c'_j][c_j] x(c)."""
    L, M = 5, np.array([[1, 2], [3j, 4]])
    x = ref.gaussian_integers(1 << L, 11)
    for j in range(L):
        mats = np.broadcast_to(np.eye(2, dtype=complex), (L, 2, 2)).copy()
        mats[j] = M
        y = ref.apply_product(x, mats)
        for c in range(1 << L):
            lo, hi = c & ~(1 << j), c | (1 << j)
            assert y[c] == M[(c >> j) & 1, 0] * x[lo] + M[(c >> j) & 1, 1] * x[hi]


@pytest.mark.parametrize("L,swz", [(8, 5), (8, 6), (10, 6), (14, 12), (4, 5)])
def test_swizzled_against_positions(L, swz):
    n = 1 << L
    pos = ref.positions(n, swz)
    assert np.array_equal(np.sort(pos), np.arange(n)) and np.array_equal(pos[pos], np.arange(n))      # an involution
    assert np.array_equal(pos & 15, np.arange(n) & 15)                                                # runs survive
    mats = ref.exact_matrices(L, 17 + L)
    x = ref.gaussian_integers(n, L + swz)           # x[i]: index order
    lies = np.empty_like(x)
    lies[pos] = x
    out = ref.apply_product_swizzled(lies, mats, swz)
    assert np.array_equal(out[pos], ref.apply_product(x, mats))
    if L > swz:
        assert not np.array_equal(pos, np.arange(n))


def test_exact_matrices_classes():
    mats = ref.exact_matrices(9, 1, classes=[0, 1, 2] * 3)
    for j, M in enumerate(mats):
        ident = np.array_equal(M, np.eye(2))
        diag = M[0, 1] == 0 and M[1, 0] == 0
        assert (ident, diag and not ident, not diag)[j % 3]
        assert not np.any(np.signbit(M.real) & (M.real == 0)) and not np.any(np.signbit(M.imag) & (M.imag == 0))
