"""
numpy reference of the product of single-site operators (csrc/site_ops_kernels.hip): y(c') = sum_c prod_j M_j[c'_j][c_j]
x(c) with spin j = index bit j.  M_j is applied by reshaping the vector to (high, 2, low) along bit j; a swizzled vector
goes through its positions.  Checked against the dense Kronecker product in tests/test_site_ops_ref.py.
"""
import numpy as np

ENTRIES = np.array([0, 1, -1, 1j, -1j, 1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j], dtype=np.complex128)


def positions(n, swz):
    """Position of element i of a vector of n elements in the XOR-swizzled layout (0: index order)."""
    i = np.arange(n, dtype=np.int64)
    return i if not swz else i ^ (((i >> swz) & ((1 << (swz - 4)) - 1)) << 4)


def apply_site(x, j, M):
    """M on bit j of the index of x (index order)."""
    L = x.size.bit_length() - 1
    v = x.reshape(1 << (L - 1 - j), 2, 1 << j)
    M = np.asarray(M, dtype=np.complex128)
    out = np.empty_like(v)
    out[:, 0, :] = M[0, 0] * v[:, 0, :] + M[0, 1] * v[:, 1, :]
    out[:, 1, :] = M[1, 0] * v[:, 0, :] + M[1, 1] * v[:, 1, :]
    return out.reshape(-1)


def apply_product(x, mats):
    """(x)_j mats[j] on x in index order."""
    y = np.asarray(x, dtype=np.complex128)
    for j, M in enumerate(mats):
        if not np.array_equal(M, np.eye(2)):
            y = apply_site(y, j, M)
    return y.copy()


def apply_product_swizzled(x_lies, mats, swz):
    """The same on a vector as it lies in the swizzled layout; the result lies the same way."""
    pos = positions(x_lies.size, swz)
    out = np.empty_like(x_lies)
    out[pos] = apply_product(x_lies[pos], mats)
    return out


def dense(mats):
    """The 2^L x 2^L matrix: site L-1 is the leftmost Kronecker factor."""
    U = np.ones((1, 1), dtype=np.complex128)
    for M in mats:
        U = np.kron(np.asarray(M, dtype=np.complex128), U)
    return U


def gaussian_integers(n, seed, bound=8):
    rng = np.random.default_rng(seed)
    return (rng.integers(-bound, bound + 1, n) + 1j * rng.integers(-bound, bound + 1, n)).astype(np.complex128)


def exact_matrices(L, seed, classes=None):
    """L matrices with entries from ENTRIES: class 0 identity, 1 diagonal, 2 general per site (random when None).  Every
    component of a product grows at most fourfold per site, so Gaussian-integer amplitudes up to 8 stay exact integers
    below 2^53 for L <= 24 in any order of evaluation."""
    rng = np.random.default_rng(seed)
    if classes is None:
        classes = rng.integers(0, 3, L)
    mats = np.empty((L, 2, 2), dtype=np.complex128)
    for j, c in enumerate(classes):
        M = ENTRIES[rng.integers(0, len(ENTRIES), (2, 2))]
        if c == 0:
            M = np.eye(2, dtype=np.complex128)
        elif c == 1:
            M[0, 1] = M[1, 0] = 0
            if M[0, 0] == 1 and M[1, 1] == 1:
                M[1, 1] = 1j
        elif M[0, 1] == 0 and M[1, 0] == 0:
            M[0, 1] = 1
        mats[j] = M + 0.0        # (no negative zeros: the classes are decided on bits)
    return mats
