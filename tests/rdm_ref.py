"""
Integer reference of the reduced density matrix, for the exact tests of csrc/rdm_kernels.hip and
csrc/rdm_sector_kernels.hip (tests/test_gpu_rdm_exact.py).  No GPU, no library call: numpy on int64.

The state is given by integer real and imaginary parts (tests/test_gpu_vec.py::ints: independent non-zero integers in
[-8, 8]).  A product a conj(b) of two amplitudes then has parts of modulus <= 2 * 64, a matrix entry sums 2^(L - k)
of them, and everything stays an integer far below 2^53: the device, whatever its order of summation and whatever it
contracts into an fma, has to return these numbers exactly.

Definition (include/dynamite_amd.h: dnm_reduced_density_matrix): rho[a, b] = sum_t psi(a, t) conj(psi(b, t)), bit i of
a row index = spin keep[i], psi zero outside the subspace.  With A[a, t] = psi(a, t) = Ar + i Ai:
    Re rho = Ar Ar^T + Ai Ai^T,    Im rho = Ai Ar^T - Ar Ai^T.
"""
import numpy as np

from test_gpu_vec import ints      # noqa: F401  (the state data of every exact case: re, im = ints(n, seed))


def popcounts(nbits):
    """popcount of 0 ... 2^nbits - 1"""
    pc = np.zeros(1, dtype=np.int64)
    for _ in range(nbits):
        pc = np.concatenate([pc, pc + 1])
    return pc


def embed(states, re, im, L, sector=0):
    """The state in the 2^L product basis as two int64 arrays: amplitude i of (re, im) is that of configuration
    states[i].  sector = +1 / -1: the state is the XParity half of that sector, states its representatives c, and
    full[c] = x, full[~c] = sector * x -- WITHOUT the 1 / sqrt 2 of (|c> + s |~c>) / sqrt 2: the matrices of this
    embedding are twice those of the normalised one, exactly (the kernel applies its factor 1/2 once, at the end)."""
    states = np.asarray(states, dtype=np.int64)
    re, im = np.asarray(re, dtype=np.int64), np.asarray(im, dtype=np.int64)
    assert states.shape == re.shape == im.shape and states.ndim == 1
    assert np.unique(states).size == states.size
    assert states.size == 0 or (0 <= states.min() and states.max() >> L == 0)
    full_re, full_im = np.zeros(1 << L, dtype=np.int64), np.zeros(1 << L, dtype=np.int64)
    full_re[states], full_im[states] = re, im
    if sector:
        assert sector in (+1, -1) and not np.any(states >> (L - 1)), "representatives have bit L-1 clear"
        flipped = states ^ ((1 << L) - 1)
        full_re[flipped], full_im[flipped] = sector * re, sector * im
    return full_re, full_im


def operand(full, L, keep):
    """A[a, t] = psi(a, t): bit i of the row index a is spin keep[i], bit j of t the j-th traced spin, ascending."""
    keep = [int(s) for s in keep]
    assert all(0 <= s < L for s in keep) and all(a < b for a, b in zip(keep, keep[1:]))
    rest = [s for s in range(L) if s not in keep]
    axes = [L - 1 - s for s in reversed(keep)] + [L - 1 - s for s in reversed(rest)]
    return np.ascontiguousarray(full.reshape((2,) * L).transpose(axes).reshape(1 << len(keep), -1))


def _gram(ar, ai):
    """(Re, Im) of A A^H in int64"""
    assert ar.dtype == np.int64 and ai.dtype == np.int64
    return ar @ ar.T + ai @ ai.T, ai @ ar.T - ar @ ai.T


def dense(full_re, full_im, L, keep):
    """(rho_re, rho_im), int64, 2^k x 2^k"""
    return _gram(operand(full_re, L, keep), operand(full_im, L, keep))


def blocks(full_re, full_im, L, keep):
    """{n: (re, im)}: dense(...)[idx][:, idx] for idx = the row indices of popcount n in ascending order, for the n that
    are feasible (some configuration of the state has n set bits among the kept spins).  Computed from the rows
    themselves, so that more than 15 kept spins (a dense matrix of 4^k entries) stay cheap; traced configurations on
    which all rows of a block vanish add nothing and are left out of the product."""
    ar, ai = operand(full_re, L, keep), operand(full_im, L, keep)
    pc = popcounts(len(keep))
    out = {}
    for n in range(len(keep) + 1):
        idx = np.nonzero(pc == n)[0]
        br, bi = ar[idx], ai[idx]
        cols = np.nonzero(np.any(br != 0, axis=0) | np.any(bi != 0, axis=0))[0]
        if cols.size:
            out[n] = _gram(np.ascontiguousarray(br[:, cols]), np.ascontiguousarray(bi[:, cols]))
    return out
