"""
tests/rdm_ref.py, the integer reference of the exact reduced-density-matrix tests, against the CPU oracle's
restatement of the reference's rdm_<SUBSPACE> (oracle.rdm), on the integer states the GPU tests use.  The oracle adds
a conj(b) in complex128 one traced configuration after the other: on this data every partial sum is an integer far
below 2^53, so its result is exact too and the comparison is an equality.  No GPU.
"""
import numpy as np
import pytest

from oracle import oracle as orc
import rdm_ref

EXPLICIT_10 = np.sort(np.random.RandomState(5).choice(1 << 10, size=341, replace=False)).astype(np.int64)


def spaces(L):
    out = [("full", orc.full(L)), ("even", orc.parity(L, 0)), ("odd", orc.parity(L, 1))]
    out += [("sc%d" % k, orc.spin_conserve(L, k)) for k in sorted({L // 2, 1})]
    if L == 10:
        out.append(("explicit", orc.explicit(L, EXPLICIT_10)))
        out.append(("explicit_unsorted", orc.explicit(L, EXPLICIT_10[np.random.RandomState(6).permutation(341)])))
    return out


KEEPS = {
    10: [[], [0], [9], [0, 1, 2], [7, 8, 9], [3, 8], [0, 2, 4, 6, 8], [1, 2, 5, 6, 9], list(range(6)), list(range(10))],
    7: [[0, 1], [2, 3, 4], [0, 3, 6], [1, 2, 3, 4, 5, 6]],
    2: [[0], [1], [0, 1]],
    1: [[0]],
}
CASES = [(L, name, keep) for L in KEEPS for name, _ in spaces(L) for keep in KEEPS[L]]


@pytest.mark.parametrize("L,name,keep", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_dense_and_blocks_against_oracle(L, name, keep):
    sub = dict(spaces(L))[name]
    n = sub.dim
    re, im = rdm_ref.ints(n, 30 + L)
    states = sub.i2s(np.arange(n))
    full_re, full_im = rdm_ref.embed(states, re, im, L)
    assert np.count_nonzero(full_re) == n and np.count_nonzero(full_im) == n
    rr, ri = rdm_ref.dense(full_re, full_im, L, keep)
    K = 1 << len(keep)
    assert rr.dtype == np.int64 and ri.dtype == np.int64 and rr.shape == ri.shape == (K, K)
    want = orc.rdm(sub, re.astype(np.float64) + 1j * im.astype(np.float64), keep)
    assert np.array_equal(rr.astype(np.float64), want.real) and np.array_equal(ri.astype(np.float64), want.imag)
    assert np.array_equal(rr, rr.T) and np.array_equal(ri, -ri.T)
    assert int(np.trace(rr)) == int(np.sum(re * re + im * im))
    if name == "full" and L >= 7 and 2 <= len(keep) < L:
        assert np.any(ri != 0)                                   # (the sign of the imaginary part is under test)
    # the blocks: the dense matrix cut by popcount; everything outside the blocks of a SpinConserve state is zero
    pc = rdm_ref.popcounts(len(keep))
    got = rdm_ref.blocks(full_re, full_im, L, keep)
    feasible = [m for m in range(len(keep) + 1) if np.any(rr[pc == m][:, pc == m]) or np.any(ri[pc == m][:, pc == m])]
    assert sorted(got) == feasible
    for m, (br, bi) in got.items():
        idx = np.nonzero(pc == m)[0]
        assert np.array_equal(br, rr[np.ix_(idx, idx)]) and np.array_equal(bi, ri[np.ix_(idx, idx)])
    if name.startswith("sc"):
        k = int(name[2:])
        assert feasible == list(range(max(0, k - (L - len(keep))), min(k, len(keep)) + 1))
        off = pc[:, None] != pc[None, :]
        assert not np.any(rr[off]) and not np.any(ri[off])


@pytest.mark.parametrize("sector", [+1, -1])
@pytest.mark.parametrize("keep", [[], [0, 1, 2], [5, 6, 7], [1, 4, 7], list(range(8))], ids=str)
def test_xparity_embedding(sector, keep):
    """XParity(SpinConserve(8, 4)): the embedding without its 1 / sqrt 2 against the oracle on the parent subspace,
    handed the same state (x on the representatives, sector * x on their complements)."""
    L, k = 8, 4
    sub = orc.spin_conserve(L, k)
    states = sub.i2s(np.arange(sub.dim))
    half = sub.dim // 2
    assert not np.any(states[:half] >> (L - 1)) and np.all(states[half:] >> (L - 1))
    re, im = rdm_ref.ints(half, 77)
    full_re, full_im = rdm_ref.embed(states[:half], re, im, L, sector)
    x = np.zeros(sub.dim, dtype=np.complex128)
    x[:half] = re + 1j * im
    x[sub.s2i(states[:half] ^ 0xff)] = sector * (re + 1j * im)
    want = orc.rdm(sub, x, keep)
    rr, ri = rdm_ref.dense(full_re, full_im, L, keep)
    assert np.array_equal(rr.astype(np.float64), want.real) and np.array_equal(ri.astype(np.float64), want.imag)
    pc = rdm_ref.popcounts(len(keep))
    got = rdm_ref.blocks(full_re, full_im, L, keep)
    assert sorted(got) == list(range(max(0, len(keep) - k), min(k, len(keep)) + 1))
    for m, (br, bi) in got.items():
        idx = np.nonzero(pc == m)[0]
        assert np.array_equal(br, rr[np.ix_(idx, idx)]) and np.array_equal(bi, ri[np.ix_(idx, idx)])
    with pytest.raises(AssertionError):
        rdm_ref.embed(states, np.ones(sub.dim, dtype=np.int64), np.ones(sub.dim, dtype=np.int64), L, sector)
