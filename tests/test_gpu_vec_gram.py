"""
The Gram matrix of many vectors in one matrix-core pass (csrc/vgram_kernels.hip, csrc/gram_tile.h, csrc/observables.cpp:
dnm_vec_gram; backend.vec_gram_ptrs).

The reference is numpy on the host, A.conj().T @ A with vector c as column c of A.  Vectors with integer amplitudes in
[-3, 3] + i [-3, 3] make every product an integer of modulus <= 18 and every sum an integer below 2^53: kernel and
reference must then agree to the last bit in any summation order.  Random vectors are held to the bound
tests/test_gpu_bond_correlations.py derives: entry (a, b) is a complex sum of n products whose moduli sum to at most
|x_a| |x_b| (Cauchy-Schwarz), so its error is at most 4 n 2^-53 |x_a| |x_b| -- derived, not measured.

The shapes are the smallest at which the kernel can go wrong: one to four tile rows with the last one partly filled,
rows that are no multiple of four, both panel sizes (2^7 rows up to two tile rows, 2^6 from three on) at their edges,
the edges of the 2^9 rows of a workgroup, a ragged last workgroup, and one case of more than 1024 shares of 512 rows,
where a workgroup takes more panels than fit in 512 rows.
"""
import numpy as np
import pytest
import torch

from dynamite_amd import backend

from test_gpu_pauli_correlations import hermitian_to_the_last_bit, int_amplitudes

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 63, 64, 65, 127, 128, 129, 511, 512, 513, 3 * 512 + 5)


def on_device(A):
    """Column c of the host matrix A as a device vector of its own allocation."""
    T = torch.from_numpy(np.ascontiguousarray(A.T)).cuda()
    return [T[c].clone() for c in range(A.shape[1])]


def gram(vecs, n=None):
    return backend.vec_gram_ptrs([v.data_ptr() for v in vecs], vecs[0].numel() if n is None else n)


def shares(nvec, n):
    """(log2 of the panel's rows, workgroups, panels, panels of a workgroup's share) of the plan"""
    _, B, nwg, _, _ = backend.vec_gram_plan(nvec, n)
    npanels = (n + (1 << B) - 1) >> B
    return B, nwg, npanels, (npanels + nwg - 1) // nwg


def int_matrix(n, nvec, seed):
    return int_amplitudes(n * nvec, seed).reshape(n, nvec)


@pytest.fixture(scope="module")
def int_columns():
    """64 integer vectors of the largest small size, on host and device: the cases take leading parts of them."""
    A = int_matrix(ROWS[-1], 64, 11)
    return A, on_device(A)


@pytest.mark.parametrize("nvec", (1, 2, 16, 17, 33, 49, 64))
def test_integer_amplitudes_exact(int_columns, nvec):
    A, dev = int_columns
    for n in ROWS:
        G = gram(dev[:nvec], n)
        ref = A[:n, :nvec].conj().T @ A[:n, :nvec]
        assert np.array_equal(G, ref), n
        assert hermitian_to_the_last_bit(G), n


def test_more_than_1024_shares():
    """17 vectors of 2^19 + 515 elements: 1024 workgroups for 4101 panels of 2^7 rows, so a share is five panels,
    the last share with rows is one panel and that panel a few rows, and the workgroups after it have none."""
    n, nvec = (1 << 19) + 515, 17
    B, nwg, npanels, per_wg = shares(nvec, n)
    assert (B, nwg) == (7, 1024) and per_wg > 1 and npanels % per_wg != 0 and nwg * per_wg > npanels + per_wg
    A = int_matrix(n, nvec, 12)
    dev = on_device(A)
    G = gram(dev)
    assert np.array_equal(G, A.conj().T @ A)
    assert hermitian_to_the_last_bit(G)


@pytest.mark.parametrize("nvec,a,b", ((64, 0, 63), (16, 0, 15), (33, 5, 32), (49, 40, 17)))
def test_planted_row(nvec, a, b):
    """All vectors zero but x_a[r] = 2 + i and x_b[r] = 1 - 3i: G has the four entries of (a, b) and zeros elsewhere,
    wherever r lies -- panel edges, share edges, the last row."""
    n = 3 * 512 + 5
    B, nwg, _, per_wg = shares(nvec, n)
    share = per_wg << B
    assert nwg > 1 and share < n
    dev = [torch.zeros(n, dtype=torch.complex128, device="cuda") for _ in range(nvec)]
    expect = np.zeros((nvec, nvec), dtype=np.complex128)
    expect[a, a], expect[b, b] = 5.0, 10.0
    expect[a, b] = np.conj(2 + 1j) * (1 - 3j)
    expect[b, a] = np.conj(expect[a, b])
    for r in (0, (1 << B) - 1, 1 << B, share - 1, share, n - 1):
        dev[a][r], dev[b][r] = 2 + 1j, 1 - 3j
        G = gram(dev)
        dev[a][r], dev[b][r] = 0, 0
        assert np.array_equal(G, expect), r


def test_alignment_and_aliasing():
    """Views into one buffer at element offsets 1, 2, 3, ...: 16-byte alignment and no more; the first pointer is
    passed twice, and its two rows and columns of G are equal bit for bit."""
    n, nvec = 3 * 512 + 5, 33
    host = int_amplitudes(n + nvec + 1, 13)
    buf = torch.from_numpy(host).cuda()
    views = [buf[1 + c:1 + c + n] for c in range(nvec)]
    assert all(v.data_ptr() % 16 == 0 for v in views) and any(v.data_ptr() % 32 == 16 for v in views)
    views.append(views[0])
    A = np.stack([host[1 + c:1 + c + n] for c in range(nvec)] + [host[1:1 + n]], axis=1)
    G = gram(views)
    assert np.array_equal(G, A.conj().T @ A)
    assert np.array_equal(G[0], G[nvec]) and np.array_equal(G[:, 0], G[:, nvec])
    assert hermitian_to_the_last_bit(G)


@pytest.mark.parametrize("nvec,n", ((64, (1 << 14) + 1), (5, 1 << 20)))
def test_random_vectors(nvec, n):
    rng = np.random.default_rng(14)
    A = rng.standard_normal((n, nvec)) + 1j * rng.standard_normal((n, nvec))
    dev = on_device(A)
    G = gram(dev)
    again = gram(dev)
    assert np.array_equal(G.view(np.float64), again.view(np.float64))      # two calls, the same bits
    assert hermitian_to_the_last_bit(G)
    norms = np.linalg.norm(A, axis=0)
    bound = 4.0 * n * 2.0 ** -53 * np.outer(norms, norms)
    err = np.abs(G - A.conj().T @ A)
    print("largest error over its bound: %.3g" % (err / bound).max())
    assert np.all(err <= bound)


def test_backend_vec_gram_refuses_long_lists():
    v = backend.Vec(8)
    with pytest.raises(ValueError, match="65 vectors"):
        backend.vec_gram([v] * 65)
    with pytest.raises(ValueError, match="0 vectors"):
        backend.vec_gram([])
    with pytest.raises(ValueError, match="different sizes"):
        backend.vec_gram([v, backend.Vec(9)])
