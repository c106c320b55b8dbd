"""
Sector-resolved reduced density matrices (csrc/rdm_sector_kernels.hip): the blocks rho_n of a SpinConserve or
XParity(SpinConserve) state's reduced density matrix, n = set bits among the kept spins, against numpy on the host --
the state embedded in the 2^L product basis, reshaped, m @ m^H, blocks cut by popcount.  Shapes are the smallest at
which each part of the kernel can go wrong: blocks under one 64 x 64 tile, ragged tile edges, several tile rows,
contiguous-low and scattered keep sets, several slices of the traced index, the fan-in tree of the slice sum.
"""
import ctypes as C
import functools
from math import comb

import numpy as np
import pytest

from dynamite_amd import _lib
from dynamite_amd import computations as cp
from dynamite_amd.states import State
from dynamite_amd.subspaces import Full, Parity, SpinConserve, XParity

gpu = pytest.mark.gpu


def popcounts(nbits):
    return np.array([bin(i).count("1") for i in range(1 << nbits)])


def embed(sub, x):
    """The state in the 2^L product basis; an XParity state as (|c> + sector |~c>) / sqrt 2 on its representatives."""
    L = sub.L
    full = np.zeros(1 << L, dtype=np.complex128)
    states = np.asarray(sub.idx_to_state(np.arange(sub.get_dimension())))
    if isinstance(sub, XParity):
        full[states] = x / np.sqrt(2)
        full[states ^ ((1 << L) - 1)] = sub.sector * x / np.sqrt(2)
    else:
        full[states] = x
    return full


def operand(full, L, keep):
    """m[a, t] = psi(a, t): bit i of the row index is spin keep[i]."""
    keep = list(keep)
    rest = [s for s in range(L) if s not in keep]
    axes = [L - 1 - s for s in reversed(keep)] + [L - 1 - s for s in reversed(rest)]
    return full.reshape((2,) * L).transpose(axes).reshape(1 << len(keep), -1)


def numpy_blocks(full, L, keep):
    m = operand(full, L, keep)
    pc = popcounts(len(keep))
    out = {}
    for n in range(len(keep) + 1):
        rows = m[pc == n]
        if np.any(rows):
            out[n] = rows @ rows.conj().T
    return out


def make(kind, L, k, seed, sector=None):
    sub = SpinConserve(L, k) if kind == "sc" else XParity(SpinConserve(L, k), sector)
    st = State(L=L, subspace=sub, state='random', seed=seed)
    return sub, st, embed(sub, st.to_numpy())


@functools.lru_cache(maxsize=None)
def sc_case(L, k):
    return make("sc", L, k, 100 + L + k)


@functools.lru_cache(maxsize=None)
def xp_case(sector):
    return make("xp", 12, 6, 7, sector)


def check_blocks(st, full, L, keep, err=1e-14):
    got = cp.reduced_density_matrix_sectors(st, keep)
    want = numpy_blocks(full, L, keep)
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    trace = 0.0
    for n in sorted(want):
        assert got[n].shape == want[n].shape == (comb(len(keep), n),) * 2
        d = np.max(np.abs(got[n] - want[n]))
        print("keep", list(keep), "n", n, "rows", got[n].shape[0], "max abs error %.2e" % d)
        assert d < err, (n, d)
        assert np.allclose(got[n], got[n].conj().T, atol=1e-17, rtol=0)
        assert np.all(np.diagonal(got[n]).imag == 0.0)
        trace += np.trace(got[n]).real
    assert abs(trace - 1) < 1e-13
    return got


SC_CASES = [
    (12, 6, list(range(6))),                      # blocks of 1, 6, 15, 20 rows: all under one tile; contiguous low keep
    (12, 6, list(range(6, 12))),                  # the other end: the general path
    (12, 6, [1, 4, 6]),
    (12, 6, [0, 2, 3, 7, 8, 11]),
    (16, 8, list(range(8))),                      # 70 rows: two tile rows with a ragged edge
    (20, 10, list(range(10))),                    # 252 rows: 4 x 4 tiles, ragged; 252 traced configurations; one launch
    (20, 10, [0, 1, 2, 3, 4, 10, 11, 12, 13, 14]),   # the same block sizes through the general path
    (14, 3, list(range(9))),                      # k < kept spins: blocks of 1, 9, 36, 84 rows, n = 4..9 infeasible
]


@gpu
@pytest.mark.parametrize("L,k,keep", SC_CASES)
def test_blocks_vs_numpy(L, k, keep):
    sub, st, full = sc_case(L, k)
    got = check_blocks(st, full, L, keep)
    lo, hi = max(0, k - (L - len(keep))), min(k, len(keep))
    assert sorted(got) == list(range(lo, hi + 1))
    if L == 12:
        # the blocks are all there is: the dense matrix is zero outside them and its spectrum is theirs
        dense = cp.reduced_density_matrix(st, keep)
        pc = popcounts(len(keep))
        assert np.abs(dense[pc[:, None] != pc[None, :]]).max() == 0.0
        for n, blk in got.items():
            idx = np.nonzero(pc == n)[0]
            assert np.max(np.abs(dense[np.ix_(idx, idx)] - blk)) < 1e-14
        w = np.sort(np.concatenate([np.linalg.eigvalsh(b) for b in got.values()]))
        assert w.shape == (1 << len(keep),) and np.max(np.abs(w - np.linalg.eigvalsh(dense))) < 1e-14


@gpu
def test_block_selection_and_arguments():
    import torch
    sub, st, full = sc_case(14, 3)
    keep = list(range(9))
    want = numpy_blocks(full, 14, keep)
    got = cp.reduced_density_matrix_sectors(st, keep, sectors=[3, 0])
    assert sorted(got) == [0, 3] and got[0].shape == (1, 1) and got[3].shape == (84, 84)
    assert np.max(np.abs(got[3] - want[3])) < 1e-14 and abs(got[0][0, 0] - want[0][0, 0]) < 1e-14
    dev = cp.reduced_density_matrix_sectors(st, keep, sectors=[2], on_device=True)
    assert torch.is_tensor(dev[2]) and dev[2].is_cuda and np.max(np.abs(dev[2].cpu().numpy() - want[2])) < 1e-14
    with pytest.raises(ValueError):
        cp.reduced_density_matrix_sectors(st, keep, sectors=[4])          # more set bits than the state has
    with pytest.raises(ValueError):
        cp.reduced_density_matrix_sectors(st, [3, 2])
    with pytest.raises(ValueError):
        cp.reduced_density_matrix_sectors(st, [0, 14])
    for other in (Full(L=8), Parity('even', L=8), XParity(Parity('even', L=8))):
        with pytest.raises(ValueError):
            cp.reduced_density_matrix_sectors(State(L=8, subspace=other, state='random', seed=1), [0, 1])
    assert cp.reduced_density_matrix_sectors(st, [])[0][0, 0] == 1


@gpu
@pytest.mark.parametrize("slices", ["3", "40"])
def test_blocks_several_slices(monkeypatch, slices):
    """The traced index cut into slices (3: 84 configurations per slice of the largest block, the smaller blocks' last
    slices short or empty; 40: more slices than the fan-in of the summation tree, most of them of one chunk or none)."""
    monkeypatch.setenv("DNM_RDM_SECTOR_SLICES", slices)
    sub, st, full = sc_case(20, 10)
    check_blocks(st, full, 20, list(range(10)))
    check_blocks(st, full, 20, [0, 1, 2, 3, 4, 10, 11, 12, 13, 14])


@gpu
@pytest.mark.parametrize("sector", [+1, -1])
def test_xparity_blocks_and_entropy(sector):
    sub, st, full = xp_case(sector)
    L = 12
    assert abs(np.vdot(full, full) - 1) < 1e-13
    for keep in (list(range(6)), list(range(6, 12)), [1, 4, 11]):
        got = check_blocks(st, full, L, keep)
        kA = len(keep)
        assert sorted(got) == list(range(kA + 1))
        for n in range(kA + 1):
            wa, wb = np.linalg.eigvalsh(got[n]), np.linalg.eigvalsh(got[kA - n])
            assert np.max(np.abs(wa - wb)) < 1e-13
        m = operand(full, L, keep)
        dense = m @ m.conj().T
        want = cp.dm_entanglement_entropy(dense)
        assert abs(cp.entanglement_entropy(st, keep) - want) < 1e-10
        assert abs(st.entanglement_entropy(keep) - want) < 1e-10
        assert abs(cp.renyi_entropy(st, keep, 2) - cp.dm_renyi_entropy(dense, 2)) < 1e-10
        w = cp.entanglement_spectrum(st, keep)
        assert w.shape == (1 << kA,) and np.max(np.abs(w - np.linalg.eigvalsh(dense))) < 1e-13
    with pytest.raises(ValueError):
        cp.reduced_density_matrix(st, [0])


@gpu
def test_more_than_fifteen_kept_spins():
    """SpinConserve(18, 2), 16 spins kept: blocks of 1, 16 and 120 rows where the dense form would be 2^16 square."""
    L, k, keep = 18, 2, list(range(16))
    sub, st, full = sc_case(L, k)
    m = full.reshape(4, 1 << 16).T
    pc = popcounts(16)
    want = []
    for n in range(3):
        rows = m[pc == n]
        assert rows.shape[0] == comb(16, n)
        want.append(np.linalg.eigvalsh(rows @ rows.conj().T))
    want = np.sort(np.concatenate(want))
    got = st.entanglement_spectrum(keep)
    assert got.shape == (137,) and np.all(np.diff(got) >= 0)
    assert np.max(np.abs(got - want)) < 1e-13
    assert abs(got.sum() - 1) < 1e-13
    blocks = cp.reduced_density_matrix_sectors(st, keep)
    assert {n: b.shape[0] for n, b in blocks.items()} == {0: 1, 1: 16, 2: 120}
    with pytest.raises((ValueError, _lib.BackendError)):
        cp.reduced_density_matrix(st, keep)


@gpu
def test_sector_route_changes_nothing():
    """SpinConserve(16, 8), 8 spins kept (2^8 = _DEVICE_EIG_FROM, where the dense route diagonalises block by block on
    the device): the entropies from the spectrum of the sector route against those of the dense matrix."""
    assert cp._DEVICE_EIG_FROM == 256
    sub, st, full = sc_case(16, 8)
    keep = list(range(8))
    dense = cp.reduced_density_matrix(st, keep)
    w = cp.entanglement_spectrum(st, keep)
    assert np.max(np.abs(w - np.linalg.eigvalsh(dense))) < 1e-13
    assert abs(cp._entropy_of_spectrum(w) - cp.dm_entanglement_entropy(dense)) < 1e-10
    assert abs(cp._renyi_of_spectrum(w, 2) - cp.dm_renyi_entropy(dense, 2)) < 1e-10
    assert abs(cp._entropy_of_spectrum(w) - cp.entanglement_entropy(st, keep)) < 1e-10
    wb = cp.entanglement_spectrum(st, list(range(8, 16)))
    assert abs(cp._entropy_of_spectrum(w) - cp._entropy_of_spectrum(wb)) < 1e-9
    # more than 15 spins kept: the entropy calls themselves take the blocks
    sub2, st2, _ = sc_case(18, 2)
    assert cp._takes_sector_route(st2, list(range(16))) and not cp._takes_sector_route(st, keep)
    sA, sB = cp.entanglement_entropy(st2, list(range(16))), cp.entanglement_entropy(st2, [16, 17])
    assert abs(sA - sB) < 1e-9 and sA > 0


@gpu
def test_xparity_entropy_against_free_fermions():
    """The ground state of 0.25 sum (XX + YY) on the open chain of 20 spins, found in XParity(SpinConserve(20, 10)): a
    filled Fermi sea, whose entropies across a cut follow from the correlation matrix of the block (Peschel)."""
    from dynamite_amd.config import config
    from dynamite_amd.operators import sigmax, sigmay, op_sum
    L, k = 20, 10
    j = np.arange(1, L + 1)
    modes = np.argsort(np.cos(np.pi * j / (L + 1)))[:k] + 1
    phi = np.sqrt(2.0 / (L + 1)) * np.sin(np.pi * np.outer(j, modes) / (L + 1))
    Cm = phi @ phi.T

    def peschel(nA):
        nu = np.linalg.eigvalsh(Cm[:nA, :nA])
        nu = nu[(nu > 1e-15) & (nu < 1 - 1e-15)]
        return float(-(nu * np.log(nu) + (1 - nu) * np.log(1 - nu)).sum())
    exact = np.sort(np.cos(np.pi * j / (L + 1)))[:k].sum()
    saved = config.L
    try:
        config.L = L
        best = None
        for sector in (+1, -1):
            sub = XParity(SpinConserve(L, k), sector)
            H = op_sum(0.25 * (sigmax(i) * sigmax(i + 1) + sigmay(i) * sigmay(i + 1)) for i in range(L - 1))
            H.L = L
            H.add_subspace(sub)
            ev, vecs = H.eigsolve(nev=1, tol=1e-11, getvecs=True, subspace=sub)
            if best is None or ev[0] < best[0]:
                best = (ev[0], vecs[0], sector)
            H.destroy_mat()
        print("ground state in sector", best[2], "energy", best[0], "exact", exact)
        assert abs(best[0] - exact) < 1e-9 * abs(exact)
        for nA in (10, 5):
            got = best[1].entanglement_entropy(list(range(nA)))
            print("kept", nA, "entropy", got, "Peschel", peschel(nA))
            assert abs(got - peschel(nA)) < 1e-7, (nA, got, peschel(nA))
    finally:
        config.L = saved


def test_sector_plan_abi():
    """dnm_rdm_sector_plan is host arithmetic: SpinConserve(36, 18), half cut, without a device."""
    lib = _lib.lib()
    spaces = {}

    def desc(sp):              # (the descriptor points into tables its subspace object owns: keep that alive)
        spaces[id(sp)] = sp
        return sp._to_c()['data']
    sub = desc(SpinConserve(36, 18))

    def plan(sub_c, keep, xsec=0):
        keep = np.ascontiguousarray(keep, dtype=np.int64)
        nb, scratch = C.c_int(), C.c_size_t()
        ns = (C.c_int32 * (keep.size + 1))()
        dims = np.zeros(keep.size + 1, dtype=np.int64)
        traced = np.zeros(keep.size + 1, dtype=np.int64)
        rc = lib.dnm_rdm_sector_plan(C.byref(sub_c), keep.size, _lib.p64(keep), xsec, C.byref(nb), ns,
                                     _lib.p64(dims), _lib.p64(traced), C.byref(scratch))
        return rc, nb.value, list(ns), dims, traced, scratch.value
    for xsec in (0, +1, -1):
        rc, nb, ns, dims, traced, scratch = plan(sub, np.arange(18), xsec)
        assert rc == 0 and nb == 19 and ns == list(range(19))
        assert list(dims) == [comb(18, n) for n in range(19)] and dims.max() == 48620
        assert list(traced) == [comb(18, 18 - n) for n in range(19)]
        assert scratch >= sum(((d + 63) // 64) * ((d + 63) // 64 + 1) // 2 for d in dims) * 64 * 64 * 16
    rc, nb, ns, dims, traced, _ = plan(desc(SpinConserve(14, 3)), np.arange(9))
    assert rc == 0 and nb == 4 and list(dims[:4]) == [1, 9, 36, 84] and list(traced[:4]) == [10, 10, 5, 1]
    rc = plan(sub, [0, 2, 1])[0]
    assert rc != 0 and b"strictly increasing" in lib.dnm_last_error()
    rc = plan(sub, [0, 36])[0]
    assert rc != 0 and b"out of range" in lib.dnm_last_error()
    rc = plan(desc(Parity('even', L=12)), [0, 1])[0]
    assert rc != 0 and b"SpinConserve" in lib.dnm_last_error()
    rc = plan(desc(SpinConserve(12, 5)), [0, 1], +1)[0]
    assert rc != 0 and b"XParity needs SpinConserve(L, L/2)" in lib.dnm_last_error()
    rc = plan(desc(SpinConserve(50, 25)), np.arange(41))[0]
    assert rc != 0 and b"at most 40" in lib.dnm_last_error()
    rc = plan(desc(SpinConserve(50, 25)), np.arange(36))[0]
    assert rc != 0 and b"2^31" in lib.dnm_last_error()
