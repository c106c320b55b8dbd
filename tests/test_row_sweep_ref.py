"""The host references of tests/row_sweep_ref.py against the oracle, bit for bit, at the shapes the GPU tests of the row
sweeps use (tests/test_gpu_row_sweeps.py), and the properties of the planted cases those tests rely on."""
import numpy as np
import pytest

import row_sweep_ref as ref
from oracle import oracle as orc
from gpu_util import orc_sub


def orc_msc(arrs):
    return orc.Msc(*arrs)


def test_planted_row_is_the_unique_maximiser_full():
    """Full, L = 21, variant B: numpy and the oracle agree bit for bit, and the planted row alone holds the maximum."""
    for index in (0, 255, (1 << 20) - 1, 1 << 20, (1 << 21) - 1, (1 << 20) + 229):
        sub, arrs, rstar = ref.norm_case('full', index, 'B')
        s = ref.row_sums(arrs, sub, sub)
        live = (rstar & 1) != (rstar >> 1 & 1)
        assert s.max() == (3.124999523162842 if live else 2.874999523162842)
        assert np.flatnonzero(s == s.max()).tolist() == [index]
        assert np.sort(s)[-2] <= s.max() - 2.0 ** (1 - 21)
        assert s.max() == orc.infnorm(orc_msc(arrs), orc_sub(sub), orc_sub(sub))


@pytest.mark.parametrize("shape", ['parity', 'sc', 'explicit'])
def test_planted_row_other_shapes(shape):
    M = ref.NORM_DIMS[shape]
    for variant, index in (('A', ref.TRIP + 229), ('B', M - 1), ('B', 0)):
        sub, arrs, rstar = ref.norm_case(shape, index, variant)
        s = ref.row_sums(arrs, sub, sub)
        assert np.flatnonzero(s == s.max()).tolist() == [index]
        assert np.sort(s)[-2] <= s.max() - 2.0 ** (1 - sub.L)
        assert s.max() == orc.infnorm(orc_msc(arrs), orc_sub(sub), orc_sub(sub))
    d = ref.diagonal(arrs, sub)
    assert np.array_equal(d, orc.precompute_diagonal(orc_msc(arrs), orc_sub(sub)))


def test_explicit_placements_hold_the_planted_state():
    M = ref.NORM_DIMS['explicit']
    for index in ref.norm_placements(M):
        states, rstar = ref.explicit_with_planted(22, M, index, seed=7)
        assert states.size == M and states[index] == rstar and np.all(np.diff(states) > 0)
        assert all(rstar ^ p in states for p in ref.PARTNER_MASKS)


def test_diagonal_full():
    sub, arrs, _ = ref.norm_case('full', 12345, 'B')
    assert np.array_equal(ref.diagonal(arrs, sub), orc.precompute_diagonal(orc_msc(arrs), orc_sub(sub)))
    assert np.array_equal(ref.diagonal(arrs, sub, 1000, 777), ref.diagonal(arrs, sub)[1000:1777])


def test_all_sixteen_pairs():
    subs, rstar = ref.pair_subspaces()
    arrs = ref.planted_operator(13, rstar, 'A')
    for ln, left in subs.items():
        for rn, right in subs.items():
            s = ref.row_sums(arrs, left, right)
            assert np.flatnonzero(s == s.max()).tolist() == [int(left.state_to_idx(rstar))], (ln, rn)
            assert s.max() == orc.infnorm(orc_msc(arrs), orc_sub(left), orc_sub(right)), (ln, rn)
            assert np.array_equal(ref.row_sums(arrs, left, right, 300, 500), s[300:800])


def _fields(L, zero_at=None):
    from dynamite_amd.operators import identity
    H = ref.planted_fields(L, 0x1234)
    if zero_at is not None:
        H = H + (-zero_at) * identity()
    return ref.marshal(H, L)


def test_conserves_planted_column():
    L = 14
    arrs = _fields(L)
    for kind in ('full', 'parity', 'sc', 'explicit'):
        right = ref.conserves_sector(kind, L)
        N = right.get_dimension()
        whole = ref.explicit(ref.states_of(right), L)
        assert ref.conserves(arrs, whole, right)[0] is True
        assert orc.check_conserves(orc_msc(arrs), orc_sub(whole), orc_sub(right)) is True
        for j in ref.conserves_columns(N, sliced=True):
            left = ref.minus_one(right, j)
            ok, cols = ref.conserves(arrs, left, right)
            assert not ok and cols.tolist() == [j]
            assert orc.check_conserves(orc_msc(arrs), orc_sub(left), orc_sub(right)) is False
            # a diagonal whose value at that column is exactly zero: forgiven
            d = ref.diagonal(arrs, right, j, 1)[0]
            z = _fields(L, zero_at=d)
            assert ref.diagonal(z, right, j, 1)[0] == 0.0 and np.count_nonzero(ref.diagonal(z, right) == 0.0) == 1
            assert ref.conserves(z, left, right)[0] is True
            assert orc.check_conserves(orc_msc(z), orc_sub(left), orc_sub(right)) is True
    for kind in ('parity', 'sc'):
        n = ref.conserves_sector(kind, L).get_dimension() + 1
        for j in ref.conserves_columns(n, sliced=True):
            left, right = ref.plus_outsider(kind, j, L)
            ok, cols = ref.conserves(arrs, left, right)
            assert not ok and cols.tolist() == [j]
            assert orc.check_conserves(orc_msc(arrs), orc_sub(left), orc_sub(right)) is False


def test_conserves_imaginary_and_cancelling():
    from dynamite_amd.operators import sigmax, sigmay
    from dynamite_amd.subspaces import SpinConserve
    L = 14
    sub = SpinConserve(L, 7)
    imag = ref.marshal(sigmax(2) * sigmay(9) + sigmay(2) * sigmax(9), L)
    assert np.all(imag[3].real == 0)
    ok, cols = ref.conserves(imag, sub, sub)
    assert not ok and cols.size > 0
    assert orc.check_conserves(orc_msc(imag), orc_sub(sub), orc_sub(sub)) is False
    real = ref.marshal(sigmax(2) * sigmax(9) + sigmay(2) * sigmay(9), L)
    assert ref.conserves(real, sub, sub)[0] is True
    assert orc.check_conserves(orc_msc(real), orc_sub(sub), orc_sub(sub)) is True


def test_conserves_xparity():
    from dynamite_amd.subspaces import SpinConserve
    L = 14
    arrs = _fields(L)
    right = SpinConserve(L, 7)
    half = right.get_dimension() // 2
    for j, with_flag in ((half, True), (2 * half - 1, True), (half - 1, False), (0, False)):
        left = ref.minus_one(right, j)
        assert ref.conserves(arrs, left, right)[0] is False
        assert ref.conserves(arrs, left, right, xparity=True)[0] is with_flag
        assert orc.check_conserves(orc_msc(arrs), orc_sub(left), orc.xparity(orc_sub(right))) is with_flag


def test_far_column_case():
    sub, arrs = ref.far_column_case(255)
    n = sub.get_dimension()
    reach, need, cols = ref.column_sets(arrs, sub, sub, 0, 1001)
    assert ref.hull(reach) == (0, n - 1) and np.array_equal(reach, need)
    assert reach.tolist() == list(range(1001)) + [n - 1]
    assert ref.local_runs(cols, 0, 1001) == [(1, 4)]
    sub, arrs = ref.far_column_case(255, with_partner=False)
    assert ref.hull(ref.column_sets(arrs, sub, sub, 0, 1000)[0]) == (0, 999)


def test_run_selection():
    runs = [(0, 1), (2, 5), (7, 9), (10, 14)]
    assert ref.select_runs(runs, 3500, 8, 1) == [(0, 256), (512, 1280), (1792, 2304), (2560, 3500)]
    assert ref.select_runs(runs, 3500, 2, 2) == [(512, 1280), (2560, 3500)]
    assert ref.select_runs(runs, 3500, 1, 2) == [(2560, 3500)]
    assert ref.select_runs([(0, 2), (3, 5)], 1280, 1, 1) is None
    m = np.zeros(40, dtype=np.uint8)
    m[[0, 9, 39]] = 1
    assert ref.coarsen(m, 5, 3).tolist() == [1, 1, 0, 0, 0, 1]
