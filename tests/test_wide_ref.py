"""The plain-Python references of tests/wide_ref.py against the oracle, bit for bit, for every (subspace, operator) pair
that tests/test_gpu_wide_sectors.py takes a reference for, and the conditions its exactness argument rests on."""
import numpy as np
import pytest

import wide_ref as w
from oracle import oracle as orc
from gpu_util import orc_sub

PAIRS = w.pairs_used()


def test_subspaces_are_what_they_say():
    for name, (L, k) in w.SC.items():
        sub = w.subspace(name)
        L_, st = w.states_of(name)
        assert L_ == L and all(w.popcount(s) == k for s in st) and st == sorted(st)
        assert np.array_equal(sub.idx_to_state(np.arange(len(st))), np.array(st, dtype=np.int64))
        assert ((k + 1) * (L + 1) > 2048) == (name in w.GLOBAL_TABLE)
    # SpinConserve(40, 38): one table fits the 2048 LDS entries of the gather kernels, two do not
    assert 39 * 41 <= 2048 < 2 * 39 * 41
    _, e = w.states_of('exp63')
    _, u = w.states_of('exp63_unsorted')
    assert sorted(u) == e and u != e and w.subspace('exp63_unsorted').rmap_indices is not None
    assert w.subspace('exp63').rmap_indices is None
    assert e[-1] >> 62 == 1 and e[0] < 1 << 16
    assert sum(1 for s in e if s >> 62) > 1 and any(s ^ ((1 << w.X_PRODUCT_SITES) - 1) in e for s in e)
    _, o = w.states_of('exp40_outsiders')
    sector = set(w.states_of('sc40_2')[1])
    assert sector < set(o) and 24 <= len(set(o) - sector) <= 64
    assert w.subspace('exp40_outsiders').rmap_indices is None


def test_operators_are_dyadic_and_take_the_paths_they_are_meant_for():
    for L in (34, 40, 50, 63):
        for op in ('chain', 'dm', 'far'):
            arrs = w.marshal(w.OPERATORS[op](L), L)
            terms = w.terms_of(arrs)                     # asserts eighths of magnitude at most 16
            masks = [m for m, _ in terms]
            assert masks[0] == 0 and all(3 << j in masks for j in range(L - 1))
            if op != 'far':
                assert len(masks) == L
            if op == 'dm':
                assert any(ci for _, ts in terms for _, _, ci in ts)
        masks = [m for m, _ in w.terms_of(w.marshal(w.far(L), L))]
        a, b, c, d = w.four_sites(L)
        assert len({a, b, c, d}) == 4
        assert 1 | 1 << (L - 1) in masks and (1 << a | 1 << b | 1 << c | 1 << d) in masks
        assert (((1 << 34) - 1) in masks) == (L <= 40)


@pytest.mark.parametrize("left,op,right,extra", PAIRS, ids=["-".join(str(v) for v in p if v) for p in PAIRS])
def test_reference_equals_the_oracle(left, op, right, extra):
    c = w.case(left, op, right, extra)
    ls, rs = c.subspaces()
    msc, lo, ro = orc.Msc(*c.arrs), orc_sub(ls), orc_sub(rs)
    assert (c.M, c.N) == (ls.get_dimension(), rs.get_dimension())
    x = w.int_vector(c.N, seed=c.N)
    y = w.apply(c, x)
    assert np.array_equal(y, orc.matvec(msc, lo, ro, x))
    assert np.array_equal(w.apply(c, x, 5, 40), y[5:45])
    assert w.infnorm(c) == orc.infnorm(msc, lo, ro)
    assert w.conserves(c)[0] is orc.check_conserves(msc, lo, ro)
    if left == right:
        assert np.array_equal(w.diagonal(c), orc.precompute_diagonal(msc, lo))
    # the exactness argument: room below 2^53
    assert np.max(np.abs(y.real)) < w.EXACT_BOUND and np.max(np.abs(y.imag)) < w.EXACT_BOUND
    if left == right:
        sums = w.fused_sums(x, y)
        assert np.max(np.abs(sums)) < w.EXACT_BOUND
        assert sums[0] == np.vdot(x, y).real and sums[1] == np.vdot(x, y).imag and sums[2] == np.vdot(y, y).real
    assert any(re or im for row in c.rows for col, re, im in row if col >= 0)


def test_verdicts_of_conserves():
    for s in w.SWEEP_SUBS:
        if s.startswith('sc'):
            assert w.conserves(w.case(s, 'chain'))[0] is True
            ok, cols = w.conserves(w.case(s, 'chain', extra='xtop'))
            assert ok is False and len(cols) == w.case(s, 'chain').N      # sigma-x takes every column out
    assert w.conserves(w.case('exp63', 'chain'))[0] is False


def test_windows_of_three_ranks_are_proper():
    """The shares of the partitioned GPU test read columns outside their own rows, and reach more than they need."""
    from dynamite_amd import backend
    for s in ('sc63_2', 'sc50_2'):
        c = w.case(s, 'far')
        for r in range(3):
            row0, m = backend.split_ownership(c.M, 3, r)
            reach, need = w.column_sets(c, row0, m)
            assert set(range(row0, row0 + m)) <= set(reach) and set(need) <= set(reach)
            assert reach[0] < row0 or reach[-1] >= row0 + m
        assert any(set(w.column_sets(c, *backend.split_ownership(c.M, 3, r))[0])
                   - set(w.column_sets(c, *backend.split_ownership(c.M, 3, r))[1]) for r in range(3))
