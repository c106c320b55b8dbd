"""tests/sc_rows_exact_ref.py -- the case table of tests/test_gpu_sc_rows_exact.py -- on the CPU:

  1. every (operator, L, k, sector) the GPU file takes a reference for is pinned to oracle.matvec bit for bit (the
     reference is tests/sc3_exact_ref.py, which asserts the 2^53 condition on the numbers of each case);
  2. from L, k and the block width alone: the block sizes C(lb, k - |H|) a case reaches, the register rows r // NT that
     hold live rows, which of the three block orders its handle runs and which workgroups return early -- the claims the
     GPU file's cases are named for;
  3. ``NEEDS``: what each kernel instance needs of the table as a whole, asserted here."""
from math import comb

import numpy as np
import pytest

import sc_rows_exact_ref as t
import sc3_exact_ref as ref
from oracle import oracle as orc


def _oracle(r, x):
    sub = orc.spin_conserve(r.L, r.k)
    if r.sector is not None:
        sub = orc.xparity(sub)
    return orc.matvec(orc.Msc(*r.arrs), sub, sub, x, nthreads=min(8, orc.max_threads()))


@pytest.mark.parametrize("pair", t.pairs_used(), ids=lambda p: "%s-%d-%d%s" % (p[0], p[1], p[2], p[3] or ""))
def test_reference_is_the_oracle(pair):
    r = t.get(*pair)
    p = t.product(*pair)
    hx = _oracle(r, np.array(p.x))
    assert np.array_equal(p.y, hx)
    assert np.array_equal(p.y_z, hx - ref.B * p.z)
    assert np.array_equal(p.y_z2, (hx - ref.B * p.z) + p.c * p.z2)
    for y, sums in ((p.y, p.sums), (p.y_z, p.sums_z)):
        d = np.sum(np.conj(p.x).astype(np.clongdouble) * y.astype(np.clongdouble))
        n2 = np.sum(y.real.astype(np.longdouble) ** 2 + y.imag.astype(np.longdouble) ** 2)
        assert (float(d.real), float(d.imag), float(n2)) == tuple(sums.tolist())
    if r.N > 1 << 20:
        ref.release()


@pytest.mark.parametrize("pair", sorted({p[:4] for p in t.PLANTED}, key=str), ids=str)
def test_columns_are_the_products_of_unit_vectors(pair):
    r = t.get(*pair)
    for j in (0, r.N // 3, r.N - 1):
        e = np.zeros(r.N, dtype=np.complex128)
        e[j] = 1
        rows, vals = r.column(j)
        got = np.zeros(r.N, dtype=np.complex128)
        got[rows] = vals
        assert np.array_equal(got, _oracle(r, e))


def test_far_small_is_what_it_says():
    """All real, eighths (wide_ref.terms_of asserted it when the Ref was built), 23 masks at (17, 13): the diagonal, 16
    adjacent bonds -- fast --, and two far hops and the four-site term -- not fast, one of the hops across the block
    boundary, the four-site term on both sides of it."""
    r = t.get('far13', 17, 7)
    assert not r.arrs[3].imag.any()
    fast = [m for m, ts in r.terms if t.is_fast(m, ts)]
    slow = [m for m, ts in r.terms if m and not t.is_fast(m, ts)]
    assert sorted(fast) == [3 << j for j in range(16)]
    assert sorted(slow) == sorted([1 | 1 << 16, 1 << 11 | 1 << 14, 1 | 1 << 12 | 1 << 13 | 1 << 16])
    r = t.get('far10', 14, 6)
    assert sorted(m for m, ts in r.terms if m and not t.is_fast(m, ts)) == sorted([1 | 1 << 13, 1 << 8 | 1 << 11,
                                                                                  1 | 1 << 9 | 1 << 10 | 1 << 13])
    assert len(t.get('graph70', 14, 6).terms) == 71


# ---------------------------------------------------------------- what each case reaches

def test_block_shapes_fill_every_register_row():
    """(14, 6) at 10 bits: blocks of 210, 252, 210, 120, 45 rows by the set bits of the high part; (17, 7) at 13 bits:
    1716, 1716, 1287, 715, 286.  Both reach all four register rows, the last one ragged."""
    for lb, want in ((10, [210, 252, 210, 120, 45]), (13, [1716, 1716, 1287, 715, 286])):
        L, k = t.BLOCK_SHAPES[lb]
        p = t.plan_of(t.get('dm', L, k), lb, order=0)
        p.check()
        assert sorted(set(p.sizes())) == sorted(set(want)) == sorted({comb(lb, k - j) for j in range(5)})
        assert p.register_rows() == [0, 1, 2, 3] and p.ragged()
        assert max(p.sizes()) == comb(lb, lb // 2) and max(p.sizes()) > 3 * t.NT[lb]
        assert (p.kind, p.swizzle, p.nperm, p.grid) == ('ascending', 0, 0, 16)
        q = t.plan_of(t.get('dm', L, k), lb, order=3)
        q.check()
        assert q.kind == 'permutation' and q.grid == q.nperm and q.early() == q.nperm - 16


def test_edge_sectors():
    for (L, k), sizes in (((14, 1), {1, 10}), ((14, 13), {1, 10}), ((12, 0), {1}), ((12, 12), {1})):
        p = t.plan_of(t.get('dm', L, k), 10, order=0)
        p.check()
        assert set(p.sizes()) == sizes and p.kind == 'ascending'


def test_swizzled_orders():
    """DNM_SC_ORDER=0 from 1024 high parts on: (20, 10) exactly 1024; (21, 10): span 2047, the grid is 2048 and the last
    workgroup has no block; (23, 3) / (23, 20) at 13 bits: 1024 workgroups of which 176 hold rows."""
    p = t.plan_of(t.get('dm', 20, 10), 10, order=0)
    p.check()
    assert (p.kind, p.h_first, p.h_last, p.grid, p.early()) == ('swizzle', 0, 1023, 1024, 0)
    assert not np.array_equal(p.visits, np.arange(1024))
    p = t.plan_of(t.get('dm', 21, 10), 10, order=0)
    p.check()
    assert (p.kind, p.h_first, p.h_last, p.grid) == ('swizzle', 0, 2046, 2048) and p.visits[-1] == -1 and p.early() == 1
    # (23, 20): the high parts run from 127 (seven ones) to 1023, the first is rounded down to 0: 1024 workgroups, 176 with
    # rows.  (23, 3) has its last high part at 0b1110000000 = 896: 897 workgroups in ASCENDING order, 176 with rows, the
    # others return early all the same; (24, 3) -- last high part 1792 -- is the few-ones sector under the swizzle.
    held = sum(comb(10, j) for j in range(4))
    p = t.plan_of(t.get('dm', 23, 20), 13, order=0)
    p.check()
    assert (p.kind, p.h_first, p.grid, p.early(), len(p.blocks)) == ('swizzle', 0, 1024, 1024 - held, held)
    p = t.plan_of(t.get('dm', 23, 3), 13, order=0)
    p.check()
    assert (p.kind, p.h_first, p.grid, p.early(), len(p.blocks)) == ('ascending', 0, 897, 897 - held, held)
    p = t.plan_of(t.get('dm', 24, 3), 13, order=0)
    p.check()
    held = sum(comb(11, j) for j in range(4))
    assert (p.kind, p.h_first, p.grid, p.early(), len(p.blocks)) == ('swizzle', 0, 2048, 2048 - held, held)


def test_default_orders():
    """g = 6 from 1024 high parts on; the production instance chooses 13 bits and a permutation by itself."""
    r = t.get('dm', 20, 10)
    p = t.plan_of(r, 10)
    p.check()
    assert p.kind == 'permutation' and p.swizzle == 1 and p.nperm >= 1024
    q = t.plan_of(r, 10, chunk=4)
    q.check()
    assert q.kind == 'permutation' and not np.array_equal(p.perm, q.perm)
    c = t.PRODUCTION
    r = t.get(c['op'], c['L'], c['k'])
    assert r.N == 1352078 and t.chosen_block(r, None) == 13
    p = t.plan_of(r, 13)
    p.check()
    assert p.kind == 'permutation' and p.h_last - p.h_first + 1 == 1024
    assert max(p.sizes()) == 1716 and p.register_rows() == [0, 1, 2, 3]
    ref.release()


def test_fallbacks_and_choices():
    for c in t.FALLBACK:
        assert t.chosen_block(t.get(c['op'], c['L'], c['k']), c['block']) == 0, c
    for c in t.CASES.values():
        lb = t.chosen_block(t.get(c['op'], c['L'], c['k'], c['sector']), c['block'])
        assert lb == (c['block'] or 0) or c in t.FALLBACK or c is t.PRODUCTION, c


def test_shares_cut_blocks():
    """The ownership boundaries of every share of the table fall inside a block."""
    from dynamite_amd import backend
    for op, L, k, lb, order, Ps in t.SHARES:
        r = t.get(op, L, k)
        for P in Ps:
            cut, kinds = 0, set()
            for q in range(P):
                row0, m = backend.split_ownership(r.N, P, q)
                p = t.plan_of(r, lb, order, None, row0, m)
                cut += len(p.partial())
                kinds.add(p.kind)
                assert set(p.blocks) <= set(p.visits[p.visits >= 0].tolist())
            assert cut >= P, (L, k, P, cut)
            assert ('swizzle' in kinds) == ((L, k) in t.SWIZZLED_SHARES), (L, k, P, kinds)


# ---------------------------------------------------------------- the table as a whole

def _reached(lb):
    out = dict(register_rows=set(), ragged=False, full=0, orders=set(), early=False, last=False, holes=False,
               sizes=set(), arms=set())
    for c in t.CASES.values():
        r = t.get(c['op'], c['L'], c['k'], c['sector'])
        if t.chosen_block(r, c['block']) != lb:
            continue
        out['arms'] |= t.arms(r, lb)
        if lb == 0:
            continue
        p = t.plan_of(r, lb, c['order'], c['chunk'])
        p.check()
        out['register_rows'] |= set(p.register_rows())
        out['ragged'] |= p.ragged()
        out['full'] = max(out['full'], max(p.sizes()))
        out['orders'].add(p.kind)
        out['early'] |= p.early() > 0
        out['last'] |= p.kind == 'swizzle' and p.visits[-1] < 0 and p.h_first + p.grid - 1 > p.h_last
        out['holes'] |= p.perm is not None and bool((p.perm == t.HOLE).any())
        out['sizes'] |= set(p.sizes())
        if r.N > 1 << 20:
            ref.release()
    return out


@pytest.mark.parametrize("lb", [10, 13])
def test_block_instances_get_what_they_need(lb):
    need, got = t.NEEDS[lb], _reached(lb)
    assert sorted(got['register_rows']) == need['register_rows'] and got['ragged'] == need['ragged']
    assert got['full'] == need['full_block'] == comb(lb, lb // 2)
    assert got['orders'] == need['orders']
    assert got['early'] and got['holes']
    assert got['last'] or not need['no_block_for_last_workgroup']
    assert {1, lb} <= got['sizes'] or not need['sizes_one_and_lb']
    assert got['arms'] == need['arms'], (need['arms'] - got['arms'], got['arms'] - need['arms'])


def test_row_kernels_get_what_they_need():
    need, got = t.NEEDS[0], _reached(0)
    assert got['arms'] == need['arms'], (need['arms'] - got['arms'], got['arms'] - need['arms'])
    rows = [c for c in t.CASES.values() if c['block'] == 0]
    assert {max(0, c['L'] - 16) for c in rows if c['sector'] is None} == need['walk_steps']
    assert any(t.get(c['op'], c['L'], c['k'], c['sector']).N % 256 for c in rows)
    assert {c['fuse'] for c in rows} == {True, False}
