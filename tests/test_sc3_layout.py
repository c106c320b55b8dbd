"""
Host logic of the SpinConserve internal vector layout (dynamite_amd/csrc/sc3.h) -- no GPU needed: the position map
is a bijection onto the non-padding slots that keeps the reference order (bsubspace_impl.h:187-245) at the level of
the top-bit blocks and inside every row, partitions hand whole blocks to the ranks, and a host-only handle of
BASELINE config 5 (SpinConserve(36, 18) on 8 ranks) plans the two tiled passes and its column windows.
"""
import ctypes as C
import math

import numpy as np
import pytest

from dynamite_amd import _lib, backend, models, msc_tools
from dynamite_amd.subspaces import SpinConserve


def _desc(L, k, a, w):
    sub = SpinConserve(L, k)
    d = _lib.Subspace.from_buffer_copy(sub._c())
    d.vec_swizzle = a | (w << 8)
    return sub, d


def _positions(d, n, part=None):
    idx = np.arange(n, dtype=np.int64)
    pos = np.empty_like(idx)
    _lib.check(_lib.lib().dnm_vec_layout_positions_host(C.byref(d), C.byref(part) if part is not None else None, n,
                                                        _lib.p64(idx), _lib.p64(pos)))
    return pos


@pytest.mark.parametrize("L,k,a,w", [(11, 5, 6, 4), (12, 6, 6, 4), (13, 3, 6, 4), (14, 7, 5, 4), (12, 0, 6, 4), (12, 12, 6, 4)])
def test_positions_are_a_bijection_that_keeps_rows_together(L, k, a, w):
    sub, d = _desc(L, k, a, w)
    n = sub.get_dimension()
    nint = C.c_int64()
    _lib.check(_lib.lib().dnm_vec_layout_size(C.byref(d), C.byref(nint)))
    pos = _positions(d, n)
    assert len(np.unique(pos)) == n and pos.min() >= 0 and pos.max() < nint.value
    assert nint.value >= n and nint.value % 8 == 0
    states = sub.idx_to_state(np.arange(n))
    # inside a row (equal bits above Lo) consecutive states sit at consecutive positions, rows start on 128-byte lines
    hi = states >> a
    same_row = hi[1:] == hi[:-1]
    assert np.all(pos[1:][same_row] == pos[:-1][same_row] + 1)
    first = np.concatenate(([True], ~same_row))
    assert np.all(pos[first] % 8 == 0)
    # blocks of equal top bits stay in the reference's order and are contiguous
    T = states >> (a + w)
    for t in np.unique(T):
        p = pos[T == t]
        later = pos[T > t]
        assert later.size == 0 or p.max() < later.min()
    # inside a block the rows are grouped by popcount(W), ascending
    W = (states >> a) & ((1 << w) - 1)
    cw = np.array([bin(int(v)).count('1') for v in W])
    for t in np.unique(T):
        sel = T == t
        order = np.argsort(pos[sel], kind='stable')
        assert np.all(np.diff(cw[sel][order]) >= 0)


@pytest.mark.parametrize("P", [2, 3, 8])
def test_partition_gives_whole_blocks(P):
    L, k, a, w = 14, 7, 6, 4
    sub, d = _desc(L, k, a, w)
    n = sub.get_dimension()
    nint = C.c_int64()
    _lib.check(_lib.lib().dnm_vec_layout_size(C.byref(d), C.byref(nint)))
    states = sub.idx_to_state(np.arange(n))
    gpos = _positions(d, n)
    i_end = n_end = 0
    for r in range(P):
        istart, ilen, nstart, nlen = backend.layout_partition(d, P, r)
        assert istart == i_end and nstart == n_end          # contiguous in both index spaces
        i_end, n_end = istart + ilen, nstart + nlen
        if nlen:
            T = states[nstart:nstart + nlen] >> (a + w)
            others = np.concatenate((states[:nstart], states[nstart + nlen:])) >> (a + w)
            assert not np.intersect1d(T, others).size       # whole blocks of equal top bits
            part = _lib.Partition(r, P)
            lp = _positions(d, nlen, part)
            assert np.array_equal(lp + istart, gpos[nstart:nstart + nlen])
    assert i_end == nint.value and n_end == n


def test_config5_plan_on_the_host():
    """SpinConserve(36, 18) on 8 ranks (BASELINE configs[4]) in the (14, 10) layout: 0.2 % padding, ranks balanced to a
    block, the two tiled passes planned, and what a rank reads beyond its own part."""
    L, k, a, w, P = 36, 18, 14, 10, 8
    sub, d = _desc(L, k, a, w)
    dim = math.comb(L, k)
    nint = C.c_int64()
    _lib.check(_lib.lib().dnm_vec_layout_size(C.byref(d), C.byref(nint)))
    assert dim < nint.value < dim * 1.004
    H = models.heisenberg(L)
    H.establish_L()
    H.reduce_msc()
    masks, offs = msc_tools.get_mask_offsets(H.msc)
    parts = [backend.layout_partition(d, P, r) for r in range(P)]
    lens = [p[1] for p in parts]
    assert max(lens) - min(lens) < 0.01 * nint.value / P
    assert sum(p[3] for p in parts) == dim
    for r in (0, 3, 7):
        h = backend.create_mat(masks, offs, H.msc['signs'], H.msc['coeffs'], d, d, False, _lib.MAT_HOST_ONLY, r, P)
        buf = C.create_string_buffer(4096)
        _lib.check(_lib.lib().dnm_mat_plan_describe(h, buf, len(buf)))
        s = buf.value.decode()
        assert "two-pass" in s and "[T 12 | W 10 | Lo 14]" in s and "13 gathered" not in s
        row0, ml = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().dnm_mat_ownership(h, C.byref(row0), C.byref(ml)))
        assert (row0.value, ml.value) == parts[r][:2]
        lo, hi = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().dnm_mat_column_window(h, C.byref(lo), C.byref(hi), None))
        assert lo.value <= row0.value and hi.value >= row0.value + ml.value - 1
        assert hi.value - lo.value + 1 <= nint.value
        _lib.check(_lib.lib().dnm_mat_destroy(h))


def test_layout_choice_depends_on_rank_count():
    """The internal layout hands whole top-bit blocks to a rank, 2^(L - 24) of them under (14, 10): it is taken on
    several ranks only where no rank stays empty and the largest share is within 10 % of the mean
    (SpinConserve.layout_usable); elsewhere vectors stay in reference order, split as PETSc splits them."""
    from dynamite_amd.subspaces import SpinConserve
    from dynamite_amd import backend, _lib
    import dynamite_amd.subspaces as S
    usable = {(26, 13, 4): False, (26, 13, 8): False, (27, 13, 8): False, (28, 14, 8): False, (28, 14, 2): True,
              (32, 16, 8): True, (34, 17, 8): True, (36, 18, 8): True, (36, 18, 4): True, (30, 15, 4): True,
              (26, 13, 1): True}
    for (L, k, P), want in usable.items():
        sub = SpinConserve(L, k)
        assert sub.layout_usable(14, 10, P) == want, (L, k, P)
        if P > 1:
            d = _lib.Subspace()
            d.type, d.L, d.k, d.ld_nchoosek = S.SPIN_CONSERVE, L, k, L + 1
            d.nchoosek = _lib.p64(sub._nchoosek)
            d.vec_swizzle = 14 | (10 << 8)
            rows = [backend.layout_partition(d, P, q)[3] for q in range(P)]
            assert sum(rows) == sub.get_dimension()
            assert want == (min(rows) > 0 and max(rows) <= 1.10 * sum(rows) / P)
    # one rank: the production choice is the internal layout from 2^22 states on
    assert SpinConserve(26, 13).vec_swizzle == (14 | (10 << 8)) and SpinConserve(24, 12).vec_swizzle == 0


# ---- site relabelling (dnm_subspace.site_perm, csrc/sc3_perm.cpp) -- host logic ---------------------------------

def _kagome_masks(name):
    from dynamite_amd import lattices
    n, edges = lattices.kagome(name)
    return n, np.array(sorted((1 << i) | (1 << j) for i, j in edges), dtype=np.int64)


def test_lattice_generator_matches_the_reference_edge_lists():
    """dynamite_amd/lattices.py against the edge lists the reference's lattice_library.basis_to_graph produces for every
    cluster of its library (tests/golden/kagome_edges.json, generated by make_golden.py): same vertex numbering."""
    import json
    import os
    from dynamite_amd import lattices
    ref = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kagome_edges.json")))
    assert set(ref) == set(lattices.KAGOME_CLUSTERS)
    for name, d in ref.items():
        n, edges = lattices.kagome(name)
        assert n == d["n"] and [list(e) for e in edges] == d["edges"], name
        deg = np.bincount(np.array(edges).ravel(), minlength=n)
        assert np.all(deg == 4)


def test_positions_under_a_site_relabelling():
    """With site_perm the position of reference index i is the plain layout's position of the state with its bits moved
    (spin s -> bit perm[s]); the map stays a bijection onto the non-padding slots."""
    L, k, a, w = 13, 6, 6, 4
    sub, d = _desc(L, k, a, w)
    n = sub.get_dimension()
    plain = _positions(d, n)
    rs = np.random.RandomState(3)
    for _ in range(3):
        perm = rs.permutation(L).astype(np.int8)
        dp = backend.with_site_perm(d, perm)
        assert backend.site_perm_of(dp) == tuple(int(b) for b in perm)
        pos = _positions(dp, n)
        assert len(np.unique(pos)) == n
        states = sub.idx_to_state(np.arange(n))
        moved = np.zeros_like(states)
        for s in range(L):
            moved |= ((states >> s) & 1) << int(perm[s])
        assert np.array_equal(pos, plain[sub.state_to_idx(moved)])
    ident = backend.with_site_perm(d, np.arange(L, dtype=np.int8))
    assert backend.site_perm_of(ident) is None and np.array_equal(_positions(ident, n), plain)
    bad = backend.with_site_perm(d, np.zeros(L, dtype=np.int8))
    with pytest.raises(_lib.BackendError):
        _positions(bad, 4)


def test_site_relabelling_is_chosen_deterministically_and_keeps_chains():
    """dnm_sc_choose_site_perm: a permutation of the spins; the identity for a nearest-neighbour chain (ties keep it,
    so chains keep their kernels); for the kagome tori no more hops between fields than the identity leaves, the same
    answer on every call; under fix_top spin L-1 stays (XParity), also when the masks are the flip-composed ones."""
    chain = np.array([3 << i for i in range(29)], dtype=np.int64)
    perm, counts = backend.choose_site_perm(chain, 30, 14, 10)
    assert np.array_equal(perm, np.arange(30)) and counts == [13, 9, 5, 1, 0, 1]

    def crossing(masks, perm, a=14, w=10):
        f = lambda b: 0 if b < a else (1 if b < a + w else 2)       # noqa: E731
        n = 0
        for m in masks.tolist():
            bits = [b for b in range(64) if (m >> b) & 1]
            n += f(int(perm[bits[0]])) != f(int(perm[bits[1]]))
        return n
    for name in ("27b", "30", "36a"):
        n, masks = _kagome_masks(name)
        perm, counts = backend.choose_site_perm(masks, n, 14, 10)
        assert sorted(perm.tolist()) == list(range(n)) and sum(counts) == len(masks)
        assert counts[3] + counts[4] + counts[5] == crossing(masks, perm) <= crossing(masks, np.arange(n))
        again, _ = backend.choose_site_perm(masks, n, 14, 10)
        assert np.array_equal(perm, again)
    n, masks = _kagome_masks("30")
    perm, counts = backend.choose_site_perm(masks, n, 14, 10, fix_top=True)
    assert perm[n - 1] == n - 1
    # XParity's reduced masks: a hop that touches spin L-1 comes as every spin but the pair (subspaces.py:632-674)
    allm = (1 << n) - 1
    reduced = np.array(sorted(m if not (m >> (n - 1)) & 1 else m ^ allm for m in masks.tolist()), dtype=np.int64)
    perm2, counts2 = backend.choose_site_perm(reduced, n, 14, 10, fix_top=True)
    assert np.array_equal(perm, perm2) and counts == counts2


def test_bond_graph_operator_plans_on_the_host():
    """A host-only handle of the 30-site kagome operator in the relabelled (14, 10) layout: bond-graph passes, the hop
    counts of the chooser; with XParity on top the flip-composed hops are gathered; the long-range model of the
    reference's harness (single-spin fields never act inside the subspace) is a chain with a cached diagonal."""
    H = models.kagome("30")
    H.establish_L()
    H.reduce_msc()
    masks, offs = msc_tools.get_mask_offsets(H.msc)
    sub, d = _desc(30, 15, 14, 10)
    perm, counts = backend.choose_site_perm(masks, 30, 14, 10)
    dp = backend.with_site_perm(d, perm)
    h = backend.create_mat(masks, offs, H.msc['signs'], H.msc['coeffs'], dp, dp, False, _lib.MAT_HOST_ONLY, 0, 1)
    buf = C.create_string_buffer(4096)
    _lib.check(_lib.lib().dnm_mat_plan_describe(h, buf, len(buf)))
    desc = buf.value.decode()
    assert "bond graph" in desc and "[T 6 | W 10 | Lo 14]" in desc and "real symmetric" in desc
    assert "%d hops in LDS, %d gathered) then lo pass" % (counts[1], counts[2] + counts[5]) in desc
    assert "%d hops in LDS, %d gathered), diagonal cached" % (counts[0], counts[3] + counts[4]) in desc
    _lib.check(_lib.lib().dnm_mat_destroy(h))
    # XParity: reduce the operator as subspaces.XParity does, spin L-1 fixed
    from dynamite_amd.subspaces import XParity
    xp = XParity(SpinConserve(30, 15), '-')
    red = xp.reduce_msc(H.msc)
    rmasks, roffs = msc_tools.get_mask_offsets(red)
    permx, cx = backend.choose_site_perm(rmasks, 30, 14, 10, fix_top=True)
    dx = backend.with_site_perm(d, permx)
    h = backend.create_mat(rmasks, roffs, red['signs'], red['coeffs'], dx, dx, True, _lib.MAT_HOST_ONLY, 0, 1)
    _lib.check(_lib.lib().dnm_mat_plan_describe(h, buf, len(buf)))
    assert "bond graph" in buf.value.decode()
    M, N, m, n = (C.c_int64() for _ in range(4))
    _lib.check(_lib.lib().dnm_mat_sizes(h, C.byref(M), C.byref(N), C.byref(m), C.byref(n)))
    nint = C.c_int64()
    _lib.check(_lib.lib().dnm_vec_layout_size(C.byref(d), C.byref(nint)))
    assert M.value == math.comb(30, 15) // 2 and m.value == nint.value // 2        # the layout's first half
    _lib.check(_lib.lib().dnm_mat_destroy(h))
    Hl = models.bench_long_range(28)
    Hl.establish_L()
    Hl.reduce_msc()
    lm, lo = msc_tools.get_mask_offsets(Hl.msc)
    _, d28 = _desc(28, 14, 14, 10)
    assert np.array_equal(backend.choose_site_perm(lm, 28, 14, 10)[0], np.arange(28))
    h = backend.create_mat(lm, lo, Hl.msc['signs'], Hl.msc['coeffs'], d28, d28, False, _lib.MAT_HOST_ONLY, 0, 1)
    _lib.check(_lib.lib().dnm_mat_plan_describe(h, buf, len(buf)))
    assert "two-pass kernels, internal layout" in buf.value.decode() and "diagonal cached" in buf.value.decode()
    _lib.check(_lib.lib().dnm_mat_destroy(h))


# ---- block ranges are PLACES of the block sequence; a share in block order 1 has no reference side --------------------

def _order1(d):
    d1 = _lib.Subspace.from_buffer_copy(d)
    d1.vec_swizzle = int(d.vec_swizzle) | (1 << 16)
    return d1


@pytest.mark.parametrize("L,k", [(15, 7), (16, 8), (17, 8)])
def test_positions_of_a_share_without_a_reference_side_are_refused(L, k):
    """Block order 1 (the solver's partition, csrc/sc3.h: sc3_code_order): a rank's share is no range of the reference
    order, so local reference indices mean nothing there -- dnm_vec_layout_positions_host refuses every share of P > 1
    ranks (rank 0 too: its blocks are not the first rows either), as its device twin does; it used to answer with the
    positions of the indices shifted by nstart = -1.  Whole vectors in order 1 and every share in order 0 keep working
    and stay bijections onto the same positions."""
    sub, d = _desc(L, k, 6, 4)
    d1 = _order1(d)
    n = sub.get_dimension()
    nint = C.c_int64()
    _lib.check(_lib.lib().dnm_vec_layout_size(C.byref(d1), C.byref(nint)))
    p0, p1 = _positions(d, n), _positions(d1, n)
    for p in (p0, p1, _positions(d1, n, _lib.Partition(0, 1))):
        assert len(np.unique(p)) == n and p.min() >= 0 and p.max() < nint.value
    assert not np.array_equal(p0, p1) and np.array_equal(p1, _positions(d1, n, _lib.Partition(0, 1)))
    ragged = 0
    for P in (2, 3):
        seen = []
        for r in range(P):
            istart, ilen, nstart, nlen = backend.layout_partition(d1, P, r)
            assert nstart == (0 if r == 0 else -1) and nlen > 0
            with pytest.raises(_lib.BackendError, match="block order 1"):
                _positions(d1, nlen, _lib.Partition(r, P))
            # the share's rows are the reference indices whose whole-vector position lies in its range of the layout
            rows = np.flatnonzero((p1 >= istart) & (p1 < istart + ilen))
            assert rows.size == nlen
            seen.append(rows)
            # order 0: the local map is the whole map cut at the share
            i0, il0, ns0, nl0 = backend.layout_partition(d, P, r)
            assert np.array_equal(_positions(d, nl0, _lib.Partition(r, P)) + i0, p0[ns0:ns0 + nl0])
        assert np.array_equal(np.sort(np.concatenate(seen)), np.arange(n))
        ragged += sum(int(rows[-1] - rows[0] + 1 != rows.size) for rows in seen[1:])
    assert ragged >= 2          # (not vacuous: shares beyond the first that are no range of the reference order)


def _xparity_arrays(L):
    """The Heisenberg chain reduced as XParity(SpinConserve(L, L/2), '+') reduces it."""
    from dynamite_amd.subspaces import XParity
    H = models.heisenberg(L)
    H.establish_L()
    H.reduce_msc()
    red = XParity(SpinConserve(L, L // 2), '+').reduce_msc(H.msc)
    masks, offs = msc_tools.get_mask_offsets(red)
    return masks, offs, red['signs'], red['coeffs']


@pytest.mark.parametrize("L", [14, 22, 24])
def test_xparity_handle_takes_the_half_whose_top_bit_is_clear(L):
    """XParity on top of SpinConserve(L, L/2) in the (6, 4) layout: the handle's vectors are the blocks whose top bit is
    clear.  From L = 22 on the layout has empty blocks (k > a + w: T = 0 at L = 22, every T with fewer than two ones at
    L = 24), the block sequence is shorter than 2^t and the half ends at a PLACE below 2^(t-1): the handle used to take
    the place 2^(t-1) and with it blocks of the other half.  Its sizes are those of the first of two shares
    (dnm_vec_layout_partition, what backend.Vec sizes an XParity vector by), half of both index spaces."""
    sub, d = _desc(L, L // 2, 6, 4)
    dim = sub.get_dimension()
    nint = C.c_int64()
    _lib.check(_lib.lib().dnm_vec_layout_size(C.byref(d), C.byref(nint)))
    T, ib = backend.layout_blocks(d)
    t = L - 10
    assert (T.size < 1 << t) == (L >= 22) and np.all(np.diff(T) > 0)
    place = int((T < 1 << (t - 1)).sum())
    assert (place < 1 << (t - 1)) == (L >= 22)
    istart, ilen, nstart, nlen = backend.layout_partition(d, 2, 0)
    assert (istart, nstart) == (0, 0) and nlen == dim // 2 and ilen == nint.value // 2 == ib[place]
    h = backend.create_mat(*_xparity_arrays(L), d, d, True, _lib.MAT_HOST_ONLY, 0, 1)
    M, N, m, n = (C.c_int64() for _ in range(4))
    _lib.check(_lib.lib().dnm_mat_sizes(h, C.byref(M), C.byref(N), C.byref(m), C.byref(n)))
    row0, ml = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().dnm_mat_ownership(h, C.byref(row0), C.byref(ml)))
    lo, hi = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().dnm_mat_column_window(h, C.byref(lo), C.byref(hi), None))
    _lib.check(_lib.lib().dnm_mat_destroy(h))
    assert (M.value, N.value) == (nlen, nlen) and (m.value, n.value) == (ilen, ilen)
    assert (row0.value, ml.value) == (0, ilen)
    assert (lo.value, hi.value) == (0, ilen - 1)          # the flip-composed hops stay inside the half
    # ... and no XParity handle on a descriptor in block order 1, where that half is no range of the layout
    with pytest.raises(_lib.BackendError, match="block order 1"):
        backend.create_mat(*_xparity_arrays(L), _order1(d), _order1(d), True, _lib.MAT_HOST_ONLY, 0, 1)


@pytest.mark.parametrize("a,w", [(6, 4), (14, 10)])
def test_first_half_by_places_is_closed_under_the_complement(a, w):
    """SpinConserve(L, L/2), every even L the layout takes (one to fifteen bits of T) up to 26: the first of two shares (whole blocks, cut by
    places of the block sequence) ends exactly where T's top bit turns on -- half the positions, half the states, no
    state of it has bit L-1 set, the next state has -- so the global flip maps the share onto the other one, which is
    what XParity on top of the layout rests on."""
    for L in range(a + w + 2 - (a + w) % 2, min(26, a + w + 15) + 1, 2):       # (1 <= t <= 15)
        sub, d = _desc(L, L // 2, a, w)
        dim = sub.get_dimension()
        nint = C.c_int64()
        _lib.check(_lib.lib().dnm_vec_layout_size(C.byref(d), C.byref(nint)))
        T, ib = backend.layout_blocks(d)
        t = L - a - w
        place = int((T < 1 << (t - 1)).sum())
        istart, ilen, nstart, nlen = backend.layout_partition(d, 2, 0)
        assert (istart, nstart, 2 * ilen, 2 * nlen) == (0, 0, nint.value, dim), L
        assert ib[place] == ilen and np.all(T[:place] < 1 << (t - 1)) and np.all(T[place:] >= 1 << (t - 1)), L
        # the reference order ascends in the state: the last row of the share and the first one after it decide
        last, nxt = (int(s) for s in sub.idx_to_state(np.array([nlen - 1, nlen])))
        assert last >> (L - 1) == 0 and nxt >> (L - 1) == 1, L
        edge = np.array([0, nlen - 1, nlen, dim - 1], dtype=np.int64)
        pos = np.empty_like(edge)
        _lib.check(_lib.lib().dnm_vec_layout_positions_host(C.byref(d), None, edge.size, _lib.p64(edge), _lib.p64(pos)))
        assert pos[0] == 0 and pos[1] < ilen <= pos[2] and pos[3] < nint.value, L
        if L <= 20:          # every state, where that is cheap
            st = np.asarray(sub.idx_to_state(np.arange(dim)), dtype=np.int64)
            p = _positions(d, dim)
            assert np.array_equal(p < ilen, (st >> (L - 1)) == 0), L
