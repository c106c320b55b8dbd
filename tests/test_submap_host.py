"""
The host side of the subspace maps and the sector weights (csrc/submap_kernels.hip, csrc/submap_rank.h:
dnm_subspace_map_plan, dnm_subspace_map_indices, dnm_subspace_map_apply, dnm_sector_weights_plan, dnm_sector_weights)
-- no GPU needed: the plan (rows, the run of a thread, workgroups that follow from the target's rows alone, tables that
fit the LDS budget of the other passes), the arguments the calls refuse before any device call, and the source
positions, signs and scale of every target row for every pair of a set of small subspaces, with both XParity sectors on
either side where the parent carries the flip, against tests/submap_ref.py (idx_to_state, state_to_idx and the table of
the four cases written out in numpy).
"""
import ctypes as C

import numpy as np
import pytest

import submap_ref
from dynamite_amd import _lib, backend
from dynamite_amd.subspaces import Auto, Explicit, Full, Parity, SpinConserve

LDS_BUDGET = 152 * 1024
KAPPA = 0.70710678118654752440


def _desc(sub, swz=0):
    d = _lib.Subspace.from_buffer_copy(sub._c())
    d.vec_swizzle = swz
    d._keep = sub
    return d


def _flip_closed_list(L, n, seed):
    """An unsorted list of n representatives (spin L - 1 up) followed by their complements in another order."""
    rng = np.random.default_rng(seed)
    reps = rng.choice(1 << (L - 1), size=n, replace=False).astype(np.int64)
    return np.concatenate([reps, (reps ^ ((1 << L) - 1))[rng.permutation(n)]])


def _auto(L, sort):
    from dynamite_amd.operators import op_sum, sigmax, sigmay
    H = op_sum([sigmax(i) * sigmax(i + 1) + sigmay(i) * sigmay(i + 1) for i in range(L - 1)])
    H.L = L
    return Auto(H, 'U' * (L // 2) + 'D' * (L // 2), sort=sort)


def small_subspaces():
    """name -> (subspace, the XParity sectors a vector on it may be taken in)"""
    rng = np.random.default_rng(5)
    return {
        'Full(8)': (Full(L=8), (0, 1, -1)),
        'Parity(8, even)': (Parity('even', L=8), (0, 1, -1)),
        'SpinConserve(8, 4)': (SpinConserve(8, 4), (0, 1, -1)),
        'SpinConserve(8, 3)': (SpinConserve(8, 3), (0,)),
        'Explicit(30 of 8, unsorted)': (Explicit(rng.choice(256, size=30, replace=False), L=8), (0,)),
        'Explicit(2 x 20 of 8, flip-closed)': (Explicit(_flip_closed_list(8, 20, 6), L=8), (0, 1, -1)),
        'Auto(8, sorted)': (_auto(8, True), (0, 1, -1)),
        'Auto(8, search order)': (_auto(8, False), (0,)),
    }


def seven_spins():
    return {
        'Full(7)': (Full(L=7), (0, 1, -1)),
        'Parity(7, odd)': (Parity('odd', L=7), (0,)),
    }


# ---- the plan -------------------------------------------------------------------------------------------------------
def test_plan_rows_run_grid_and_lds():
    sc, full = _desc(SpinConserve(14, 7)), _desc(Full(L=14))
    assert backend.subspace_map_plan(sc, full) == (3432, 1 << 14, 1, 16, 8 * 15 * 8)
    assert backend.subspace_map_plan(full, sc) == (1 << 14, 3432, 4, 4, 8 * 15 * 8)
    assert backend.subspace_map_plan(sc, full, 1, 0) == (1716, 1 << 14, 1, 16, 8 * 15 * 8)
    assert backend.subspace_map_plan(full, sc, -1, 1) == (1 << 13, 1716, 4, 2, 8 * 15 * 8)
    assert backend.subspace_map_plan(sc, sc) == (3432, 3432, 4, 4, 2 * 8 * 15 * 8)
    assert backend.subspace_map_plan(_desc(SpinConserve(9, 0)), _desc(Full(L=9))) == (1, 512, 1, 1, 10 * 8)
    par, full13 = _desc(Parity('odd', L=13), 5), _desc(Full(L=13))
    assert backend.subspace_map_plan(par, full13) == (1 << 12, 1 << 13, 1, 8, 0)
    ex = _desc(Explicit(np.arange(1000) * 3, L=14))
    assert backend.subspace_map_plan(ex, full) == (1000, 1 << 14, 1, 16, 0)
    assert backend.subspace_map_plan(full, ex) == (1 << 14, 1000, 1, 1, 0)
    # the grid is capped, and the largest tables fit the LDS budget of the other passes
    big = _desc(SpinConserve(36, 18))
    rows = int(SpinConserve(36, 18).get_dimension())
    assert backend.subspace_map_plan(big, _desc(Full(L=36))) == (rows, 1 << 36, 1, 4096, -(-19 * 37 * 8 // 16) * 16)
    wide = _desc(SpinConserve(63, 31))
    lds = backend.subspace_map_plan(wide, _desc(SpinConserve(63, 32)))[4]
    assert lds == -(-(32 * 64 * 8 + 33 * 64 * 8) // 16) * 16 and lds <= LDS_BUDGET


def test_plan_outputs_may_be_null():
    a, b = _desc(Full(L=12)), _desc(SpinConserve(12, 6))
    nw = C.c_int()
    _lib.check(_lib.lib().dnm_subspace_map_plan(C.byref(a), 0, C.byref(b), 0, None, None, None, C.byref(nw), None))
    assert nw.value == 1
    _lib.check(_lib.lib().dnm_subspace_map_plan(C.byref(a), 0, C.byref(b), 0, None, None, None, None, None))
    _lib.check(_lib.lib().dnm_sector_weights_plan(C.byref(a), 0, None, None))


def test_sector_weights_plan():
    # pairs of rows where the flip sums come with the bins, single rows elsewhere; L + 3 sums per workgroup
    for d, sec, items in ((_desc(Full(L=12)), 0, 2048), (_desc(Full(L=11)), 1, 1024), (_desc(SpinConserve(12, 6)), 0, 462),
                          (_desc(SpinConserve(12, 5)), 0, 792), (_desc(Parity('odd', L=13)), 0, 4096),
                          (_desc(Full(L=30)), 0, 1 << 29)):
        nw, scratch = backend.sector_weights_plan(d, sec)
        assert nw == min(2048, max(1, -(-items // 1024)))
        assert scratch == (nw + 1) * (int(d.L) + 3) * 8
    assert (63 + 3) * 256 * 8 <= LDS_BUDGET


# ---- refusals: each is decided before any device call ---------------------------------------------------------------
def _message(rc):
    assert rc != 0
    msg = _lib.lib().dnm_last_error().decode()
    assert msg
    return msg


def _ref(d):
    return C.byref(d) if d is not None else None


def _refused_everywhere(src, dst, ssec=0, dsec=0):
    """The plan, the index table and the map itself (with pointers that are never followed) refuse alike."""
    L = _lib.lib()
    msgs = [_message(L.dnm_subspace_map_plan(_ref(src), ssec, _ref(dst), dsec, None, None, None, None, None))]
    rows = np.zeros(1, dtype=np.int64)
    idx = np.zeros(2, dtype=np.int64)
    sign = np.zeros(2, dtype=np.int8)
    scale = C.c_double()
    msgs.append(_message(L.dnm_subspace_map_indices(_ref(src), ssec, _ref(dst), dsec, 1, _lib.p64(rows), _lib.p64(idx),
                                                    sign.ctypes.data_as(C.POINTER(C.c_int8)), C.byref(scale))))
    msgs.append(_message(L.dnm_subspace_map_apply(C.c_void_p(0x1000), _ref(src), ssec, C.c_void_p(0x2000), _ref(dst), dsec,
                                                  None)))
    assert msgs[0] == msgs[1] == msgs[2]
    return msgs[0]


def _weights_refused(d, sec=0, flip=False):
    L = _lib.lib()
    out = np.zeros(70)
    fl = np.zeros(2)
    msg = _message(L.dnm_sector_weights(C.c_void_p(0x1000), _ref(d), sec, _lib.pf64(out), _lib.pf64(fl) if flip else None,
                                        None))
    assert not out.any() and not fl.any()
    return msg


def test_null_arguments_and_aliasing():
    L = _lib.lib()
    a, b = _desc(Full(L=8)), _desc(SpinConserve(8, 4))
    assert 'null' in _refused_everywhere(None, b)
    assert 'null' in _refused_everywhere(a, None)
    assert 'null' in _message(L.dnm_subspace_map_apply(None, C.byref(a), 0, C.c_void_p(0x2000), C.byref(b), 0, None))
    assert 'null' in _message(L.dnm_subspace_map_apply(C.c_void_p(0x1000), C.byref(a), 0, None, C.byref(b), 0, None))
    assert 'same vector' in _message(L.dnm_subspace_map_apply(C.c_void_p(0x1000), C.byref(a), 0, C.c_void_p(0x1000),
                                                              C.byref(b), 0, None))
    scale = C.c_double()
    assert 'null' in _message(L.dnm_subspace_map_indices(C.byref(a), 0, C.byref(b), 0, 1, None, None, None, C.byref(scale)))
    out = np.zeros(9)
    assert 'null' in _message(L.dnm_sector_weights(None, C.byref(a), 0, _lib.pf64(out), None, None))
    assert 'null' in _message(L.dnm_sector_weights(C.c_void_p(0x1000), None, 0, _lib.pf64(out), None, None))
    assert 'null' in _message(L.dnm_sector_weights(C.c_void_p(0x1000), C.byref(a), 0, None, None, None))
    assert 'null' in _message(L.dnm_sector_weights_plan(None, 0, None, None))


def test_descriptors_that_are_refused():
    full8, sc84 = _desc(Full(L=8)), _desc(SpinConserve(8, 4))
    # different L on the two sides
    assert 'L=9' in _refused_everywhere(full8, _desc(Full(L=9)))
    # L outside [1, 63], more than 62 index bits
    for bad_L in (0, 64):
        d = _desc(Full(L=8))
        d.L = bad_L
        assert 'out of range' in _refused_everywhere(d, full8)
        assert 'out of range' in _refused_everywhere(full8, d)
        assert 'out of range' in _weights_refused(d)
    d = _desc(Full(L=8))
    d.L = 63
    assert '62 index bits' in _refused_everywhere(d, _desc(SpinConserve(63, 1)))
    assert '62 index bits' in _weights_refused(d)
    # an unknown subspace type
    d = _desc(Full(L=8))
    d.type = 7
    assert 'unknown subspace type 7' in _refused_everywhere(d, full8)
    assert 'unknown subspace type 7' in _refused_everywhere(full8, d)
    assert 'unknown subspace type 7' in _weights_refused(d)
    # a sector other than 0, +1, -1
    assert 'sector 2' in _refused_everywhere(full8, sc84, 2, 0)
    assert 'sector -3' in _refused_everywhere(full8, sc84, 0, -3)
    assert 'sector 2' in _weights_refused(full8, 2)
    # a non-null site_perm
    perm = np.arange(8, dtype=np.int8)
    d = _desc(SpinConserve(8, 4))
    d.site_perm = perm.ctypes.data_as(C.POINTER(C.c_int8))
    assert 'site_perm' in _refused_everywhere(d, full8)
    assert 'site_perm' in _refused_everywhere(full8, d)
    assert 'site_perm' in _weights_refused(d)
    # the SpinConserve internal layout
    d = _desc(SpinConserve(8, 4), 2 | (2 << 8))
    assert 'reference order' in _refused_everywhere(d, full8)
    assert 'reference order' in _refused_everywhere(full8, d)
    assert 'reference order' in _weights_refused(d)
    # a swizzle shift outside {0} and [5, 24]
    for shift in (3, 4, 25, -1):
        assert 'vec_swizzle' in _refused_everywhere(_desc(Full(L=8), shift), sc84)
        assert 'vec_swizzle' in _refused_everywhere(sc84, _desc(Parity('even', L=8), shift))
        assert 'vec_swizzle' in _weights_refused(_desc(Full(L=8), shift))
    assert 'vec_swizzle' in _refused_everywhere(_desc(Explicit([1, 2, 5], L=8), 5), full8)


def test_parents_that_cannot_carry_the_flip():
    full = _desc(Full(L=7))
    par7 = _desc(Parity('odd', L=7))
    assert 'even' in _refused_everywhere(par7, full, 1, 0)
    assert 'even' in _refused_everywhere(full, par7, 0, -1)
    assert 'even' in _weights_refused(par7, 1)
    full8 = _desc(Full(L=8))
    sc83 = _desc(SpinConserve(8, 3))
    assert 'k = L / 2' in _refused_everywhere(sc83, full8, -1, 0)
    assert 'k = L / 2' in _refused_everywhere(full8, sc83, 0, 1)
    assert 'k = L / 2' in _weights_refused(sc83, 1)
    odd = _desc(Explicit([1, 2, 254], L=8))
    assert 'odd dimension' in _refused_everywhere(odd, full8, 1, 0)
    assert 'odd dimension' in _refused_everywhere(full8, odd, 0, 1)
    # rows dim / 2 - 1 and dim / 2 must have bit L - 1 clear and set
    for states in ([1, 130, 2, 253], [1, 2, 3, 253], [129, 130, 254, 253]):
        d = _desc(Explicit(states, L=8))
        assert 'representatives' in _refused_everywhere(d, full8, 1, 0)
        assert 'representatives' in _refused_everywhere(full8, d, 0, -1)
        assert 'representatives' in _weights_refused(d, -1)
    good = _desc(Explicit([1, 2, 254, 253], L=8))
    assert backend.subspace_map_plan(good, full8, 1, 0)[:2] == (2, 256)
    # the plain subspaces themselves are fine
    assert backend.subspace_map_plan(par7, full)[:2] == (64, 128)
    assert backend.subspace_map_plan(sc83, full8)[:2] == (56, 256)


def test_flip_sums_refused_where_the_flip_is_not_defined():
    for d in (_desc(Explicit([1, 2, 254, 253], L=8)), _desc(Parity('odd', L=7)), _desc(SpinConserve(8, 3))):
        assert 'flip' in _weights_refused(d, 0, flip=True)


def test_rows_out_of_range_are_refused():
    a, b = _desc(Full(L=8)), _desc(SpinConserve(8, 4))
    for rows, sec in (([70], 0), ([-1], 0), ([35], 1)):
        with pytest.raises(_lib.BackendError, match='row'):
            backend.subspace_map_indices(a, b, rows, 0, sec)
    assert backend.subspace_map_indices(a, b, [], 0, 0)[0].shape == (0, 2)


# ---- the index table against numpy ----------------------------------------------------------------------------------
def _check_pair(name_s, sub_s, sec_s, swz_s, name_d, sub_d, sec_d, swz_d):
    idx, sign, scale = backend.subspace_map_indices(_desc(sub_s, swz_s), _desc(sub_d, swz_d),
                                                    np.arange(submap_ref.rows_of((sub_d, sec_d, swz_d))), sec_s, sec_d)
    want_idx, want_sign, want_scale = submap_ref.map_indices((sub_s, sec_s, swz_s), (sub_d, sec_d, swz_d))
    what = (name_s, sec_s, swz_s, name_d, sec_d, swz_d)
    assert np.array_equal(idx, want_idx), what
    assert np.array_equal(sign, want_sign), what
    assert scale == want_scale and scale in (1.0, KAPPA), what
    assert idx.max() < submap_ref.rows_of((sub_s, sec_s, swz_s)) and idx.min() >= -1
    return int((idx >= 0).sum())


@pytest.mark.parametrize('family', [small_subspaces, seven_spins], ids=['eight spins', 'seven spins'])
def test_indices_of_every_pair(family):
    subs = family()
    terms = 0
    for name_s, (sub_s, secs_s) in subs.items():
        for name_d, (sub_d, secs_d) in subs.items():
            for sec_s in secs_s:
                for sec_d in secs_d:
                    terms += _check_pair(name_s, sub_s, sec_s, 0, name_d, sub_d, sec_d, 0)
    assert terms > 1000


def test_indices_of_an_embedding_are_a_bijection_onto_the_sector():
    sc, full = SpinConserve(8, 4), Full(L=8)
    idx, sign, scale = backend.subspace_map_indices(_desc(sc), _desc(full), np.arange(256))
    hit = idx[:, 0] >= 0
    assert hit.sum() == 70 and np.array_equal(np.sort(idx[hit, 0]), np.arange(70)) and scale == 1.0
    assert np.array_equal(np.flatnonzero(hit), sc.idx_to_state(np.arange(70)))
    assert (idx[:, 1] == -1).all() and np.array_equal(sign[:, 0], hit.astype(np.int8))


@pytest.mark.parametrize('shifts', [(5, 0), (0, 5), (5, 5), (6, 5)])
def test_indices_with_a_swizzle_forced_on_either_side(shifts):
    s_s, s_d = shifts
    full, par, sc = Full(L=12), Parity('odd', L=13), SpinConserve(12, 6)
    full13 = Full(L=13)
    for sec_s, sec_d in ((0, 0), (1, 0), (0, -1), (1, 1), (-1, 1)):
        _check_pair('Full(12)', full, sec_s, s_s, 'Full(12)', full, sec_d, s_d)
        _check_pair('Full(12)', full, sec_s, s_s, 'SpinConserve(12, 6)', sc, sec_d, 0)
        _check_pair('SpinConserve(12, 6)', sc, sec_s, 0, 'Full(12)', full, sec_d, s_d)
        if sec_s == 0:          # (Parity with odd L carries no sector)
            _check_pair('Parity(13)', par, 0, s_s, 'Full(13)', full13, sec_d, s_d)
        if sec_d == 0:
            _check_pair('Full(13)', full13, sec_s, s_s, 'Parity(13)', par, 0, s_d)
