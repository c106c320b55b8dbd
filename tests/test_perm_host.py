"""
The host side of the site-permutation pass (csrc/perm_kernels.hip, csrc/perm_rank.h: dnm_perm_plan,
dnm_perm_partner_indices, dnm_perm_apply, dnm_perm_dots) -- no GPU needed: the plan (workgroups that follow from the
number of rows alone, tables that fit the LDS budget of the other passes), the arguments the calls refuse before any
device call, and the source of every row for every permutation of a fixed set against numpy (idx_to_state, move the
bits, state_to_idx; under XParity the global flip written out).  P_pi moves the spin at site i to site pi(i): the source
configuration of a row has bit i equal to bit pi(i) of the row's.  For the permutation of a three-site rotation the
indices are those of backend.cyc_partner_indices.
"""
import ctypes as C
from math import comb

import numpy as np
import pytest

from dynamite_amd import _lib, backend
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve

LDS_BUDGET = 152 * 1024


def _raw_spin_conserve(L, k):
    """A SpinConserve descriptor filled in by hand (the Python class stops at 63 spins, the C ABI of this pass at 64)."""
    tab = np.array([[comb(n, m) for n in range(L + 1)] for m in range(k + 1)], dtype=np.int64)
    d = _lib.Subspace()
    d.type, d.L, d.k, d.ld_nchoosek = 3, L, k, L + 1
    d.nchoosek = tab.ctypes.data_as(C.POINTER(C.c_int64))
    d._keep = tab
    return d


def _desc(sub, swz=0):
    d = _lib.Subspace.from_buffer_copy(sub._c())
    d.vec_swizzle = swz
    d._keep = sub
    return d


def perm_set(L):
    """Identity, a transposition with site L - 1, the reversal, the shifts by 1 and by L - 1, a three-cycle through
    L - 1, two seeded random ones."""
    h = L // 2
    ident = np.arange(L)
    swap = ident.copy()
    swap[[h, L - 1]] = [L - 1, h]
    cyc = ident.copy()
    cyc[[1, L - 1, h + 1]] = [L - 1, h + 1, 1]
    rng = np.random.default_rng(100 + L)
    return np.array([ident, swap, ident[::-1], (ident + 1) % L, (ident + L - 1) % L, cyc, rng.permutation(L),
                     rng.permutation(L)], dtype=np.int32)


def source(cfg, perm):
    """bit i of the source = bit perm[i] of cfg"""
    src = np.zeros_like(cfg)
    for i, p in enumerate(perm):
        src |= ((cfg >> np.int64(p)) & 1) << np.int64(i)
    return src


def position(i, S):
    return i ^ (((i >> S) & ((1 << (S - 4)) - 1)) << 4) if S else i


# ---- the plan -------------------------------------------------------------------------------------------------------
ROWS = [
    (lambda: _desc(Full(L=4)), 16, 0),
    (lambda: _desc(Full(L=12)), 1 << 12, 0),
    (lambda: _desc(Parity('odd', L=13)), 1 << 12, 0),
    (lambda: _desc(SpinConserve(12, 6)), 924, 7 * 13 * 8),
    (lambda: _desc(SpinConserve(34, 2)), 561, 3 * 35 * 8),
    (lambda: _desc(SpinConserve(12, 0)), 1, 13 * 8),
    (lambda: _desc(Full(L=19)), 1 << 19, 0),
    (lambda: _desc(Full(L=30)), 1 << 30, 0),
    (lambda: _raw_spin_conserve(64, 1), 64, 2 * 65 * 8),
]


def test_plan_follows_from_the_rows_alone():
    """ceil(rows / 1024) workgroups, at most 4096, whatever the subspace or the number of permutations; the tables of a
    launch are the binomials and 68 bytes per permutation, rounded up to 16."""
    for make, rows, table in ROWS:
        d = make()
        want = min(4096, max(1, -(-rows // 1024)))
        for n in (1, 2, 20, 64):
            nw, lds, scratch = backend.perm_plan(d, n)
            assert nw == want, (rows, n)
            assert lds == -(-(table + 68 * n) // 16) * 16
            assert scratch == lds + nw * 2 * n * 8 + 2 * n * 8
            assert backend.perm_plan(d, n) == (nw, lds, scratch)


def test_plan_lds_of_the_largest_tables():
    for d in (_desc(SpinConserve(36, 18)), _raw_spin_conserve(64, 32)):
        nw, lds, _ = backend.perm_plan(d, 64)
        table = (int(d.k) + 1) * (int(d.L) + 1) * 8
        assert table + 64 * 64 <= lds <= LDS_BUDGET
        assert nw == 4096


def test_plan_outputs_may_be_null():
    d = _desc(Full(L=12))
    nw = C.c_int()
    _lib.check(_lib.lib().dnm_perm_plan(C.byref(d), 5, C.byref(nw), None, None))
    assert nw.value == 4
    _lib.check(_lib.lib().dnm_perm_plan(C.byref(d), 5, None, None, None))


# ---- refusals: each is decided before any device call ---------------------------------------------------------------
def _perms(perms):
    p = np.ascontiguousarray(perms, dtype=np.int32)
    return p, p.ctypes.data_as(C.POINTER(C.c_int32))


def _message(rc):
    assert rc != 0
    msg = _lib.lib().dnm_last_error().decode()
    assert msg
    return msg


def _plan_refused(d, n=3):
    return _message(_lib.lib().dnm_perm_plan(C.byref(d) if d is not None else None, n, None, None, None))


def _identities(d, n):
    L = int(d.L) if d is not None and 1 <= int(d.L) <= 64 else 8
    return np.tile(np.arange(L, dtype=np.int32), (max(n, 1), 1))


def _apply_refused(d, perms=None, xsec=0, x=0x1000, y=0x2000, n=None, give=True, coef=True):
    """dnm_perm_apply with pointers that are never followed: the call is refused first."""
    if perms is None:
        perms = _identities(d, 3 if n is None else n)
    p, pp = _perms(perms)
    c = np.zeros(2 * 128)
    return _message(_lib.lib().dnm_perm_apply(C.c_void_p(x), C.c_void_p(y), C.byref(d) if d is not None else None, xsec,
                                              len(perms) if n is None else n, pp if give else None,
                                              _lib.pf64(c) if coef else None, 0, None))


def _dots_refused(d, perms=None, xsec=0, phi=0x1000, psi=0x1000, n=None, give=True, out=True):
    if perms is None:
        perms = _identities(d, 3 if n is None else n)
    p, pp = _perms(perms)
    o = np.zeros(2 * 128)
    return _message(_lib.lib().dnm_perm_dots(C.c_void_p(phi), C.c_void_p(psi), C.byref(d) if d is not None else None,
                                             xsec, len(perms) if n is None else n, pp if give else None,
                                             _lib.pf64(o) if out else None, None))


def _partners_refused(d, perms=None, xsec=0, rows=(0,), n=None, give=True):
    if perms is None:
        perms = _identities(d, 1 if n is None else n)
    p, pp = _perms(perms)
    rows = np.asarray(rows, dtype=np.int64)
    idx = np.zeros(rows.size * 128, dtype=np.int64)
    sign = np.zeros(rows.size * 128, dtype=np.int8)
    return _message(_lib.lib().dnm_perm_partner_indices(C.byref(d), xsec, len(perms) if n is None else n, pp, rows.size,
                                                        _lib.p64(rows), _lib.p64(idx) if give else None,
                                                        sign.ctypes.data_as(C.POINTER(C.c_int8))))


def _explicit():
    rng = np.random.default_rng(11)
    states = rng.choice(1 << 20, size=300, replace=False).astype(np.int64) | (np.int64(1) << 39)
    return Explicit(states, L=40)


def test_refusals_of_the_subspace():
    bad = []
    bad.append((_desc(_explicit()), "Explicit"))
    d = _lib.Subspace()
    d.type, d.L = 99, 8
    bad.append((d, "unknown subspace type"))
    sub = SpinConserve(22, 11)
    d = _desc(sub, 6 | (4 << 8))
    bad.append((d, "reference order"))
    d = _desc(sub)
    perm = np.arange(22, dtype=np.int8)
    d.site_perm = perm.ctypes.data_as(C.POINTER(C.c_int8))
    bad.append((d, "site_perm"))
    d = _desc(Full(L=12))
    d.site_perm = perm.ctypes.data_as(C.POINTER(C.c_int8))
    bad.append((d, "site_perm"))
    d = _raw_spin_conserve(64, 1)
    d.L, d.ld_nchoosek = 65, 66
    bad.append((d, "L=65"))
    d = _lib.Subspace()
    d.type, d.L = 0, 0
    bad.append((d, "L=0"))
    d = _lib.Subspace()
    d.type, d.L = 0, 64
    bad.append((d, "2^64 rows"))
    for shift in (3, 4, 25):
        bad.append((_desc(Full(L=12), shift), "vec_swizzle %d" % shift))
    bad.append((_desc(Parity('even', L=12), 4), "vec_swizzle 4"))
    for d, word in bad:
        for msg in (_plan_refused(d), _apply_refused(d), _dots_refused(d), _partners_refused(d)):
            assert word in msg, (word, msg)
            assert "site permutation" in msg
    assert "null" in _plan_refused(None)
    assert "null" in _apply_refused(None)
    assert "null" in _dots_refused(None)


def test_refusals_of_the_arguments():
    ok = _desc(Full(L=8))
    assert "null" in _apply_refused(ok, x=0)
    assert "null" in _apply_refused(ok, y=0)
    assert "null" in _apply_refused(ok, give=False)
    assert "null" in _apply_refused(ok, coef=False)
    assert "null" in _dots_refused(ok, phi=0)
    assert "null" in _dots_refused(ok, psi=0)
    assert "null" in _dots_refused(ok, give=False)
    assert "null" in _dots_refused(ok, out=False)
    assert "null" in _partners_refused(ok, give=False)
    # the pass gathers: x and y must be two vectors
    assert "same vector" in _apply_refused(ok, x=0x3000, y=0x3000)
    for n in (0, -1, 65):
        assert "permutations" in _plan_refused(ok, n=n)
        assert "permutations" in _apply_refused(ok, n=n)
        assert "permutations" in _dots_refused(ok, n=n)
        assert "permutations" in _partners_refused(ok, n=n)
    assert backend.perm_plan(ok, 64)[0] == 1
    ident = np.arange(8)
    for row, why in (([0, 1, 2, 3, 4, 5, 6, 6], "a repeated site"), ([0, 1, 2, 3, 4, 5, 6, 8], "a site outside"),
                     ([-1, 1, 2, 3, 4, 5, 6, 7], "a negative site"), ([1, 1, 1, 1, 1, 1, 1, 1], "one site")):
        for perms, at in (([row], 0), ([ident, ident[::-1], row], 2)):
            for msg in (_apply_refused(ok, perms=perms), _dots_refused(ok, perms=perms),
                        _partners_refused(ok, perms=perms)):
                assert "permutation %d is not a bijection" % at in msg, (why, msg)
    assert "bijection" in _apply_refused(_desc(SpinConserve(8, 4)), perms=[[0, 1, 2, 3, 4, 5, 7, 7]])
    for xsec in (2, -2, 7):
        assert "xparity_sector" in _apply_refused(ok, xsec=xsec)
        assert "xparity_sector" in _dots_refused(ok, xsec=xsec)
        assert "xparity_sector" in _partners_refused(ok, xsec=xsec)
    for d in (_desc(Parity('even', L=11)), _desc(SpinConserve(12, 5)), _desc(SpinConserve(11, 5))):
        for xsec in (+1, -1):
            assert "global flip" in _apply_refused(d, xsec=xsec)
            assert "global flip" in _dots_refused(d, xsec=xsec)
            assert "global flip" in _partners_refused(d, xsec=xsec)
    assert "row" in _partners_refused(ok, rows=(256,))
    assert "row" in _partners_refused(ok, rows=(-1,))
    assert "row" in _partners_refused(ok, xsec=1, rows=(128,))


def test_refusals_of_the_python_layer():
    d = _desc(Full(L=8))
    with pytest.raises(ValueError, match='length'):
        backend.perm_partner_indices(d, [np.arange(7)], [0])
    with pytest.raises(RuntimeError, match='bijection'):
        backend.perm_partner_indices(d, [[0, 0, 2, 3, 4, 5, 6, 7]], [0])
    with pytest.raises(RuntimeError, match='permutations'):
        backend.perm_partner_indices(d, np.tile(np.arange(8), (65, 1)), [0])


# ---- partner indices ------------------------------------------------------------------------------------------------
PLAIN = [
    pytest.param(lambda: Full(L=10), 0, id="full10"),
    pytest.param(lambda: Full(L=10), 6, id="full10_swizzled"),
    pytest.param(lambda: Full(L=10), 5, id="full10_swizzle5"),
    pytest.param(lambda: Parity('even', L=11), 0, id="parity11_even"),
    pytest.param(lambda: Parity('odd', L=11), 0, id="parity11_odd"),
    pytest.param(lambda: Parity('odd', L=12), 6, id="parity12_odd_swizzled"),
    pytest.param(lambda: SpinConserve(12, 6), 0, id="sc12_6"),
    pytest.param(lambda: SpinConserve(13, 4), 0, id="sc13_4"),
    pytest.param(lambda: SpinConserve(34, 2), 0, id="sc34_2"),
    pytest.param(lambda: SpinConserve(12, 0), 0, id="sc12_0"),
    pytest.param(lambda: SpinConserve(12, 12), 0, id="sc12_12"),
]


@pytest.mark.parametrize("make,swz", PLAIN)
def test_partner_indices(make, swz):
    """Rows and results are positions in the vector as it lies: the reference-order index taken through the swizzle."""
    sub = make()
    L, dim = sub.L, sub.get_dimension()
    perms = perm_set(L)
    rows = np.arange(dim, dtype=np.int64)
    idx, sign = backend.perm_partner_indices(_desc(sub, swz), perms, rows)
    assert idx.shape == sign.shape == (dim, len(perms)) and idx.dtype == np.int64 and sign.dtype == np.int8
    cfg = np.asarray(sub.idx_to_state(position(rows, swz)), dtype=np.int64)
    for g, perm in enumerate(perms):
        want = np.asarray(sub.state_to_idx(source(cfg, perm)), dtype=np.int64)
        assert np.all(want >= 0)
        assert np.array_equal(idx[:, g], position(want, swz)), (g, np.argwhere(idx[:, g] != position(want, swz))[:4])
        # a permutation of sites is a permutation of the rows
        assert np.array_equal(np.sort(idx[:, g]), rows)
    assert np.array_equal(sign, np.ones_like(sign))
    assert np.array_equal(idx[:, 0], rows)
    if swz:
        assert not np.array_equal(position(rows, swz), rows)


XPARITY = [
    pytest.param(lambda: Full(L=10), 0, id="x_full10"),
    pytest.param(lambda: Full(L=10), 6, id="x_full10_swizzled"),
    pytest.param(lambda: Parity('even', L=12), 0, id="x_parity12_even"),
    pytest.param(lambda: Parity('odd', L=12), 0, id="x_parity12_odd"),
    pytest.param(lambda: Parity('even', L=12), 6, id="x_parity12_even_swizzled"),
    pytest.param(lambda: SpinConserve(12, 6), 0, id="x_sc12_6"),
]


@pytest.mark.parametrize("sector", [+1, -1])
@pytest.mark.parametrize("make,swz", XPARITY)
def test_partner_indices_xparity(make, swz, sector):
    """The rows are the parent's first dim / 2: bit L - 1 clear.  Where bit L - 1 of the source is set the amplitude is
    the sector's sign times that of the complement, again a representative."""
    sub = make()
    L, half = sub.L, sub.get_dimension() // 2
    perms = perm_set(L)
    rows = np.arange(half, dtype=np.int64)
    idx, sign = backend.perm_partner_indices(_desc(sub, swz), perms, rows, sector)
    cfg = np.asarray(sub.idx_to_state(position(rows, swz)), dtype=np.int64)
    assert not np.any((cfg >> (L - 1)) & 1)
    everything = (np.int64(1) << L) - 1
    for g, perm in enumerate(perms):
        src = source(cfg, perm)
        top = ((src >> (L - 1)) & 1) == 1
        want = np.asarray(sub.state_to_idx(np.where(top, src ^ everything, src)), dtype=np.int64)
        assert np.all((want >= 0) & (want < half))
        assert np.array_equal(idx[:, g], position(want, swz)), (g, np.argwhere(idx[:, g] != position(want, swz))[:4])
        assert np.array_equal(sign[:, g], np.where(top, sector, 1)), g
        # some row takes the branch wherever the permutation moves a spin to site L - 1
        assert bool(np.any(top)) == (perm[L - 1] != L - 1)
        assert np.array_equal(np.sort(idx[:, g]), rows)


CYC = [
    pytest.param(lambda: Full(L=10), 0, id="full10"),
    pytest.param(lambda: Parity('odd', L=11), 0, id="parity11_odd"),
    pytest.param(lambda: SpinConserve(12, 6), 0, id="sc12_6"),
    pytest.param(lambda: SpinConserve(13, 4), 0, id="sc13_4"),
    pytest.param(lambda: Full(L=10), 1, id="x_full10"),
    pytest.param(lambda: Parity('even', L=12), -1, id="x_parity12_even"),
    pytest.param(lambda: SpinConserve(12, 6), -1, id="x_sc12_6"),
]


@pytest.mark.parametrize("make,sector", CYC)
def test_three_cycles_are_the_rotations_of_the_chirality_pass(make, sector):
    """The rotation of the triple (a, b, c) is the permutation pi(a) = b, pi(b) = c, pi(c) = a, all else fixed."""
    sub = make()
    L = sub.L
    h = L // 2
    triples = [(0, 1, 2), (0, 2, 1), (0, h, L - 1), (L - 1, 0, h), (h, L - 1, 0), (L - 3, L - 2, L - 1), (3, 7, 5)]
    perms = np.tile(np.arange(L, dtype=np.int32), (len(triples), 1))
    for m, (a, b, c) in enumerate(triples):
        perms[m, [a, b, c]] = [b, c, a]
    rows = np.arange(sub.get_dimension() // (2 if sector else 1), dtype=np.int64)
    idx, sign = backend.perm_partner_indices(_desc(sub), perms, rows, sector)
    cidx, csign = backend.cyc_partner_indices(_desc(sub), triples, rows, sector)
    assert np.array_equal(idx, cidx) and np.array_equal(sign, csign)
    assert np.any(idx != rows[:, None])
