"""
The host side of the bond-swap pass (csrc/swap_kernels.hip, dnm_swap_moments_plan, dnm_swap_moments,
dnm_swap_partner_indices) -- no GPU needed: the plan (tile rows of the (n + 1) x (n + 1) result, a panel that fits the
LDS budget, a number of workgroups that follows from the number of rows alone), the arguments the calls refuse before
any device call, and the partner of every row for every bond against numpy (idx_to_state, exchange the two bits,
state_to_idx; under XParity the global flip written out).
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


def _desc(sub):
    d = _lib.Subspace.from_buffer_copy(sub._c())
    d.vec_swizzle = 0
    d._keep = sub
    return d


# ---- the plan -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 31, 32, 47, 48, 63])
def test_plan_tile_rows(n):
    for d in (_desc(Full(L=20)), _desc(Parity('even', L=21)), _desc(SpinConserve(22, 11))):
        tr, pb, nw, lds, sb = backend.swap_moments_plan(d, n)
        assert tr == -(-(n + 1) // 16) and 1 <= tr <= 4
        assert pb == (9 if tr == 1 else 7)
        assert (1 << pb) * (16 * tr + 1) * 16 <= lds <= LDS_BUDGET
        nt = tr * (tr + 1) // 2
        assert sb == nw * (nt + tr * tr) * 256 * 8
        assert backend.swap_moments_plan(d, n) == (tr, pb, nw, lds, sb)


def test_plan_lds_of_the_largest_tables():
    for d in (_desc(SpinConserve(36, 18)), _raw_spin_conserve(64, 32)):
        tr, pb, nw, lds, _ = backend.swap_moments_plan(d, 63)
        table = (int(d.k) + 1) * (int(d.L) + 1) * 8
        assert tr == 4 and pb >= 6
        assert lds == (1 << pb) * 65 * 16 + table and lds <= LDS_BUDGET
        assert nw == 1024


ROWS = [
    (lambda: _desc(Full(L=4)), 16),
    (lambda: _desc(Full(L=12)), 1 << 12),
    (lambda: _desc(Parity('odd', L=13)), 1 << 12),
    (lambda: _desc(SpinConserve(12, 6)), 924),
    (lambda: _desc(SpinConserve(34, 2)), 561),
    (lambda: _desc(SpinConserve(12, 0)), 1),
    (lambda: _desc(Full(L=19)), 1 << 19),
    (lambda: _desc(Full(L=30)), 1 << 30),
    (lambda: _raw_spin_conserve(64, 1), 64),
]


def test_plan_workgroups_follow_from_the_rows_alone():
    """ceil(rows / 512), at most 1024: whatever the subspace, the number of bonds or the panel."""
    for make, rows in ROWS:
        d = make()
        want = min(1024, max(1, -(-rows // 512)))
        for n in (1, 15, 16, 40, 63):
            assert backend.swap_moments_plan(d, n)[2] == want, (rows, n)


def test_plan_outputs_may_be_null():
    d = _desc(Full(L=10))
    nw = C.c_int()
    _lib.check(_lib.lib().dnm_swap_moments_plan(C.byref(d), 5, None, None, C.byref(nw), None, None))
    assert nw.value == 2


# ---- refusals: each is decided before any device call ---------------------------------------------------------------
def _bonds(pairs):
    b = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1)
    return b, b.ctypes.data_as(C.POINTER(C.c_int32))


def _plan_refused(d, n=3):
    rc = _lib.lib().dnm_swap_moments_plan(C.byref(d) if d is not None else None, n, None, None, None, None, None)
    assert rc != 0
    msg = _lib.lib().dnm_last_error().decode()
    assert msg
    return msg


def _call_refused(d, pairs=((0, 1), (1, 2), (0, 2)), xsec=0, x=0x1000, out=True, n=None, give_bonds=True):
    """dnm_swap_moments with a pointer that is never followed: the call is refused first."""
    buf = np.zeros(2 * 64 * 64)
    b, bp = _bonds(pairs)
    rc = _lib.lib().dnm_swap_moments(C.c_void_p(x), C.byref(d) if d is not None else None, xsec,
                                     len(pairs) if n is None else n, bp if give_bonds else None,
                                     _lib.pf64(buf) if out else None, None)
    assert rc != 0
    msg = _lib.lib().dnm_last_error().decode()
    assert msg
    return msg


def _partners_refused(d, pairs=((0, 1),), xsec=0, rows=(0,), give=True):
    b, bp = _bonds(pairs)
    rows = np.asarray(rows, dtype=np.int64)
    idx = np.zeros(rows.size * len(pairs), dtype=np.int64)
    sign = np.zeros(rows.size * len(pairs), dtype=np.int8)
    rc = _lib.lib().dnm_swap_partner_indices(C.byref(d), xsec, len(pairs), bp, rows.size, _lib.p64(rows),
                                             _lib.p64(idx) if give else None, sign.ctypes.data_as(C.POINTER(C.c_int8)))
    assert rc != 0
    return _lib.lib().dnm_last_error().decode()


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
    d = _desc(sub)
    d.vec_swizzle = 6 | (4 << 8)
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
    d.type, d.L = 0, 65
    bad.append((d, "L=65"))
    d = _lib.Subspace()
    d.type, d.L = 0, 0
    bad.append((d, "L=0"))
    for shift in (3, 4, 25):
        d = _desc(Full(L=12))
        d.vec_swizzle = shift
        bad.append((d, "vec_swizzle %d" % shift))
    d = _desc(Parity('even', L=12))
    d.vec_swizzle = 4
    bad.append((d, "vec_swizzle 4"))
    for d, word in bad:
        assert word in _plan_refused(d)
        assert word in _call_refused(d)
        assert word in _partners_refused(d)
    assert "null" in _plan_refused(None)
    assert "null" in _call_refused(None)


def test_refusals_of_the_arguments():
    ok = _desc(Full(L=8))
    assert "null" in _call_refused(ok, x=0)
    assert "null" in _call_refused(ok, out=False)
    assert "null" in _call_refused(ok, give_bonds=False)
    assert "null" in _partners_refused(ok, give=False)
    for n in (0, -1, 64):
        assert "bonds" in _plan_refused(ok, n=n)
        assert "bonds" in _call_refused(ok, pairs=[(0, 1)] * 64, n=n)
    assert backend.swap_moments_plan(ok, 63)[0] == 4
    for pairs, word in ((((0, 1), (2, 8)), "outside"), (((0, 1), (-1, 2)), "outside"), (((3, 3),), "itself")):
        assert word in _call_refused(ok, pairs=pairs)
        assert word in _partners_refused(ok, pairs=pairs)
    assert "outside" in _call_refused(_desc(SpinConserve(8, 4)), pairs=((0, 8),))
    for xsec in (2, -2, 7):
        assert "xparity_sector" in _call_refused(ok, xsec=xsec)
        assert "xparity_sector" in _partners_refused(ok, xsec=xsec)
    for d in (_desc(Parity('even', L=11)), _desc(SpinConserve(12, 5)), _desc(SpinConserve(11, 5))):
        for xsec in (+1, -1):
            assert "global flip" in _call_refused(d, xsec=xsec)
            assert "global flip" in _partners_refused(d, xsec=xsec)
    assert "row" in _partners_refused(ok, rows=(256,))
    assert "row" in _partners_refused(ok, rows=(-1,))
    assert "row" in _partners_refused(ok, xsec=1, rows=(128,))


# ---- partner indices ------------------------------------------------------------------------------------------------
def bond_set(L):
    """Bonds at site 0 and at site L - 1, adjacent and far pairs, both orders, one repeat."""
    return [(0, 1), (1, 0), (0, L - 1), (L - 1, 0), (L - 2, L - 1), (L - 1, L // 2), (1, L - 2), (L // 2, L // 2 + 1),
            (2, L // 2), (0, L // 2), (L - 1, 1), (0, 1), (3, 7), (L - 3, 2)]


def exchanged(cfg, a, b):
    differ = ((cfg >> a) ^ (cfg >> b)) & 1
    return cfg ^ (differ << a) ^ (differ << b)


PLAIN = [
    pytest.param(lambda: Full(L=10), id="full10"),
    pytest.param(lambda: Parity('even', L=11), id="parity11_even"),
    pytest.param(lambda: Parity('odd', L=11), id="parity11_odd"),
    pytest.param(lambda: SpinConserve(12, 6), id="sc12_6"),
    pytest.param(lambda: SpinConserve(34, 2), id="sc34_2"),
    pytest.param(lambda: SpinConserve(12, 0), id="sc12_0"),
    pytest.param(lambda: SpinConserve(12, 12), id="sc12_12"),
]


@pytest.mark.parametrize("make", PLAIN)
def test_partner_indices(make):
    sub = make()
    L, dim = sub.L, sub.get_dimension()
    bonds = bond_set(L)
    rows = np.arange(dim, dtype=np.int64)
    idx, sign = backend.swap_partner_indices(_desc(sub), bonds, rows)
    assert idx.shape == sign.shape == (dim, len(bonds)) and idx.dtype == np.int64 and sign.dtype == np.int8
    cfg = np.asarray(sub.idx_to_state(rows), dtype=np.int64)
    for m, (a, b) in enumerate(bonds):
        want = np.asarray(sub.state_to_idx(exchanged(cfg, a, b)), dtype=np.int64)
        assert np.all(want >= 0)
        assert np.array_equal(idx[:, m], want), (a, b, np.argwhere(idx[:, m] != want)[:4])
        # a swap is a permutation of the rows
        assert np.array_equal(np.sort(idx[:, m]), rows)
    assert np.array_equal(sign, np.ones_like(sign))


XPARITY = [
    pytest.param(lambda: Full(L=10), id="x_full10"),
    pytest.param(lambda: Parity('even', L=12), id="x_parity12_even"),
    pytest.param(lambda: Parity('odd', L=12), id="x_parity12_odd"),
    pytest.param(lambda: SpinConserve(12, 6), id="x_sc12_6"),
]


@pytest.mark.parametrize("sector", [+1, -1])
@pytest.mark.parametrize("make", XPARITY)
def test_partner_indices_xparity(make, sector):
    """The rows are the parent's first dim / 2: bit L - 1 clear.  Where the exchange sets bit L - 1 the amplitude is the
    sector's sign times that of the complement, again a representative."""
    sub = make()
    L, half = sub.L, sub.get_dimension() // 2
    bonds = bond_set(L)
    rows = np.arange(half, dtype=np.int64)
    idx, sign = backend.swap_partner_indices(_desc(sub), bonds, rows, sector)
    cfg = np.asarray(sub.idx_to_state(rows), dtype=np.int64)
    assert not np.any((cfg >> (L - 1)) & 1)
    everything = (np.int64(1) << L) - 1
    flipped_any = False
    for m, (a, b) in enumerate(bonds):
        sw = exchanged(cfg, a, b)
        top = ((sw >> (L - 1)) & 1) == 1
        want = np.asarray(sub.state_to_idx(np.where(top, sw ^ everything, sw)), dtype=np.int64)
        assert np.all((want >= 0) & (want < half))
        assert np.array_equal(idx[:, m], want), (a, b, np.argwhere(idx[:, m] != want)[:4])
        assert np.array_equal(sign[:, m], np.where(top, sector, 1)), (a, b)
        assert not np.any(top) or L - 1 in (a, b)
        flipped_any |= bool(np.any(top))
        assert np.array_equal(np.sort(idx[:, m]), rows)
    assert flipped_any
