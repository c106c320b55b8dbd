"""
The host side of the three-site rotation (scalar chirality) pass (csrc/cyc_kernels.hip, dnm_cyc_moments_plan,
dnm_cyc_moments, dnm_cyc_partner_indices) -- no GPU needed: the plan (that of the bond-swap pass for the same number of
columns: tile rows of the (n + 1) x (n + 1) result, a panel that fits the LDS budget, a number of workgroups that
follows from the number of rows alone), the arguments the calls refuse before any device call, and the partner of every
row for every triple against numpy (idx_to_state, rotate the three bits, state_to_idx; under XParity the global flip
written out).
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
        tr, pb, nw, lds, sb = backend.cyc_moments_plan(d, n)
        assert tr == -(-(n + 1) // 16) and 1 <= tr <= 4
        assert pb == (9 if tr == 1 else 7)
        assert (1 << pb) * (16 * tr + 1) * 16 <= lds <= LDS_BUDGET
        table = (int(d.k) + 1) * (int(d.L) + 1) * 8 if int(d.type) == 3 else 0
        assert lds == (1 << pb) * (16 * tr + 1) * 16 + table
        nt = tr * (tr + 1) // 2
        assert sb == nw * (nt + tr * tr) * 256 * 8
        assert backend.cyc_moments_plan(d, n) == (tr, pb, nw, lds, sb)
        # the bond-swap plan for the same number of columns
        assert backend.swap_moments_plan(d, n) == (tr, pb, nw, lds, sb)


def test_plan_lds_of_the_largest_tables():
    for d in (_desc(SpinConserve(36, 18)), _raw_spin_conserve(64, 32)):
        tr, pb, nw, lds, _ = backend.cyc_moments_plan(d, 63)
        table = (int(d.k) + 1) * (int(d.L) + 1) * 8
        assert tr == 4 and pb >= 6
        assert lds == (1 << pb) * 65 * 16 + table and lds <= LDS_BUDGET
        assert nw == 1024
        assert backend.swap_moments_plan(d, 63)[:4] == (tr, pb, nw, lds)


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
    """ceil(rows / 512), at most 1024: whatever the subspace, the number of triples or the panel."""
    for make, rows in ROWS:
        d = make()
        want = min(1024, max(1, -(-rows // 512)))
        for n in (1, 15, 16, 40, 63):
            assert backend.cyc_moments_plan(d, n)[2] == want, (rows, n)


def test_plan_outputs_may_be_null():
    d = _desc(Full(L=10))
    nw = C.c_int()
    _lib.check(_lib.lib().dnm_cyc_moments_plan(C.byref(d), 5, None, None, C.byref(nw), None, None))
    assert nw.value == 2
    _lib.check(_lib.lib().dnm_cyc_moments_plan(C.byref(d), 5, None, None, None, None, None))


# ---- refusals: each is decided before any device call ---------------------------------------------------------------
def _cycles(triples):
    c = np.ascontiguousarray(triples, dtype=np.int32).reshape(-1)
    return c, c.ctypes.data_as(C.POINTER(C.c_int32))


def _plan_refused(d, n=3):
    rc = _lib.lib().dnm_cyc_moments_plan(C.byref(d) if d is not None else None, n, None, None, None, None, None)
    assert rc != 0
    msg = _lib.lib().dnm_last_error().decode()
    assert msg
    return msg


def _call_refused(d, triples=((0, 1, 2), (1, 2, 3), (0, 3, 2)), xsec=0, x=0x1000, out=True, n=None, give_cycles=True):
    """dnm_cyc_moments with a pointer that is never followed: the call is refused first."""
    buf = np.zeros(2 * 64 * 64)
    c, cp = _cycles(triples)
    rc = _lib.lib().dnm_cyc_moments(C.c_void_p(x), C.byref(d) if d is not None else None, xsec,
                                    len(triples) if n is None else n, cp if give_cycles else None,
                                    _lib.pf64(buf) if out else None, None)
    assert rc != 0
    msg = _lib.lib().dnm_last_error().decode()
    assert msg
    return msg


def _partners_refused(d, triples=((0, 1, 2),), xsec=0, rows=(0,), give=True):
    c, cp = _cycles(triples)
    rows = np.asarray(rows, dtype=np.int64)
    idx = np.zeros(rows.size * len(triples), dtype=np.int64)
    sign = np.zeros(rows.size * len(triples), dtype=np.int8)
    rc = _lib.lib().dnm_cyc_partner_indices(C.byref(d), xsec, len(triples), cp, rows.size, _lib.p64(rows),
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
        for msg in (_plan_refused(d), _call_refused(d), _partners_refused(d)):
            assert word in msg
            assert "chirality" in msg and "bond" not in msg
    assert "null" in _plan_refused(None)
    assert "null" in _call_refused(None)


def test_refusals_of_the_arguments():
    ok = _desc(Full(L=8))
    assert "null" in _call_refused(ok, x=0)
    assert "null" in _call_refused(ok, out=False)
    assert "null" in _call_refused(ok, give_cycles=False)
    assert "null" in _partners_refused(ok, give=False)
    for n in (0, -1, 64):
        assert "cycles" in _plan_refused(ok, n=n)
        assert "cycles" in _call_refused(ok, triples=[(0, 1, 2)] * 64, n=n)
    assert backend.cyc_moments_plan(ok, 63)[0] == 4
    for triples in (((0, 1, 2), (2, 8, 3)), ((0, 1, 2), (-1, 2, 3)), ((0, 1, 8),), ((8, 1, 0),)):
        assert "outside" in _call_refused(ok, triples=triples)
        assert "outside" in _partners_refused(ok, triples=triples)
    for triples in (((3, 3, 4),), ((3, 4, 4),), ((4, 3, 4),), ((0, 1, 2), (5, 5, 5))):
        assert "distinct" in _call_refused(ok, triples=triples)
        assert "distinct" in _partners_refused(ok, triples=triples)
    assert "outside" in _call_refused(_desc(SpinConserve(8, 4)), triples=((0, 1, 8),))
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


def test_the_bond_swap_messages_are_as_they_were():
    """The two passes share their checks and their plan; each names itself."""
    d = _lib.Subspace()
    d.type, d.L = 0, 64
    rc = _lib.lib().dnm_swap_moments_plan(C.byref(d), 3, None, None, None, None, None)
    assert rc != 0 and _lib.lib().dnm_last_error().decode() == "bond-swap moments: 2^64 rows"
    assert _plan_refused(d) == "chirality moments: 2^64 rows"
    ok = _desc(Full(L=8))
    rc = _lib.lib().dnm_swap_moments_plan(C.byref(ok), 64, None, None, None, None, None)
    assert rc != 0 and _lib.lib().dnm_last_error().decode() == "bond-swap moments: 64 bonds (1 to 63 in one call)"


# ---- partner indices ------------------------------------------------------------------------------------------------
def triple_set(L):
    """Triples at site 0 and at site L - 1, adjacent and far, both senses, every position of site L - 1, one repeat."""
    h = L // 2
    return [(0, 1, 2), (0, 2, 1), (2, 1, 0), (0, h, L - 1), (0, L - 1, h), (L - 1, 0, h), (h, L - 1, 0),
            (L - 3, L - 2, L - 1), (L - 1, L - 2, L - 3), (L - 2, L - 1, 1), (1, h, h + 1), (3, 7, 5), (0, 1, 2),
            (L - 1, 1, L - 2), (h, 0, 1)]


def rotated(cfg, a, b, c):
    """bit a <- bit b, bit b <- bit c, bit c <- bit a"""
    xa, xb, xc = (cfg >> a) & 1, (cfg >> b) & 1, (cfg >> c) & 1
    one = np.int64(1)
    return (cfg & ~((one << a) | (one << b) | (one << c))) | (xb << a) | (xc << b) | (xa << c)


def test_the_rotation_is_p_ab_p_bc():
    """Column 1 + m is C_m psi with C_m = P_ab P_bc (P_bc first), in the convention (P psi)(r) = psi(P r)."""
    cfg = np.arange(1 << 5, dtype=np.int64)

    def exchanged(v, a, b):
        differ = ((v >> a) ^ (v >> b)) & 1
        return v ^ (differ << a) ^ (differ << b)

    for a, b, c in ((0, 1, 2), (4, 0, 2), (3, 1, 4)):
        psi = np.random.default_rng(5).standard_normal(cfg.size)
        p_bc = psi[exchanged(cfg, b, c)]
        p_ab_p_bc = p_bc[exchanged(cfg, a, b)]
        assert np.array_equal(psi[rotated(cfg, a, b, c)], p_ab_p_bc)
        # the opposite rotation of (a, b, c) is the rotation of (a, c, b)
        assert np.array_equal(rotated(rotated(cfg, a, b, c), a, c, b), cfg)


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
    triples = triple_set(L)
    rows = np.arange(dim, dtype=np.int64)
    idx, sign = backend.cyc_partner_indices(_desc(sub), triples, rows)
    assert idx.shape == sign.shape == (dim, len(triples)) and idx.dtype == np.int64 and sign.dtype == np.int8
    cfg = np.asarray(sub.idx_to_state(rows), dtype=np.int64)
    for m, (a, b, c) in enumerate(triples):
        want = np.asarray(sub.state_to_idx(rotated(cfg, a, b, c)), dtype=np.int64)
        assert np.all(want >= 0)
        assert np.array_equal(idx[:, m], want), (a, b, c, np.argwhere(idx[:, m] != want)[:4])
        # a rotation is a permutation of the rows
        assert np.array_equal(np.sort(idx[:, m]), rows)
    assert np.array_equal(sign, np.ones_like(sign))
    assert np.array_equal(idx[:, 0], idx[:, 12])


XPARITY = [
    pytest.param(lambda: Full(L=10), id="x_full10"),
    pytest.param(lambda: Parity('even', L=12), id="x_parity12_even"),
    pytest.param(lambda: Parity('odd', L=12), id="x_parity12_odd"),
    pytest.param(lambda: SpinConserve(12, 6), id="x_sc12_6"),
]


@pytest.mark.parametrize("sector", [+1, -1])
@pytest.mark.parametrize("make", XPARITY)
def test_partner_indices_xparity(make, sector):
    """The rows are the parent's first dim / 2: bit L - 1 clear.  Where the rotation sets bit L - 1 the amplitude is the
    sector's sign times that of the complement, again a representative."""
    sub = make()
    L, half = sub.L, sub.get_dimension() // 2
    triples = triple_set(L)
    rows = np.arange(half, dtype=np.int64)
    idx, sign = backend.cyc_partner_indices(_desc(sub), triples, rows, sector)
    cfg = np.asarray(sub.idx_to_state(rows), dtype=np.int64)
    assert not np.any((cfg >> (L - 1)) & 1)
    everything = (np.int64(1) << L) - 1
    flipped = 0
    for m, (a, b, c) in enumerate(triples):
        rot = rotated(cfg, a, b, c)
        top = ((rot >> (L - 1)) & 1) == 1
        want = np.asarray(sub.state_to_idx(np.where(top, rot ^ everything, rot)), dtype=np.int64)
        assert np.all((want >= 0) & (want < half))
        assert np.array_equal(idx[:, m], want), (a, b, c, np.argwhere(idx[:, m] != want)[:4])
        assert np.array_equal(sign[:, m], np.where(top, sector, 1)), (a, b, c)
        assert not np.any(top) or L - 1 in (a, b, c)
        # some row takes the branch wherever the triple holds site L - 1
        assert bool(np.any(top)) == (L - 1 in (a, b, c))
        flipped += int(np.any(top))
        assert np.array_equal(np.sort(idx[:, m]), rows)
    assert flipped == sum(L - 1 in t for t in triples) >= 6
