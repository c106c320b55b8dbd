"""
The host side of the sigma+ sigma- pass (csrc/pm_kernels.hip, dnm_pm_moments_plan, dnm_pm_moments,
dnm_pm_partner_indices) -- no GPU needed: the plan (tile rows of the L x L result, a panel that fits in the LDS of a
compute unit, a number of workgroups that follows from the subspace alone, the bytes of the partial tiles), the
arguments the calls refuse before any device call, and the partner indices of SpinConserve rows against numpy.

sigma_minus(j) sets bit j, so the rows of SpinConserve(L, k) are the configurations with k + 1 set bits and the partner
of a row for site j, a set bit of it, is the row with that bit cleared: every index of sector k appears L - k times.
"""
import ctypes as C
from math import comb

import numpy as np
import pytest

from dynamite_amd import _lib, backend
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve


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


PLAN = [
    ("full4", lambda: _desc(Full(L=4)), 4, 16),
    ("full16", lambda: _desc(Full(L=16)), 16, 1 << 16),
    ("full17", lambda: _desc(Full(L=17)), 17, 1 << 17),
    ("full30", lambda: _desc(Full(L=30)), 30, 1 << 30),
    ("parity17", lambda: _desc(Parity('even', L=17)), 17, 1 << 16),
    ("sc34_2", lambda: _desc(SpinConserve(34, 2)), 34, comb(34, 3)),
    ("sc50_2", lambda: _desc(SpinConserve(50, 2)), 50, comb(50, 3)),
    ("sc64_1", lambda: _raw_spin_conserve(64, 1), 64, comb(64, 2)),
]


@pytest.mark.parametrize("name,make,L,rows", PLAN, ids=[c[0] for c in PLAN])
def test_plan(name, make, L, rows):
    d = make()
    tr, pb, nw, lds, sb = backend.pm_moments_plan(d)
    assert tr == -(-L // 16)
    assert (1 << pb) * 16 * tr * 16 <= lds <= 160 * 1024
    nt = tr * (tr + 1) // 2
    assert sb == nw * (nt + tr * tr) * 256 * 8
    # every row lies in the panels of some workgroup; a sweep of a million rows is shared out
    assert nw >= 1 and nw <= max(1, -(-rows >> pb))
    if rows >= 1 << 20:
        assert nw > 1
    assert backend.pm_moments_plan(d) == (tr, pb, nw, lds, sb)


def test_plan_panel_of_two_tile_rows():
    """L = 30: 128 rows of 32 sites, so that two workgroups share the LDS of a compute unit."""
    tr, pb, _, lds, _ = backend.pm_moments_plan(_desc(Full(L=30)))
    assert (tr, pb) == (2, 7) and 2 * lds <= 160 * 1024


def test_plan_outputs_may_be_null():
    d = _desc(Full(L=10))
    nw = C.c_int()
    _lib.check(_lib.lib().dnm_pm_moments_plan(C.byref(d), None, None, C.byref(nw), None, None))
    assert nw.value >= 1


# ---- refusals: each is decided before any device call ---------------------------------------------------------------
def _plan_refused(d):
    rc = _lib.lib().dnm_pm_moments_plan(C.byref(d) if d is not None else None, None, None, None, None, None)
    assert rc != 0
    msg = _lib.lib().dnm_last_error().decode()
    assert msg
    return msg


def _call_refused(d, x=0x1000, out=True):
    """dnm_pm_moments with a pointer that is never followed: the call is refused first."""
    buf = np.zeros(2 * 64 * 64)
    rc = _lib.lib().dnm_pm_moments(C.c_void_p(x), C.byref(d) if d is not None else None,
                                   _lib.pf64(buf) if out else None, None)
    assert rc != 0
    msg = _lib.lib().dnm_last_error().decode()
    assert msg
    return msg


def _explicit():
    rng = np.random.default_rng(11)
    states = rng.choice(1 << 20, size=300, replace=False).astype(np.int64) | (np.int64(1) << 39)
    return Explicit(states, L=40)


def test_refusals():
    bad = []
    d = _desc(_explicit())
    bad.append((d, "Explicit"))
    sub = SpinConserve(22, 11)
    d = _desc(sub)
    d.vec_swizzle = 6 | (4 << 8)
    bad.append((d, "reference order"))
    d = _desc(sub)
    perm = np.arange(22, dtype=np.int8)
    d.site_perm = perm.ctypes.data_as(C.POINTER(C.c_int8))
    bad.append((d, "site_perm"))
    d = _raw_spin_conserve(64, 1)
    d.L, d.ld_nchoosek = 65, 66
    bad.append((d, "L=65"))
    d = _lib.Subspace()
    d.type, d.L = 0, 65
    bad.append((d, "L=65"))
    for d, word in bad:
        assert word in _plan_refused(d)
        assert word in _call_refused(d)
    assert "null" in _plan_refused(None)
    assert "null" in _call_refused(None)
    ok = _desc(Full(L=8))
    assert "null" in _call_refused(ok, x=0)
    assert "null" in _call_refused(ok, out=False)


def test_partner_indices_refusals():
    def refused(d, n, rows):
        out = np.zeros(max(1, n) * 64, dtype=np.int64)
        rc = _lib.lib().dnm_pm_partner_indices(C.byref(d), n, _lib.p64(rows) if rows is not None else None,
                                               _lib.p64(out))
        assert rc != 0
        return _lib.lib().dnm_last_error().decode()
    assert "SpinConserve" in refused(_desc(Full(L=8)), 1, np.zeros(1, dtype=np.int64))
    d = _desc(SpinConserve(12, 6))
    assert "row" in refused(d, 1, np.array([comb(12, 7)], dtype=np.int64))
    assert "row" in refused(d, 1, np.array([-1], dtype=np.int64))
    assert "null" in refused(d, 1, None)
    assert "row" in refused(_desc(SpinConserve(12, 12)), 1, np.zeros(1, dtype=np.int64))      # no neighbouring sector


# ---- partner indices ------------------------------------------------------------------------------------------------
PARTNERS = [(16, 8), (34, 2), (63, 1), (12, 1), (12, 11), (12, 12), (12, 0)]


@pytest.mark.parametrize("L,k", PARTNERS, ids=["sc%d_%d" % c for c in PARTNERS])
def test_partner_indices(L, k):
    sub = SpinConserve(L, k)
    d = _desc(sub)
    nrows = comb(L, k + 1)                  # the neighbouring sector (none for k = L)
    if nrows <= 20000:
        rows = np.arange(nrows, dtype=np.int64)
    else:
        rng = np.random.default_rng(1000 * L + k)
        rows = np.unique(np.concatenate([np.arange(64), np.arange(nrows - 64, nrows),
                                         rng.integers(0, nrows, 20000)])).astype(np.int64)
    got = backend.pm_partner_indices(d, rows)
    assert got.shape == (rows.size, L)
    if nrows == 0:
        return
    cfg = np.asarray(SpinConserve(L, k + 1).idx_to_state(rows), dtype=np.int64)
    for j in range(L):
        bit = (cfg >> j) & 1
        want = np.where(bit == 1, np.asarray(sub.state_to_idx(cfg ^ (np.int64(1) << j)), dtype=np.int64), -1)
        assert np.array_equal(got[:, j], want), (j, np.argwhere(got[:, j] != want)[:4])
    if rows.size == nrows:
        hit = got[got >= 0]
        assert np.array_equal(np.bincount(hit, minlength=sub.get_dimension()), np.full(sub.get_dimension(), L - k))
