"""
The plans of the three observable passes, pinned exactly (dnm_pm_moments_plan, dnm_swap_moments_plan,
dnm_zz_moments_plan; host only -- no GPU needed).  The number of workgroups fixes the order of the sums and with it the
bits of a result, the panel fixes the time: the rule is written out here once more, in Python, and every output of a
plan is compared with it by ==.

The panel scheme (csrc/gram_tile.h): NB tile rows of 16 columns, rows of 16 NB + 1 amplitudes of 16 bytes, a panel of
2^B rows with B = 9 at one tile row and 7 from two on, lowered down to 6 while the panel and the binomial table exceed
152 KB of LDS; the partial tiles are NB (NB + 1) / 2 + NB^2 tiles of 256 doubles per workgroup.
  sigma+ sigma-: L columns, the rows of sector k + 1 (SpinConserve; table of (k + 2) x (L + 1) binomials, none without
                 rows), one workgroup per panel, at most 1024
  bond swaps:    nbonds + 1 columns, the rows of the subspace (table of (k + 1) x (L + 1) binomials), one workgroup per
                 2^9 rows, at most 1024
  sigma-z:       L + 1 columns and no panel: one workgroup per 2048 rows, at most 1024, lower-triangle tiles only
"""
import ctypes as C
from math import comb

import pytest

from dynamite_amd import _lib, backend
from dynamite_amd.subspaces import Full, Parity, SpinConserve

from test_pm_moments_host import _desc, _raw_spin_conserve

LDS_BUDGET = 152 * 1024
MAX_WG = 1024


def gram_rule(ncols, nrows, table_bytes, nwg_of):
    """(tile rows, log2 of the panel's rows, workgroups, bytes of LDS, bytes of partial tiles); nwg_of(panels) = the
    workgroups before the clamp to [1, 1024]"""
    nb = -(-ncols // 16)
    row_bytes = (16 * nb + 1) * 16
    B = 9 if nb == 1 else 7
    while B > 6 and (row_bytes << B) + table_bytes > LDS_BUDGET:
        B -= 1
    npanels = (nrows + (1 << B) - 1) >> B
    nwg = max(1, min(nwg_of(npanels), MAX_WG))
    return nb, B, nwg, (row_bytes << B) + table_bytes, nwg * (nb * (nb + 1) // 2 + nb * nb) * 256 * 8


def pm_rule(kind, L, k):
    if kind == "sc":
        nrows = comb(L, k + 1)
        table = (k + 2) * (L + 1) * 8 if nrows else 0
    else:
        nrows, table = 1 << (L - (kind == "parity")), 0
    return gram_rule(L, nrows, table, lambda npanels: npanels)


def swap_rule(kind, L, k, nbonds):
    if kind == "sc":
        nrows, table = comb(L, k), (k + 1) * (L + 1) * 8
    else:
        nrows, table = 1 << (L - (kind == "parity")), 0
    return gram_rule(nbonds + 1, nrows, table, lambda npanels: (nrows + 511) >> 9)


SUBSPACES = ([("full", L, 0) for L in (1, 4, 16, 17, 30, 32, 33, 48, 49, 62)]
             + [("parity", L, 0) for L in (2, 17, 33)]
             + [("sc", L, k) for L, k in ((16, 8), (30, 15), (32, 16), (34, 2), (50, 2), (12, 12), (12, 0))])
IDS = ["%s%d_%d" % c if c[0] == "sc" else "%s%d" % c[:2] for c in SUBSPACES]


def _make(kind, L, k):
    return _desc(Full(L=L) if kind == "full" else Parity('even', L=L) if kind == "parity" else SpinConserve(L, k))


@pytest.mark.parametrize("kind,L,k", SUBSPACES, ids=IDS)
def test_pm_plan(kind, L, k):
    assert backend.pm_moments_plan(_make(kind, L, k)) == pm_rule(kind, L, k)


def test_pm_plan_raw_64_spins():
    assert backend.pm_moments_plan(_raw_spin_conserve(64, 1)) == pm_rule("sc", 64, 1)


@pytest.mark.parametrize("kind,L,k", SUBSPACES, ids=IDS)
def test_swap_plan(kind, L, k):
    d = _make(kind, L, k)
    for nbonds in (1, 15, 16, 31, 47, 48, 63):
        assert backend.swap_moments_plan(d, nbonds) == swap_rule(kind, L, k, nbonds), nbonds


ZZ_L = (4, 15, 16, 31, 47, 63)


@pytest.mark.parametrize("L", ZZ_L)
def test_zz_plan(L):
    """A plan depends on L and the number of rows alone; more rows than the subspace has are refused."""
    sub = Full(L=L) if L < 63 else SpinConserve(63, 8)
    d, dim = _desc(sub), sub.get_dimension()
    assert L < 63 or dim >= 1 << 30
    for nrows in (0, 1, 2047, 2048, 2049, 1 << 20, 1 << 30):
        if nrows > dim:
            tr, nw, sb = C.c_int(), C.c_int(), C.c_size_t()
            assert _lib.lib().dnm_zz_moments_plan(C.byref(d), nrows, C.byref(tr), C.byref(nw), C.byref(sb)) != 0
            continue
        nb = -(-(L + 1) // 16)
        nwg = max(1, min((nrows + 2047) // 2048, MAX_WG))
        assert backend.zz_moments_plan(d, nrows) == (nb, nwg, nwg * (nb * (nb + 1) // 2) * 256 * 8), nrows
