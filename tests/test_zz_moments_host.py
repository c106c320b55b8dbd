"""
The plan of the sigma-z moments sweep (dnm_zz_moments_plan, host only -- no GPU needed): tile rows of the
(L + 1) x (L + 1) result, a number of workgroups that follows from the number of rows alone, the bytes of their partial
tiles, and the arguments the call refuses.
"""
import ctypes as C

import numpy as np
import pytest

from dynamite_amd import _lib, backend
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve


def _explicit():
    rng = np.random.default_rng(11)
    states = rng.choice(1 << 20, size=300, replace=False).astype(np.int64) | (np.int64(1) << 39)
    return Explicit(states, L=40)


CASES = [
    ("full4", lambda: Full(L=4), 1),
    ("full15", lambda: Full(L=15), 1),
    ("full16", lambda: Full(L=16), 2),
    ("full30", lambda: Full(L=30), 2),
    ("parity17", lambda: Parity('even', L=17), 2),
    ("sc34_2", lambda: SpinConserve(34, 2), 3),
    ("sc50_2", lambda: SpinConserve(50, 2), 4),
    ("sc63_1", lambda: SpinConserve(63, 1), 4),
    ("explicit40", _explicit, 3),
]


def _desc(sub):
    """The subspace's descriptor in index order (what the growth of the plan is checked on: any number of rows)."""
    d = _lib.Subspace.from_buffer_copy(sub._c())
    d.vec_swizzle = 0
    d._keep = sub
    return d


@pytest.mark.parametrize("name,make,tile_rows", CASES, ids=[c[0] for c in CASES])
def test_plan(name, make, tile_rows):
    sub = make()
    d = _desc(sub)
    L, dim = sub.L, sub.get_dimension()
    assert tile_rows == -(-(L + 1) // 16)
    sizes = sorted({0, 1, 63, 64, 65, 255, 256, 2047, 2048, 2049, 4096, 100000, dim // 3, dim // 2, dim - 1, dim})
    sizes = [n for n in sizes if 0 <= n <= dim]
    last = 0
    for n in sizes:
        tr, nw, sb = backend.zz_moments_plan(d, n)
        assert tr == tile_rows
        assert nw >= 1 and nw >= last, (n, nw, last)
        assert sb == nw * (tr * (tr + 1) // 2) * 256 * 8
        last = nw
    if dim >= 1 << 20:
        assert last > 1           # (a sweep of a million rows is shared out)


def test_plan_outputs_may_be_null():
    d = _desc(Full(L=10))
    nw = C.c_int()
    _lib.check(_lib.lib().dnm_zz_moments_plan(C.byref(d), 1024, None, C.byref(nw), None))
    assert nw.value >= 1


def _refused(d, nrows):
    tr, nw, sb = C.c_int(), C.c_int(), C.c_size_t()
    rc = _lib.lib().dnm_zz_moments_plan(C.byref(d), nrows, C.byref(tr), C.byref(nw), C.byref(sb))
    assert rc != 0
    msg = _lib.lib().dnm_last_error().decode()
    assert msg
    return msg


def test_plan_refuses():
    # 64 spins: the shifted configuration has no room for the constant column
    d = _lib.Subspace()
    d.type, d.L = 0, 64
    assert "L=64" in _refused(d, 16)
    # negative number of rows, more rows than the subspace has
    d = _desc(Full(L=8))
    assert "rows" in _refused(d, -1)
    assert "rows" in _refused(d, 257)
    # a swizzled block whose size the swizzle does not map onto itself
    d.vec_swizzle = 5
    assert "swizzle" in _refused(d, 48)
    # the SpinConserve internal layout: the caller converts
    sub = SpinConserve(22, 11)
    d = _desc(sub)
    d.vec_swizzle = 6 | (4 << 8)
    assert "reference order" in _refused(d, sub.get_dimension())
    # a relabelled subspace
    d = _desc(sub)
    perm = np.arange(22, dtype=np.int8)
    d.site_perm = perm.ctypes.data_as(C.POINTER(C.c_int8))
    assert "site_perm" in _refused(d, sub.get_dimension())
