"""
The host side of the two-spin Pauli pass (csrc/pauli_kernels.hip, csrc/pauli_cols.h, dnm_pauli_moments_plan,
dnm_pauli_moments, dnm_pauli_partner_indices) -- no GPU needed: the plan (tile rows of the (n + 1) x (n + 1) result, a
panel that fits the LDS, a number of workgroups that follows from the number of rows alone), the arguments the calls
refuse before any device call, and the partner and sign of every row for every column: the Gram matrix built in numpy
from that table, with the zeros of a Parity sector and the phase of sigma-y, against <psi|sigma_a sigma_b|psi> from the
dense matrices of Operator.to_numpy.
"""
import ctypes as C

import numpy as np
import pytest

from dynamite_amd import _lib, backend
from dynamite_amd.operators import sigmax, sigmay, sigmaz
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve

LDS_BYTES = 160 * 1024


def _desc(sub):
    d = _lib.Subspace.from_buffer_copy(sub._c())
    d.vec_swizzle = 0
    d._keep = sub
    return d


def _raw(type_, L, space=0):
    d = _lib.Subspace()
    d.type, d.L, d.space = type_, L, space
    return d


# ---- the plan -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [15, 16, 47, 48, 63])
def test_plan_tile_rows(n):
    for d in (_desc(Full(L=20)), _desc(Parity('even', L=21)), _desc(Parity('odd', L=21))):
        tr, pb, nw, lds, sb = backend.pauli_moments_plan(d, n)
        assert tr == -(-(n + 1) // 16) and 1 <= tr <= 4
        assert (1 << pb) * (16 * tr + 1) * 16 <= lds <= LDS_BYTES
        nt = tr * (tr + 1) // 2
        assert sb == nw * (nt + tr * tr) * 256 * 8
        assert nw == min(1024, (1 << 20) // 512)
        assert backend.pauli_moments_plan(d, n) == (tr, pb, nw, lds, sb)


def test_plan_outputs_may_be_null():
    d = _desc(Full(L=10))
    nw = C.c_int()
    _lib.check(_lib.lib().dnm_pauli_moments_plan(C.byref(d), 5, None, None, C.byref(nw), None, None))
    assert nw.value == 2
    _lib.check(_lib.lib().dnm_pauli_moments_plan(C.byref(d), 5, None, None, None, None, None))


# ---- refusals: each is decided before any device call ---------------------------------------------------------------
def _cols(pairs):
    c = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1)
    return c, c.ctypes.data_as(C.POINTER(C.c_int32))


def _plan_refused(d, n=3):
    rc = _lib.lib().dnm_pauli_moments_plan(C.byref(d) if d is not None else None, n, None, None, None, None, None)
    assert rc != 0
    msg = _lib.lib().dnm_last_error().decode()
    assert msg
    return msg


def _call_refused(d, cols=((0, 1), (1, 2), (2, 3)), x=0x1000, out=True, n=None, give_cols=True):
    """dnm_pauli_moments with a pointer that is never followed: the call is refused first."""
    buf = np.zeros(2 * 64 * 64)
    c, cp = _cols(cols)
    rc = _lib.lib().dnm_pauli_moments(C.c_void_p(x), C.byref(d) if d is not None else None,
                                      len(cols) if n is None else n, cp if give_cols else None,
                                      _lib.pf64(buf) if out else None, None)
    assert rc != 0
    msg = _lib.lib().dnm_last_error().decode()
    assert msg
    return msg


def _partners_refused(d, cols=((0, 1),), rows=(0,), give=True, give_cols=True, n=None):
    c, cp = _cols(cols)
    rows = np.asarray(rows, dtype=np.int64)
    idx = np.zeros(rows.size * len(cols), dtype=np.int64)
    sign = np.zeros(rows.size * len(cols), dtype=np.int8)
    rc = _lib.lib().dnm_pauli_partner_indices(C.byref(d) if d is not None else None, len(cols) if n is None else n,
                                              cp if give_cols else None, rows.size, _lib.p64(rows),
                                              _lib.p64(idx) if give else None, sign.ctypes.data_as(C.POINTER(C.c_int8)))
    assert rc != 0
    msg = _lib.lib().dnm_last_error().decode()
    assert msg
    return msg


def _explicit():
    rng = np.random.default_rng(11)
    states = rng.choice(1 << 20, size=300, replace=False).astype(np.int64) | (np.int64(1) << 39)
    return Explicit(states, L=40)


def test_refusals_of_the_subspace():
    bad = []
    bad.append((_desc(_explicit()), "Explicit"))
    bad.append((_desc(SpinConserve(12, 6)), "flip leaves the sector"))
    bad.append((_desc(SpinConserve(12, 6)), "dnm_zz_moments"))
    bad.append((_desc(SpinConserve(12, 6)), "dnm_pm_moments"))
    bad.append((_raw(99, 8), "unknown subspace type"))
    bad.append((_raw(0, 65), "L=65"))
    bad.append((_raw(0, 0), "L=0"))
    bad.append((_raw(1, 65), "L=65"))
    bad.append((_raw(0, 63), "63 index bits"))
    bad.append((_raw(0, 64), "64 index bits"))
    bad.append((_raw(1, 64), "63 index bits"))
    perm = np.arange(12, dtype=np.int8)
    for sub in (Full(L=12), Parity('odd', L=12)):
        d = _desc(sub)
        d.site_perm = perm.ctypes.data_as(C.POINTER(C.c_int8))
        bad.append((d, "site_perm"))
        for shift in (3, 4, 25, -1):
            d = _desc(sub)
            d.vec_swizzle = shift
            bad.append((d, "vec_swizzle %d" % shift))
    for space in (2, -1):
        bad.append((_raw(1, 12, space), "parity space"))
    for d, word in bad:
        assert word in _plan_refused(d)
        assert word in _call_refused(d)
        assert word in _partners_refused(d)
    assert "null" in _plan_refused(None)
    assert "null" in _call_refused(None)
    assert "null" in _partners_refused(None)
    # the largest descriptors that pass
    assert backend.pauli_moments_plan(_raw(0, 62), 63)[0] == 4
    assert backend.pauli_moments_plan(_raw(1, 63, 1), 63)[2] == 1024
    for shift in (5, 24):
        d = _desc(Full(L=12))
        d.vec_swizzle = shift
        assert backend.pauli_moments_plan(d, 1)[0] == 1


def test_refusals_of_the_arguments():
    ok = _desc(Full(L=8))
    assert "null" in _call_refused(ok, x=0)
    assert "null" in _call_refused(ok, out=False)
    assert "null" in _call_refused(ok, give_cols=False)
    assert "null" in _partners_refused(ok, give=False)
    assert "null" in _partners_refused(ok, give_cols=False)
    for n in (0, -1, 64):
        assert "columns" in _plan_refused(ok, n=n)
        assert "columns" in _call_refused(ok, cols=[(0, 1)] * 64, n=n)
        assert "columns" in _partners_refused(ok, cols=[(0, 1)] * 64, n=n)
    assert backend.pauli_moments_plan(ok, 63)[0] == 4
    for cols, word in ((((0, 1), (8, 2)), "outside"), (((0, 1), (-1, 2)), "outside"), (((3, 0),), "kind"),
                       (((3, 4),), "kind"), (((3, -1),), "kind")):
        assert word in _call_refused(ok, cols=cols)
        assert word in _partners_refused(ok, cols=cols)
    assert "outside" in _call_refused(_desc(Parity('even', L=8)), cols=((8, 1),))
    assert "row" in _partners_refused(ok, rows=(256,))
    assert "row" in _partners_refused(ok, rows=(-1,))
    assert "row" in _partners_refused(_desc(Parity('even', L=8)), rows=(128,))


# ---- partner indices ------------------------------------------------------------------------------------------------
PAULI = {1: sigmax, 2: sigmay, 3: sigmaz}
PHASE = {1: 1.0, 2: -1j, 3: 1.0}


def dense(kind, site, L):
    op = PAULI[kind](site)
    op.L = L
    return np.asarray(op.to_numpy(sparse=False))


@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=6), id="full6"),
                                  pytest.param(lambda: Parity('even', L=7), id="parity7_even"),
                                  pytest.param(lambda: Parity('odd', L=7), id="parity7_odd")])
def test_gram_from_the_partner_table(make):
    """All rows, all 3 L columns.  A[:, 1 + c] = sign * psi[idx]; G = A^H A with the entries between a flipping and a
    non-flipping column of a Parity sector set to zero and the phase -i of sigma-y on rows (conjugated) and columns is
    <psi|sigma_a sigma_b|psi> of the state embedded in the full space, to 1e-12 <psi|psi>: sums of at most 128 terms in
    double precision."""
    sub = make()
    L, dim = sub.L, sub.get_dimension()
    parity = isinstance(sub, Parity)
    cols = [(j, k) for j in range(L) for k in (1, 2, 3)]
    rows = np.arange(dim, dtype=np.int64)
    idx, sign = backend.pauli_partner_indices(_desc(sub), cols, rows)
    assert idx.shape == sign.shape == (dim, 3 * L) and idx.dtype == np.int64 and sign.dtype == np.int8
    assert np.all((idx >= 0) & (idx < dim)) and np.all(np.abs(sign) == 1)
    rng = np.random.default_rng(L)
    psi = rng.standard_normal(dim) + 1j * rng.standard_normal(dim)
    A = np.empty((dim, 3 * L + 1), dtype=np.complex128)
    A[:, 0] = psi
    flips = np.zeros(3 * L + 1, dtype=bool)
    phase = np.ones(3 * L + 1, dtype=np.complex128)
    for c, (j, k) in enumerate(cols):
        # a column is a permutation of the rows
        assert np.array_equal(np.sort(idx[:, c]), rows)
        assert np.array_equal(idx[:, c] == rows, np.full(dim, k == 3 or (parity and j == 0)))
        A[:, 1 + c] = sign[:, c] * psi[idx[:, c]]
        flips[1 + c] = k != 3
        phase[1 + c] = PHASE[k]
    G = A.conj().T @ A
    if parity:
        G[flips[:, None] != flips[None, :]] = 0.0
    got = np.conj(phase)[:, None] * G * phase[None, :]
    full = np.zeros(1 << L, dtype=np.complex128)
    full[np.asarray(sub.idx_to_state(rows), dtype=np.int64)] = psi
    ops = [np.eye(1 << L)] + [dense(k, j, L) for j, k in cols]
    images = np.stack([op @ full for op in ops], axis=1)
    want = images.conj().T @ images
    norm2 = np.vdot(psi, psi).real
    err = np.max(np.abs(got - want))
    print("%r: largest error %.3e (bound %.3e)" % (sub, err, 1e-12 * norm2))
    assert err <= 1e-12 * norm2
    # the products the definitions fix
    for j in range(L):
        x, y, z = 1 + 3 * j, 2 + 3 * j, 3 + 3 * j
        assert abs(got[x, y] - 1j * got[0, z]) <= 1e-12 * norm2
        assert abs(got[x, x] - norm2) <= 1e-12 * norm2
