"""
The four observable sweeps built on csrc/gram_tile.h -- sigma+ sigma- (csrc/pm_kernels.hip), bond swaps
(swap_kernels.hip), three-site rotations (cyc_kernels.hip) and single-site Paulis (pauli_kernels.hip) -- through the C
ABI, one call at a time: dnm_pm_moments, dnm_swap_moments, dnm_cyc_moments and dnm_pauli_moments on device buffers of
the test's own, with descriptors taken from the subspace objects (raw ones for L = 64).  Nothing goes through State,
which would normalise.

Exact cases: real and imaginary parts of every amplitude are independent non-zero integers in [-8, 8]
(tests/test_gpu_vec.py::ints).  A product of two parts has modulus <= 64 and a component of an entry of G sums 2 rows
of them: integers far below 2^53 (tests/gram_ref.py asserts it case by case) on the matrix cores, in the sum of the
wavefronts through LDS and in the sum of the workgroups alike, so any order of summation gives the same value and the
tests assert EQUALITY with the int64 reference of tests/gram_ref.py.  Equality of values, not of bit patterns: the
mirrored triangle holds -im, which is -0.0 where a sum is zero.

Buffers: the state lies between 64 NaN amplitudes on each side (a masked fetch that reads anyway and multiplies by zero,
or a partner index one off the end, shows as NaN); ``out`` is a host array, pre-filled with a sentinel and between 64
sentinels.  After every call: the values equal the reference, no sentinel or NaN is left and the guards are intact, G
equals its conjugate transpose and has a real diagonal, the device state with its guards is bit-identical to its
upload, and a second call returns the same bytes.

CASES is the table of the exact cases; tests/test_gram_ref.py (no GPU) computes the plan of each and proves which
kernel instances, panels and workgroup shares the table reaches.

Rounding cases (one per fill, normal deviates) against numpy.longdouble; the bound is derived beside them.
"""
import collections
import ctypes as C
import functools
from math import comb

import numpy as np
import pytest

from dynamite_amd import _lib, backend
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve
import gram_ref
import test_gpu_vec
from test_gpu_vec import Buf, G, NAN, SENT, cplx, gamma, ints, same_bits, vec_pos
from test_gram_plan_host import gram_rule

pytestmark = pytest.mark.gpu

LD = np.longdouble
TYPE = {"full": 0, "parity": 1, "sc": 3}           # dnm_subspace.type (include/dynamite_amd.h)
WIDTHS = (16, 17, 48, 49, 64)                       # columns of A: one to four tile rows, the last two ragged and full


# ---------------------------------------------------------------- the lists of bonds, triples and Pauli columns

def _fill(base, n, L, seed, draw):
    rs = np.random.RandomState(7000 + 64 * L + seed)
    out = list(base)
    while len(out) < n:
        it = draw(rs)
        if it is not None:
            out.append(it)
    return out[:n]


def bonds(L, n, seed=1):
    """Site 0 (Parity's missing bit) and site L - 1 (the complement under XParity) in either position, adjacent and
    far pairs, both orientations, a repeat; then seeded random pairs."""
    T, M = L - 1, L // 2
    base = [(0, 1), (1, 0), (0, T), (T, 0), (T - 1, T), (T, M), (0, 1), (M, M + 1), (1, T - 1), (T, T - 1)]
    base = [p for p in base if p[0] != p[1] and min(p) >= 0 and max(p) < L]

    def draw(rs):
        a, b = (int(v) for v in rs.randint(0, L, 2))
        return (a, b) if a != b else None
    return _fill(base, n, L, seed, draw)


def triples(L, n, seed=2):
    """Site 0 and site L - 1 in each position of the triple, adjacent and far sites, both orientations, a repeat; then
    seeded random triples."""
    T, M = L - 1, L // 2
    base = [(0, 1, 2), (0, 2, 1), (T, 0, 1), (1, T, 0), (0, 1, T), (T, T - 1, T - 2), (0, M, T), (0, 1, 2), (2, 0, T - 1),
            (M, T, M - 1)]
    base = [t for t in base if len(set(t)) == 3 and min(t) >= 0 and max(t) < L]

    def draw(rs):
        t = tuple(int(v) for v in rs.randint(0, L, 3))
        return t if len(set(t)) == 3 else None
    return _fill(base, n, L, seed, draw)


def paulis(L, n, seed=3):
    """Sign-only columns before flipping ones in the caller's order, a flipping column at site 0 (mask 0 on Parity), all
    three kinds at one site, site L - 1, repeats; then seeded random columns (repeats among them: 3 L may be < n)."""
    T = L - 1
    base = [(1 % L, 3), (0, 3), (0, 1), (2 % L, 1), (2 % L, 2), (2 % L, 3), (0, 2), (T, 1), (T, 2), (T, 3), (0, 1),
            (1 % L, 3)]
    return _fill(base, n, L, seed, lambda rs: (int(rs.randint(0, L)), int(rs.randint(1, 4))))


ITEMS = {"swap": bonds, "cyc": triples, "pauli": paulis}


# ---------------------------------------------------------------- the case table

Case = collections.namedtuple("Case", "name sweep kind L k space xsec items swz")
CASES = []


def add(sweep, kind, L, k=0, space=0, xsec=0, width=None, items=None, swz=(0,), note=""):
    if sweep != "pm" and items is None:
        items = ITEMS[sweep](L, width - 1)
    sub = {"full": "Full(%d)" % L, "parity": "Parity(%d,%d)" % (L, space), "sc": "SC(%d,%d)" % (L, k)}[kind]
    name = "%s-%s%s%s%s" % (sweep, sub, {0: "", 1: "-x+", -1: "-x-"}[xsec],
                            "" if sweep == "pm" else "-w%d" % (len(items) + 1), "-" + note if note else "")
    assert name not in [c.name for c in CASES], name
    CASES.append(Case(name, sweep, kind, L, k, space, xsec, None if items is None else tuple(items), tuple(swz)))


# every kernel instance at its smallest shape: TYPE x tile rows, both sectors of XParity over each parent
for _sweep in ("swap", "cyc"):
    for _w in WIDTHS:
        add(_sweep, "full", 10, width=_w)
        add(_sweep, "parity", 11, space=0, width=_w)
        add(_sweep, "parity", 11, space=1, width=_w)
        add(_sweep, "sc", 12, 6, width=_w)
        for _x in (1, -1):
            add(_sweep, "full", 10, xsec=_x, width=_w)
            add(_sweep, "parity", 12, space=0, xsec=_x, width=_w)
            add(_sweep, "parity", 12, space=1, xsec=_x, width=_w)
            add(_sweep, "sc", 12, 6, xsec=_x, width=_w)
for _w in WIDTHS:
    add("pauli", "full", 10, width=_w)
    add("pauli", "parity", 11, space=0, width=_w)
    add("pauli", "parity", 11, space=1, width=_w)
# sigma+ sigma- has L columns: tile rows 1 to 4 need L up to 16, 32, 48, 64
add("pm", "full", 10)
add("pm", "parity", 11, space=0)
add("pm", "parity", 11, space=1)
add("pm", "sc", 12, 6)
add("pm", "full", 17)
add("pm", "parity", 18, space=1)
add("pm", "sc", 18, 3)
add("pm", "sc", 34, 2)
add("pm", "sc", 50, 2)
# lowered panels: a binomial table of (k + 1)(L + 1) 8 bytes beside the panel, and the mirror sectors for contrast
for _sweep in ("swap", "cyc"):
    for _w in (16, 17, 48, 64):
        add(_sweep, "sc", 63, 60, width=_w)
    for _w in (16, 64):
        add(_sweep, "sc", 63, 3, width=_w)
add("pm", "sc", 63, 59)
add("pm", "sc", 63, 2)
# L = 64: bit 63 of a configuration
add("pm", "sc", 64, 1)
for _sweep in ("swap", "cyc"):
    for _w in (16, 49):
        add(_sweep, "sc", 64, 2, width=_w)
# several panels per workgroup, a ragged last panel, workgroups with nothing to do
add("pm", "sc", 20, 9)
add("pm", "full", 18)
add("pm", "parity", 19, space=0)
for _sweep in ("swap", "cyc"):
    add(_sweep, "sc", 22, 11, width=16)
    add(_sweep, "sc", 22, 11, width=17)
    add(_sweep, "sc", 22, 11, xsec=-1, width=17)
# swizzles below every panel (5, 6), and the production shift once per sweep
for _sweep in ("swap", "cyc", "pauli"):
    add(_sweep, "full", 12, width=16, swz=(0, 5, 6))
    add(_sweep, "full", 13, width=17, swz=(0, 5, 6))
    add(_sweep, "parity", 13, space=0, width=17, swz=(0, 5, 6))
    add(_sweep, "parity", 13, space=1, width=16, swz=(0, 5, 6))
    add(_sweep, "full", 20, width=16, swz=(0, 16))
for _sweep in ("swap", "cyc"):
    add(_sweep, "full", 12, xsec=1, width=17, swz=(0, 5, 6))
    add(_sweep, "parity", 14, space=1, xsec=-1, width=17, swz=(0, 5, 6))
add("pm", "full", 12, swz=(0, 5, 6))
add("pm", "full", 13, swz=(0, 5, 6))
add("pm", "parity", 13, space=0, swz=(0, 5, 6))
add("pm", "parity", 13, space=1, swz=(0, 5, 6))
add("pm", "full", 20, swz=(16,))
# small ends: dimension 1, dimension 2 under XParity, one column, fewer rows than a panel
for _sweep in ("swap", "cyc"):
    add(_sweep, "sc", 12, 0, width=16)
    add(_sweep, "sc", 12, 12, width=16)
    add(_sweep, "full", 6, width=4)
    add(_sweep, "parity", 6, space=1, width=17)
    add(_sweep, "sc", 6, 3, width=16)
add("pm", "sc", 12, 0)
add("pm", "sc", 12, 12)                 # no configuration has a spin left to lower: zeros, without a launch
add("pm", "sc", 12, 11)                 # one row
add("pm", "full", 1)
add("pm", "parity", 2, space=0)
add("pm", "full", 6)
add("pauli", "full", 1, items=[(0, 2)])
add("pauli", "parity", 2, space=1, items=[(0, 1), (1, 3), (1, 2)])
add("pauli", "parity", 6, space=0, width=16)
for _x in (1, -1):
    add("swap", "full", 2, xsec=_x, items=[(0, 1), (1, 0)])
    add("swap", "parity", 2, space=0, xsec=_x, items=[(1, 0)])
    add("swap", "sc", 2, 1, xsec=_x, items=[(0, 1)])
    add("cyc", "full", 3, xsec=_x, items=[(0, 1, 2), (2, 1, 0)])
    add("cyc", "parity", 4, space=0, xsec=_x, items=[(3, 0, 1)])
    add("cyc", "sc", 4, 2, xsec=_x, items=[(3, 1, 0), (0, 1, 3)])
add("swap", "full", 10, items=[(9, 0)], note="one")
add("swap", "sc", 12, 6, xsec=-1, items=[(0, 11)], note="one")
add("cyc", "parity", 11, space=1, items=[(10, 0, 5)], note="one")
add("pauli", "parity", 11, space=0, items=[(0, 2)], note="one")

BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------- subspaces, descriptors, plans (host only)

def ref_sub(case):
    return gram_ref.Sub(case.kind, case.L, case.k, case.space)


@functools.lru_cache(maxsize=None)
def space(kind, L, k, sp):
    """The subspace objects (kept alive: a descriptor points into the tables of its object)."""
    return Full(L=L) if kind == "full" else Parity(sp, L=L) if kind == "parity" else SpinConserve(L, k)


def raw_spin_conserve(L, k):
    """A SpinConserve descriptor filled in by hand: the Python class stops at 63 spins, these passes at 64."""
    tab = np.array([[comb(n, m) for n in range(L + 1)] for m in range(k + 1)], dtype=np.int64)
    d = _lib.Subspace()
    d.type, d.L, d.k, d.ld_nchoosek = TYPE["sc"], L, k, L + 1
    d.nchoosek = tab.ctypes.data_as(C.POINTER(C.c_int64))
    d._keep = tab
    return d


def descriptor(case, swz=0):
    if case.L == 64:
        assert case.kind == "sc" and swz == 0
        return raw_spin_conserve(case.L, case.k)
    sub = space(case.kind, case.L, case.k, case.space)
    d = _lib.Subspace.from_buffer_copy(sub._c())
    d.vec_swizzle = swz
    d._keep = sub
    assert d.type == TYPE[case.kind] and d.L == case.L and d.space == case.space and d.k == case.k
    return d


Plan = collections.namedtuple("Plan", "type nb B B_unlowered nwg nrows npanels per_wg busy ragged")


def plan_of(case):
    """What the sweep of a case is launched with.  The rule is the one written out in tests/test_gram_plan_host.py; where
    the ABI has a plan entry for the call (no XParity sector: the entries take none) its answer is asserted to be the
    rule's.  busy: the workgroups that have a panel (the others store zeros); ragged: the last panel is not full."""
    L, k = case.L, case.k
    if case.sweep == "pm":
        ncols = L
        if case.kind == "sc":
            nrows = comb(L, k + 1)
            table = (k + 2) * (L + 1) * 8 if nrows else 0
        else:
            nrows, table = 1 << (L - (case.kind == "parity")), 0
        nwg_of = lambda npanels: npanels
    else:
        ncols = len(case.items) + 1
        dim = comb(L, k) if case.kind == "sc" else 1 << (L - (case.kind == "parity"))
        table = (k + 1) * (L + 1) * 8 if case.kind == "sc" else 0
        nrows = dim // 2 if case.xsec else dim
        nwg_of = lambda npanels: (nrows + 511) >> 9
    rule = gram_rule(ncols, nrows, table, nwg_of)
    if not case.xsec:
        d = descriptor(case)
        n = ncols - 1
        got = {"pm": lambda: backend.pm_moments_plan(d), "swap": lambda: backend.swap_moments_plan(d, n),
               "cyc": lambda: backend.cyc_moments_plan(d, n), "pauli": lambda: backend.pauli_moments_plan(d, n)}[case.sweep]()
        assert got == rule, (case.name, got, rule)
    nb, B, nwg = rule[:3]
    npanels = (nrows + (1 << B) - 1) >> B
    per_wg = -(-npanels // nwg) if npanels else 0
    busy = -(-npanels // per_wg) if npanels else 0
    return Plan(TYPE[case.kind], nb, B, 9 if nb == 1 else 7, nwg, nrows, npanels, per_wg, busy,
                bool(nrows % (1 << B)))


# ---------------------------------------------------------------- one call between guards

def big_ints(n, seed):
    """ints(n, seed) without leaving tens of megabytes in its cache for the rest of the session"""
    re, im = ints(n, seed)
    if n > 1 << 18:
        test_gpu_vec._INTS.pop((n, seed), None)
    return re, im


def items_c(items, per):
    a = np.ascontiguousarray(items, dtype=np.int32).reshape(-1, per)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


PER = {"swap": 2, "cyc": 3, "pauli": 2}


def raw_call(sweep, desc, xsec, items, xptr, out):
    """the entry point of a sweep on ``out`` (complex128 host array: the matrix begins G elements in); the return code"""
    L = _lib.lib()
    op = out[G:].view(np.float64).ctypes.data_as(C.POINTER(C.c_double))
    if sweep == "pm":
        return L.dnm_pm_moments(xptr, C.byref(desc), op, None)
    a, ip = items_c(items, PER[sweep])
    if sweep == "swap":
        return L.dnm_swap_moments(xptr, C.byref(desc), xsec, a.shape[0], ip, op, None)
    if sweep == "cyc":
        return L.dnm_cyc_moments(xptr, C.byref(desc), xsec, a.shape[0], ip, op, None)
    return L.dnm_pauli_moments(xptr, C.byref(desc), a.shape[0], ip, op, None)


def run(case, x, swz=0):
    """The sweep of a case on the state x (index order; laid out by vec_pos here) between guards: the matrix.  Asserts
    what holds whatever the values: guards, no sentinel or NaN, Hermitian to the last bit, a real diagonal, the state
    untouched, a second call with the same bytes."""
    n = x.size
    assert n == gram_ref.state_size(ref_sub(case), case.xsec)
    lay = np.empty(n, dtype=np.complex128)
    lay[vec_pos(np.arange(n, dtype=np.int64), swz)] = x           # element i lies at position vec_pos(i)
    xb = Buf(lay, NAN)
    desc = descriptor(case, swz)
    D = case.L if case.sweep == "pm" else len(case.items) + 1
    outs = []
    for _ in range(2):
        out = np.full(D * D + 2 * G, SENT, dtype=np.complex128)
        rc = raw_call(case.sweep, desc, case.xsec, case.items, xb.ptr, out)
        assert rc == 0, _lib.lib().dnm_last_error().decode()
        guard = np.full(G, SENT, dtype=np.complex128)
        assert same_bits(out[:G], guard) and same_bits(out[G + D * D:], guard), "guard of out overwritten"
        outs.append(out[G:G + D * D].reshape(D, D))
    assert same_bits(xb.get(), lay), "the state was written"      # (get: its NaN guards hold their bits too)
    g = outs[0]
    what = "%s swizzle %d" % (case.name, swz)
    assert same_bits(g, outs[1]), what + ": a second call returns other bytes"
    assert not np.any(g.real == SENT.real) and not np.any(g.imag == SENT.imag), "sentinel left in " + what
    assert np.all(np.isfinite(g.view(np.float64))), "NaN or Inf in " + what
    assert np.array_equal(g, g.conj().T), what + " is not Hermitian to the last bit"
    assert np.all(g.diagonal().imag == 0.0), what + " has a complex diagonal"
    return g


def assert_equal_int(g, ref, what):
    rr, ri = ref
    assert g.shape == rr.shape == ri.shape, (what, g.shape, rr.shape)
    bad = (g.real != rr.astype(np.float64)) | (g.imag != ri.astype(np.float64))
    if np.any(bad):
        w = np.argwhere(bad)
        a, b = w[0]
        raise AssertionError("%s: %d of %d entries differ, the first at (%d, %d): got %r, reference (%d, %d)"
                             % (what, len(w), g.size, a, b, g[a, b], rr[a, b], ri[a, b]))


def check(case, xr, xi):
    ref = gram_ref.reference(case.sweep, ref_sub(case), case.xsec, case.items, xr, xi)
    x = cplx(xr, xi)
    for swz in case.swz:
        assert_equal_int(run(case, x, swz), ref, "%s swizzle %d" % (case.name, swz))
    return ref


# ---------------------------------------------------------------- exact cases

@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_exact(name):
    case = BY_NAME[name]
    n = gram_ref.state_size(ref_sub(case), case.xsec)
    xr, xi = big_ints(n, 90 + CASES.index(case) % 7)
    re, im = check(case, xr, xi)
    assert re[0, 0] > 0 or (case.sweep == "pm" and case.k == case.L)
    if re.shape[0] > 2 and n > 16:
        assert np.any(im != 0)                                    # (an imaginary part to get the sign of)


PLANTED = ["swap-SC(12,6)-w17", "swap-SC(12,6)-x--w48", "cyc-SC(12,6)-w16", "cyc-Parity(11,1)-w49", "pm-SC(12,6)",
           "pm-Full(10)", "pm-Parity(11,0)", "pauli-Parity(11,1)-w64", "swap-Full(10)-w17"]


@pytest.mark.parametrize("where", ["first", "last", "end_of_first_panel", "start_of_last_panel"])
@pytest.mark.parametrize("name", PLANTED)
def test_planted_amplitude(name, where):
    """A single non-zero amplitude 3 - 2i: at the first row, at the last, at the last row of the first panel and at the
    first row of the last (on SpinConserve ragged) panel of the vector.  G holds 13 where both columns fetch that
    amplitude on the same row, and exact zeros everywhere else."""
    case = BY_NAME[name]
    n = gram_ref.state_size(ref_sub(case), case.xsec)
    B = plan_of(case).B
    assert n > 1 << B
    at = {"first": 0, "last": n - 1, "end_of_first_panel": (1 << B) - 1, "start_of_last_panel": ((n - 1) >> B) << B}[where]
    xr, xi = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    xr[at], xi[at] = 3, -2
    re, im = check(case, xr, xi)
    # (sigma+ sigma- on Full never fetches the last amplitude: no site of the configuration of all ones is clear)
    assert np.any(re != 0) or (case.sweep == "pm" and case.kind == "full" and where == "last")
    assert set(np.unique(re)) <= {0, 13, -13} and not np.any(im)


# ---------------------------------------------------------------- refusals

def _explicit():
    rng = np.random.default_rng(11)
    states = np.sort(rng.choice(1 << 20, size=300, replace=False).astype(np.int64) | (np.int64(1) << 39))
    return Explicit(states, L=40)


def _desc_of(sub):
    d = _lib.Subspace.from_buffer_copy(sub._c())
    d.vec_swizzle = 0
    d._keep = sub
    return d


def _refusals():
    """(sweep, descriptor maker, xsec, items, a word of the message) -- each is decided by pm_check, swap_check, cyc_check
    or pauli_check before any device call"""
    full, par_odd, par_even = (lambda: _desc_of(Full(L=10)), lambda: _desc_of(Parity(0, L=11)),
                               lambda: _desc_of(Parity(1, L=12)))
    sc, sc_half = lambda: _desc_of(SpinConserve(12, 5)), lambda: _desc_of(SpinConserve(12, 6))
    good = {"swap": [(0, 1)], "cyc": [(0, 1, 2)], "pauli": [(0, 1)], "pm": None}

    def with_(make, **fields):
        def f():
            d = make()
            for key, v in fields.items():
                if key == "site_perm":
                    perm = np.arange(64, dtype=np.int8)
                    d._perm = perm
                    v = perm.ctypes.data_as(C.POINTER(C.c_int8))
                setattr(d, key, v)
            return d
        return f

    out = []
    for sweep in gram_ref.SWEEPS:
        out.append((sweep, lambda: _desc_of(_explicit()), 0, good[sweep], "Explicit"))
        for bad in (-1, 3, 4, 25):
            out.append((sweep, with_(full, vec_swizzle=bad), 0, good[sweep], "vec_swizzle"))
            out.append((sweep, with_(par_odd, vec_swizzle=bad), 0, good[sweep], "vec_swizzle"))
        out.append((sweep, with_(full, site_perm=True), 0, good[sweep], "site_perm"))
        out.append((sweep, with_(full, L=0), 0, good[sweep], "L=0"))
        out.append((sweep, with_(full, L=65), 0, good[sweep], "L=65"))
        out.append((sweep, with_(par_odd, space=2), 0, good[sweep], "parity space"))
        out.append((sweep, with_(full, type=7), 0, good[sweep], "type"))
    out.append(("pauli", sc, 0, good["pauli"], "SpinConserve"))
    for sweep in ("pm", "swap", "cyc"):
        out.append((sweep, with_(sc, site_perm=True), 0, good[sweep], "site_perm"))
        out.append((sweep, with_(sc, vec_swizzle=6 | (4 << 8)), 0, good[sweep], "reference order"))
        out.append((sweep, with_(sc, vec_swizzle=5), 0, good[sweep], "reference order"))
        out.append((sweep, with_(sc, k=13), 0, good[sweep], "k=13"))
    for sweep, mk in (("swap", bonds), ("cyc", triples), ("pauli", paulis)):
        out.append((sweep, full, 0, mk(10, 64), "64 "))
        out.append((sweep, full, 0, [], "0 "))
    for items, word in (([(0, 1), (3, 12)], "outside"), ([(-1, 2)], "outside"), ([(0, 1), (4, 4)], "itself")):
        for make in (full, par_odd, sc):
            out.append(("swap", make, 0, items, word))
    for items, word in (([(0, 1, 12)], "outside"), ([(0, -1, 2)], "outside"), ([(12, 1, 2)], "outside"),
                        ([(0, 1, 2), (4, 5, 4)], "distinct"), ([(3, 3, 5)], "distinct"), ([(3, 5, 5)], "distinct")):
        for make in (full, par_odd, sc):
            out.append(("cyc", make, 0, items, word))
    for items, word in (([(10, 1)], "outside"), ([(0, 3), (-1, 3)], "outside"), ([(0, 0)], "kind"), ([(0, 4)], "kind")):
        for make in (full, lambda: _desc_of(Parity(1, L=10))):
            out.append(("pauli", make, 0, items, word))
    for sweep in ("swap", "cyc"):
        out.append((sweep, par_odd, 1, good[sweep], "even"))
        out.append((sweep, par_odd, -1, good[sweep], "even"))
        out.append((sweep, sc, -1, good[sweep], "k = L / 2"))
        out.append((sweep, with_(sc_half, L=13, ld_nchoosek=14), 1, good[sweep], "k = L / 2"))
        out.append((sweep, full, 2, good[sweep], "xparity_sector"))
        out.append((sweep, par_even, -2, good[sweep], "xparity_sector"))
        out.append((sweep, with_(full, L=1), 1, [], "L=1"))
    return out


REFUSALS = _refusals()


@pytest.mark.parametrize("i", range(len(REFUSALS)), ids=["%s-%s-%d" % (r[0], r[4].strip().replace(" ", "_"), n)
                                                        for n, r in enumerate(REFUSALS)])
def test_refusal(i):
    """non-zero, a message with the word, and ``out`` as it was"""
    sweep, make, xsec, items, word = REFUSALS[i]
    desc = make()
    xb = Buf(np.ones(1 << 12, dtype=np.complex128), NAN)      # (a refusal never reads it)
    out = np.full(64 * 64 + 2 * G, SENT, dtype=np.complex128)
    if sweep != "pm" and len(items) == 0:
        # (an empty list still needs a pointer that is not null: null is another refusal)
        a = np.zeros(4, dtype=np.int32)
        L = _lib.lib()
        ip, op = a.ctypes.data_as(C.POINTER(C.c_int32)), out[G:].view(np.float64).ctypes.data_as(C.POINTER(C.c_double))
        rc = (L.dnm_pauli_moments(xb.ptr, C.byref(desc), 0, ip, op, None) if sweep == "pauli" else
              getattr(L, "dnm_%s_moments" % sweep)(xb.ptr, C.byref(desc), xsec, 0, ip, op, None))
    else:
        rc = raw_call(sweep, desc, xsec, items, xb.ptr, out)
    assert rc != 0
    msg = _lib.lib().dnm_last_error().decode()
    assert word in msg, msg
    assert same_bits(out, np.full(out.size, SENT, dtype=np.complex128)), "a refused call wrote to out"


# ---------------------------------------------------------------- rounding cases
# A component of an entry of G is a sum of 2 rows products of two parts of amplitudes (Re: ar br + ai bi; Im: ar bi -
# ai br, the kernel's Q[a][b] - Q[b][a] with rows products in each Q) over the rows of A; the factors +-1 of an XParity
# sector or of a Pauli column are exact.  A product is rounded once, or not at all on the matrix cores' fused chain, and
# then passes at most 2 rows - 1 additions on its way to the result, in whatever order the MFMA steps, the sum of the
# four wavefronts, the sum of the workgroups and the final difference add: at most 2 rows roundings on any path, so
#     |got - ref| <= gamma(2 rows) * sum |products|,    gamma(n) = n u / (1 - n u),  u = 2^-53,
# for any order of a sum of 2 rows products (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  The
# rows a panel pads with are zeros and add nothing.  Derived, not measured; no margin added.

ROUNDING = [
    ("sigma+ sigma-, Full", "pm-Full(10)", 0),
    ("sigma+ sigma-, SpinConserve", "pm-SC(12,6)", 0),
    ("swap, Full", "swap-Full(13)-w17", 6),
    ("swap, SpinConserve", "swap-SC(12,6)-w48", 0),
    ("swap, XParity", "swap-SC(12,6)-x--w17", 0),
    ("rotation, SpinConserve", "cyc-SC(12,6)-w49", 0),
    ("Pauli, Parity", "pauli-Parity(11,1)-w64", 0),
]


@pytest.mark.parametrize("what,name,swz", ROUNDING, ids=[r[0].replace(" ", "_") for r in ROUNDING])
def test_rounding(what, name, swz):
    case = BY_NAME[name]
    sub = ref_sub(case)
    n = gram_ref.state_size(sub, case.xsec)
    rs = np.random.RandomState(4242 + len(name))
    x = rs.standard_normal(n) + 1j * rs.standard_normal(n)
    g = run(case, x, swz)
    Ar, Ai = gram_ref.operand(case.sweep, sub, case.xsec, case.items, x.real.astype(LD), x.imag.astype(LD))
    rows = Ar.shape[0]
    ref_r, q = Ar.T @ Ar + Ai.T @ Ai, Ar.T @ Ai
    ref_i = q - q.T
    aR, aI = np.abs(Ar), np.abs(Ai)
    mag_r, mq = aR.T @ aR + aI.T @ aI, aR.T @ aI
    mag_i = mq + mq.T
    mask = gram_ref.sector_mask(case.sweep, sub, case.items)
    if mask is not None:                                         # (written as zeros: the bound there is 0)
        for m in (ref_r, ref_i, mag_r, mag_i):
            m[mask] = 0
    er, ei = np.abs(g.real.astype(LD) - ref_r), np.abs(g.imag.astype(LD) - ref_i)
    live_r, live_i = mag_r > 0, mag_i > 0
    worst = max(float(np.max(er[live_r] / mag_r[live_r])), float(np.max(ei[live_i] / mag_i[live_i])))
    print("%s: %d rows, max |got - ref| / sum|products| = %.3g = %.2f u, bound gamma(%d) = %.3g = %.0f u"
          % (what, rows, worst, worst / 2.0 ** -53, 2 * rows, gamma(2 * rows), gamma(2 * rows) / 2.0 ** -53))
    assert np.all(er <= gamma(2 * rows) * mag_r) and np.all(ei <= gamma(2 * rows) * mag_i), what
