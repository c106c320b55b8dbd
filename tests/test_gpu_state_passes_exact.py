"""
The three passes that turn a state into another state -- site permutations (csrc/perm_kernels.hip), subspace maps and
sector weights (csrc/submap_kernels.hip), products of single-site operators (csrc/site_ops_kernels.hip) -- through the C
ABI, one call at a time: dnm_perm_apply, dnm_perm_dots, dnm_subspace_map_apply, dnm_sector_weights and
dnm_site_ops_apply on device buffers of the test's own, with descriptors filled in here (by hand for Explicit lists and
for L = 64).  Nothing goes through State or backend.Vec.

Exact cases: real and imaginary parts of every amplitude are independent non-zero integers in [-8, 8]
(tests/test_gpu_vec.py::ints), coefficients of perm_apply Gaussian integers of modulus <= 4, site matrices have entries
from {0, +-1, +-i, +-1+-i}.  Every intermediate is then an integer far below 2^53 (tests/state_pass_ref.py asserts it
case by case), so any order of summation gives the same value and the tests assert EQUALITY with the integer reference:
of bits for the permutations, the maps and the weights (a copy moves bits; kappa * integer is rounded once on both
sides with the same constant), of values for the site products (0 * -1 is -0.0 on the device).

Buffers: every device vector lies between 64 NaN amplitudes (inputs) or 64 sentinels (outputs) on each side; every host
output is pre-filled with a sentinel between 64 sentinels.  After every call: the values equal the reference, no
sentinel or NaN is left, the guards are intact, the inputs with their guards are bit-identical to their upload, and a
second call returns the same bytes.

PERM_CASES, MAP_CASES, WEIGHT_CASES and SITE_CASES are the tables of the exact cases; tests/test_state_pass_ref.py (no
GPU) computes the plan of each and proves which kernel instances and regimes the tables reach.

Rounding cases (one per kernel family, normal deviates) against numpy.longdouble; each bound is derived beside its case.
"""
import collections
import ctypes as C
import functools
import os

import numpy as np
import pytest

from dynamite_amd import _lib
from dynamite_amd.subspaces import Full, Parity, SpinConserve
import site_ops_ref
import state_pass_ref as ref
from test_gpu_gram_exact import big_ints, raw_spin_conserve
from test_gpu_site_permutations import perm_set
from test_gpu_vec import Buf, G, NAN, SENT, cplx, gamma, ints, same_bits, vec_pos

pytestmark = pytest.mark.gpu

LD = np.longdouble
FULL, PARITY, EXPLICIT, SC = 0, 1, 2, 3            # dnm_subspace.type (include/dynamite_amd.h)
KIND_TYPE = {"full": FULL, "parity": PARITY, "ex": EXPLICIT, "sc": SC}
f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
assert vec_pos(0x155, 6) == int(ref.vec_pos(0x155, 6))     # (the two statements of the layout agree)


# ---------------------------------------------------------------- subspaces: specs, lists, references, descriptors
# A spec is ("full", L), ("parity", L, space), ("sc", L, k) or ("ex", name of a list); a side is (spec, sector,
# swizzle).

def _flip_closed(L, nreps, seed):
    """representatives (spin L - 1 up) in the first half of the list, their complements, shuffled, in the second"""
    rng = np.random.default_rng(seed)
    reps = set()
    while len(reps) < nreps:
        reps.add(int(rng.integers(0, 1 << min(L - 1, 62))) & ((1 << (L - 1)) - 1))
    reps = [sorted(reps)[i] for i in rng.permutation(nreps)]
    return reps + [reps[i] ^ ((1 << L) - 1) for i in rng.permutation(nreps)]


def _random_states(L, n, seed, sort):
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < n:
        out.add(int(rng.integers(0, 1 << min(L, 62))) | (int(rng.integers(0, 2)) << (L - 1)))
    out = sorted(out)
    return out if sort else [out[i] for i in rng.permutation(n)]


@functools.lru_cache(maxsize=None)
def explicit_list(name):
    """(L, the list) of a named Explicit subspace"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "e14flip":
        return 14, _flip_closed(14, 1100, 15)
    if name == "e14par":                 # the states of Parity(14, even) in index order: a flip-closed list
        return 14, [int(c) for c in ref.Sub("parity", 14, space=0).configs()]
    if name == "e14":
        return 14, _random_states(14, 3000, 16, sort=True)
    if name == "e13sorted":
        return 13, _random_states(13, 1000, 14, sort=True)
    if name == "e13unsorted":
        return 13, _random_states(13, 1000, 14, sort=False)
    if name == "e13wide":                # two listed states of more than L bits: in no subspace of 13 spins
        lst = _random_states(13, 1000, 14, sort=False)
        lst[17], lst[500] = (1 << 13) | 5, (1 << 20) | (1 << 13) | lst[500]
        return 13, lst
    if name in ("e50sub", "e50super"):
        sc = [int(c) for c in ref.Sub("sc", 50, 2).configs()]
        if name == "e50sub":
            return 50, [sc[i] for i in rng.permutation(len(sc))[:600]]
        others = [s for s in _random_states(50, 300, 51, sort=True) if bin(s).count("1") != 2]
        lst = sc + others
        return 50, [lst[i] for i in rng.permutation(len(lst))]
    if name == "e63":                    # 40 of the 63 states of SpinConserve(63, 1), sites 0 and 62 among them
        one = [1 << j for j in [0, 62, 61] + list(range(3, 40))]
        lst = one + [s for s in _random_states(63, 200, 63, sort=True) if bin(s).count("1") != 1]
        return 63, [lst[i] for i in rng.permutation(len(lst))]
    if name == "e63flip":
        return 63, _flip_closed(63, 500, 64)
    if name == "e40":
        return 40, _random_states(40, 3000, 40, sort=True)
    if name == "e40flip":
        return 40, _flip_closed(40, 400, 41)
    raise KeyError(name)


def spec_L(spec):
    return explicit_list(spec[1])[0] if spec[0] == "ex" else spec[1]


def spec_name(spec):
    if spec[0] == "ex":
        return spec[1]
    return {"full": "Full(%d)", "parity": "Parity(%d,%d)", "sc": "SC(%d,%d)"}[spec[0]] % spec[1:]


def side_name(side):
    spec, sec, swz = side
    return spec_name(spec) + {0: "", 1: "+", -1: "-"}[sec] + ("s%d" % swz if swz else "")


@functools.lru_cache(maxsize=None)
def ref_sub(spec):
    if spec[0] == "ex":
        L, lst = explicit_list(spec[1])
        return ref.Sub("explicit", L, states=lst)
    if spec[0] == "parity":
        return ref.Sub("parity", spec[1], space=spec[2])
    if spec[0] == "sc":
        return ref.Sub("sc", spec[1], k=spec[2])
    return ref.Sub("full", spec[1])


def ref_side(side):
    return (ref_sub(side[0]), side[1], side[2])


def raw_explicit(L, states):
    """An Explicit descriptor filled in by hand: the list, its sorted copy, and the list indices of the sorted states
    where the list is not sorted itself."""
    sm = np.array(states, dtype=np.uint64).view(np.int64)
    order = np.argsort(sm, kind="stable").astype(np.int64)
    rs = np.ascontiguousarray(sm[order])
    d = _lib.Subspace()
    d.type, d.L, d.dim = EXPLICIT, L, sm.size
    d.state_map, d.rmap_states = _lib.p64(sm), _lib.p64(rs)
    d._keep = [sm, rs]
    if not np.array_equal(order, np.arange(sm.size)):
        d.rmap_indices = _lib.p64(order)
        d._keep.append(order)
    return d


@functools.lru_cache(maxsize=None)
def _space(spec):
    """The subspace objects (kept alive: a descriptor points into the tables of its object)."""
    return Full(L=spec[1]) if spec[0] == "full" else Parity(spec[2], L=spec[1]) if spec[0] == "parity" else \
        SpinConserve(spec[1], spec[2])


def descriptor(spec, swz=0):
    if spec[0] == "ex":
        d = raw_explicit(*explicit_list(spec[1]))
    elif spec[0] == "sc" and spec[1] == 64:
        d = raw_spin_conserve(spec[1], spec[2])         # (the Python class stops at 63 spins)
    else:
        sub = _space(spec)
        d = _lib.Subspace.from_buffer_copy(sub._c())
        d._keep = sub
    d.vec_swizzle = swz
    assert d.type == KIND_TYPE[spec[0]] and d.L == spec_L(spec)
    return d


def lib():
    return _lib.lib()


def err():
    return lib().dnm_last_error().decode()


def data(n, seed):
    """n amplitudes with independent non-zero integer parts in [-8, 8]: ((re, im) int64, complex128)"""
    re, im = big_ints(n, seed)
    return (re, im), cplx(re, im)


def clean(got, what):
    assert not np.any(got.view(np.float64) == SENT.real) and not np.any(got.view(np.float64) == SENT.imag), \
        "sentinel left in " + what
    assert np.all(np.isfinite(got.view(np.float64))), "NaN or Inf in " + what


def assert_bits(got, want, what):
    if not same_bits(got, want):
        bad = np.flatnonzero((got.view(np.uint64).reshape(-1, 2) != want.view(np.uint64).reshape(-1, 2)).any(axis=1))
        raise AssertionError("%s: %d of %d rows differ, the first at %d: got %r, reference %r"
                             % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))


def host_out(n):
    """n doubles pre-filled with a sentinel between 64 sentinels: (array, pointer to the payload)"""
    a = np.full(n + 2 * G, SENT.real, dtype=np.float64)
    return a, a[G:].ctypes.data_as(f64p)


def host_payload(a, n, what):
    guard = np.full(G, SENT.real)
    assert same_bits(a[:G], guard) and same_bits(a[G + n:], guard), "guard of %s overwritten" % what
    got = a[G:G + n]
    assert not np.any(got == SENT.real), "sentinel left in " + what
    assert np.all(np.isfinite(got)), "NaN or Inf in " + what
    return got.copy()


# ================================================================ site permutations

def permutations(L, n):
    """n site permutations of L sites: the set of tests/test_gpu_site_permutations.py::perm_set (identity, a
    transposition with site L - 1, the reversal, the shifts by 1 and L - 1, a three-cycle through L - 1, two random
    ones), a transposition of the sites 0 and L - 2, one whose inverse differs from it at every site; then seeded random
    ones, and a repeat at the end."""
    rng = np.random.default_rng(300 + L)
    ident = np.arange(L)
    if L < 4:
        base = [ident, ident[::-1], (ident + 1) % L]
    else:
        swap = ident.copy()
        swap[[0, L - 2]] = [L - 2, 0]
        while True:
            far = rng.permutation(L)
            if np.all(far != np.argsort(far)):
                break
        base = list(perm_set(L)) + [swap, far]
    out = [np.asarray(p) for p in base]
    while len(out) < n:
        out.append(rng.permutation(L))
    out = out[:n]
    if n > len(base):
        out[-1] = out[1]
    return np.ascontiguousarray(out, dtype=np.int32)


MODULUS_4 = [(a, b) for a in range(-4, 5) for b in range(-4, 5) if 0 < a * a + b * b <= 16]


def coefficients(n, seed):
    """n Gaussian integers of modulus <= 4; the first has a real and an imaginary part, so that a case of one
    permutation sees both"""
    rng = np.random.default_rng(400 + seed)
    out = [MODULUS_4[i] for i in rng.integers(0, len(MODULUS_4), n)]
    both = [c for c in MODULUS_4 if c[0] and c[1]]
    out[0] = both[int(rng.integers(0, len(both)))]
    return out


PermCase = collections.namedtuple("PermCase", "name spec xsec swz nperm only")
PERM_CASES = []
NPERMS = (1, 2, 3, 5, 8, 9, 17, 33, 64)            # gp_log2 0 to 6, with idle lanes in a group


def perm_add(spec, xsec=0, swz=(0,), nperm=1, only=None):
    name = "%s%s-n%d%s" % (spec_name(spec), {0: "", 1: "+", -1: "-"}[xsec], nperm, "-" + only if only else "")
    assert name not in [c.name for c in PERM_CASES], name
    PERM_CASES.append(PermCase(name, spec, xsec, tuple(swz), nperm, only))


for _n in NPERMS:
    _swz = (0, 5, 6) if _n in (1, 5) else (0,)
    for _spec in (("full", 10), ("parity", 11, 0), ("parity", 11, 1), ("parity", 12, 0)):
        perm_add(_spec, swz=_swz, nperm=_n)
    perm_add(("sc", 12, 6), nperm=_n)
    perm_add(("sc", 13, 4), nperm=_n)                              # 715 rows = 3 mod PERM_RUN
    for _x in (1, -1):
        perm_add(("full", 10), _x, swz=_swz, nperm=_n)
        perm_add(("parity", 12, 0), _x, swz=_swz, nperm=_n)
        perm_add(("sc", 12, 6), _x, nperm=_n)                      # 462 rows = 2 mod PERM_RUN
        perm_add(("sc", 16, 8), _x, nperm=_n)                      # 6435 rows = 3 mod PERM_RUN, 7 workgroups
for _n in (1, 3):
    perm_add(("full", 20), swz=(16,), nperm=_n)                    # the production shift
    perm_add(("sc", 12, 0), nperm=_n)                              # dimension 1
    perm_add(("sc", 12, 12), nperm=_n)
for _n in (1, 5):
    perm_add(("sc", 15, 4), nperm=_n)                              # 1365 rows = 1 mod PERM_RUN, a second workgroup
    perm_add(("sc", 14, 5), nperm=_n)                              # 2002 rows = 2 mod PERM_RUN
    perm_add(("sc", 18, 2), nperm=_n)                              # 153 rows = 1 mod PERM_RUN
    perm_add(("sc", 3, 1), nperm=_n)                               # fewer rows than one run
    perm_add(("sc", 2, 1), nperm=_n)
for _n in (1, 2):
    for _x in (1, -1):
        perm_add(("full", 2), _x, nperm=_n)                        # dimension 2 under XParity
        perm_add(("parity", 2, 0), _x, nperm=_n)                   # ... and 1
        perm_add(("sc", 2, 1), _x, nperm=_n)
for _n in (1, 9):                                                  # wide: bits 33 to 63 of a configuration
    for _spec in (("sc", 34, 2), ("sc", 50, 2), ("sc", 63, 2), ("sc", 64, 1), ("sc", 64, 2)):
        perm_add(_spec, nperm=_n)
perm_add(("full", 23), nperm=1, only="apply")                      # 2^23 rows: every thread strides the grid twice
perm_add(("full", 23), nperm=1, only="dots")
PERM_BY_NAME = {c.name: c for c in PERM_CASES}


def perm_side(case, swz=0):
    return (case.spec, case.xsec, swz)


def call_perm_apply(desc, xsec, perms, coef, x, y0):
    """dnm_perm_apply between guards, twice: the result.  y0: what y holds before (accumulate), or None."""
    n = x.size
    cf = np.array(coef, dtype=np.float64).reshape(-1)
    xb = Buf(x, NAN)
    outs = []
    for _ in range(2):
        yb = Buf(np.full(n, SENT) if y0 is None else y0)
        rc = lib().dnm_perm_apply(xb.ptr, yb.ptr, C.byref(desc), xsec, perms.shape[0], perms.ctypes.data_as(i32p),
                                  cf.ctypes.data_as(f64p), int(y0 is not None), None)
        assert rc == 0, err()
        outs.append(yb.get())                                      # (asserts the guards)
    assert same_bits(xb.get(), x), "the state was written"
    assert same_bits(outs[0], outs[1]), "a second call returns other bytes"
    clean(outs[0], "perm_apply")
    return outs[0]


def call_perm_dots(desc, xsec, perms, phi, psi):
    n = perms.shape[0]
    fb, pb = Buf(phi, NAN), Buf(psi, NAN)
    outs = []
    for _ in range(2):
        out, op = host_out(2 * n)
        rc = lib().dnm_perm_dots(fb.ptr, pb.ptr, C.byref(desc), xsec, n, perms.ctypes.data_as(i32p), op, None)
        assert rc == 0, err()
        outs.append(host_payload(out, 2 * n, "perm_dots"))
    assert same_bits(fb.get(), phi) and same_bits(pb.get(), psi), "a state was written"
    assert same_bits(outs[0], outs[1]), "a second call returns other bytes"
    return outs[0].reshape(n, 2)


@pytest.mark.parametrize("name", [c.name for c in PERM_CASES])
def test_perm_exact(name):
    """perm_apply without and with accumulate (y pre-filled with integers), the plain permutation at n = 1 (the bits
    of x), and perm_dots, in every layout of the case"""
    case = PERM_BY_NAME[name]
    L, seed = spec_L(case.spec), PERM_CASES.index(case) % 5
    perms = permutations(L, case.nperm)
    coef = coefficients(case.nperm, seed)
    for swz in case.swz:
        side = ref_side(perm_side(case, swz))
        n = ref.rows_of(side)
        desc = descriptor(case.spec, swz)
        (xr, xi), x = data(n, 20 + seed)
        if case.only != "apply":
            (yr, yi), y0 = data(n, 30 + seed)
        what = "%s swizzle %d" % (name, swz)
        if case.only != "dots":
            want = ref.perm_apply((xr, xi), side, perms, coef)
            assert_bits(call_perm_apply(desc, case.xsec, perms, coef, x, None), cplx(*want), what + " apply")
            if n > 4:
                assert np.any(want[0] != xr) or case.nperm == 1
        if case.only is None:
            want = ref.perm_apply((xr, xi), side, perms, coef, y=(yr, yi))
            assert_bits(call_perm_apply(desc, case.xsec, perms, coef, x, y0), cplx(*want), what + " accumulate")
            if case.nperm == 1:
                for p in permutations(L, 9):
                    one = np.ascontiguousarray(p.reshape(1, L))
                    want = ref.perm_apply((xr, xi), side, one, [(1, 0)])
                    assert_bits(call_perm_apply(desc, case.xsec, one, [(1, 0)], x, None), cplx(*want), what + " plain")
        if case.only != "apply":
            want = np.array(ref.perm_dots((yr, yi), (xr, xi), side, perms), dtype=np.float64)
            got = call_perm_dots(desc, case.xsec, perms, y0, x)
            assert same_bits(got, want), (what, got[:4], want[:4])
            assert np.any(want[:, 1] != 0) or n < 3


# ================================================================ subspace maps

MapCase = collections.namedtuple("MapCase", "name src dst zero")
MAP_CASES = []
SECTOR_PAIRS = [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)]


def map_add(src, dst, zero=False, note=""):
    src, dst = tuple(src) + (0,) * (3 - len(src)), tuple(dst) + (0,) * (3 - len(dst))
    name = "%s>%s%s" % (side_name(src), side_name(dst), "-" + note if note else "")
    assert name not in [c.name for c in MAP_CASES], name
    MAP_CASES.append(MapCase(name, src, dst, zero))


T14 = [("full", 14), ("parity", 14, 1), ("sc", 14, 7), ("ex", "e14flip")]         # each carries the flip
# all 16 (source, target) instances in every mode: plain -> plain, both sectors -> plain, plain -> both sectors,
# sector -> sector equal and opposite (zeros)
for _s in T14:
    for _d in T14:
        for _ss, _ds in SECTOR_PAIRS:
            map_add((_s, _ss), (_d, _ds), zero=_ss * _ds == -1)
# independent swizzles on the two sides, Full -> Full (a pure change of swizzle) among them
for _s in T14[:2]:
    for _d in T14[:2]:
        for _a in (0, 5, 6):
            for _b in (0, 5, 6):
                if _a or _b:
                    map_add((_s, 0, _a), (_d, 0, _b))
                    map_add((_s, 1, _a), (_d, 0, _b))
                    map_add((_s, 0, _a), (_d, -1, _b))
# L = 13: subspaces that do not carry the flip, lists sorted, unsorted and with states of more than L bits
for _e in ("e13sorted", "e13unsorted", "e13wide"):
    for _o in (("full", 13), ("parity", 13, 1), ("parity", 13, 0), ("sc", 13, 6), ("sc", 13, 4)):
        map_add((("ex", _e),), (_o,))
        map_add((_o,), (("ex", _e),))
    for _x in (1, -1):
        map_add((("ex", _e),), (("full", 13), _x, 5))
        map_add((("full", 13), _x, 6), (("ex", _e),))
map_add((("ex", "e13sorted"),), (("ex", "e13unsorted"),))
map_add((("ex", "e13wide"),), (("ex", "e13sorted"),))
map_add((("ex", "e13unsorted"),), (("ex", "e13wide"),))
map_add((("ex", "e14flip"),), (("ex", "e14par"),))
map_add((("ex", "e14"),), (("sc", 14, 7),))
map_add((("sc", 14, 7), 1), (("ex", "e14"),))
map_add((("ex", "e14par"), 1), (("ex", "e14flip"), 1))
map_add((("sc", 13, 4),), (("sc", 13, 6),), zero=True)                            # disjoint sectors
map_add((("parity", 13, 0),), (("parity", 13, 1),), zero=True)
map_add((("parity", 13, 1), 0, 5), (("parity", 13, 1), 0, 6))
# SpinConserve targets with rows = 1, 2, 3 mod SUBMAP_RUN (and back)
for _spec, _x in ((("sc", 15, 4), 0), (("sc", 18, 2), 0), (("sc", 14, 5), 0), (("sc", 13, 4), 0), (("sc", 12, 6), 1),
                  (("sc", 16, 8), -1), (("sc", 3, 1), 0)):
    _f = ("full", _spec[1])
    map_add((_f, 0, 5 if _spec[1] > 5 else 0), (_spec, _x), note="ragged")
    map_add((_spec, _x), (_f,), note="ragged")
# wide subspaces
map_add((("sc", 50, 2),), (("ex", "e50sub"),))
map_add((("ex", "e50sub"),), (("sc", 50, 2),))
map_add((("sc", 50, 2),), (("ex", "e50super"),))
map_add((("ex", "e50super"),), (("sc", 50, 2),))
map_add((("sc", 63, 1),), (("ex", "e63"),))
map_add((("ex", "e63"),), (("sc", 63, 1),))
map_add((("sc", 63, 1),), (("sc", 63, 1),))
map_add((("sc", 63, 1),), (("sc", 63, 62),), zero=True)
for _x in (1, -1):
    map_add((("ex", "e63flip"),), (("ex", "e63flip"), _x))
    map_add((("ex", "e63flip"), _x), (("ex", "e63flip"),))
    map_add((("ex", "e63flip"), _x), (("ex", "e63flip"), _x))
    map_add((("ex", "e63flip"), _x), (("ex", "e63flip"), -_x), zero=True)
    map_add((("ex", "e63flip"), _x), (("ex", "e63"),), zero=True)                # (no state in common)
# 2^23 target rows: every thread strides the grid twice
map_add((("parity", 23, 1),), (("full", 23),), note="stride")
MAP_BY_NAME = {c.name: c for c in MAP_CASES}


def call_map(src, dst, x):
    """dnm_subspace_map_apply between guards, twice: the target vector as it lies"""
    sd, dd = descriptor(src[0], src[2]), descriptor(dst[0], dst[2])
    n = ref.rows_of(ref_side(dst))
    xb = Buf(x, NAN)
    outs = []
    for _ in range(2):
        yb = Buf(np.full(n, SENT))
        rc = lib().dnm_subspace_map_apply(xb.ptr, C.byref(sd), src[1], yb.ptr, C.byref(dd), dst[1], None)
        assert rc == 0, err()
        outs.append(yb.get())
    assert same_bits(xb.get(), x), "the state was written"
    assert same_bits(outs[0], outs[1]), "a second call returns other bytes"
    clean(outs[0], "the map")
    return outs[0]


@pytest.mark.parametrize("name", [c.name for c in MAP_CASES])
def test_map_exact(name):
    case = MAP_BY_NAME[name]
    src, dst = ref_side(case.src), ref_side(case.dst)
    _, x = data(ref.rows_of(src), 40 + MAP_CASES.index(case) % 5)
    want = ref.map_apply(x, src, dst)
    got = call_map(case.src, case.dst, x)
    assert_bits(got, want, name)
    assert bool(np.any(want)) != case.zero, "the case is not what it claims"


def test_closed_form_complement_is_the_looked_up_one():
    """plain -> sector takes the complement's amplitude from row dim - 1 - i on Parity(14, even) and from a search on
    the same states as an Explicit list: the same data gives the same bytes, from and to either"""
    par, lst = (("parity", 14, 0), 0, 0), (("ex", "e14par"), 0, 0)
    _, x = data(1 << 13, 46)
    for sec in (1, -1):
        outs = [call_map(s, (d[0], sec, 0), x) for s in (par, lst) for d in (par, lst)]
        want = ref.map_apply(x, ref_side(par), ref_side((par[0], sec, 0)))
        for got in outs:
            assert_bits(got, want, "sector %d" % sec)
        assert np.count_nonzero(want) > 4000


PLANTED_MAPS = ["SC(14,7)>Full(14)", "Full(14)>SC(14,7)", "Full(14)+>Parity(14,1)", "Parity(14,1)>Full(14)-",
                "e14>SC(14,7)", "Full(14)s5>Full(14)s6", "SC(14,7)->e14flip-", "Parity(14,1)>e14flip"]


@pytest.mark.parametrize("where", ["first", "last", "1023", "1024"])
@pytest.mark.parametrize("name", PLANTED_MAPS)
def test_map_planted_amplitude(name, where):
    """A single amplitude 3 - 2i at the first row of the source, the last, row 1023 and row 1024: the result holds it
    (times +-kappa in the kappa modes) where the reference says, and exact zeros everywhere else."""
    case = MAP_BY_NAME[name]
    src, dst = ref_side(case.src), ref_side(case.dst)
    n = ref.rows_of(src)
    assert n > 1025
    x = np.zeros(n, dtype=np.complex128)
    x[{"first": 0, "last": n - 1, "1023": 1023, "1024": 1024}[where]] = 3 - 2j
    want = ref.map_apply(x, src, dst)
    got = call_map(case.src, case.dst, x)
    assert_bits(got, want, name + " " + where)
    assert np.count_nonzero(got) <= 2
    scale = 1.0 if ref.map_mode(src, dst) == ref.COPY else ref.KAPPA
    assert set(np.unique(np.abs(got.real))) <= {0.0, 3 * scale} and set(np.unique(np.abs(got.imag))) <= {0.0, 2 * scale}


def test_a_copy_moves_every_bit():
    """plain -> plain and sector -> sector compute nothing: signed zeros, subnormals and NaN payloads arrive as they
    are (the output buffer is checked for its guards, not for NaN)"""
    bits = np.random.default_rng(3).integers(0, 1 << 63, size=2 * 3432, dtype=np.int64)
    bits[:4] = [np.int64(-1 << 63), 1, 0x7ff8000000000123, np.int64(-1 << 63) | 5]
    x = bits.view(np.complex128)
    for src, dst in (((("sc", 14, 7), 0, 0), (("full", 14), 0, 6)), ((("sc", 14, 7), 0, 0), (("sc", 14, 7), 0, 0))):
        want = ref.map_apply(x, ref_side(src), ref_side(dst))
        sd, dd = descriptor(src[0], src[2]), descriptor(dst[0], dst[2])
        xb, yb = Buf(x, NAN), Buf(np.full(want.size, SENT))
        assert lib().dnm_subspace_map_apply(xb.ptr, C.byref(sd), 0, yb.ptr, C.byref(dd), 0, None) == 0, err()
        assert same_bits(yb.get(), want) and same_bits(xb.get(), x)


# ================================================================ sector weights

WeightCase = collections.namedtuple("WeightCase", "name side")
WEIGHT_CASES = []


def weight_add(spec, sector=0, swz=0):
    side = (spec, sector, swz)
    WEIGHT_CASES.append(WeightCase(side_name(side), side))


# small L: the four instances in each branch they have (pairs, sector, plain)
weight_add(("full", 12))
weight_add(("full", 12), swz=5)
weight_add(("full", 13), 1)
weight_add(("full", 13), -1, 6)
weight_add(("parity", 12, 0), swz=6)
weight_add(("parity", 14, 1))
weight_add(("parity", 14, 1), 1)
weight_add(("parity", 14, 0), -1, 5)
weight_add(("parity", 13, 1))
weight_add(("parity", 13, 0), swz=6)
weight_add(("sc", 12, 6))
weight_add(("sc", 14, 7))
weight_add(("sc", 14, 7), 1)
weight_add(("sc", 14, 7), -1)
weight_add(("sc", 13, 4))
weight_add(("sc", 14, 5))
weight_add(("ex", "e14"))
weight_add(("ex", "e13wide"))
weight_add(("ex", "e14flip"))
weight_add(("ex", "e14flip"), 1)
weight_add(("ex", "e14par"), -1)
# large L: (L + 3) * 2048 bytes of dynamic LDS, above 64 KB from L = 30
weight_add(("sc", 34, 2))
weight_add(("sc", 50, 2))
weight_add(("sc", 63, 1))
weight_add(("sc", 63, 62))
weight_add(("ex", "e40"))
weight_add(("ex", "e40flip"), 1)
weight_add(("ex", "e63"))
weight_add(("ex", "e63flip"))
weight_add(("ex", "e63flip"), 1)
weight_add(("ex", "e63flip"), -1)
# the stride: 2^22 pairs and 2^22 rows, twice the 2048 * 1024 a launch covers without striding
weight_add(("full", 23))
weight_add(("parity", 23, 1))
WEIGHT_BY_NAME = {c.name: c for c in WEIGHT_CASES}


def call_weights(side, x, flip):
    """dnm_sector_weights on host outputs between sentinels, twice: (mag, flip or None)"""
    L = spec_L(side[0])
    desc = descriptor(side[0], side[2])
    xb = Buf(x, NAN)
    outs = []
    for _ in range(2):
        mag, mp = host_out(L + 1)
        fl, fp = host_out(2)
        rc = lib().dnm_sector_weights(xb.ptr, C.byref(desc), side[1], mp, fp if flip else None, None)
        assert rc == 0, err()
        if not flip:
            assert same_bits(fl, np.full(fl.size, SENT.real)), "flip_out written though null was passed"
        outs.append((host_payload(mag, L + 1, "the bins"), host_payload(fl, 2, "the flip sums") if flip else None))
    assert same_bits(xb.get(), x), "the state was written"
    assert same_bits(outs[0][0], outs[1][0]), "a second call returns other bins"
    assert not flip or same_bits(outs[0][1], outs[1][1]), "a second call returns other flip sums"
    return outs[0]


def check_weights(side, xr, xi, what):
    rside = ref_side(side)
    mag2, flip2 = ref.sector_weights((xr, xi), rside)
    norm2 = 2 * int(np.sum(xr * xr + xi * xi))
    assert sum(mag2) == norm2 and (flip2 is None or sum(flip2) == norm2)
    x = cplx(xr, xi)
    for flip in ((False, True) if flip2 is not None else (False,)):
        mag, fl = call_weights(side, x, flip)
        assert same_bits(mag * 2, np.array(mag2, dtype=np.float64)), (what, mag, mag2)
        assert 2 * mag.sum() == norm2
        if flip:
            assert same_bits(fl * 2, np.array(flip2, dtype=np.float64)), (what, fl, flip2)
            assert 2 * fl.sum() == norm2
    return flip2


@pytest.mark.parametrize("name", [c.name for c in WEIGHT_CASES])
def test_weights_exact(name):
    side = WEIGHT_BY_NAME[name].side
    n = ref.rows_of(ref_side(side))
    (xr, xi), _ = data(n, 50 + WEIGHT_CASES.index(WEIGHT_BY_NAME[name]) % 5)
    flip2 = check_weights(side, xr, xi, name)
    assert (flip2 is not None) == (ref.weights_branch(ref_side(side)) != "plain")
    if ref.weights_branch(ref_side(side)) == "pairs" and n > 64:
        assert flip2[0] != flip2[1]


PLANTED_WEIGHTS = [c.name for c in WEIGHT_CASES if spec_L(c.side[0]) < 23 and ref_sub(c.side[0]).dim > 2100]


@pytest.mark.parametrize("name", PLANTED_WEIGHTS)
def test_weights_planted_rows(name):
    """Zeros but for a few rows: both ends, the rows around each multiple of 1024 a workgroup starts at, and n - 1,
    n / 2 - 1, n / 2 -- the two ends of the descending second stream of the pairs branch."""
    side = WEIGHT_BY_NAME[name].side
    n = ref.rows_of(ref_side(side))
    rows = sorted({r for r in (0, 1, 1023, 1024, 2047, 2048, n - 1025, n - 1024, n - 2, n - 1, n // 2 - 1, n // 2)
                   if 0 <= r < n})
    pr, pi = ints(len(rows), 9)
    xr, xi = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    xr[rows], xi[rows] = pr, pi
    check_weights(side, xr, xi, name)


# ================================================================ products of site operators

SiteCase = collections.namedtuple("SiteCase", "name L classes seed single")
SITE_CASES = []


def site_cases(tb):
    """The cases under a tile of tb index bits: the sizes of test_gpu_site_ops.py::test_product_exact (all sites
    general, and random mixes of identity, diagonal and general), every site alone with a non-symmetric matrix, a
    diagonal site outside the tile, an all-diagonal product.  The names say ``tb`` where the size follows the tile."""
    out = []
    for L, nm in [(v, "L%d" % v) for v in (1, 2, 3, 4, 5, 8, 12)] + [(tb, "tb"), (tb + 1, "tb+1")]:
        out.append(SiteCase("general-" + nm, L, (2,) * L, 10 * L, None))
        for seed in (1, 2):
            out.append(SiteCase("mixed%d-%s" % (seed, nm), L, None, 10 * L + seed, None))
    L3 = 4 + 2 * (tb - 4) + 1
    # three passes: tb - 4 general sites above bit 3 fill a pass (the four low sites stay out of it: identity)
    out.append(SiteCase("three-passes", L3, (0,) * 4 + (2,) * (L3 - 4), 7, None))
    for j in range(14):                 # (site 13 exists under thirteen tile bits only: under twelve, site 12 again)
        out.append(SiteCase("alone-site%d" % j, tb + 1, None, 9, min(j, tb)))
    L = tb + 3          # two general sites and tb - 3 diagonal ones above bit 3: the tile has room for tb - 6 of those
    out.append(SiteCase("diagonal-outside", L, (1, 2, 0, 1, 2, 1, 1, 2) + (1,) * (L - 8), 31, None))
    # (added after the study of value changes: the factor of the sites outside the tile was held by two shapes only)
    out.append(SiteCase("diagonal-top", tb + 1, (2,) * 4 + (1,) * (tb - 3), 34, None))          # site tb alone outside
    out.append(SiteCase("diagonal-outside-2", tb + 2, (2, 0, 2, 1) + (1,) * (tb - 2), 35, None))
    out.append(SiteCase("all-diagonal", tb + 2, (1,) * (tb + 2), 32, None))
    out.append(SiteCase("all-diagonal-L3", 3, (1,) * 3, 33, None))
    return out


def site_matrices(case):
    if case.single is not None:
        mats = np.broadcast_to(np.eye(2, dtype=np.complex128), (case.L, 2, 2)).copy()
        mats[case.single] = [[1, 2], [3j, 4]]
        return mats
    mats = site_ops_ref.exact_matrices(case.L, case.seed, classes=None if case.classes is None else list(case.classes))
    for j in range(case.L):            # a diagonal site has two entries that differ
        if case.classes is not None and case.classes[j] == 1 and mats[j, 0, 0] == mats[j, 1, 1]:
            mats[j, 1, 1] = mats[j, 0, 0] * 1j if mats[j, 0, 0] != 0 else 1
    return mats


def site_swizzles(L):
    return [0] + [s for s in (5, 6, 12) if L > s]


def site_desc(L, swz):
    return descriptor(("full", L), swz)


def call_site_ops(L, swz, mats, lies, in_place):
    """dnm_site_ops_apply between guards, twice: the result as it lies"""
    import torch
    desc = site_desc(L, swz)
    m = np.ascontiguousarray(mats, dtype=np.complex128).view(np.float64)
    outs = []
    for _ in range(2):
        xb = Buf(lies, SENT if in_place else NAN)
        yb = xb if in_place else Buf(np.full(lies.size, SENT))
        rc = lib().dnm_site_ops_apply(xb.ptr, yb.ptr, C.byref(desc), m.ctypes.data_as(f64p), None)
        assert rc == 0, err()
        torch.cuda.synchronize()                                  # (the call is asynchronous on the stream)
        outs.append(yb.get())
        if not in_place:
            assert same_bits(xb.get(), lies), "the state was written"
    assert same_bits(outs[0], outs[1]), "a second call returns other bytes"
    clean(outs[0], "the product")
    return outs[0]


def check_site_case(case):
    mats = site_matrices(case)
    L = case.L
    (xr, xi), _ = data(1 << L, 60 + case.seed % 5)
    wr, wi = ref.site_product((xr, xi), mats)                     # index order
    assert case.classes is None or np.any(wr != xr) or np.any(wi != xi)       # (a random mix may be all identity)
    swzs = site_swizzles(L) if L <= 16 else [12]         # (2^21 and 2^23 amplitudes: the production-like shift only)
    for swz in swzs:
        pos = ref.vec_pos(np.arange(1 << L, dtype=np.int64), swz)
        lies = np.empty(1 << L, dtype=np.complex128)
        lies[pos] = cplx(xr, xi)
        for in_place in (False, True):
            got = call_site_ops(L, swz, mats, lies, in_place)[pos]
            bad = np.flatnonzero((got.real != wr) | (got.imag != wi))
            assert bad.size == 0, (case.name, swz, in_place, bad[:8], got[bad[:2]], wr[bad[:2]], wi[bad[:2]])


@pytest.fixture(params=[12, 13])
def tile_bits(request):
    """Twelve bits is the default (site_ops_kernel<256>); thirteen (site_ops_kernel<512>) comes from the experiment
    knob, which the library reads at every call (csrc/dnm_common.h: knob), so it is set and restored in this process."""
    old = os.environ.get("DNM_SITE_OPS_TILE_BITS")
    assert os.environ.get("DNM_EXPERIMENTAL") == "1"
    os.environ["DNM_SITE_OPS_TILE_BITS"] = str(request.param)
    eye = np.broadcast_to(np.eye(2, dtype=np.complex128), (6, 2, 2)).copy().view(np.float64)
    tb = C.c_int()
    assert lib().dnm_site_ops_plan(C.byref(site_desc(6, 0)), eye.ctypes.data_as(f64p), C.byref(tb), None, None, None,
                                   None) == 0
    assert tb.value == request.param
    yield request.param
    if old is None:
        del os.environ["DNM_SITE_OPS_TILE_BITS"]
    else:
        os.environ["DNM_SITE_OPS_TILE_BITS"] = old


@pytest.mark.parametrize("i", range(len(site_cases(12))), ids=[c.name for c in site_cases(12)])
def test_site_product_exact(tile_bits, i):
    """(under thirteen tile bits the sizes that follow the tile grow by one and the three passes take L = 23)"""
    check_site_case(site_cases(tile_bits)[i])


# ================================================================ refusals

def _with(spec, swz=0, **fields):
    def make():
        d = descriptor(spec, swz)
        for key, v in fields.items():
            if key == "site_perm":
                d._perm = np.arange(64, dtype=np.int8)
                v = d._perm.ctypes.data_as(C.POINTER(C.c_int8))
            if key in ("nchoosek", "state_map", "rmap_states") and v is None:
                v = C.POINTER(C.c_int64)()
            setattr(d, key, v)
        return d
    return make


def _side_refusals():
    """(descriptor maker, sector, a word of the message): what submap_check_side refuses on either side of a map and in
    the sector weights"""
    F, P13, S = ("full", 10), ("parity", 13, 1), ("sc", 10, 4)
    odd = lambda: raw_explicit(10, [1, 2, 1000])
    halves = lambda: raw_explicit(10, [1, 513, 2, 1022])        # (row dim / 2 - 1 has spin 9 down)
    return [(_with(F, type=7), 0, "type"), (_with(F, L=0), 0, "L=0"), (_with(F, L=64), 0, "L=64"),
            (_with(F, L=63), 0, "62 index bits"), (_with(F, site_perm=True), 0, "site_perm"),
            (_with(S, site_perm=True), 0, "site_perm"), (_with(S, vec_swizzle=6 | (4 << 8)), 0, "reference order"),
            (_with(S, vec_swizzle=5), 0, "reference order"), (_with(("ex", "e13sorted"), vec_swizzle=5), 0, "Explicit"),
            (_with(F, vec_swizzle=-1), 0, "vec_swizzle"), (_with(F, vec_swizzle=3), 0, "vec_swizzle"),
            (_with(F, vec_swizzle=4), 0, "vec_swizzle"), (_with(P13, vec_swizzle=25), 0, "vec_swizzle"),
            (_with(F), 2, "sector 2"), (_with(F), -2, "sector -2"), (_with(P13, space=2), 0, "parity space"),
            (_with(S, nchoosek=None), 0, "SpinConserve descriptor"), (_with(S, ld_nchoosek=10), 0, "SpinConserve descriptor"),
            (_with(S, k=11), 0, "SpinConserve descriptor"), (_with(S, k=-1), 0, "SpinConserve descriptor"),
            (_with(("ex", "e13sorted"), state_map=None), 0, "Explicit descriptor"),
            (_with(("ex", "e13sorted"), rmap_states=None), 0, "Explicit descriptor"),
            (_with(("ex", "e13sorted"), dim=0), 0, "Explicit descriptor"),
            (_with(P13), 1, "even"), (_with(P13), -1, "even"), (_with(S), 1, "k = L / 2"), (_with(("sc", 10, 5), k=4), -1, "k = L / 2"),
            (odd, 1, "odd dimension"), (halves, -1, "first half")]


SIDE_REFUSALS = _side_refusals()
GOOD_MATS = np.broadcast_to(np.eye(2, dtype=np.complex128), (64, 2, 2)).copy()
GOOD_MATS[:, 0, 1] = 1


def _bad_mats(j, part, value):
    m = GOOD_MATS.copy().view(np.float64)
    m[j, 1, 2 + part] = value
    return m.view(np.complex128)


def _perm_refusals():
    """(descriptor maker or None, sector, nperm, perms or None, a word of the message): perm_check and what it calls"""
    F, P, S = ("full", 10), ("parity", 11, 1), ("sc", 12, 5)
    good = lambda L: permutations(L, 2)

    def bad(L, at, value):
        p = good(L).copy()
        p[1, at] = value
        return p
    out = [(None, 0, 2, good(10), "null"), (lambda: raw_explicit(10, [1, 2, 7]), 0, 2, good(10), "Explicit"),
           (_with(F, type=7), 0, 2, good(10), "type"), (_with(F, L=0), 0, 2, good(10), "L=0"),
           (_with(F, L=65), 0, 2, good(10), "L=65"), (_with(F, L=63), 0, 2, permutations(63, 2), "2^63"),
           (_with(P, L=64), 0, 2, permutations(64, 2), "2^63"),
           (_with(S, k=13), 0, 2, good(12), "k=13"), (_with(S, k=-1), 0, 2, good(12), "k=-1"),
           (_with(S, vec_swizzle=5), 0, 2, good(12), "reference order"),
           (_with(S, vec_swizzle=6 | (4 << 8)), 0, 2, good(12), "reference order"),
           (_with(S, site_perm=True), 0, 2, good(12), "site_perm"), (_with(F, site_perm=True), 0, 2, good(10), "site_perm"),
           (_with(P, space=2), 0, 2, good(11), "parity space"),
           (_with(F), 2, 2, good(10), "xparity_sector"), (_with(F), -2, 2, good(10), "xparity_sector"),
           (_with(F, L=1), 1, 1, permutations(1, 1), "L=1"), (_with(P), 1, 2, good(11), "even"),
           (_with(P), -1, 2, good(11), "even"), (_with(S), 1, 2, good(12), "k = L / 2"),
           (_with(("sc", 12, 6), L=13, ld_nchoosek=14), -1, 2, permutations(13, 2), "k = L / 2"),
           (_with(F), 0, 0, good(10), "0 permutations"), (_with(F), 0, 65, permutations(10, 65), "65 permutations"),
           (_with(F), 0, 2, bad(10, 3, 4), "bijection"), (_with(F), 0, 2, bad(10, 0, 10), "bijection"),
           (_with(F), 0, 2, bad(10, 9, -1), "bijection"), (_with(S), 0, 2, bad(12, 11, 12), "bijection"),
           (_with(P), 0, 2, bad(11, 5, 6), "bijection")]
    for s in (-1, 3, 4, 25):
        out.append((_with(F, vec_swizzle=s), 0, 2, good(10), "vec_swizzle"))
        out.append((_with(P, vec_swizzle=s), 0, 2, good(11), "vec_swizzle"))
    return out


PERM_REFUSALS = _perm_refusals()


class Scene:
    """Two device vectors and the host outputs of a refusal test: a refused call leaves every one as it was."""

    def __init__(self, n=4096):
        self.x0 = cplx(*ints(n, 70))
        self.x, self.y = Buf(self.x0, NAN), Buf(np.full(n, SENT))
        self.out, self.op = host_out(256)
        self.out2, self.op2 = host_out(2)

    def refused(self, rc, word):
        assert rc != 0
        assert word in err(), err()
        assert same_bits(self.x.get(), self.x0), "a refused call wrote to its input"
        assert same_bits(self.y.get(), np.full(self.y.n, SENT)), "a refused call wrote to its output"
        for o in (self.out, self.out2):
            assert same_bits(o, np.full(o.size, SENT.real)), "a refused call wrote to a host output"


@pytest.mark.parametrize("i", range(len(PERM_REFUSALS)),
                         ids=["%s-%d" % (r[4].replace(" ", "_"), n) for n, r in enumerate(PERM_REFUSALS)])
def test_perm_refusal(i):
    make, xsec, nperm, perms, word = PERM_REFUSALS[i]
    s = Scene()
    d = make() if make else None
    dp = C.byref(d) if d is not None else None
    pp = perms.ctypes.data_as(i32p)
    coef = np.ones(2 * 65)
    s.refused(lib().dnm_perm_apply(s.x.ptr, s.y.ptr, dp, xsec, nperm, pp, coef.ctypes.data_as(f64p), 0, None), word)
    s.refused(lib().dnm_perm_dots(s.x.ptr, s.x.ptr, dp, xsec, nperm, pp, s.op, None), word)


def test_perm_argument_refusals():
    s = Scene()
    d = descriptor(("full", 10))
    p = permutations(10, 2)
    pp, cp, L = p.ctypes.data_as(i32p), np.ones(4).ctypes.data_as(f64p), lib()
    s.refused(L.dnm_perm_apply(None, s.y.ptr, C.byref(d), 0, 2, pp, cp, 0, None), "null")
    s.refused(L.dnm_perm_apply(s.x.ptr, None, C.byref(d), 0, 2, pp, cp, 0, None), "null")
    s.refused(L.dnm_perm_apply(s.x.ptr, s.y.ptr, C.byref(d), 0, 2, None, cp, 0, None), "null")
    s.refused(L.dnm_perm_apply(s.x.ptr, s.y.ptr, C.byref(d), 0, 2, pp, None, 0, None), "null")
    s.refused(L.dnm_perm_apply(s.x.ptr, s.x.ptr, C.byref(d), 0, 2, pp, cp, 0, None), "same vector")
    s.refused(L.dnm_perm_dots(None, s.x.ptr, C.byref(d), 0, 2, pp, s.op, None), "null")
    s.refused(L.dnm_perm_dots(s.x.ptr, None, C.byref(d), 0, 2, pp, s.op, None), "null")
    s.refused(L.dnm_perm_dots(s.x.ptr, s.x.ptr, C.byref(d), 0, 2, None, s.op, None), "null")
    s.refused(L.dnm_perm_dots(s.x.ptr, s.x.ptr, C.byref(d), 0, 2, pp, None, None), "null")


@pytest.mark.parametrize("i", range(len(SIDE_REFUSALS)),
                         ids=["%s-%d" % (r[2].replace(" ", "_"), n) for n, r in enumerate(SIDE_REFUSALS)])
def test_map_and_weights_side_refusal(i):
    """on the source of a map, on its target, and in the sector weights"""
    make, sec, word = SIDE_REFUSALS[i]
    s = Scene()
    bad = make()
    good = descriptor(("full", int(bad.L) if 1 <= bad.L <= 62 else 10))
    L = lib()
    named = "descriptor" not in word and word != "parity space"      # (those three come without the side's name)
    s.refused(L.dnm_subspace_map_apply(s.x.ptr, C.byref(bad), sec, s.y.ptr, C.byref(good), 0, None), word)
    assert "(source)" in err() or not named
    s.refused(L.dnm_subspace_map_apply(s.x.ptr, C.byref(good), 0, s.y.ptr, C.byref(bad), sec, None), word)
    assert "(target)" in err() or not named
    s.refused(L.dnm_sector_weights(s.x.ptr, C.byref(bad), sec, s.op, s.op2, None), word)
    s.refused(L.dnm_sector_weights(s.x.ptr, C.byref(bad), sec, s.op, None, None), word)


def test_map_and_weights_argument_refusals():
    s = Scene()
    L = lib()
    f10, f9, sc = descriptor(("full", 10)), descriptor(("full", 9)), descriptor(("sc", 10, 5))
    s.refused(L.dnm_subspace_map_apply(None, C.byref(f10), 0, s.y.ptr, C.byref(sc), 0, None), "null")
    s.refused(L.dnm_subspace_map_apply(s.x.ptr, C.byref(f10), 0, None, C.byref(sc), 0, None), "null")
    s.refused(L.dnm_subspace_map_apply(s.x.ptr, None, 0, s.y.ptr, C.byref(sc), 0, None), "null")
    s.refused(L.dnm_subspace_map_apply(s.x.ptr, C.byref(f10), 0, s.y.ptr, None, 0, None), "null")
    s.refused(L.dnm_subspace_map_apply(s.x.ptr, C.byref(f10), 0, s.x.ptr, C.byref(f10), 0, None), "same vector")
    s.refused(L.dnm_subspace_map_apply(s.x.ptr, C.byref(f10), 0, s.y.ptr, C.byref(f9), 0, None), "L=9")
    s.refused(L.dnm_sector_weights(None, C.byref(f10), 0, s.op, s.op2, None), "null")
    s.refused(L.dnm_sector_weights(s.x.ptr, None, 0, s.op, s.op2, None), "null")
    s.refused(L.dnm_sector_weights(s.x.ptr, C.byref(f10), 0, None, s.op2, None), "null")
    # the flip sums where the subspace does not carry the flip
    for spec in (("sc", 10, 4), ("parity", 11, 0), ("ex", "e13sorted"), ("ex", "e14flip")):
        s.refused(L.dnm_sector_weights(s.x.ptr, C.byref(descriptor(spec)), 0, s.op, s.op2, None), "flip_out")


SITE_REFUSALS = [
    (None, GOOD_MATS, "null"), (_with(("full", 10)), None, "null"), (_with(("parity", 11, 0)), GOOD_MATS, "Full space"),
    (_with(("sc", 10, 5)), GOOD_MATS, "Full space"), (lambda: raw_explicit(10, [1, 2, 5]), GOOD_MATS, "Full space"),
    (_with(("full", 10), site_perm=True), GOOD_MATS, "site_perm"), (_with(("full", 10), L=0), GOOD_MATS, "L=0"),
    (_with(("full", 10), L=63), GOOD_MATS, "L=63"), (_with(("full", 10), vec_swizzle=4), GOOD_MATS, "vec_swizzle"),
    (_with(("full", 10), vec_swizzle=-1), GOOD_MATS, "vec_swizzle"), (_with(("full", 10), vec_swizzle=25), GOOD_MATS, "vec_swizzle"),
    (_with(("full", 10)), _bad_mats(9, 0, np.nan), "site 9"), (_with(("full", 10)), _bad_mats(0, 1, np.inf), "site 0"),
    (_with(("full", 10)), _bad_mats(4, 1, -np.inf), "site 4"),
]


@pytest.mark.parametrize("i", range(len(SITE_REFUSALS)),
                         ids=["%s-%d" % (r[2].replace(" ", "_"), n) for n, r in enumerate(SITE_REFUSALS)])
def test_site_ops_refusal(i):
    import torch
    make, mats, word = SITE_REFUSALS[i]
    s = Scene()
    d = make() if make else None
    dp = C.byref(d) if d is not None else None
    mp = None if mats is None else np.ascontiguousarray(mats).view(np.float64).ctypes.data_as(f64p)
    rcs = [lib().dnm_site_ops_apply(s.x.ptr, s.y.ptr, dp, mp, None), lib().dnm_site_ops_apply(s.x.ptr, s.x.ptr, dp, mp, None)]
    torch.cuda.synchronize()
    for rc in rcs:
        s.refused(rc, word)
    if d is not None and mp is not None:
        good = descriptor(("full", 10))
        gp = GOOD_MATS.view(np.float64).ctypes.data_as(f64p)
        s.refused(lib().dnm_site_ops_apply(None, s.y.ptr, C.byref(good), gp, None), "null")
        s.refused(lib().dnm_site_ops_apply(s.x.ptr, None, C.byref(good), gp, None), "null")


# ================================================================ rounding cases
# u = 2^-53, gamma(n) = n u / (1 - n u).  A sum of m terms, each a product rounded once (or not at all where the compiler
# fuses it into the addition), passes at most m - 1 additions on the way to the result in whatever order they are made:
# at most m roundings on any path, so |got - ref| <= gamma(m) * sum |terms| (Higham, Accuracy and Stability of
# Numerical Algorithms, section 4.2).  Factors +-1 are exact.  Derived before the run; no margin added.

def normal(n, seed):
    rs = np.random.RandomState(4300 + seed)
    return rs.standard_normal(n) + 1j * rs.standard_normal(n)


def report(what, err_, mag, terms):
    live = mag > 0
    worst = float(np.max(err_[live] / mag[live]))
    print("%s: max |got - ref| / sum|terms| = %.3g = %.2f u, bound gamma(%d) = %.0f u"
          % (what, worst, worst / 2.0 ** -53, terms, gamma(terms) / 2.0 ** -53))
    assert np.all(err_ <= gamma(terms) * mag), what


def test_rounding_perm_apply():
    """A component of y[r] is y0 + sum_g (cr vr - ci vi): 2 n products and the old value, 2 n + 1 terms."""
    case = PERM_BY_NAME["SC(12,6)--n8"]
    side = ref_side(perm_side(case))
    n, npm = ref.rows_of(side), case.nperm
    perms = permutations(12, npm)
    x, y0, c = normal(n, 1), normal(n, 2), normal(npm, 3)
    got = call_perm_apply(descriptor(case.spec), case.xsec, perms, [(z.real, z.imag) for z in c], x, y0)
    re, im, mr, mi = y0.real.astype(LD), y0.imag.astype(LD), np.abs(y0.real).astype(LD), np.abs(y0.imag).astype(LD)
    for g in range(npm):
        pos, s = ref.perm_gather(side, perms[g])
        vr, vi = s * x.real[pos].astype(LD), s * x.imag[pos].astype(LD)
        cr, ci = LD(c[g].real), LD(c[g].imag)
        re, im = re + cr * vr - ci * vi, im + cr * vi + ci * vr
        mr, mi = mr + abs(cr * vr) + abs(ci * vi), mi + abs(cr * vi) + abs(ci * vr)
    report("perm_apply, - sector of SpinConserve(12, 6), 8 permutations",
           np.concatenate([np.abs(got.real - re), np.abs(got.imag - im)]), np.concatenate([mr, mi]), 2 * npm + 1)


def test_rounding_perm_dots():
    """A component of out[g] sums 2 products per row: 2 rows terms, through the lanes, the waves and the workgroups."""
    case = PERM_BY_NAME["Parity(12,0)+-n5"]
    side = ref_side(perm_side(case, 6))
    n = ref.rows_of(side)
    perms = permutations(12, 5)
    phi, psi = normal(n, 4), normal(n, 5)
    got = call_perm_dots(descriptor(case.spec, 6), case.xsec, perms, phi, psi)
    fr, fi = phi.real.astype(LD), phi.imag.astype(LD)
    errs, mags = [], []
    for g in range(5):
        pos, s = ref.perm_gather(side, perms[g])
        vr, vi = s * psi.real[pos].astype(LD), s * psi.imag[pos].astype(LD)
        errs += [abs(got[g, 0] - np.sum(fr * vr + fi * vi)), abs(got[g, 1] - np.sum(fr * vi - fi * vr))]
        mags += [np.sum(np.abs(fr * vr) + np.abs(fi * vi)), np.sum(np.abs(fr * vi) + np.abs(fi * vr))]
    report("perm_dots, + sector of Parity(12, even), swizzle 6, 5 permutations", np.array(errs), np.array(mags), 2 * n)


def test_rounding_map_to_sector():
    """y = (p + t m) kappa with kappa the double of the kernel: one addition and one product, 2 roundings on 2 terms."""
    src, dst = (("full", 14), 0, 5), (("sc", 14, 7), -1, 0)
    x = normal(1 << 14, 6)
    got = call_map(src, dst, x)
    idx, sign, scale = ref.map_terms(ref_side(src), ref_side(dst))
    assert scale == ref.KAPPA and np.all(idx >= 0)
    parts = x.view(np.float64).reshape(-1, 2).astype(LD)
    a, b = parts[idx[:, 0]] * sign[:, :1], parts[idx[:, 1]] * sign[:, 1:]
    want, mag = (a + b) * LD(ref.KAPPA), (np.abs(a) + np.abs(b)) * LD(ref.KAPPA)
    report("map Full(14) -> - sector of SpinConserve(14, 7)", np.abs(got.view(np.float64).reshape(-1, 2) - want).reshape(-1),
           mag.reshape(-1), 2)


def test_rounding_sector_weights():
    """A bin sums re^2 + im^2 over its rows: at most 2 rows terms.  F+- sums |a +- b|^2 / 2 over the pairs: each of the
    2 pairs squares carries the rounding of its sum twice besides its own, 2 pairs + 2 roundings on a path; the halving
    is exact."""
    side = (("full", 13), 0, 6)
    n = 1 << 13
    x = normal(n, 7)
    mag, fl = call_weights(side, x, True)
    rside = ref_side(side)
    cfg = ref.row_configs(rside)
    k = ref.popcount(cfg)
    w = x.real.astype(LD) ** 2 + x.imag.astype(LD) ** 2
    want = np.array([np.sum(w[k == kk]) for kk in range(14)])
    report("sector weights, bins, Full(13), swizzle 6", np.abs(mag - want), want, 2 * n)
    first = np.flatnonzero(((cfg >> np.uint64(12)) & np.uint64(1)) == 0)
    mate, _ = ref.amplitude_of(rside, cfg[first] ^ ref.all_sites(13))
    a, b = x[first], x[mate]
    sq = lambda z: z.real.astype(LD) ** 2 + z.imag.astype(LD) ** 2
    wantf = np.array([np.sum(sq(a.astype(np.clongdouble) + b)) / 2, np.sum(sq(a.astype(np.clongdouble) - b)) / 2])
    report("sector weights, flip sums, Full(13), swizzle 6", np.abs(fl - wantf), wantf, n + 2)


def test_rounding_site_product():
    """A general level forms m0 v0 + m1 v1 per component from 4 products, rounded one by one (no contraction): a
    product, the sum inside a complex product and the sum of the two, 3 roundings per level on a path, 3 L after L
    levels; sum |terms| is the product of the matrices of moduli of the parts on the moduli of the parts of x."""
    L = 13
    rs = np.random.RandomState(4308)
    mats = rs.standard_normal((L, 2, 2)) + 1j * rs.standard_normal((L, 2, 2))
    x = normal(1 << L, 8)
    got = call_site_ops(L, 6, mats, x[ref.vec_pos(np.arange(1 << L), 6)], False)[ref.vec_pos(np.arange(1 << L), 6)]
    yr, yi = x.real.astype(LD), x.imag.astype(LD)
    ar, ai = np.abs(yr), np.abs(yi)
    for j in range(L):
        m = mats[j]
        shape = (-1, 2, 1 << j)
        vr, vi, br, bi = yr.reshape(shape), yi.reshape(shape), ar.reshape(shape), ai.reshape(shape)
        outr, outi, magr, magi = (np.empty_like(vr) for _ in range(4))
        for a in range(2):
            outr[:, a], outi[:, a], magr[:, a], magi[:, a] = 0, 0, 0, 0
            for b in range(2):
                mr, mi = LD(m[a, b].real), LD(m[a, b].imag)
                outr[:, a] += mr * vr[:, b] - mi * vi[:, b]
                outi[:, a] += mr * vi[:, b] + mi * vr[:, b]
                magr[:, a] += abs(mr) * br[:, b] + abs(mi) * bi[:, b]
                magi[:, a] += abs(mr) * bi[:, b] + abs(mi) * br[:, b]
        yr, yi, ar, ai = outr.reshape(-1), outi.reshape(-1), magr.reshape(-1), magi.reshape(-1)
    report("site product, Full(13), swizzle 6, 13 general sites",
           np.concatenate([np.abs(got.real - yr), np.abs(got.imag - yi)]), np.concatenate([ar, ai]), 3 * L)
