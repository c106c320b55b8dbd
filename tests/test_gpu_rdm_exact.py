"""
The reduced-density-matrix kernels (csrc/rdm_kernels.hip, csrc/rdm_sector_kernels.hip and the matrix-core tile they
share, csrc/rdm_tile.h) through the C ABI, one call at a time: dnm_reduced_density_matrix and dnm_rdm_sector_blocks on
device buffers of the test's own, with descriptors taken from the subspace objects.  Nothing goes through State, which
would normalise.

Exact cases: real and imaginary parts of every amplitude are independent non-zero integers in [-8, 8]
(tests/test_gpu_vec.py::ints).  A product of two parts has modulus <= 64 and a component of a matrix entry sums 2 T of
them (T traced configurations): every intermediate value is an integer far below 2^53, on the matrix cores, in the fma
chains of the vector-unit forms and in the plain adds of the slice tree alike, so any order of summation and any
contraction gives the same value and the tests assert EQUALITY with the int64 reference of tests/rdm_ref.py.  Equality
of values, not of bit patterns: the mirrored triangle holds -si, which is -0.0 where a sum is zero.  An XParity state is
embedded without its 1 / sqrt 2 and compared with twice the result (the kernel's factor 1/2 is exact).

Buffers: the state lies between 64 NaN amplitudes on each side (a masked fetch that reads anyway and multiplies by zero
shows as NaN); every output is filled with a sentinel beforehand and lies between 64 sentinels, the blocks of one
sector call back to back in one allocation with 64 sentinels between them.  Of every output the tests assert that no
sentinel is left in it, that it equals its conjugate transpose exactly and that its diagonal is real.

Rounding cases (one per kernel path, normal deviates) against numpy.longdouble: per entry and component
|got - ref| <= gamma(2 T) * sum |products|; the derivation stands beside them.
"""
import ctypes as C
import functools
from math import comb

import numpy as np
import pytest

from dynamite_amd import _lib
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve
from gpu_util import rand_state
import rdm_ref
import test_gpu_vec
from test_gpu_vec import Buf, G, NAN, SENT, cplx, gamma, ints, same_bits, vec_pos

pytestmark = pytest.mark.gpu

LD = np.longdouble


# ---------------------------------------------------------------- subspaces, states, references

@functools.lru_cache(maxsize=None)
def space(name, L):
    """The subspace objects (kept alive: a descriptor points into the tables of its object)."""
    if name == "full":
        return Full(L=L)
    if name in ("even", "odd"):
        return Parity(name, L=L)
    if name == "sc_half":
        return SpinConserve(L, L // 2)
    if name == "sc_one":
        return SpinConserve(L, 1)
    top = (1 << L) - 1
    if name == "explicit_third":                # a seeded random third of the states
        rs = np.random.RandomState(300 + L)
        return Explicit(np.sort(rs.choice(1 << L, size=(1 << L) // 3, replace=False)), L=L)
    if name == "explicit_inner":                # neither state 0 nor state 2^L - 1, but their neighbours 1 and 2^L - 2
        rs = np.random.RandomState(400 + L)
        pick = 2 + rs.choice(top - 3, size=(1 << L) // 2, replace=False)
        states = np.sort(np.concatenate([[1, top - 1], pick]))
        assert states[0] == 1 and states[-1] == top - 1 and np.unique(states).size == states.size
        return Explicit(states, L=L)
    raise KeyError(name)


def descriptor(sub, swz=0):
    """The subspace's descriptor with the vector layout the test lays its data out in."""
    d = _lib.Subspace.from_buffer_copy(sub._c())
    d.vec_swizzle = swz
    return d


def swizzles(name, L):
    """Full and Parity take vec_swizzle 0, 5 and 6 (mat.cpp: view_from_c; only sizes that are multiples of 2^S); every
    other type here takes reference order alone."""
    if name == "full":
        return [0] + [S for S in (5, 6) if L >= S]
    if name in ("even", "odd"):
        return [0] + [S for S in (5, 6) if L - 1 >= S]
    return [0]


def big_ints(n, seed):
    """ints(n, seed) without leaving tens of megabytes in its cache for the rest of the session"""
    re, im = ints(n, seed)
    if n > 1 << 20:
        test_gpu_vec._INTS.pop((n, seed), None)
    return re, im


_SEED = {"full": 1, "even": 2, "odd": 3, "sc_half": 4, "sc_one": 5, "explicit_third": 6, "explicit_inner": 7}
_STATES = {}


def int_state(name, L):
    """(subspace, x as complex128 in index order, (full_re, full_im)); kept for L <= 14"""
    if (name, L) in _STATES:
        return _STATES[(name, L)]
    sub = space(name, L)
    n = sub.get_dimension()
    re, im = big_ints(n, 50 + _SEED[name])
    states = np.arange(n, dtype=np.int64) if name == "full" else sub.idx_to_state(np.arange(n, dtype=np.int64))
    out = (sub, cplx(re, im), rdm_ref.embed(states, re, im, L))
    if L <= 14:
        _STATES[(name, L)] = out
    return out


@functools.lru_cache(maxsize=None)
def dense_reference(name, L, keep):
    sub, x, (full_re, full_im) = int_state(name, L)
    return rdm_ref.dense(full_re, full_im, L, list(keep))


def check_output(rho, what=""):
    """What every output has to satisfy, whatever its values."""
    assert rho.ndim == 2 and rho.shape[0] == rho.shape[1]
    assert not np.any(rho.real == SENT.real) and not np.any(rho.imag == SENT.imag), "sentinel left in " + what
    assert np.all(np.isfinite(rho.view(np.float64))), "NaN or Inf in " + what
    assert np.array_equal(rho, rho.conj().T), what + " is not Hermitian to the last bit"
    assert np.all(rho.diagonal().imag == 0.0), what + " has a complex diagonal"


def assert_equal_int(rho, ref, mult, what):
    """mult * rho == ref = (re, im) in int64, entry by entry"""
    rr, ri = ref
    assert rho.shape == rr.shape == ri.shape, (what, rho.shape, rr.shape)
    bad_r, bad_i = mult * rho.real != rr.astype(np.float64), mult * rho.imag != ri.astype(np.float64)
    if np.any(bad_r) or np.any(bad_i):
        w = np.argwhere(bad_r | bad_i)
        a, b = w[0]
        raise AssertionError("%s: %d of %d entries differ, the first at (%d, %d): got %r * %d, reference (%d, %d)"
                             % (what, len(w), rho.size, a, b, rho[a, b], mult, rr[a, b], ri[a, b]))
    assert np.array_equal(mult * rho.real, rr.astype(np.float64))
    assert np.array_equal(mult * rho.imag, ri.astype(np.float64))


# ---------------------------------------------------------------- dense form

def run_dense(sub, x, keep, swz=0):
    """dnm_reduced_density_matrix of the state x (index order; laid out by vec_pos here) between guards"""
    n = x.size
    assert swz == 0 or n % (1 << swz) == 0
    lay = np.empty(n, dtype=np.complex128)
    lay[vec_pos(np.arange(n, dtype=np.int64), swz)] = x          # element i lies at position vec_pos(i)
    xb = Buf(lay, NAN)
    K = 1 << len(keep)
    rb = Buf(np.full(K * K, SENT))
    keep_a = np.ascontiguousarray(keep, dtype=np.int64)
    desc = descriptor(sub, swz)
    _lib.check(_lib.lib().dnm_reduced_density_matrix(xb.ptr, C.byref(desc), keep_a.size, _lib.p64(keep_a), rb.ptr,
                                                     None))
    rho = rb.get().reshape(K, K)                                  # (asserts the guards of rho)
    if n <= 1 << 22:
        assert same_bits(xb.get(), lay)                           # the state is read, never written
    return rho


def exact_bound_holds(L, k):
    """2 T products of modulus <= 64 per component (and as many again where the reference doubles an XParity state):
    every partial sum, in any order, is an integer of modulus <= 2 * T * 64 * 2, exact in a double"""
    T = 1 << (L - k)
    assert 2 * T * 64 * 2 < 2 ** 53
    return T


# path, L, keep: the smallest shapes at which each path can fail (T = 2^(L - k) traced configurations)
DENSE_ROWS = [
    # streaming kernel, k = 1, 2
    ("stream", 12, (0,)), ("stream", 12, (11,)), ("stream", 12, (3, 8)),
    ("stream, one tree level (64 slices)", 17, (5,)),
    ("stream, two tree levels (2048 slices)", 22, (21,)),
    ("stream, T = 1", 1, (0,)), ("stream, T = 1, k = 2", 2, (0, 1)), ("stream, T = 2", 2, (1,)),
    # vector-unit tiles, k = 3, 4, 5: 64, 16 and 4 groups over the traced index, with and without wave shuffles
    ("tile 8", 12, (0, 1, 2)), ("tile 8", 12, (9, 10, 11)), ("tile 8", 12, (1, 5, 10)),
    ("tile 16", 12, (0, 1, 2, 3)), ("tile 16", 12, (8, 9, 10, 11)), ("tile 16", 12, (0, 3, 7, 11)),
    ("tile 32", 12, (0, 1, 2, 3, 4)), ("tile 32", 12, (7, 8, 9, 10, 11)), ("tile 32", 12, (1, 2, 6, 9, 11)),
    ("tile 8, T below one chunk", 8, (0, 1, 2)), ("tile 32, T below one chunk", 6, (1, 2, 3, 4, 5)),
    ("tile 8, T = 1", 3, (0, 1, 2)), ("tile 32, T = 1", 5, (0, 1, 2, 3, 4)),
    # one matrix-core tile, k = 6
    ("mfma, T = 1", 6, tuple(range(6))), ("mfma, T = 4 < a chunk of 16", 8, (0, 1, 3, 4, 6, 7)),
    ("mfma, four chunks", 12, tuple(range(6))), ("mfma, 128 slices: the tree runs", 17, tuple(range(11, 17))),
    # several matrix-core tiles, off-diagonal ones included
    ("mfma, three tiles", 12, (0, 2, 4, 6, 8, 10, 11)),
    ("mfma, 36 tiles", 13, tuple(range(9))), ("mfma, 36 tiles", 13, tuple(range(4, 13))),
    ("mfma, the most segments", 14, (0, 2, 4, 6, 8, 10, 12)),
]
SUBSPACES = ["even", "odd", "sc_half", "sc_one", "explicit_third", "explicit_inner"]
DENSE_CASES = [("full", L, keep) for _, L, keep in DENSE_ROWS] + \
              [(name, L, keep) for name in SUBSPACES for _, L, keep in DENSE_ROWS if 12 <= L <= 14]


def _case_id(v):
    return "".join(str(v).split())


@pytest.mark.parametrize("name,L,keep", DENSE_CASES, ids=_case_id)
def test_dense_exact(name, L, keep):
    exact_bound_holds(L, len(keep))
    sub, x, full = int_state(name, L)
    ref = dense_reference(name, L, keep) if L <= 14 else rdm_ref.dense(full[0], full[1], L, list(keep))
    del full
    assert np.any(ref[1] != 0) or len(keep) == 1 or name == "sc_one"     # (an imaginary part to get the sign of)
    for swz in swizzles(name, L):
        rho = run_dense(sub, x, list(keep), swz)
        what = "%s L=%d keep=%s swizzle %d" % (name, L, list(keep), swz)
        check_output(rho, what)
        assert_equal_int(rho, ref, 1, what)


def test_dense_exact_streaming_cap_second_trip():
    """L = 24, keep = [11] on the Full space: T = 2^23 traced configurations on the streaming kernel's cap of 4096
    workgroups of 256 threads with 4 configurations in flight = 2^22 per trip, so the grid-stride loop runs twice (and
    its `tr < T` mask is evaluated on a second trip).  The one case above 2^22 amplitudes; state and reference (a 2 x 2
    matrix: two strided dot products) are built in numpy."""
    L, keep = 24, [11]
    exact_bound_holds(L, 1)
    n = 1 << L
    re, im = big_ints(n, 24)
    r = re.reshape(1 << 12, 2, 1 << 11)
    i = im.reshape(1 << 12, 2, 1 << 11)
    r0, r1, i0, i1 = r[:, 0, :], r[:, 1, :], i[:, 0, :], i[:, 1, :]
    d0, d1 = int(np.sum(r0 * r0 + i0 * i0)), int(np.sum(r1 * r1 + i1 * i1))
    # rho[1, 0] = sum psi(1) conj(psi(0))
    o_re, o_im = int(np.sum(r1 * r0 + i1 * i0)), int(np.sum(i1 * r0 - r1 * i0))
    ref = (np.array([[d0, o_re], [o_re, d1]], dtype=np.int64), np.array([[0, -o_im], [o_im, 0]], dtype=np.int64))
    assert o_im != 0
    x = cplx(re, im)
    del re, im, r, i, r0, r1, i0, i1
    rho = run_dense(Full(L=L), x, keep)
    check_output(rho, "L=24")
    assert_equal_int(rho, ref, 1, "L=24 keep=[11]")


# ---------------------------------------------------------------- sector form

@functools.lru_cache(maxsize=None)
def sc_space(L, k):
    return SpinConserve(L, k)


def sector_plan(desc, keep, xsec):
    """dnm_rdm_sector_plan: [(n, rows, traced configurations)] in ascending n"""
    keep_a = np.ascontiguousarray(keep, dtype=np.int64)
    nb, scratch = C.c_int(), C.c_size_t()
    ns = (C.c_int32 * (keep_a.size + 1))()
    dims = np.zeros(keep_a.size + 1, dtype=np.int64)
    traced = np.zeros(keep_a.size + 1, dtype=np.int64)
    _lib.check(_lib.lib().dnm_rdm_sector_plan(C.byref(desc), keep_a.size, _lib.p64(keep_a), xsec, C.byref(nb), ns,
                                              _lib.p64(dims), _lib.p64(traced), C.byref(scratch)))
    return [(int(ns[i]), int(dims[i]), int(traced[i])) for i in range(nb.value)]


def run_sector(desc, x, keep, xsec, plan, sel):
    """dnm_rdm_sector_blocks for the blocks `sel`, in that order.  One allocation holds room for EVERY block of the
    plan, in ascending n, back to back with G sentinels before, between and behind them; block sel[i] is handed the
    room of its n.  Everything outside the selected blocks must keep its sentinels bit for bit."""
    import torch
    offs, pos = {}, G
    for n, d, _ in plan:
        offs[n] = pos
        pos += d * d + G
    dims = {n: d for n, d, _ in plan}
    host = np.full(pos, SENT, dtype=np.complex128)
    t = torch.from_numpy(host).cuda()
    keep_a = np.ascontiguousarray(keep, dtype=np.int64)
    sel_c = (C.c_int32 * len(sel))(*sel)
    ptrs = (C.c_void_p * len(sel))(*[t.data_ptr() + 16 * offs[n] for n in sel])
    xb = Buf(x, NAN)
    _lib.check(_lib.lib().dnm_rdm_sector_blocks(xb.ptr, C.byref(desc), keep_a.size, _lib.p64(keep_a), xsec, len(sel),
                                                sel_c, ptrs, None))
    now = t.cpu().numpy()
    assert same_bits(xb.get(), x)
    mine = np.zeros(pos, dtype=bool)
    out = {}
    for n in sel:
        sl = slice(offs[n], offs[n] + dims[n] * dims[n])
        mine[sl] = True
        out[n] = now[sl].reshape(dims[n], dims[n]).copy()
    assert np.array_equal(now[~mine].view(np.uint64), host[~mine].view(np.uint64)), \
        "written outside the selected blocks (guards, or the room of a block that was not asked for)"
    return out


def sector_state(L, k, xsec):
    """(x complex128, states): the whole SpinConserve(L, k) state, or the XParity half on its representatives (the
    first half of the parent's basis)"""
    sub = sc_space(L, k)
    n = sub.get_dimension()
    if xsec:
        assert n % 2 == 0
        n //= 2
    re, im = ints(n, 70 + L + k + xsec)
    return re, im, sub.idx_to_state(np.arange(n, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def sector_reference(L, k, keep, xsec):
    re, im, states = sector_state(L, k, xsec)
    full_re, full_im = rdm_ref.embed(states, re, im, L, xsec)
    return rdm_ref.blocks(full_re, full_im, L, list(keep))


def check_sector(L, k, keep, xsec, sel=None):
    exact_bound_holds(L, len(keep))
    keep = list(keep)
    kA = len(keep)
    desc = descriptor(sc_space(L, k))
    re, im, states = sector_state(L, k, xsec)
    ref = sector_reference(L, k, tuple(keep), xsec)
    plan = sector_plan(desc, keep, xsec)
    assert [n for n, _, _ in plan] == sorted(ref) == list(range(max(0, k - (L - kA)), min(k, kA) + 1))
    for n, d, tr in plan:
        assert d == comb(kA, n) == ref[n][0].shape[0] and tr == comb(L - kA, k - n)
    sel = [n for n, _, _ in plan] if sel is None else sel
    got = run_sector(desc, cplx(re, im), keep, xsec, plan, sel)
    assert list(got) == list(sel)
    for n in sel:
        what = "SpinConserve(%d, %d) xparity %+d keep=%s block n=%d" % (L, k, xsec, keep, n)
        check_output(got[n], what)
        assert_equal_int(got[n], ref[n], 2 if xsec else 1, what)
    return got


XSECS = [0, +1, -1]
SECTOR_CASES = [
    # blocks of 1, 6, 15, 20 rows (1, 3, 3, 1 for three kept spins): all under one tile
    (12, 6, tuple(range(6))), (12, 6, tuple(range(6, 12))), (12, 6, (1, 4, 11)), (12, 6, (0, 2, 3, 7, 8, 11)),
    # 70 rows: two tile rows, ragged; the contiguous path, under XParity walked downwards across the tile boundary
    (16, 8, tuple(range(8))),
    # the same sizes by the general path: bit L-1 kept, kept beside low contiguous spins, traced
    (16, 8, tuple(range(8, 16))), (16, 8, (0, 1, 2, 3, 4, 5, 6, 15)), (16, 8, (1, 2, 3, 4, 5, 6, 7, 8)),
    # every spin kept: one block of 70 rows, T = 1, no traced spin
    (8, 4, tuple(range(8))),
    # nothing kept: the 1 x 1 block is the squared norm
    (8, 4, ()), (12, 6, ()),
]


@pytest.mark.parametrize("xsec", XSECS)
@pytest.mark.parametrize("L,k,keep", SECTOR_CASES, ids=_case_id)
def test_sector_exact(L, k, keep, xsec):
    got = check_sector(L, k, keep, xsec)
    if not keep:
        re, im, _ = sector_state(L, k, xsec)
        assert got[0][0, 0] == float(np.sum(re * re + im * im))


@pytest.mark.parametrize("L,k,keep", [(14, 3, tuple(range(9))), (18, 2, tuple(range(16)))], ids=_case_id)
def test_sector_exact_fewer_set_bits_than_kept_spins(L, k, keep):
    """k < kept spins: one-row blocks beside many-row ones in one launch (1, 9, 36, 84 rows; 1, 16, 120 rows where the
    dense form would be 2^16 square), the n above k infeasible.  SpinConserve only (XParity needs L = 2 k)."""
    got = check_sector(L, k, keep, 0)
    assert sorted(got) == list(range(k + 1)) and got[0].shape == (1, 1)


@pytest.mark.parametrize("xsec", XSECS)
@pytest.mark.parametrize("slices", [None, "3", "40"])
@pytest.mark.parametrize("keep", [tuple(range(10)), (0, 1, 2, 3, 4, 10, 11, 12, 13, 14)], ids=_case_id)
def test_sector_exact_several_tiles_and_slices(monkeypatch, keep, slices, xsec):
    """SpinConserve(20, 10), 10 spins kept: 252 rows, 4 x 4 tiles with a ragged edge, by the contiguous and the general
    path; the traced index in the slices the plan chooses, in 3 (the smaller blocks' last slices short or empty) and in
    40 (more than the fan-in of the slice tree)."""
    if slices is None:
        monkeypatch.delenv("DNM_RDM_SECTOR_SLICES", raising=False)
    else:
        monkeypatch.setenv("DNM_RDM_SECTOR_SLICES", slices)
    check_sector(20, 10, keep, xsec)


@pytest.mark.parametrize("xsec", XSECS)
@pytest.mark.parametrize("sel", [[8, 4, 0], [5]], ids=_case_id)
def test_sector_exact_selection(sel, xsec):
    """Blocks asked for out of order, and one alone: each lands in the room handed over for it, and the room of the
    blocks that were not asked for keeps its sentinels (run_sector)."""
    got = check_sector(16, 8, tuple(range(8)), xsec, sel=sel)
    assert list(got) == sel


# ---------------------------------------------------------------- rounding cases
# A component of an entry is a sum of 2 T products (Re: ar br + ai bi, Im: ai br - ar bi over the T traced
# configurations).  Every product is rounded once, or not at all where it is contracted into an fma or runs on the
# matrix cores' fused chain, and then passes at most 2 T - 1 additions on its way to the result, in whatever order the
# kernel, its wave shuffles, its LDS stage and the slice tree add: at most 2 T roundings on any path, so
#     |got - ref| <= gamma(2 T) * sum |products|,    gamma(n) = n u / (1 - n u),  u = 2^-53.
# The factors +-1 of an XParity sector and the final 1/2 are exact.  Derived, not measured; no margin added.

def _ld_parts(z):
    return np.asarray(z.real, dtype=LD), np.asarray(z.imag, dtype=LD)


def _within(got, br, bi, T, mult, what):
    """got (complex128) times mult against B B^H in longdouble, B = br + i bi"""
    ref_r, ref_i = br @ br.T + bi @ bi.T, bi @ br.T - br @ bi.T
    ar_, ai_ = np.abs(br), np.abs(bi)
    mag_r, mag_i = ar_ @ ar_.T + ai_ @ ai_.T, ai_ @ ar_.T + ar_ @ ai_.T
    er = np.abs(mult * np.asarray(got.real, dtype=LD) - ref_r)
    ei = np.abs(mult * np.asarray(got.imag, dtype=LD) - ref_i)
    worst = max(float(np.max(er / mag_r)), float(np.max(ei / mag_i)))
    print("%s: max |got - ref| / sum|products| = %.3g = %.2f u, bound gamma(%d) = %.3g"
          % (what, worst, worst / 2.0 ** -53, 2 * T, gamma(2 * T)))
    assert np.all(er <= gamma(2 * T) * mag_r) and np.all(ei <= gamma(2 * T) * mag_i), what


@pytest.mark.parametrize("what,keep", [("streaming kernel", (3, 8)), ("vector-unit tile of 16", (0, 3, 7, 11)),
                                       ("matrix cores, three tiles", (0, 2, 4, 6, 8, 10, 11))], ids=_case_id)
def test_dense_rounding(what, keep):
    L = 12
    x = rand_state(1 << L, 12)
    rho = run_dense(Full(L=L), x, list(keep), 6)
    check_output(rho, what)
    xr, xi = _ld_parts(x)
    _within(rho, rdm_ref.operand(xr, L, keep), rdm_ref.operand(xi, L, keep), 1 << (L - len(keep)), 1, what)


@pytest.mark.parametrize("what,keep,xsec", [("sector, contiguous", tuple(range(8)), 0),
                                            ("sector, general, XParity", tuple(range(8, 16)), -1)], ids=_case_id)
def test_sector_rounding(what, keep, xsec):
    L, k = 16, 8
    sub = sc_space(L, k)
    n = sub.get_dimension() // (2 if xsec else 1)
    x = rand_state(n, 16)
    states = sub.idx_to_state(np.arange(n, dtype=np.int64))
    full = np.zeros(1 << L, dtype=np.complex128)
    full[states] = x
    if xsec:
        full[states ^ ((1 << L) - 1)] = xsec * x
    desc = descriptor(sub)
    plan = sector_plan(desc, list(keep), xsec)
    got = run_sector(desc, x, list(keep), xsec, plan, [m for m, _, _ in plan])
    fr, fi = _ld_parts(full)
    ar, ai = rdm_ref.operand(fr, L, keep), rdm_ref.operand(fi, L, keep)
    pc = rdm_ref.popcounts(len(keep))
    for m, d, tr in plan:
        check_output(got[m], what)
        rows = np.nonzero(pc == m)[0]
        cols = np.nonzero(np.any(ar[rows] != 0, axis=0))[0]
        assert rows.size == d and cols.size == tr                 # T of this block: its traced configurations
        _within(got[m], ar[np.ix_(rows, cols)], ai[np.ix_(rows, cols)], tr, 2 if xsec else 1, "%s, n = %d" % (what, m))
