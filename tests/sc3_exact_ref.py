"""Exact host reference for the SpinConserve multiply in the three-field internal layout (csrc/sc3_kernels.hip,
csrc/sc3g_kernels.hip):  y = H x - b z + c z2  and the fused sums (Re <x, y>, Im <x, y>, |y|^2) on SpinConserve(L, k)
and on XParity(SpinConserve(L, L / 2), +-), at dimensions from 1 to 5.2 million rows.

The conventions are those of tests/wide_ref.py: every coefficient is a multiple of 1/8 of modulus at most 16, every
amplitude a Gaussian integer, b and c are dyadic (3/8 and -1/4 + 5/8 i); the arithmetic is done in int64 on arrays of
states, in eighths, and divided once at the end.  What it gives is what any double-precision kernel must give value for
value, in any order of summation and with or without fma, as long as every partial sum stays below 2^53 in units of
1/64: ``Ref.apply`` and ``fused_sums`` ASSERT that on the numbers of the case at hand -- for an entry of y on the sum
of the moduli of its products, for the sums on the sum of the moduli of their terms, so that no order of summation can
leave the exact range.

One term is applied at a time from the MSC definition  H[row, col] += (-1)^popcount(bra & sign) * coeff,
bra = ket ^ mask, col = index of bra (rows whose bra leaves the subspace contribute nothing).  The index of a state is
looked up in a dense table of 2^L entries (L <= 26) or by bisection of the ascending states.  An XParity sector is the
first half of the parent's states (spin L-1 up) with the operator rewritten by XParity.reduce_msc, as
tests/test_gpu_layout_handles.py::_xparity_reference does.

tests/test_sc3_exact_ref.py pins this reference to the oracle, bit for bit, on every (operator, subspace) pair of
``pairs_used()``, and to tests/wide_ref.py at two tiny shapes."""
import functools

import numpy as np

import wide_ref
from dynamite_amd import lattices, msc_tools
from dynamite_amd.operators import sigmax, sigmay, sigmaz, op_sum
from dynamite_amd.subspaces import SpinConserve, XParity

LIMIT = 1 << 53                 # of units of 1/64
B8 = 3                          # b = 3/8
C8 = (-2, 5)                    # c = -1/4 + 5/8 i
B, CC = B8 / 8, complex(C8[0] / 8, C8[1] / 8)
CR8 = -2                        # real arithmetic: c = -1/4


# ---------------------------------------------------------------------------------------------------------------------
# states
# ---------------------------------------------------------------------------------------------------------------------

def sc_states(L, k):
    """The states of L spins with k set bits, ascending (the order of SpinConserve), as int64: level by level,
    S(n, j) = S(n-1, j) ++ (S(n-1, j-1) | 2^(n-1))."""
    empty = np.zeros(0, dtype=np.int64)
    prev = {0: np.zeros(1, dtype=np.int64)}
    for n in range(1, L + 1):
        cur = {}
        for j in range(max(0, k - (L - n)), min(k, n) + 1):
            lo = prev.get(j, empty)
            hi = prev.get(j - 1, empty) | np.int64(1 << (n - 1))
            cur[j] = np.concatenate([lo, hi])
        prev = cur
    out = prev[k]
    assert out.size == 1 or np.all(out[1:] > out[:-1])
    return out


def parity_of(v):
    """popcount(v) & 1 of an int64 array"""
    return (np.bitwise_count(v) & 1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# operators: multiples of 1/8, modulus at most 16 (wide_ref.terms_of asserts it)
# ---------------------------------------------------------------------------------------------------------------------

def _hop(i, j):
    return sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j)


def _dmt(i, j):
    return sigmax(i) * sigmay(j) - sigmay(i) * sigmax(j)


def chain_nnn(L):
    """wide_ref.chain plus next-nearest ZZ: diagonal terms that see Lo and the fields above it (the grouped diagonal)."""
    return wide_ref.chain(L) + op_sum(((5 * i) % 7 - 3 or 2) / 8 * sigmaz(i) * sigmaz(i + 2) for i in range(L - 2))


def chain_hops(L):
    """Symmetric hops alone: no diagonal (the DIAGM 0 instances), real symmetric."""
    return op_sum(wide_ref.bond_couplings(j)[0] / 8 * _hop(j, j + 1) for j in range(L - 1))


def chain_hops_dm(L):
    """Direction-dependent complex hops alone: no diagonal."""
    return chain_hops(L) + op_sum(wide_ref.bond_couplings(j)[1] / 8 * _dmt(j, j + 1) for j in range(L - 1))


def chain_long(L):
    """wide_ref.chain plus ZZ between all pairs: more mixed diagonal patterns than the on-the-fly diagonal takes, the
    handle needs the cached diagonal."""
    return wide_ref.chain(L) + op_sum(((i + 2 * j) % 5 - 2 or 1) / 8 * sigmaz(i) * sigmaz(j)
                                      for i in range(L) for j in range(i + 2, L))


def chain_xp(L):
    """A real symmetric chain without fields (fields anticommute with the global flip): hops and ZZ."""
    return op_sum(wide_ref.bond_couplings(j)[0] / 8 * _hop(j, j + 1) +
                  wide_ref.bond_couplings(j)[2] / 8 * sigmaz(j) * sigmaz(j + 1) for j in range(L - 1))


def kagome(name):
    """The kagome torus ``name`` with a different dyadic exchange and ZZ coupling per bond."""
    n, edges = lattices.kagome(name)
    return op_sum(((3 * e) % 11 - 5 or 4) / 8 * _hop(i, j) + ((5 * e) % 13 - 6 or 7) / 8 * sigmaz(i) * sigmaz(j)
                  for e, (i, j) in enumerate(edges))


def pair_graph(L, seed, nbonds=None, complex_hops=False, fields=True):
    """tests/test_gpu_sc3_graph.py::pair_graph with dyadic couplings: J (XX + YY) + Jz ZZ on random pairs (any distance),
    optionally D (XY - YX), optionally fields; J, Jz, D, h non-zero integers in [-8, 8] over 8."""
    rs = np.random.RandomState(seed)
    pairs = [(i, j) for i in range(L) for j in range(i + 1, L)]
    pick = rs.choice(len(pairs), size=min(len(pairs), nbonds or 2 * L), replace=False)
    eighth = lambda: int(rs.choice([-1, 1]) * rs.randint(1, 9)) / 8
    terms = []
    for q in pick:
        i, j = pairs[q]
        J, Jz, D = eighth(), eighth(), eighth()
        terms.append(J * _hop(i, j) + Jz * sigmaz(i) * sigmaz(j))
        if complex_hops:
            terms.append(D * _dmt(i, j))
    if fields:
        terms += [eighth() * sigmaz(i) for i in range(L)]
    return op_sum(terms)


def dense_lo(L):
    """All 91 pairs of the 14 Lo spins of the (14, 10) layout plus a chain through the rest (test_lo_hops_by_rank_tables):
    more LDS hops than the lo pass's partner table takes."""
    rs = np.random.RandomState(9)
    pairs = [(i, j) for i in range(14) for j in range(i + 1, 14)] + [(i, i + 1) for i in range(13, L - 1)]
    eighth = lambda: int(rs.choice([-1, 1]) * rs.randint(1, 5)) / 8
    return op_sum(eighth() * _hop(i, j) + eighth() * sigmaz(i) * sigmaz(j) for i, j in pairs)


def graph_xp(L):
    """A real bond graph without fields, for the XParity sectors: random pairs, plus bonds from spin L-1 -- whose hops
    come composed with the global flip -- to the first and the last spin of Lo and to a spin of W of the (6, 4) layout."""
    return pair_graph(L, seed=21, nbonds=2 * L + 2, complex_hops=False, fields=False) + \
        op_sum(c / 8 * _hop(i, L - 1) + d / 8 * sigmaz(i) * sigmaz(L - 1) for i, c, d in ((0, 3, -2), (5, -5, 1), (7, 2, 3)))


def lo_bits(L):
    """The Lo field of the layout the cases on L spins run in: 14 spins in the (14, 10) instances (L = 25), else 6."""
    return 14 if L >= 25 else 6


def fly_graph(L, groups, complex_hops):
    """A bond graph with fields whose diagonal the bond-graph passes evaluate ON THE FLY in the subspace's own labelling:
    hops J (XX + YY) (optionally D (XY - YX)) on random pairs at any distance, but ZZ only where it does not make a
    mixed pattern -- on pairs inside Lo or outside Lo -- plus ZZ bonds that cross out of Lo from exactly ``groups``
    (1 to 4) distinct Lo spins, the first, the last and two inner ones, each to a spin of W and to a spin of T.  The
    handle splits the diagonal into the Lo-only table, the (T, W) terms and ``groups`` patterns that see Lo through
    one spin (csrc/sc3_tables.cpp: split_diagonal; more than four would need the cached diagonal)."""
    a = lo_bits(L)
    w = 10 if a == 14 else 4
    rs = np.random.RandomState(100 * L + 10 * groups + complex_hops)
    pairs = [(i, j) for i in range(L) for j in range(i + 1, L)]
    pick = rs.choice(len(pairs), size=2 * L, replace=False)
    eighth = lambda: int(rs.choice([-1, 1]) * rs.randint(1, 9)) / 8
    terms = []
    for q in pick:
        i, j = pairs[q]
        J, Jz, D = eighth(), eighth(), eighth()
        terms.append(J * _hop(i, j))
        if (i < a) == (j < a):
            terms.append(Jz * sigmaz(i) * sigmaz(j))
        if complex_hops:
            terms.append(D * _dmt(i, j))
    for s in (0, a - 1, 2, 3)[:groups]:
        terms += [eighth() * sigmaz(s) * sigmaz(a + 1 + s % 2), eighth() * sigmaz(s) * sigmaz(min(L - 1, a + w + s % 2))]
    terms += [eighth() * sigmaz(i) for i in range(L)]
    return op_sum(terms)


OPERATORS = {
    # with fields, 2 / 3 / 4 mixed diagonal patterns: real, and (c) with XY - YX
    'fly2': lambda L: fly_graph(L, 2, False), 'fly3': lambda L: fly_graph(L, 3, False),
    'fly4': lambda L: fly_graph(L, 4, False), 'fly2c': lambda L: fly_graph(L, 2, True),
    'fly4c': lambda L: fly_graph(L, 4, True),
    'chain': wide_ref.chain, 'dm': wide_ref.dm, 'nnn': chain_nnn, 'hops': chain_hops, 'hops_dm': chain_hops_dm,
    'long': chain_long, 'chain_xp': chain_xp, 'graph_xp': graph_xp,
    'kagome12': lambda L: kagome("12"), 'kagome15': lambda L: kagome("15"), 'dense_lo': dense_lo,
    # the pair_graph family: with / without fields x with / without XY - YX
    'graph': lambda L: pair_graph(L, seed=10 * L, complex_hops=False, fields=False),
    'graph_f': lambda L: pair_graph(L, seed=10 * L + 1, complex_hops=False, fields=True),
    'graph_c': lambda L: pair_graph(L, seed=10 * L + 2, complex_hops=True, fields=False),
    'graph_cf': lambda L: pair_graph(L, seed=10 * L + 3, complex_hops=True, fields=True),
}
REAL_OPS = ('fly2', 'fly3', 'fly4', 'chain', 'nnn', 'hops', 'long', 'chain_xp', 'graph_xp', 'kagome12', 'kagome15',
            'dense_lo', 'graph', 'graph_f')
GRAPH_OPS = ('fly2', 'fly3', 'fly4', 'fly2c', 'fly4c', 'graph_xp', 'kagome12', 'kagome15', 'dense_lo', 'graph',
             'graph_f', 'graph_c', 'graph_cf')


def operator(name, L):
    """A fresh operator object of that name on L spins."""
    H = OPERATORS[name](L)
    H.L = L
    return H


# ---------------------------------------------------------------------------------------------------------------------
# one (operator, subspace) pair and its exact answers
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _states(L, k, half):
    """The states of SpinConserve(L, k), or the first half of them (spin L-1 up: the representatives of XParity)."""
    st = sc_states(L, k)
    if half:
        st = st[:st.size // 2]
        assert not (st >> (L - 1)).any()
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def _table(L, k, half):
    """index of every state of L spins in that subspace, -1 outside it (shared by the operators on it)"""
    st = _states(L, k, half)
    t = np.full(1 << L, -1, dtype=np.int32)
    t[st] = np.arange(st.size, dtype=np.int32)
    return t


class Ref:
    """Operator ``op`` on SpinConserve(L, k) (sector None) or on the XParity sector '+' / '-' of it.  ``arrs``: the
    operator's MSC arrays as dnm_mat_create receives them (reduced to the sector), ``terms``: the same in eighths."""

    def __init__(self, op, L, k, sector=None, arrs=None):
        self.op, self.L, self.k, self.sector = op, L, k, sector
        if arrs is None:
            H = operator(op, L)
            H.reduce_msc()
            msc = H.msc
            if sector is not None:
                msc = self.subspace().reduce_msc(msc)
            masks, offs = msc_tools.get_mask_offsets(msc)
            arrs = (np.ascontiguousarray(masks, dtype=np.int64), np.ascontiguousarray(offs, dtype=np.int64),
                    np.ascontiguousarray(msc['signs'], dtype=np.int64),
                    np.ascontiguousarray(msc['coeffs'], dtype=np.complex128))
        self.arrs = arrs
        self.terms = wide_ref.terms_of(arrs)
        assert sector is None or L == 2 * k
        self.states = _states(L, k, sector is not None)
        self.N = self.states.size
        # the largest sum over a row of |Re| + |Im| of its elements, in eighths: bounds the moduli of an entry's products
        self.rowsum8 = sum(sum(abs(r) + abs(i) for _, r, i in ts) for _, ts in self.terms)

    def subspace(self):
        """The dynamite_amd subspace (a fresh object: descriptors follow the process's layout knobs)."""
        sc = SpinConserve(self.L, self.k)
        return sc if self.sector is None else XParity(sc, self.sector)

    def index(self, states):
        """Index of each state in the subspace, -1 outside it."""
        if self.L <= 26:
            return _table(self.L, self.k, self.sector is not None)[states].astype(np.int64)
        pos = np.minimum(np.searchsorted(self.states, states), self.N - 1)
        return np.where(self.states[pos] == states, pos, -1)

    @staticmethod
    def _element(ts, bra):
        """The sum of a mask's terms on the column states ``bra``, in eighths: (re, im) int64 arrays."""
        re = np.zeros(bra.size, dtype=np.int64)
        im = np.zeros(bra.size, dtype=np.int64)
        for sg, cr, ci in ts:
            s = 1 - 2 * parity_of(bra & np.int64(sg))
            if cr:
                re += cr * s
            if ci:
                im += ci * s
        return re, im

    def apply8(self, xr, xi):
        """H x in eighths: (re, im) int64."""
        assert xr.shape == xi.shape == (self.N,) and xr.dtype == xi.dtype == np.int64
        yr = np.zeros(self.N, dtype=np.int64)
        yi = np.zeros(self.N, dtype=np.int64)
        for mask, ts in self.terms:
            if mask == 0:
                re, im = self._element(ts, self.states)
                yr += re * xr - im * xi
                yi += re * xi + im * xr
                continue
            if self.sector is None:       # the bra keeps k set bits iff half of the mask's bits are set in the ket
                rows = np.flatnonzero(np.bitwise_count(self.states & np.int64(mask)) * 2 == bin(mask).count('1'))
                bra = self.states[rows] ^ np.int64(mask)
                col = self.index(bra)
                assert rows.size == 0 or col.min() >= 0
            else:
                bra = self.states ^ np.int64(mask)
                col = self.index(bra)
                rows = np.flatnonzero(col >= 0)
                col, bra = col[rows], bra[rows]
            re, im = self._element(ts, bra)
            ar, ai = xr[col], xi[col]
            yr[rows] += re * ar - im * ai
            yi[rows] += re * ai + im * ar
        return yr, yi

    def rounding_reference(self, x):
        """For a vector of doubles: (Re y, Im y) of y = H x in numpy.longdouble (64 bits: every product exact, every sum
        rounded at 2^-64), the sums of the moduli of the products of each component, and per row the number of non-zero
        elements -- what a bound gamma(n) * sum |products| needs."""
        LD = np.longdouble
        xr, xi = x.real.astype(LD), x.imag.astype(LD)
        ar, ai = np.abs(xr), np.abs(xi)
        yr, yi, mr, mi = (np.zeros(self.N, dtype=LD) for _ in range(4))
        cnt = np.zeros(self.N, dtype=np.int64)
        for mask, ts in self.terms:
            if self.sector is None and mask:
                rows = np.flatnonzero(np.bitwise_count(self.states & np.int64(mask)) * 2 == bin(mask).count('1'))
                bra = self.states[rows] ^ np.int64(mask)
                col = self.index(bra)
            else:
                bra = self.states ^ np.int64(mask)
                col = self.index(bra)
                rows = np.flatnonzero(col >= 0)
                col, bra = col[rows], bra[rows]
            re, im = self._element(ts, bra)
            yr[rows] += (re * xr[col] - im * xi[col]) / 8
            yi[rows] += (re * xi[col] + im * xr[col]) / 8
            mr[rows] += (np.abs(re) * ar[col] + np.abs(im) * ai[col]) / 8
            mi[rows] += (np.abs(re) * ai[col] + np.abs(im) * ar[col]) / 8
            cnt[rows] += (re != 0) | (im != 0)
        return yr, yi, mr, mi, cnt

    def apply(self, x, z=None, z2=None, c8=C8, hx8=None):
        """y = H x - b z + c z2 exactly (z, z2 may be None) and the three fused sums of x and that y; b = 3/8,
        c = c8 / 8.  Asserts the 2^53 condition on the numbers of this case.  hx8: ``apply8`` of x, if at hand."""
        xr, xi = ints(x)
        yr, yi = self.apply8(xr, xi) if hx8 is None else (hx8[0].copy(), hx8[1].copy())
        amax = int(max(np.abs(xr).max(), np.abs(xi).max()))
        bound = self.rowsum8 * 2 * amax
        if z is not None:
            zr, zi = ints(z)
            yr -= B8 * zr
            yi -= B8 * zi
            bound += B8 * int(max(np.abs(zr).max(), np.abs(zi).max()))
        if z2 is not None:
            assert z is not None
            ur, ui = ints(z2)
            yr += c8[0] * ur - c8[1] * ui
            yi += c8[0] * ui + c8[1] * ur
            bound += (abs(c8[0]) + abs(c8[1])) * int(max(np.abs(ur).max(), np.abs(ui).max()))
        assert 8 * bound < LIMIT, (self.op, self.L, self.k, bound)
        y = np.empty(self.N, dtype=np.complex128)
        y.real = yr / 8.0
        y.imag = yi / 8.0
        return y, fused_sums8(xr, xi, yr, yi)

    def column(self, j):
        """Column j of H exactly: (rows, values) with one entry per mask whose bra ... is state j and whose row lies in
        the subspace (zero elements included), rows ascending and distinct."""
        s = int(self.states[j])
        acc = {}
        for mask, ts in self.terms:
            r = int(self.index(np.array([s ^ mask], dtype=np.int64))[0])
            if r < 0:
                continue
            re = im = 0
            for sg, cr, ci in ts:
                sign = -1 if bin(s & sg).count('1') & 1 else 1
                re, im = re + sign * cr, im + sign * ci
            a = acc.get(r, (0, 0))
            acc[r] = (a[0] + re, a[1] + im)
        rows = np.array(sorted(acc), dtype=np.int64)
        vals = np.array([complex(acc[r][0] / 8, acc[r][1] / 8) for r in rows.tolist()], dtype=np.complex128)
        return rows, vals


def ints(x):
    """(re, im) of a vector of Gaussian integers as int64; asserts that they are integers."""
    x = np.asarray(x, dtype=np.complex128)
    r, i = x.real.astype(np.int64), x.imag.astype(np.int64)
    assert np.array_equal(r, x.real) and np.array_equal(i, x.imag)
    return r, i


def fused_sums8(xr, xi, yr, yi):
    """(Re <x, y>, Im <x, y>, |y|^2) of an integer x and a y in eighths, <x, y> = sum conj(x_i) y_i, exact; asserts
    that the sum of the moduli of the terms of each -- what any partial sum in any order is bounded by -- stays below
    2^53 in units of 1/64."""
    ax, ay = np.abs(xr) + np.abs(xi), np.abs(yr) + np.abs(yi)
    assert float(ax.max()) * float(ay.max()) * ax.size < 2.0 ** 62       # (the int64 sums below cannot wrap)
    assert 8 * int(np.sum(ax * ay)) < LIMIT, 8 * int(np.sum(ax * ay)) / LIMIT
    dn = int(np.sum(yr * yr + yi * yi))
    assert dn < LIMIT, dn / LIMIT
    dr = int(np.sum(xr * yr + xi * yi))
    di = int(np.sum(xr * yi - xi * yr))
    return np.array([dr / 8, di / 8, dn / 64])


def int_vector(n, seed, amp=8, real=False):
    """Gaussian integers with parts in [-amp, amp] (``real``: integers) as complex128, vectorised."""
    rs = np.random.RandomState(seed)
    x = rs.randint(-amp, amp + 1, size=n).astype(np.float64) + 0j
    if not real:
        x.imag = rs.randint(-amp, amp + 1, size=n)
    return x


@functools.lru_cache(maxsize=None)
def get(op, L, k, sector=None):
    return Ref(op, L, k, sector)


AMP = {}


class Product:
    """x, z, z2 of a pair (integer vectors; ``real``: real ones) and the exact answers of every ABI entry, computed once
    and shared read-only: y and sums of  H x,  H x - b z,  H x - b z + c z2  (real: c = -1/4)."""

    def __init__(self, ref, real):
        n, amp = ref.N, AMP.get((ref.L, ref.k), 8)
        seed = 1000 * ref.L + 10 * ref.k + len(ref.op)
        self.x, self.z, self.z2 = (int_vector(n, seed + i, amp, real) for i in range(3))
        self.c8 = (CR8, 0) if real else C8
        self.c = complex(self.c8[0] / 8, self.c8[1] / 8)
        hx8 = ref.apply8(*ints(self.x))
        self.y, self.sums = ref.apply(self.x, hx8=hx8)
        self.y_z, self.sums_z = ref.apply(self.x, self.z, hx8=hx8)
        self.y_z2, _ = ref.apply(self.x, self.z, self.z2, self.c8, hx8=hx8)
        for a in (self.x, self.z, self.z2, self.y, self.y_z, self.y_z2, self.sums, self.sums_z):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def product(op, L, k, sector=None, real=False):
    return Product(get(op, L, k, sector), real)


def release():
    """Drop everything kept for sharing (a case of 5.2 million rows keeps 0.8 GB)."""
    for f in (product, get, _table, _states):
        f.cache_clear()


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_sc3_exact.py: (operator, L, k, sector, real) -- kept here so that the CPU test pins every
# reference the GPU file takes
# ---------------------------------------------------------------------------------------------------------------------

SMALL_SHAPES = [(11, 5), (12, 6), (13, 4), (14, 7), (12, 1), (12, 11), (12, 0), (12, 12)]
CHAIN_OPS = ('chain', 'dm', 'nnn', 'hops', 'hops_dm', 'long')
GRAPHS = ('graph', 'graph_f', 'graph_c', 'graph_cf')

# name -> (operator, L, k, sector, real)
CASES = {}
for _L, _k in SMALL_SHAPES:
    for _o in CHAIN_OPS + GRAPHS:
        CASES['%s-%d-%d' % (_o, _L, _k)] = (_o, _L, _k, None, False)
        if _o in REAL_OPS:
            CASES['%s-%d-%d-real' % (_o, _L, _k)] = (_o, _L, _k, None, True)
for _o in ('dm', 'chain', 'graph_cf'):
    CASES['%s-16-8' % _o] = (_o, 16, 8, None, False)
CASES['chain-16-8-real'] = ('chain', 16, 8, None, True)
for _n, _L, _k in (('kagome12', 12, 6), ('kagome15', 15, 7)):
    CASES['%s-%d-%d' % (_n, _L, _k)] = (_n, _L, _k, None, False)
    CASES['%s-%d-%d-real' % (_n, _L, _k)] = (_n, _L, _k, None, True)
for _s in '+-':
    for _o, _L in (('chain_xp', 14), ('graph_xp', 14), ('chain_xp', 22), ('graph_xp', 22)):
        CASES['%s-%d-%d%s' % (_o, _L, _L // 2, _s)] = (_o, _L, _L // 2, _s, False)
        CASES['%s-%d-%d%s-real' % (_o, _L, _L // 2, _s)] = (_o, _L, _L // 2, _s, True)
# the (14, 10) production instances
for _k in (3, 22):
    for _o, _r in (('dm', False), ('chain', True), ('graph_cf', False), ('graph_f', True), ('dense_lo', False)):
        CASES['%s-25-%d%s' % (_o, _k, '-real' if _r else '')] = (_o, 25, _k, None, _r)
CASES['dm-25-12'] = ('dm', 25, 12, None, False)
CASES['graph_f-25-12-real'] = ('graph_f', 25, 12, None, True)

# bond graphs whose diagonal is evaluated on the fly, on (6, 4) shapes and on the (14, 10) instance
FLY = {'fly2': 2, 'fly3': 3, 'fly4': 4, 'fly2c': 2, 'fly4c': 4}       # name -> mixed patterns
FLY_SHAPES = [(12, 6), (13, 4), (14, 7), (12, 11), (25, 3), (25, 22)]
for _o in FLY:
    for _L, _k in FLY_SHAPES:
        CASES['%s-%d-%d' % (_o, _L, _k)] = (_o, _L, _k, None, False)
        if _o in REAL_OPS:
            CASES['%s-%d-%d-real' % (_o, _L, _k)] = (_o, _L, _k, None, True)

PLANTED = [('dm', 13, 6, None), ('dm', 25, 3, None), ('graph_c', 13, 6, None), ('chain_xp', 14, 7, '-')]
SHARES = [('dm', 15, 7, None), ('dm', 16, 8, None)]


def pairs_used():
    """Every (operator, L, k, sector, real) the GPU tests take a reference for (planted columns and shares: complex)."""
    out = set(CASES.values()) | {p + (False,) for p in PLANTED + SHARES}
    return sorted(out, key=str)
