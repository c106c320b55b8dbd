"""Exact host reference for operators on WIDE subspaces of SMALL dimension: 33 to 63 spins, a few hundred to a few
thousand states (SpinConserve with two magnons or two holes, Explicit lists with states up to bit 62).  These are the
only shapes on which the row kernels walk positions above 32, shift by more than 31 and take parities of 63-bit words.

Everything here is plain Python: states are Python ``int`` (no fixed width anywhere), the inverse map is a dict, one
term is applied at a time from the MSC definition  H[row, col] += (-1)^popcount(bra & sign) * coeff,  bra = ket ^ mask,
col = index of bra in the right subspace (rows whose bra leaves it contribute nothing).

Every coefficient is a multiple of 1/8 and every amplitude a Gaussian integer, so the arithmetic is done in integers
(coefficients times 8) and divided by 8 at the end: the results are exact.  They are also what any double-precision
kernel must give bit for bit, in any order of summation and with or without fma, as long as every intermediate stays
below 2^53 in units of 1/64 -- ``EXACT_BOUND`` is that condition with room, tests/test_wide_ref.py asserts it.
Elements with both a real and an imaginary part are (3, 4) multiples, so that their modulus (the infinity norm sums
moduli) is a multiple of 5/8 and sqrt / hypot give it exactly.

tests/test_wide_ref.py pins these references against the oracle, bit for bit."""
import functools
import random
from math import comb, isqrt

import numpy as np

from dynamite_amd import msc_tools
from dynamite_amd.operators import sigmax, sigmay, sigmaz, sigma_plus, sigma_minus, op_sum, op_product
from dynamite_amd.subspaces import Explicit, SpinConserve

EXACT_BOUND = 2.0 ** 53 / 2.0 ** 10      # largest |y| entry and fused sum the exactness argument is taken to hold for

SC = {'sc63_2': (63, 2), 'sc63_61': (63, 61), 'sc63_1': (63, 1), 'sc63_62': (63, 62), 'sc50_2': (50, 2),
      'sc40_38': (40, 38), 'sc34_2': (34, 2), 'sc34_32': (34, 32), 'sc40_2': (40, 2)}
GLOBAL_TABLE = ('sc63_61', 'sc63_62')    # (k + 1) * (L + 1) > 2048: the binomial table stays in global memory
X_PRODUCT_SITES = 34                     # the sigma-x product of 'far' covers the lowest 34 sites


# ---------------------------------------------------------------------------------------------------------------------
# subspaces: (L, states in index order as Python ints)
# ---------------------------------------------------------------------------------------------------------------------

def sc_states(L, k):
    """The states of L spins with k set bits in ascending order (the colex order of SpinConserve), by Gosper's step."""
    if k == 0:
        return [0]
    out, x, top = [], (1 << k) - 1, 1 << L
    while x < top:
        out.append(x)
        c = x & -x
        r = x + c
        x = (((r ^ x) >> 2) // c) | r
    assert len(out) == comb(L, k)
    return out


def far_masks(L):
    """The non-zero masks of the 'far' operator on L spins (every bond, the two far hops, the four-site term, the
    sigma-x product)."""
    a, b, c, d = four_sites(L)
    return ([3 << j for j in range(L - 1)] + [1 | 1 << (L - 1), 1 << a | 1 << b | 1 << c | 1 << d,
                                              (1 << X_PRODUCT_SITES) - 1])


@functools.lru_cache(maxsize=None)
def exp63_states():
    """About 1500 sorted states below 2^63: 22 random seeds (one with bit 62 set, one below 2^16) and everything one
    mask of the 'far' operator makes of a seed, so that every kind of term has partners inside the list."""
    rng = random.Random(63)
    seeds = [rng.getrandbits(63) for _ in range(20)] + [rng.getrandbits(62) | 1 << 62, rng.getrandbits(16)]
    st = set(seeds)
    for s in seeds:
        st.update(s ^ m for m in far_masks(63))
    out = sorted(st)
    assert 1400 <= len(out) <= 1600 and out[-1] >> 62 == 1 and out[0] < 1 << 16 and out[-1] < 1 << 63
    return out


@functools.lru_cache(maxsize=None)
def exp40_outsider_states():
    """The states of SpinConserve(40, 2) plus 48 states of other magnetisation, sorted: what the sigma-x product of
    'far' makes of 24 of the sector's states (30 to 34 set bits), and 24 of them with one more spin flipped."""
    rng = random.Random(40)
    sector = sc_states(40, 2)
    picks = rng.sample(sector, 24)
    extra = {s ^ ((1 << X_PRODUCT_SITES) - 1) for s in picks} | {s ^ (1 << rng.randrange(40)) for s in rng.sample(sector, 24)}
    assert len(extra) == 48 and not extra & set(sector)
    return sorted(set(sector) | extra)


@functools.lru_cache(maxsize=None)
def states_of(name):
    """(L, states in index order) of a subspace by name."""
    if name in SC:
        return SC[name][0], sc_states(*SC[name])
    if name == 'exp63':
        return 63, exp63_states()
    if name == 'exp63_unsorted':
        st = list(exp63_states())
        random.Random(7).shuffle(st)
        return 63, st
    assert name == 'exp40_outsiders', name
    return 40, exp40_outsider_states()


def subspace(name):
    """The dynamite_amd subspace of that name (a fresh object: descriptors follow the process's layout knobs)."""
    if name in SC:
        return SpinConserve(*SC[name])
    L, st = states_of(name)
    return Explicit(np.array(st, dtype=np.int64), L=L)


# ---------------------------------------------------------------------------------------------------------------------
# operators: multiples of 1/8, magnitude at most 16
# ---------------------------------------------------------------------------------------------------------------------

def four_sites(L):
    """The sites of the four-site term: (0, 17, 33, L - 1); at L = 34 the third one moves down to 32."""
    return 0, 17, min(33, L - 2), L - 1


def bond_couplings(j):
    """(J, D, Jz) of bond j in eighths: J and D a (3, 4) multiple that grows along the chain (so |2J + 2iD| = 10 m / 8
    exactly), Jz = +-(j + 1): no two bonds alike."""
    m = 1 + j // 2
    J, D = (3 * m, 4 * m) if j % 2 == 0 else (-4 * m, 3 * m)
    return J, D, (j + 1) * (-1 if j % 3 == 1 else 1)


def field(i):
    return (3 * i) % 17 - 8


def chain(L):
    """XX + YY + ZZ bonds with a different coupling per bond and a field per site (adjacent bonds only)."""
    hop = lambda i, j: sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j)
    H = op_sum(bond_couplings(j)[0] / 8 * hop(j, j + 1) + bond_couplings(j)[2] / 8 * sigmaz(j) * sigmaz(j + 1)
               for j in range(L - 1))
    return H + op_sum(field(i) / 8 * sigmaz(i) for i in range(L) if field(i))


def dm(L):
    """The chain plus XY - YX on every bond: imaginary coefficients, an up / down element pair that are conjugates."""
    return chain(L) + op_sum(bond_couplings(j)[1] / 8 * (sigmax(j) * sigmay(j + 1) - sigmay(j) * sigmax(j + 1))
                             for j in range(L - 1))


def far(L, x_product=None):
    """The chain plus a hop between sites 0 and L-1, a second hop on bond (15, 16) -- it straddles the 16-bit unranking
    table -- a ZZ between sites 0 and L-1, sigma+ sigma- sigma+ sigma- + h.c. on ``four_sites`` and (x_product; default:
    L <= 40) the product of sigma-x over the lowest 34 sites.  All real."""
    hop = lambda i, j: sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j)
    a, b, c, d = four_sites(L)
    quad = op_product([sigma_plus(a), sigma_minus(b), sigma_plus(c), sigma_minus(d)])
    quad = quad + op_product([sigma_minus(a), sigma_plus(b), sigma_minus(c), sigma_plus(d)])
    H = chain(L) + 0.625 * hop(0, L - 1) + 1.75 * hop(15, 16) + (-1.375) * sigmaz(0) * sigmaz(L - 1) + 0.125 * quad
    if x_product is None:
        x_product = L <= 40
    if x_product:
        H = H + 0.875 * op_product(sigmax(i) for i in range(X_PRODUCT_SITES))
    return H


OPERATORS = {'chain': chain, 'dm': dm, 'far': far}


def marshal(H, L):
    """(masks, mask_offsets, signs, coeffs) of an operator, as dnm_mat_create receives them."""
    H.L = L
    H.reduce_msc()
    masks, offs = msc_tools.get_mask_offsets(H.msc)
    return (np.ascontiguousarray(masks, dtype=np.int64), np.ascontiguousarray(offs, dtype=np.int64),
            np.ascontiguousarray(H.msc['signs'], dtype=np.int64), np.ascontiguousarray(H.msc['coeffs'], dtype=np.complex128))


def terms_of(arrs):
    """[(mask, [(sign, 8 Re c, 8 Im c), ...]), ...] in Python ints; asserts the coefficients are eighths."""
    masks, offs, signs, coeffs = arrs
    out = []
    for i in range(len(masks)):
        ts = []
        for t in range(int(offs[i]), int(offs[i + 1])):
            re8, im8 = float(coeffs[t].real) * 8, float(coeffs[t].imag) * 8
            assert re8 == int(re8) and im8 == int(im8) and abs(coeffs[t]) <= 16, coeffs[t]
            ts.append((int(signs[t]), int(re8), int(im8)))
        out.append((int(masks[i]), ts))
    return out


def popcount(v):
    return bin(v).count('1')


# ---------------------------------------------------------------------------------------------------------------------
# one (left, right, operator) case and its exact answers
# ---------------------------------------------------------------------------------------------------------------------

class Case:
    """An operator between two named subspaces.  ``rows[r]``: the matrix elements of row r as (column, 8 Re, 8 Im), one
    per mask whose bra lies in the right subspace (zero elements included: they are reached, not needed)."""

    def __init__(self, left, right, op, arrs):
        self.left, self.right, self.op = left, right, op
        self.arrs = arrs
        self.terms = terms_of(arrs)
        self.L, self.lstates = states_of(left)
        Lr, self.rstates = states_of(right)
        assert Lr == self.L
        self.M, self.N = len(self.lstates), len(self.rstates)
        rindex = {s: i for i, s in enumerate(self.rstates)}
        self.rows = []
        for ket in self.lstates:
            row = []
            for mask, ts in self.terms:
                bra = ket ^ mask
                col = rindex.get(bra)
                if col is None:
                    continue
                re = im = 0
                for sg, cr, ci in ts:
                    if popcount(bra & sg) & 1:
                        re, im = re - cr, im - ci
                    else:
                        re, im = re + cr, im + ci
                row.append((col, re, im))
            self.rows.append(row)

    @property
    def nmasks(self):
        return len(self.terms)

    def subspaces(self):
        return subspace(self.left), subspace(self.right)


@functools.lru_cache(maxsize=None)
def case(left, op, right=None, extra=None):
    """The case of operator ``op`` ('chain', 'dm', 'far') from ``right`` (default: left) to ``left``.
    extra = 'xtop': plus a single sigma-x on the top site, L - 1 (site 62 of 63 spins): it takes every state out of a
    magnetisation sector."""
    right = right or left
    L = states_of(left)[0]
    H = OPERATORS[op](L)
    if extra == 'xtop':
        H = H + 0.5 * sigmax(L - 1)
    else:
        assert extra is None
    return Case(left, right, op, marshal(H, L))


def int_vector(n, seed):
    """Gaussian integers in [-8, 8] as complex128."""
    rng = random.Random(seed)
    return np.array([complex(rng.randint(-8, 8), rng.randint(-8, 8)) for _ in range(n)], dtype=np.complex128)


def _ints(x):
    out = []
    for v in x:
        r, i = int(v.real), int(v.imag)
        assert r == v.real and i == v.imag
        out.append((r, i))
    return out


def apply(c, x, row0=0, m=None):
    """Rows [row0, row0 + m) of H x, exact: integer arithmetic in eighths, one division at the end."""
    xs = _ints(x)
    assert len(xs) == c.N
    m = c.M - row0 if m is None else m
    y = np.empty(m, dtype=np.complex128)
    for r in range(m):
        yr = yi = 0
        for col, re, im in c.rows[row0 + r]:
            xr, xi = xs[col]
            yr += re * xr - im * xi
            yi += re * xi + im * xr
        assert abs(yr) < 1 << 53 and abs(yi) < 1 << 53
        y[r] = complex(yr / 8, yi / 8)
    return y


def row_sums(c):
    """sum over the masks of |element| of every row, exact: every element here has an integer modulus in eighths."""
    out = []
    for row in c.rows:
        s = 0
        for _, re, im in row:
            q = re * re + im * im
            a = isqrt(q)
            assert a * a == q, (re, im)
            s += a
        out.append(s / 8)
    return out


def infnorm(c):
    return max(row_sums(c))


def diagonal(c):
    """The terms of mask 0 on each state of the left subspace."""
    assert c.terms[0][0] == 0 and all(im == 0 for _, _, im in c.terms[0][1])
    out = np.empty(c.M)
    for r, ket in enumerate(c.lstates):
        d = 0
        for sg, cr, _ in c.terms[0][1]:
            d += -cr if popcount(ket & sg) & 1 else cr
        out[r] = d / 8
    return out


def conserves(c):
    """(verdict, violating columns): a column violates when some mask takes its state out of the LEFT subspace with a
    non-zero sum of that mask's terms (CheckConserves looks from the right subspace)."""
    lset = set(c.lstates)
    bad = []
    for j, bra in enumerate(c.rstates):
        for mask, ts in c.terms:
            if bra ^ mask in lset:
                continue
            re = im = 0
            for sg, cr, ci in ts:
                s = -1 if popcount(bra & sg) & 1 else 1
                re, im = re + s * cr, im + s * ci
            if re or im:
                bad.append(j)
                break
    return not bad, bad


def column_sets(c, row0, m):
    """(reach, need) of the rows [row0, row0 + m): every column some mask reaches, and those with a non-zero element."""
    reach, need = set(), set()
    for row in c.rows[row0:row0 + m]:
        for col, re, im in row:
            reach.add(col)
            if re or im:
                need.add(col)
    return sorted(reach), sorted(need)


def fused_sums(x, y):
    """(Re <x, y>, Im <x, y>, |y|^2) of an integer x and a y in eighths, exact."""
    xs = _ints(x)
    ys = _ints(np.asarray(y) * 8)
    dr = sum(a * c + b * d for (a, b), (c, d) in zip(xs, ys))
    di = sum(a * d - b * c for (a, b), (c, d) in zip(xs, ys))
    dn = sum(c * c + d * d for c, d in ys)
    assert max(abs(dr), abs(di)) < 1 << 53 and dn < 1 << 53
    return np.array([dr / 8, di / 8, dn / 64])


# ---------------------------------------------------------------------------------------------------------------------
# the handles the GPU tests multiply on (tests/test_wide_sectors_host.py builds every one of them on the host)
# ---------------------------------------------------------------------------------------------------------------------

OPERATORS['farx'] = lambda L: far(L, x_product=True)      # Explicit lists hold partners under the product at any L

SC_NAMES = ('sc63_2', 'sc63_61', 'sc63_1', 'sc63_62', 'sc50_2', 'sc40_38', 'sc34_2', 'sc34_32')
FUSED_SUBS = ('sc63_2', 'sc63_61', 'sc40_38')
SWEEP_SUBS = ('sc63_2', 'sc63_61', 'sc40_38', 'exp63')
RECT = ('sc40_2', 'exp40_outsiders')                       # (left, right) of the rectangular pair
FORCE_GATHER = 1                                           # DNM_MAT_FORCE_GATHER

ROWS, GATHER, BLOCK = 'one row per thread', 'row-gather', 'block form'      # what dnm_mat_plan_describe says

# name -> (left, right, operator, flags, knobs, route)
HANDLES = {}
for _s in SC_NAMES:
    for _o in ('chain', 'dm', 'far'):
        HANDLES['rows-%s-%s' % (_s, _o)] = (_s, _s, _o, 0, {}, ROWS)
for _s in FUSED_SUBS:
    HANDLES['unfused-%s-dm' % _s] = (_s, _s, 'dm', 0, {'DNM_ROW_FUSE': '0'}, ROWS)
    for _o in ('dm', 'far'):
        HANDLES['gather-%s-%s' % (_s, _o)] = (_s, _s, _o, FORCE_GATHER, {}, GATHER)
for _s in ('exp63', 'exp63_unsorted'):
    for _o in ('dm', 'farx'):
        HANDLES['gather-%s-%s' % (_s, _o)] = (_s, _s, _o, 0, {}, GATHER)
HANDLES['gather-exp63-farx-two-buckets'] = ('exp63', 'exp63', 'farx', 0, {'DNM_BUCKET_BITS': '1'}, GATHER)
for _o in ('dm', 'far'):
    HANDLES['gather-rect-%s' % _o] = (RECT[0], RECT[1], _o, 0, {}, GATHER)
    HANDLES['gather-rect-transposed-%s' % _o] = (RECT[1], RECT[0], _o, 0, {}, GATHER)
for _s in ('sc34_2', 'sc34_32'):
    for _o in ('chain', 'dm'):
        HANDLES['block-%s-%s' % (_s, _o)] = (_s, _s, _o, 0, {'DNM_SC_BLOCK': '13'}, BLOCK)


def pairs_used():
    """Every (left, operator, right, extra) the GPU tests take a reference for."""
    out = {(l, o, r, None) for l, r, o, _, _, _ in HANDLES.values()}
    out |= {(s, 'chain', s, x) for s in SWEEP_SUBS for x in (None, 'xtop')}
    out |= {(RECT[0], 'chain', RECT[1], None), (RECT[1], 'chain', RECT[0], None)}
    out |= {(s, 'far', s, None) for s in ('sc63_2', 'sc50_2')}
    return sorted(out, key=str)


@functools.lru_cache(maxsize=None)
def product(left, op, right=None, extra=None):
    """(x, H x) of a case on its integer vector, computed once and shared (read-only)."""
    c = case(left, op, right, extra)
    x = int_vector(c.N, seed=c.N + len(op))
    y = apply(c, x)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y
