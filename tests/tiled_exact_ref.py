"""Exact host reference for the tiled multiply of Full and Parity subspaces (csrc/matvec_kernels.hip: tile_pass_body,
tile_pass_kernel, tile_pass_flip_kernel):  y = H x - b z + c z2  and the fused sums (Re <x, y>, Im <x, y>, |y|^2).

The conventions are those of tests/sc3_exact_ref.py: every coefficient is a multiple of 1/8 of modulus at most 16, every
amplitude a Gaussian integer with parts in [-8, 8], b = 3/8, c = -1/4 + 5/8 i (real arithmetic: c = -1/4); the arithmetic
is done in int64 on arrays of states, in eighths, one mask at a time, and divided once at the end.  While a case is
computed ``Ref.apply`` ASSERTS that the sum of the moduli of all products of every entry of y, and of the terms of each
fused sum, stays below 2^53 in units of 1/64 (OutOfExactRange otherwise): any order of summation, any grouping of a
mask's terms into records or tables and any fma contraction then gives the same VALUE.  The per-entry sum is taken over the TERMS (not the elements)
and doubled: the kernels add a mask's terms two or sixteen at a time, and the flip-flop form of a bond a (XX + YY) + d ZZ
evaluates (d - a) ZZ - a + 2a [exchange], whose moduli exceed those of the terms by at most 2 |a| per bond.

Operators are written down directly as MSC arrays (mask, sign, coefficient: H[row, col] += (-1)^popcount(col & sign) *
coeff, col = row ^ mask) from Pauli strings -- a Y contributes a factor i, so a string with an odd number of Ys has an
imaginary coefficient, as dnm_mat_create expects.  No model constructor of the package is used: theirs are not dyadic.

tests/test_tiled_exact_ref.py pins this reference to the oracle on every (operator, subspace, arithmetic) triple the
GPU file uses."""
import functools

import numpy as np

LIMIT = 1 << 53                 # of units of 1/64
B8 = 3                          # b = 3/8
C8 = (-2, 5)                    # c = -1/4 + 5/8 i
CR8 = (-2, 0)                   # real arithmetic: c = -1/4
B = B8 / 8


class OutOfExactRange(Exception):
    """a partial sum of the case could leave the integers below 2^53 in units of 1/64"""


def parity_of(v):
    return (np.bitwise_count(v) & 1).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# Pauli strings -> MSC arrays
# ---------------------------------------------------------------------------------------------------------------------

def P(c8, x=(), y=(), z=()):
    """c8 / 8 times the product of X on the sites ``x``, Y on ``y`` and Z on ``z`` (disjoint): (mask, sign, 8 Re, 8 Im)."""
    x, y, z = tuple(x), tuple(y), tuple(z)
    assert len(set(x + y + z)) == len(x + y + z)
    mask = sum(1 << s for s in x + y)
    sign = sum(1 << s for s in y + z)
    ph = (1, 1j, -1, -1j)[len(y) % 4] * c8
    return mask, sign, int(ph.real), int(ph.imag)


def msc(strings):
    """MSC arrays (masks, mask_offsets, signs, coeffs) of a list of P(...): equal (mask, sign) summed, zeros dropped,
    masks ascending and the terms of a mask by ascending sign."""
    acc = {}
    for m, s, re, im in strings:
        a = acc.get((m, s), (0, 0))
        acc[(m, s)] = (a[0] + re, a[1] + im)
    keys = sorted(k for k, v in acc.items() if v != (0, 0))
    masks = sorted({k[0] for k in keys})
    offs, signs, coeffs = [0], [], []
    for m in masks:
        for k in keys:
            if k[0] == m:
                re, im = acc[k]
                assert re * re + im * im <= (16 * 8) ** 2
                assert (re == 0) == bool(bin(m & k[1]).count('1') & 1) and (re == 0 or im == 0)
                signs.append(k[1])
                coeffs.append(complex(re / 8, im / 8))
        offs.append(len(signs))
    return (np.array(masks, dtype=np.int64), np.array(offs, dtype=np.int64), np.array(signs, dtype=np.int64),
            np.array(coeffs, dtype=np.complex128))


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


# ---------------------------------------------------------------------------------------------------------------------
# operators: coefficients in eighths, no two bonds alike
# ---------------------------------------------------------------------------------------------------------------------

def _J(j):
    """hop of bond j in eighths (a of a (XX + YY)): non-zero, sign and size change along the chain"""
    return ((3 * j) % 7 + 1) * (-1 if j % 3 == 1 else 1)


def _hop(a8, i, j):
    return [P(a8, x=(i, j)), P(a8, y=(i, j))]


def _dm(d8, i, j):
    return [P(d8, x=(i,), y=(j,)), P(-d8, y=(i,), x=(j,))]


def _field(i):
    return (5 * i) % 17 - 8


def chain(L):
    """a (XX + YY) + d ZZ on adjacent sites plus fields: d = a on every third bond (an isotropic bond: its ZZ term leaves
    the diagonal of the flip-flop form altogether), else another value; the planner runs the bonds as flip-flop records."""
    s = []
    for j in range(L - 1):
        s += _hop(_J(j), j, j + 1)
        s.append(P(_J(j) if j % 3 == 0 else (j % 5) + 1 - 2 * _J(j), z=(j, j + 1)))
    return s + [P(_field(i), z=(i,)) for i in range(L) if _field(i)]


def hops(L):
    """The chain without ZZ and without fields: no diagonal at all, FP.dconst = 0"""
    s = []
    for j in range(L - 1):
        s += _hop(_J(j), j, j + 1)
    return s


def dm(L):
    """The chain plus D (XY - YX) on every bond: complex hops"""
    s = chain(L)
    for j in range(L - 1):
        s += _dm(((2 * j) % 5 + 1) * (-1 if j % 2 else 1), j, j + 1)
    return s


def long_range(L):
    """ZZ between all pairs, a field and an X on every site: many diagonal terms outside the tile, across its boundary
    and on the k bits (dext, every dbucket slot, the Walsh-Hadamard butterfly), single-flip masks off the diagonal"""
    s = [P(((i + 2 * j) % 9 - 4) or 3, z=(i, j)) for i in range(L) for j in range(i + 1, L)]
    s += [P(_field(i) or 1, z=(i,)) for i in range(L)]
    s += [P((i % 4) + 1, x=(i,)) for i in range(L)]
    return s


def nnn(L):
    """The chain plus ZZ at distances 2 and 3: three terms and more share their sign mask inside a tile and differ
    outside it -- what the planner sums once per workgroup (grouped diagonal, DevPass::gbucket)"""
    s = chain(L)
    s += [P(((5 * i) % 7 - 3) or 2, z=(i, i + 2)) for i in range(L - 2)]
    s += [P(((3 * i) % 5 - 2) or 4, z=(i, i + 3)) for i in range(L - 3)]
    return s


def syk_like(L):
    """Many terms per mask: for a few masks of one to four flipped sites -- low sites, the top sites, mixed -- every
    choice of X or Y on the flipped sites times a few Z dressings, all with different dyadic coefficients, real and
    imaginary: what the planner runs as table records (plan.h: DevTab).  A ZZ chain and fields for a diagonal."""
    rs = np.random.RandomState(7 * L)
    c = lambda: int(rs.choice([-1, 1]) * rs.randint(1, 9))
    groups = [((0,), 3), ((L - 1,), 3), ((1, 2), 2), ((3, L - 2), 2), ((L - 3, L - 1), 2), ((0, 4, 5), 1),
              ((2, L - 2, L - 1), 1), ((1, 3, L // 2), 2), ((0, 1, 2, 3), 1), ((4, 5, L - 2, L - 1), 1),
              ((2, L // 2, L // 2 + 1, L - 1), 1)]
    s = []
    for sites, ndress in groups:
        rest = [q for q in range(L) if q not in sites]
        for d in range(ndress):
            zs = tuple(rest[(3 * d + 2 * i) % len(rest)] for i in range(d))          # 0, 1, 2 dressing sites
            zs = tuple(sorted(set(zs)))
            for sel in range(1 << len(sites)):
                ys = tuple(q for b, q in enumerate(sites) if (sel >> b) & 1)
                xs = tuple(q for q in sites if q not in ys)
                s.append(P(c(), x=xs, y=ys, z=zs))
    s += [P((j % 4) + 1, z=(j, j + 1)) for j in range(L - 1)]
    s += [P(_field(i), z=(i,)) for i in range(L) if _field(i)]
    return s


def xstring(L):
    """X strings whose masks touch thread bits, k bits and bits outside the tile at once, some with Z dressings (sign
    masks on the k bits: k-variant records) and some with a pair of Ys; plus one Y string (imaginary)."""
    h = L // 2
    s = [P(5, x=range(L)), P(-3, x=range(0, L, 2)), P(2, x=range(1, L, 2), z=(0,)),
         P(7, x=(0, h, L - 1)), P(-6, x=(0, h, L - 1), z=(1, L - 2)), P(4, x=(1, 7, L - 1), z=(L - 2,)),
         P(3, x=(2, L - 2), y=(h, L - 1)), P(-1, x=(6, 7)), P(1, x=(6, 7), z=(L - 1,)), P(2, x=(L - 3,), z=(L - 1, 0)),
         P(3, y=(0,), x=(h, L - 1)), P(-2, y=(L - 1,), z=(3,)), P(6, x=(h,)), P(-5, x=(h, h + 1), z=(h - 1,))]
    return s + [P(_field(i), z=(i,)) for i in range(L) if _field(i)] + [P(2, z=(0, L - 1))]


def pk_flip0(L):
    """Real symmetric, for real-packed handles: terms that flip site 0 ALONE -- a lane swap inside one element"""
    s = [P(3, x=(0,)), P(-2, x=(0,), z=(1,)), P(5, x=(0,), z=(L - 1,)), P(1, x=(0,), z=(4, L - 2)), P(4, x=(0,), z=(L // 2,))]
    return s + [P(_field(i), z=(i,)) for i in range(1, L) if _field(i)] + [P(2, z=(j, j + 1)) for j in range(1, L - 1)]


def pk_flip0x(L):
    """Real symmetric: terms that flip site 0 together with one other site, inside the tile and outside it"""
    s = []
    for j, a in ((1, 3), (2, -5), (5, 2), (L // 2, 7), (L - 2, -1), (L - 1, 4)):
        s += [P(a, x=(0, j)), P(a - 1 or 2, y=(0, j))]
    s += [P(-3, x=(0, 3), z=(L - 1,)), P(2, x=(0, L - 1), z=(2, 3))]
    return s + [P(_field(i), z=(i,)) for i in range(L) if _field(i)] + [P(3, z=(j, j + 1)) for j in range(L - 1)]


def pk_sign0(L):
    """Real symmetric: sign bits on site 0 and no flip of site 0 -- the two lanes of an element get opposite signs"""
    s = [P(4, z=(0,)), P(-3, z=(0, 1)), P(2, z=(0, L - 1)), P(1, z=(0, L // 2)), P(5, z=(0, 2, 3)),
         P(3, x=(1,), z=(0,)), P(-2, x=(L - 1,), z=(0,)), P(6, x=(2, 3), z=(0,)), P(-4, x=(3, L - 2), z=(0, L - 1)),
         P(2, y=(1, L - 1), z=(0,)), P(1, x=(L // 2,), z=(0, 1)), P(7, x=(4,)), P(-1, x=(L - 2, L - 1))]
    return s + [P(_field(i), z=(i,)) for i in range(1, L) if _field(i)]


def dsel(L):
    """The chain plus ZZ(6, 9) and ZZ(5, 10): across the boundary of a tile [0, 8) they and the chain's own ZZ(7, 8) have
    three distinct parts outside and three distinct parts inside -- no group, MAXDSEL selector masks of the table form"""
    assert L >= 11
    return chain(L) + [P(3, z=(6, 9)), P(-5, z=(5, 10))]


def dext(L):
    """Hops everywhere, diagonal terms on the sites 8 and above only: outside a tile [0, 8) -- the dext list alone"""
    assert L >= 10
    return hops(L) + [P(_field(i) or 2, z=(i,)) for i in range(8, L)] + [P(3, z=(j, j + 1)) for j in range(8, L - 1)]


def low8(L):
    """The chain on the sites 0 .. 7 of a longer register: nothing couples the tiles [0, 8) to each other"""
    assert L > 8
    return chain(8)


def low12(L):
    """The chain with complex hops on the sites 0 .. 11 of a longer register"""
    assert L > 12
    return dm(12)


OPERATORS = {'low8': low8, 'low12': low12, 'dsel': dsel, 'dext': dext, 'chain': chain, 'hops': hops, 'dm': dm, 'long_range': long_range, 'nnn': nnn, 'syk': syk_like,
             'xstring': xstring, 'pk_flip0': pk_flip0, 'pk_flip0x': pk_flip0x, 'pk_sign0': pk_sign0}
REAL_OPS = ('chain', 'hops', 'long_range', 'nnn', 'pk_flip0', 'pk_flip0x', 'pk_sign0', 'dsel', 'dext', 'low8')


@functools.lru_cache(maxsize=None)
def arrays(op, L):
    a = msc(OPERATORS[op](L))
    for v in a:
        v.setflags(write=False)
    return a


# ---------------------------------------------------------------------------------------------------------------------
# subspaces: ('full',), ('parity', space)
# ---------------------------------------------------------------------------------------------------------------------

def sub_dim(sub, L):
    return 1 << (L if sub[0] == 'full' else L - 1)


def sub_states(sub, L):
    i = np.arange(sub_dim(sub, L), dtype=np.int64)
    return i if sub[0] == 'full' else (i << 1) | (parity_of(i) ^ sub[1])


def sub_index(sub, L, st):
    """index of each state, -1 outside the subspace"""
    if sub[0] == 'full':
        return st
    return np.where(parity_of(st) == sub[1], st >> 1, -1)


def ints(x):
    x = np.asarray(x, dtype=np.complex128)
    r, i = x.real.astype(np.int64), x.imag.astype(np.int64)
    assert np.array_equal(r, x.real) and np.array_equal(i, x.imag)
    return r, i


def int_vector(n, seed, amp=8, real=False):
    rs = np.random.RandomState(seed)
    x = rs.randint(-amp, amp + 1, size=n).astype(np.float64) + 0j
    if not real:
        x.imag = rs.randint(-amp, amp + 1, size=n)
    return x


def fused_sums8(xr, xi, yr, yi):
    """(Re <x, y>, Im <x, y>, |y|^2) of an integer x and a y in eighths, exact; asserts that the sum of the moduli of the
    terms of each stays below 2^53 in units of 1/64."""
    ax, ay = np.abs(xr) + np.abs(xi), np.abs(yr) + np.abs(yi)
    assert float(ax.max()) * float(ay.max()) * ax.size < 2.0 ** 62
    if not (8 * int(np.sum(ax * ay)) < LIMIT and int(np.sum(ay * ay)) < LIMIT):
        raise OutOfExactRange("a fused sum")
    dn = int(np.sum(yr * yr + yi * yi))
    dr = int(np.sum(xr * yr + xi * yi))
    di = int(np.sum(xr * yi - xi * yr))
    return np.array([dr / 8, di / 8, dn / 64])


class Ref:
    """Operator ``op`` on L spins from the subspace ``right`` to ``left`` (default: the same)."""

    def __init__(self, op, L, left=('full',), right=None, arrs=None):
        self.op, self.L, self.left, self.right = op, L, left, right or left
        self.arrs = arrays(op, L) if arrs is None else arrs
        self.terms = terms_of(self.arrs)
        self.M, self.N = sub_dim(self.left, L), sub_dim(self.right, L)
        self.rows = sub_states(self.left, L)
        self.square = self.left == self.right

    def _element(self, ts, bra):
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
        """(Re, Im) of H x in eighths and, per row, the sum over the TERMS of |coefficient| |x_col|_1 in eighths."""
        assert xr.shape == xi.shape == (self.N,)
        yr = np.zeros(self.M, dtype=np.int64)
        yi = np.zeros(self.M, dtype=np.int64)
        mod = np.zeros(self.M, dtype=np.int64)
        ax = np.abs(xr) + np.abs(xi)
        for mask, ts in self.terms:
            bra = self.rows ^ np.int64(mask)
            col = sub_index(self.right, self.L, bra)
            if col.min() < 0:
                rows = np.flatnonzero(col >= 0)
                if rows.size == 0:
                    continue
                col, bra = col[rows], bra[rows]
            else:
                rows = slice(None)
            re, im = self._element(ts, bra)
            ar, ai = xr[col], xi[col]
            yr[rows] += re * ar - im * ai
            yi[rows] += re * ai + im * ar
            mod[rows] += sum(abs(cr) + abs(ci) for _, cr, ci in ts) * ax[col]
        return yr, yi, mod

    def apply(self, x, z=None, z2=None, c8=C8, hx8=None):
        """y = H x - b z + c z2 exactly and the three fused sums of x and that y (square handles); asserts the 2^53
        condition per row and per sum on the numbers of this case."""
        xr, xi = ints(x)
        yr, yi, mod = self.apply8(xr, xi) if hx8 is None else (hx8[0].copy(), hx8[1].copy(), hx8[2].copy())
        mod = 2 * mod
        if z is not None:
            zr, zi = ints(z)
            yr -= B8 * zr
            yi -= B8 * zi
            mod += B8 * (np.abs(zr) + np.abs(zi))
        if z2 is not None:
            assert z is not None
            ur, ui = ints(z2)
            yr += c8[0] * ur - c8[1] * ui
            yi += c8[0] * ui + c8[1] * ur
            mod += (abs(c8[0]) + abs(c8[1])) * (np.abs(ur) + np.abs(ui))
        if not 8 * int(mod.max()) < LIMIT:
            raise OutOfExactRange("a row of %s, L = %d: %d" % (self.op, self.L, int(mod.max())))
        y = np.empty(self.M, dtype=np.complex128)
        y.real = yr / 8.0
        y.imag = yi / 8.0
        return y, (fused_sums8(xr, xi, yr, yi) if self.square else None)

    def column(self, j):
        """Column j of H exactly, dense: complex128[M]"""
        e = np.zeros(self.N, dtype=np.int64)
        e[j] = 1
        yr, yi, _ = self.apply8(e, np.zeros_like(e))
        return (yr + 1j * yi) / 8.0

    def rounding_reference(self, x, exchanges=()):
        """For a vector of doubles: (Re y, Im y) of y = H x in numpy.longdouble, the sums of the moduli of the products
        that go into each component, and per row the number n of fused multiply-adds of a component.
        The diagonal is ONE product per row, D(row) x_row: the kernels sum the (dyadic) diagonal terms exactly before they
        multiply.  Off the diagonal the moduli are summed over the TERMS, which bounds every grouping of a mask's terms
        into records and tables, and a term counts one fma if its coefficient is real and two if it is imaginary.
        ``exchanges``: [(mask, c8)] of the bonds a handle runs as flip-flop exchanges (c = 2a): on the rows whose two
        bits differ the product is c x_partner, as the terms say; on the rows whose bits agree the exchange multiplies
        c by the row's OWN amplitude, and the diagonal the kernel multiplies by is D - c there."""
        LD = np.longdouble
        xr, xi = x.real.astype(LD), x.imag.astype(LD)
        ar, ai = np.abs(xr), np.abs(xi)
        yr, yi, mr, mi = (np.zeros(self.M, dtype=LD) for _ in range(4))
        n = np.zeros(self.M, dtype=np.int64)
        exch = dict(exchanges)
        D8 = np.zeros(self.M, dtype=np.int64)
        for mask, ts in self.terms:
            bra = self.rows ^ np.int64(mask)
            col = sub_index(self.right, self.L, bra)
            rows = np.flatnonzero(col >= 0)
            col, bra = col[rows], bra[rows]
            re, im = self._element(ts, bra)
            yr[rows] += (re * xr[col] - im * xi[col]) / 8
            yi[rows] += (re * xi[col] + im * xr[col]) / 8
            if mask == 0:
                assert self.square and not im.any()
                D8[rows] += re
                continue
            if mask in exch:
                assert self.square and not im.any()
                differ = parity_of(self.rows[rows] & np.int64(mask)) == 1
                assert np.all(re[differ] == exch[mask]) and not re[~differ].any()
                c = abs(exch[mask]) / LD(8)
                mr[rows] += np.where(differ, c * ar[col], c * ar[rows])
                mi[rows] += np.where(differ, c * ai[col], c * ai[rows])
                D8[rows[~differ]] -= exch[mask]
                n[rows] += 1
                continue
            sre = sum(abs(cr) for _, cr, _ in ts)
            sim = sum(abs(ci) for _, _, ci in ts)
            mr[rows] += (sre * ar[col] + sim * ai[col]) / 8
            mi[rows] += (sre * ai[col] + sim * ar[col]) / 8
            n[rows] += sum(1 if ci == 0 else 2 for _, _, ci in ts)
        has = np.zeros(self.M, dtype=bool)
        if self.square and self.terms and self.terms[0][0] == 0:
            has[:] = True
            mr += np.abs(D8) * ar / 8
            mi += np.abs(D8) * ai / 8
        return yr, yi, mr, mi, n + has


@functools.lru_cache(maxsize=None)
def get(op, L, left=('full',), right=None):
    return Ref(op, L, left, right)


FALLBACK = []          # cases whose amplitudes had to drop to [-2, 2]: (op, L, left, right, real); none so far


class Product:
    """x, z, z2 of a case (Gaussian integers; ``real``: integers) and the exact answers of every ABI entry, computed once
    and shared read-only: y and sums of  H x,  H x - b z,  H x - b z + c z2."""

    def __init__(self, ref, real):
        seed = 1000 * ref.L + 7 * len(ref.op) + (0 if ref.left[0] == 'full' else 1 + ref.left[1]) + (50 if real else 0)
        self.c8 = CR8 if real else C8
        self.c = complex(self.c8[0] / 8, self.c8[1] / 8)
        for amp in (8, 2):
            self.x = int_vector(ref.N, seed, amp, real)
            self.z, self.z2 = (int_vector(ref.M, seed + i, amp, real) for i in (1, 2))
            try:
                hx8 = ref.apply8(*ints(self.x))
                self.y, self.sums = ref.apply(self.x, hx8=hx8)
                if ref.square:
                    self.y_z, self.sums_z = ref.apply(self.x, self.z, hx8=hx8)
                    self.y_z2, _ = ref.apply(self.x, self.z, self.z2, self.c8, hx8=hx8)
                break
            except OutOfExactRange:
                if amp == 2:
                    raise
                FALLBACK.append((ref.op, ref.L, ref.left, ref.right, real))
        self.amp = amp
        for a in vars(self).values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def product(op, L, left=('full',), right=None, real=False):
    return Product(get(op, L, left, right), real)


def release():
    for f in (product, get):
        f.cache_clear()


# ---------------------------------------------------------------------------------------------------------------------
# the case table of tests/test_gpu_tiled_exact.py -- kept here so that tests/test_tiled_exact_ref.py can pin every
# reference the GPU file takes and prove, from DNM_MAT_HOST_ONLY handles, what every case runs
# ---------------------------------------------------------------------------------------------------------------------

MAT_USE_GLDS, MAT_REAL_PACKED = 2, 16          # include/dynamite_amd.h
FULL_, P0, P1 = ('full',), ('parity', 0), ('parity', 1)
BASE_KNOBS = {"DNM_GBITS": 3, "DNM_TILE_BITS": 8, "DNM_LOG_ROWS": 2, "DNM_PLAN_MODE": 2, "DNM_AMIN": 3}


class Case:
    """op on L spins, right -> left, dnm_mat_create flags, the knobs in the environment while the handle is made, the
    vector layout S (dnm_subspace.vec_swizzle), real arithmetic, the kernel instance of every local pass in turn and
    the (B, logR) of the plan."""

    def __init__(self, op, L, left, right, flags, knobs, S, instances):
        self.op, self.L, self.left, self.right, self.flags, self.S = op, L, left, right, flags, S
        self.knobs = dict(BASE_KNOBS)
        self.knobs.update(knobs)
        self.real = bool(flags & MAT_REAL_PACKED)
        self.instances = tuple(instances)
        self.pair = (self.knobs["DNM_TILE_BITS"], self.knobs["DNM_LOG_ROWS"])
        self.square = left == right


CASES = {}


def _case(name, op, L, inst, sub=FULL_, right=None, flags=0, S=6, pair=None, **kn):
    assert name not in CASES
    CASES[name] = Case(op, L, sub, right or sub, flags, {"DNM_" + k: v for k, v in kn.items()}, S, inst.split())
    if pair:          # passes with table records take rows per thread of their own (passes.cpp: pass_geometry)
        CASES[name].pair = pair


# B = 8, logR = 2: one wavefront per workgroup; L = 8 a single tile, L = 10 four workgroups with gathers, L = 12 a
# contiguous pass and a window pass that accumulates
_case("chain-8", "chain", 8, "FLIP+DT")
_case("chain-10", "chain", 10, "FLIP+DT")
_case("chain-12", "chain", 12, "FLIP FLIP+DT")
_case("chain-10-nodbt", "chain", 10, "FLIP", DIAG_BLOCK_TABLE=0)
_case("chain-10-lists", "chain", 10, "FLIP", DIAG_TABLE=0)
_case("chain-10-glds", "chain", 10, "FLIP+DT+GLDS", flags=MAT_USE_GLDS)
_case("chain-10-glds-nodbt", "chain", 10, "FLIP+GLDS", flags=MAT_USE_GLDS, DIAG_BLOCK_TABLE=0)
_case("chain-12-glds", "chain", 12, "FLIP+GLDS FLIP+DT+GLDS", flags=MAT_USE_GLDS)
_case("chain-10-noflip", "chain", 10, "DT", FLIPFLOP=0)
_case("chain-12-noflip-glds", "chain", 12, "GLDS DT+GLDS", flags=MAT_USE_GLDS, FLIPFLOP=0)
_case("hops-8", "hops", 8, "plain-early")
_case("hops-12", "hops", 12, "FLIP plain-early")
_case("hops-12-glds", "hops", 12, "FLIP+GLDS GLDS", flags=MAT_USE_GLDS)
_case("dm-8", "dm", 8, "DT")
_case("dm-10", "dm", 10, "DT")
_case("dm-12", "dm", 12, "plain-early DT")
_case("dm-10-glds", "dm", 10, "DT+GLDS", flags=MAT_USE_GLDS)
_case("dm-10-glds-nodbt", "dm", 10, "GLDS", flags=MAT_USE_GLDS, DIAG_BLOCK_TABLE=0)
_case("dm-12-glds", "dm", 12, "GLDS DT+GLDS", flags=MAT_USE_GLDS)
_case("long_range-10", "long_range", 10, "DT")
_case("long_range-12", "long_range", 12, "plain-early TAB")
_case("long_range-10-lists", "long_range", 10, "plain-early", DIAG_TABLE=0)
_case("long_range-12-nogroups", "long_range", 12, "plain-early plain-early", DIAG_GROUPS=0)
_case("nnn-10", "nnn", 10, "FLIP+DT")
_case("nnn-12", "nnn", 12, "plain-early TAB")
_case("nnn-12-nogroups", "nnn", 12, "FLIP FLIP", DIAG_GROUPS=0)
_case("dsel-11", "dsel", 11, "FLIP+DT")
_case("dext-10", "dext", 10, "FLIP", DIAG_TABLE=0)
_case("dsel-11-glds", "dsel", 11, "FLIP+DT+GLDS", flags=MAT_USE_GLDS)
_case("dsel-11-noflip", "dsel", 11, "DT", FLIPFLOP=0)
_case("dext-11-glds", "dext", 11, "FLIP+GLDS", flags=MAT_USE_GLDS, DIAG_TABLE=0)
_case("long_range-12-lists", "long_range", 12, "plain-early plain-early", DIAG_TABLE=0, DIAG_GROUPS=0)
_case("long_range-10-lists-glds", "long_range", 10, "GLDS", flags=MAT_USE_GLDS, DIAG_TABLE=0)
_case("syk-8", "syk", 8, "TAB")
_case("syk-10", "syk", 10, "TAB")
_case("syk-12", "syk", 12, "TAB")
_case("syk-12-b10", "syk", 12, "TAB", TILE_BITS=10, pair=(10, 3))
_case("syk-12-b10r4", "syk", 12, "TAB", TILE_BITS=10, TAB_LOG_ROWS=4, pair=(10, 4))
_case("syk-12-r2", "syk", 12, "TAB", TAB_LOG_ROWS=2)
_case("syk-10-records", "syk", 10, "DT", TAB_RECORDS=0)
_case("xstring-10", "xstring", 10, "DT")
_case("xstring-12", "xstring", 12, "plain-early DT")
# Parity 0 and 1, and the rectangular pairs
_case("chain-12-p0", "chain", 12, "FLIP+DT", sub=P0)
_case("chain-12-p1", "chain", 12, "FLIP+DT", sub=P1)
_case("dm-12-p1", "dm", 12, "DT", sub=P1)
_case("nnn-12-p0", "nnn", 12, "TAB", sub=P0)
_case("syk-12-p0", "syk", 12, "TAB", sub=P0)
_case("syk-12-p1", "syk", 12, "TAB", sub=P1)
_case("xstring-12-p1", "xstring", 12, "DT", sub=P1)
_case("long_range-12-p1", "long_range", 12, "TAB", sub=P1)
_case("long_range-11-p01", "long_range", 11, "DT", sub=P0, right=P1)
_case("long_range-11-p10", "long_range", 11, "DT", sub=P1, right=P0)
_case("xstring-11-p10", "xstring", 11, "plain-early", sub=P1, right=P0)
_case("xstring-11-p01", "xstring", 11, "plain-early", sub=P0, right=P1)
_case("syk-11-p01", "syk", 11, "TAB", sub=P0, right=P1)
# real-packed handles
for _o in ("pk_flip0", "pk_flip0x", "pk_sign0", "chain", "long_range", "nnn"):
    _case("%s-11-real" % _o, _o, 11, "PACK", flags=MAT_REAL_PACKED)
for _o in ("pk_flip0", "pk_flip0x", "pk_sign0"):
    _case("%s-13-real" % _o, _o, 13, "PACK", flags=MAT_REAL_PACKED)
# (one pass, everything outside its tile gathered: site-0 flips and site-0 signs in gathered records)
_case("pk_flip0x-13-real-m1", "pk_flip0x", 13, "PACK", flags=MAT_REAL_PACKED, PLAN_MODE=1)
_case("pk_sign0-13-real-m1", "pk_sign0", 13, "PACK", flags=MAT_REAL_PACKED, PLAN_MODE=1)
_case("chain-13-real", "chain", 13, "PACK PACK", flags=MAT_REAL_PACKED)
_case("long_range-13-real", "long_range", 13, "PACK PACK", flags=MAT_REAL_PACKED)
_case("pk_flip0x-12-p0-real", "pk_flip0x", 12, "PACK", sub=P0, flags=MAT_REAL_PACKED)
_case("pk_sign0-12-p1-real", "pk_sign0", 12, "PACK", sub=P1, flags=MAT_REAL_PACKED)
# the twelve (B, logR) of tile_config_supported at L = B + 2: the flip-flop instance and, with DNM_FLIPFLOP=0, the plain one
PAIRS = ((8, 2), (10, 2), (11, 2), (12, 2), (10, 3), (10, 4), (11, 3), (11, 4), (12, 3), (12, 4), (13, 3), (13, 4))
for _B, _r in PAIRS:
    _case("chain-b%dr%d-flip" % (_B, _r), "chain", _B + 2, "FLIP", TILE_BITS=_B, LOG_ROWS=_r, DIAG_BLOCK_TABLE=0)
    _case("chain-b%dr%d-plain" % (_B, _r), "chain", _B + 2, "plain-early", TILE_BITS=_B, LOG_ROWS=_r, DIAG_BLOCK_TABLE=0,
          FLIPFLOP=0)
    _case("dm-b%dr%d" % (_B, _r), "dm", _B + 2, "DT", TILE_BITS=_B, LOG_ROWS=_r)
# DNM_CACHE_POLICY: the default is 226 = gathers early (32) + streaming loads (2) and stores (64) of y + the late add of y
# (128).  On top of that default the two bits it lacks, 1 (stores through the L2: 227) and 4 (streaming tile loads: 230);
# each bit alone on top of the gather bit -- 33, 34, 36, 96, 160 --, the gather bit alone, and the default with bit 32
# cleared (194): late gathers, which also turns the flip-flop records and the diagonal tables off (passes.cpp:
# decide_flip_bonds, build_diag_tables)
POLICIES = (32, 33, 34, 36, 96, 160, 194, 227, 230)
for _p in POLICIES:
    _late = _p == 194
    _case("dm-12-cp%d" % _p, "dm", 12, "plain-late plain-late" if _late else "plain-early DT", CACHE_POLICY=_p)
    _case("chain-12-cp%d" % _p, "chain", 12, "plain-late plain-late" if _late else "FLIP FLIP+DT", CACHE_POLICY=_p)
    _case("nnn-12-cp%d" % _p, "nnn", 12, "plain-late TAB" if _late else "plain-early TAB", CACHE_POLICY=_p)
    _case("chain-13-real-cp%d" % _p, "chain", 13, "PACK PACK", flags=MAT_REAL_PACKED, CACHE_POLICY=_p)
# vector layouts 0 and 5 (6 is the one above)
for _S in (0, 5):
    # (in index order the diagonal rides on the first pass, in a swizzled layout on the last: plan.h, diag_last)
    _case("chain-12-s%d" % _S, "chain", 12, "FLIP FLIP+DT" if _S else "FLIP+DT FLIP", S=_S)
    _case("dm-12-s%d" % _S, "dm", 12, "plain-early DT" if _S else "DT plain-early", S=_S)
    _case("syk-12-s%d" % _S, "syk", 12, "TAB", S=_S)
    _case("xstring-12-s%d" % _S, "xstring", 12, "plain-early DT" if _S else "DT plain-early", S=_S)
    _case("chain-12-p1-s%d" % _S, "chain", 12, "FLIP+DT", sub=P1, S=_S)
    _case("pk_flip0x-13-real-s%d" % _S, "pk_flip0x", 13, "PACK", flags=MAT_REAL_PACKED, S=_S)
    _case("chain-13-real-s%d" % _S, "chain", 13, "PACK PACK", flags=MAT_REAL_PACKED, S=_S)
# shift 8: the half blocks that the partner passes of a partition of four write (offset 2^9) lie inside the swizzle's field
_case("chain-12-s8", "chain", 12, "FLIP FLIP+DT", S=8)
_case("dm-12-s8", "dm", 12, "plain-early DT", S=8)
# plan modes 0 (tile-only passes) and 1 (one pass, everything else gathered), other run lengths and group bits
_case("chain-12-m0", "chain", 12, "FLIP FLIP+DT", PLAN_MODE=0)
_case("chain-12-m1", "chain", 12, "FLIP+DT", PLAN_MODE=1)
_case("dm-14-m0", "dm", 14, "plain-early DT", TILE_BITS=10, PLAN_MODE=0, AMIN=4, GBITS=6)
_case("dm-14-m1", "dm", 14, "DT", TILE_BITS=10, PLAN_MODE=1, AMIN=4, GBITS=6)
_case("dm-14-m2", "dm", 14, "DT", TILE_BITS=10, PLAN_MODE=2, AMIN=4, GBITS=6)
_case("syk-14-m0", "syk", 14, "TAB TAB", TILE_BITS=10, PLAN_MODE=0, AMIN=4, GBITS=6, pair=(10, 3))
# operators that leave the top site alone: every range of workgroups along the top bit reads and writes its own amplitudes
_case("low8-10", "low8", 10, "FLIP+DT")
_case("low12-13-m0", "low12", 13, "plain-early DT", PLAN_MODE=0)
# L = 20: a contiguous pass and a window pass over 1024 workgroups
_case("dm-20", "dm", 20, "plain-early DT", TILE_BITS=10, LOG_ROWS=4, AMIN=4, GBITS=6)
_case("chain-20", "chain", 20, "FLIP FLIP+DT", TILE_BITS=12, LOG_ROWS=3, AMIN=4, GBITS=6)
# the production layout (shift 16: the swizzle moves amplitudes beyond 2^16 only)
_case("chain-18-prod", "chain", 18, "FLIP FLIP+DT", TILE_BITS=12, LOG_ROWS=4, PLAN_MODE=0, GBITS=6, S=16)

SHARES = [("chain-12", 2), ("chain-12", 4), ("long_range-12", 2), ("long_range-12", 4), ("dm-12-s0", 4), ("chain-12-s8", 4), ("dm-12-s8", 4)]
EMULATED = ["chain-8", "hops-8", "dm-10", "syk-10", "xstring-10", "long_range-10", "nnn-12", "syk-12-p1",
            "pk_flip0-11-real", "pk_flip0x-11-real", "pk_sign0-11-real", "long_range-11-p01"]
PLANTED = ["chain-12", "dm-12", "syk-12", "xstring-12", "nnn-12", "chain-12-p1", "pk_flip0-13-real", "pk_flip0x-13-real",
           "pk_sign0-13-real", "pk_flip0x-13-real-m1", "chain-13-real", "dm-12-s0", "chain-12-s5", "long_range-11-p01", "dm-14-m0"]
PARTS = ["chain-10", "dm-10", "syk-10", "chain-12-m1", "pk_flip0x-11-real", "low8-10", "low12-13-m0", "chain-10-glds"]
ROUNDING = [("FLIP / FLIP+DT", "chain-12"), ("plain and DT, complex records", "dm-12"), ("TAB, table records", "syk-12"),
            ("TAB, grouped diagonal", "nnn-12"), ("bucket lists", "long_range-10-lists"), ("PACK", "chain-13-real"), ("PACK, site 0", "pk_flip0x-13-real-m1"),
            ("late gathers", "dm-12-cp194"), ("GLDS", "dm-12-glds")]


def triples_used():
    """every (operator, L, left, right, real) the GPU tests take a reference for"""
    return sorted({(c.op, c.L, c.left, c.right, c.real) for c in CASES.values()}, key=str)
