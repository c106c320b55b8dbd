"""
The int64 reference of the four Gram-panel observable sweeps (csrc/pm_kernels.hip, swap_kernels.hip, cyc_kernels.hip,
pauli_kernels.hip), host only.  For each sweep the operand matrix A is built from the definition at the top of the
kernel file and G = A^H A is formed as two int64 arrays, re and im:
    Re G = Ar^T Ar + Ai^T Ai,    Im G = Ar^T Ai - (Ar^T Ai)^T        (conj(a) b = ar br + ai bi + i (ar bi - ai br)).

Nothing here calls dnm_*_partner_indices or reads pm_rank.h, swap_rank.h, cyc_rank.h or pauli_cols.h: those are the
code under test.  Configurations are uint64 (bit j = site j, so L = 64 is served), enumerated and ranked here:
  Full            index = configuration
  Parity(space)   index = configuration >> 1; bit 0 makes the number of set bits even (space 0) or odd (space 1)
  SpinConserve    the configurations of k set bits in ascending (= colexicographic) order; the rank of one is
                  sum_i C(p_i, i + 1) over the positions p_0 < p_1 < ... of its set bits (``colex_rank``), which the
                  look-up by bisection used for the columns must and does reproduce (tests/test_gram_ref.py)
  XParity sector s of a parent: the vector holds the parent's first dim / 2 rows (bit L - 1 clear); the amplitude of a
                  configuration with bit L - 1 set is s times that of its complement.

A subspace is ``Sub(kind, L, k=0, space=0)`` with kind in 'full', 'parity', 'sc'; the sweeps are 'pm', 'swap', 'cyc'
and 'pauli'; ``items`` are the site pairs (a, b) of the bonds, the triples (a, b, c) of a rotation (bit a <- bit b <- bit
c <- bit a) or the columns (site, kind) of the Pauli sweep (kind 1: sigma-x, 2: i sigma-y, 3: sigma-z).
"""
import functools
from math import comb

import numpy as np

U64 = np.uint64
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)
SWEEPS = ("pm", "swap", "cyc", "pauli")


def popcount(c):
    c = np.ascontiguousarray(c, dtype=U64)
    return _POP8[c.view(np.uint8).reshape(-1, 8)].sum(axis=1)


def bit(c, j):
    """bit j of every configuration, as int64"""
    return ((c >> U64(j)) & U64(1)).astype(np.int64)


def ones(L):
    return U64((1 << L) - 1)


@functools.lru_cache(maxsize=8)
def combs(n, t):
    """The configurations of n sites with t set bits, ascending (read-only uint64)."""
    if t < 0 or t > n:
        out = np.zeros(0, dtype=U64)
    elif t > n - t:
        # the complements of the configurations of n - t set bits: complementing reverses the order
        out = (ones(n) ^ combs(n, n - t))[::-1].copy()
    else:
        # row[s]: the configurations of the sites below p with s set bits -- those without bit p, then those with it
        row = [np.zeros(1, dtype=U64)] + [np.zeros(0, dtype=U64)] * t
        for p in range(n):
            b = U64(1 << p)
            row = [row[0]] + [np.concatenate([row[s], row[s - 1] | b]) for s in range(1, t + 1)]
        out = row[t]
    assert out.size == (comb(n, t) if 0 <= t <= n else 0)
    out.setflags(write=False)
    return out


def colex_rank(c, L):
    """sum_i C(p_i, i + 1) over the set bits p_0 < p_1 < ... of every configuration (int64)"""
    c = np.ascontiguousarray(c, dtype=U64)
    rank = np.zeros(c.size, dtype=np.int64)
    cnt = np.zeros(c.size, dtype=np.int64)
    for p in range(L):
        b = bit(c, p)
        cnt += b
        table = np.array([comb(p, s) if comb(p, s) < 2 ** 63 else 0 for s in range(L + 2)], dtype=np.int64)
        rank += b * table[cnt]
    return rank


class Sub:
    def __init__(self, kind, L, k=0, space=0):
        assert kind in ("full", "parity", "sc") and 1 <= L <= 64
        assert kind == "sc" or L <= 24, "Full and Parity are enumerated: small L only"
        self.kind, self.L = kind, L
        self.k = k if kind == "sc" else 0
        self.space = space if kind == "parity" else 0
        self.dim = comb(L, k) if kind == "sc" else 1 << (L - (kind == "parity"))

    def __repr__(self):
        return {"full": "Full(%d)" % self.L, "parity": "Parity(%d, %d)" % (self.L, self.space),
                "sc": "SpinConserve(%d, %d)" % (self.L, self.k)}[self.kind]

    def configs(self):
        """the configuration of every index, in index order (read-only)"""
        return _configs(self.kind, self.L, self.k, self.space)

    def index(self, c):
        """the index of every configuration; each must lie in the subspace"""
        c = np.ascontiguousarray(c, dtype=U64)
        if self.kind == "full":
            assert not np.any(c >> U64(self.L))
            return c.astype(np.int64)
        if self.kind == "parity":
            assert not np.any(c >> U64(self.L)) and np.all((popcount(c) & 1) == self.space)
            return (c >> U64(1)).astype(np.int64)
        all_c = self.configs()
        i = np.searchsorted(all_c, c)
        assert np.all(i < all_c.size) and np.array_equal(all_c[np.minimum(i, all_c.size - 1)], c), \
            "a configuration outside %r" % self
        return i.astype(np.int64)


@functools.lru_cache(maxsize=8)
def _configs(kind, L, k, space):
    if kind == "sc":
        return combs(L, k)
    if kind == "full":
        out = np.arange(1 << L, dtype=U64)
    else:
        idx = np.arange(1 << (L - 1), dtype=U64)
        out = (idx << U64(1)) | ((popcount(idx) & 1) ^ space).astype(U64)
    out.setflags(write=False)
    return out


def state_size(sub, xsec=0):
    """amplitudes of the vector a sweep is handed"""
    assert xsec == 0 or sub.dim % 2 == 0
    return sub.dim // 2 if xsec else sub.dim


def row_configs(sweep, sub, xsec=0):
    """The configurations of the rows of A.  sigma+ sigma-: every configuration (Full), those of the opposite parity in
    the order of their index bits (Parity), those of k + 1 set bits (SpinConserve(L, k)).  The other sweeps: the
    subspace's own, or the representatives of an XParity sector -- for the flipping columns of the Pauli sweep on
    Parity the configurations of the opposite parity at the same indices (``column`` takes care of that)."""
    assert sweep in SWEEPS
    if sweep == "pm":
        assert xsec == 0
        if sub.kind == "sc":
            return combs(sub.L, sub.k + 1)
        return Sub(sub.kind, sub.L, space=sub.space ^ 1).configs()
    c = sub.configs()
    if xsec:
        assert sweep != "pauli" and xsec in (1, -1) and sub.L >= 2 and c.size % 2 == 0
        h = c.size // 2
        assert not np.any(bit(c[:h], sub.L - 1)) and np.all(bit(c[h:], sub.L - 1) == 1)
        c = c[:h]
    return c


def _fold(new, sub, xsec):
    """(index into the vector, factor) of the amplitudes of the configurations ``new``"""
    sgn = np.ones(new.size, dtype=np.int64)
    if xsec:
        top = bit(new, sub.L - 1)
        new = np.where(top == 1, new ^ ones(sub.L), new)
        sgn = np.where(top == 1, xsec, 1).astype(np.int64)
    idx = sub.index(new)
    assert not xsec or np.all(idx < sub.dim // 2)
    return idx, sgn


def column(sweep, sub, xsec, item, rows):
    """One column of A on the rows of configurations ``rows``: (idx, sgn), A[r] = sgn[r] * x[idx[r]] (sgn 0: the entry is
    zero and idx[r] is 0).  item None: the state's own column (not for 'pm', whose columns are its sites)."""
    rows = np.ascontiguousarray(rows, dtype=U64)
    L = sub.L
    if item is None:
        assert sweep != "pm"
        return _fold(rows, sub, xsec)
    if sweep == "pm":
        j = int(item)
        assert 0 <= j < L
        has = bit(rows, j)
        idx = np.zeros(rows.size, dtype=np.int64)
        sel = has == 1
        idx[sel] = sub.index(rows[sel] ^ U64(1 << j))
        return idx, has
    if sweep == "swap":
        a, b = (int(v) for v in item)
        assert a != b and 0 <= a < L and 0 <= b < L
        differ = (bit(rows, a) ^ bit(rows, b)).astype(U64)
        return _fold(rows ^ (differ * U64((1 << a) | (1 << b))), sub, xsec)
    if sweep == "cyc":
        a, b, c = (int(v) for v in item)
        assert len({a, b, c}) == 3 and all(0 <= s < L for s in (a, b, c))
        ba, bb, bc = bit(rows, a).astype(U64), bit(rows, b).astype(U64), bit(rows, c).astype(U64)
        new = rows & ~U64((1 << a) | (1 << b) | (1 << c))
        new = new | (bb << U64(a)) | (bc << U64(b)) | (ba << U64(c))      # bit a <- bit b <- bit c <- bit a
        return _fold(new, sub, xsec)
    site, kind = (int(v) for v in item)
    assert sweep == "pauli" and xsec == 0 and sub.kind in ("full", "parity") and 0 <= site < L and kind in (1, 2, 3)
    flips, signs = kind in (1, 2), kind in (2, 3)
    # (sigma psi)(r) on the rows r the column lives on: a flip leaves a Parity sector, so a flipping column holds the
    # configurations of the opposite parity -- at the same index, the sector's own with site 0 flipped
    r = rows ^ U64(1) if (flips and sub.kind == "parity") else rows
    sgn = 1 - 2 * bit(r, site) if signs else np.ones(rows.size, dtype=np.int64)
    idx = sub.index(r ^ U64(1 << site) if flips else r)
    return idx, sgn


def column_items(sweep, sub, items):
    if sweep == "pm":
        assert items is None
        return list(range(sub.L))
    items = [tuple(int(v) for v in it) for it in items]
    assert 1 <= len(items) <= 63
    return [None] + items


def partner_table(sweep, sub, xsec, items, rows):
    """(idx, sgn), each (len(rows), columns), of the rows of configurations ``rows``"""
    cols = [column(sweep, sub, xsec, it, rows) for it in column_items(sweep, sub, items)]
    return np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1)


def operand(sweep, sub, xsec, items, xr, xi):
    """(Ar, Ai): the operand matrix of the state x = xr + i xi (index order), in the dtype of xr"""
    xr, xi = np.asarray(xr), np.asarray(xi)
    assert xr.shape == xi.shape == (state_size(sub, xsec),) and xr.dtype == xi.dtype
    rows = row_configs(sweep, sub, xsec)
    its = column_items(sweep, sub, items)
    Ar = np.zeros((rows.size, len(its)), dtype=xr.dtype)
    Ai = np.zeros((rows.size, len(its)), dtype=xr.dtype)
    for n, it in enumerate(its):
        idx, sgn = column(sweep, sub, xsec, it, rows)
        assert idx.size == 0 or (idx.min() >= 0 and idx.max() < xr.size)
        s = sgn.astype(xr.dtype)
        Ar[:, n] = s * xr[idx]
        Ai[:, n] = s * xi[idx]
    return Ar, Ai


def sector_mask(sweep, sub, items):
    """Pauli sweep on Parity: True where an entry of G pairs a flipping with a non-flipping column (the state's own
    among the latter) -- two vectors on different sectors, whose product is zero.  None elsewhere."""
    if sweep != "pauli" or sub.kind != "parity":
        return None
    fl = np.array([False] + [int(kind) in (1, 2) for _, kind in items])
    return fl[:, None] != fl[None, :]


def gram_int(Ar, Ai):
    """G = A^H A as (re, im), int64.  A component of an entry sums 2 * rows products of two parts: asserted below 2^53
    in the sum of their moduli, so that the same sum is exact in doubles in any order."""
    assert Ar.dtype == np.int64 and Ai.dtype == np.int64 and Ar.shape == Ai.shape
    amax = int(max(np.abs(Ar).max(initial=0), np.abs(Ai).max(initial=0)))
    assert 2 * Ar.shape[0] * amax * amax < 2 ** 53, "not exact in doubles"
    if Ar.shape[0] * Ar.shape[1] <= 1 << 20:
        q = Ar.T @ Ai
        return Ar.T @ Ar + Ai.T @ Ai, q - q.T
    # Tall operands: numpy multiplies int64 matrices without BLAS, seconds for 10^7 entries.  Blocks of 2^16 rows are
    # multiplied in doubles instead -- a block's sums stay below 2^17 amax^2, exact in any order -- and the blocks
    # are added in int64.  Column 0 and the diagonal are formed in int64 throughout and compared.
    n = Ar.shape[1]
    re, q = np.zeros((n, n), dtype=np.int64), np.zeros((n, n), dtype=np.int64)
    assert (1 << 17) * amax * amax < 2 ** 53
    diag, re0, im0 = (np.zeros(n, dtype=np.int64) for _ in range(3))
    for lo in range(0, Ar.shape[0], 1 << 16):
        br, bi = Ar[lo:lo + (1 << 16)], Ai[lo:lo + (1 << 16)]
        fr, fi = br.astype(np.float64), bi.astype(np.float64)
        re += (fr.T @ fr + fi.T @ fi).astype(np.int64)
        q += (fr.T @ fi).astype(np.int64)
        diag += (br * br + bi * bi).sum(axis=0)
        re0 += (br[:, :1] * br + bi[:, :1] * bi).sum(axis=0)
        im0 += (br[:, :1] * bi - bi[:, :1] * br).sum(axis=0)
    im = q - q.T
    assert np.array_equal(re.diagonal(), diag) and np.array_equal(re[0], re0) and np.array_equal(im[0], im0)
    return re, im


def reference(sweep, sub, xsec, items, xr, xi):
    """(re, im) int64 of the sweep's result for the integer state xr + i xi"""
    Ar, Ai = operand(sweep, sub, xsec, items, np.asarray(xr, dtype=np.int64), np.asarray(xi, dtype=np.int64))
    re, im = gram_int(Ar, Ai)
    mask = sector_mask(sweep, sub, items)
    if mask is not None:
        re[mask] = 0
        im[mask] = 0
    return re, im
