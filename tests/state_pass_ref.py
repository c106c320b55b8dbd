"""
The integer reference of the three passes that turn a state into another state (csrc/perm_kernels.hip,
csrc/submap_kernels.hip, csrc/site_ops_kernels.hip), host only: plain numpy and Python integers, written from the
definitions at the top of the three kernel files.

Nothing here calls idx_to_state, state_to_idx, dnm_*_partner_indices or dnm_subspace_map_indices, and nothing was read
off csrc/subspace.h, perm_rank.h, submap_rank.h or pm_rank.h: those are the code under test.  Configurations are uint64
(bit j = site j, so L = 64 is served), enumerated and ranked here:
  Full            index = configuration
  Parity(space)   index = configuration >> 1; bit 0 makes the number of set bits even (space 0) or odd (space 1)
  SpinConserve    the configurations of k set bits in ascending (= colexicographic) order, enumerated site by site; the
                  rank of one is sum_i C(p_i, i + 1) over the positions p_0 < p_1 < ... of its set bits, from math.comb
  Explicit        list order; a configuration is found by numpy.searchsorted on a sorted copy of the list
  XParity sector s over a parent: the vector holds the parent's first dim / 2 rows (the representatives, bit L - 1
                  clear); the amplitude of a configuration with bit L - 1 set is s times that of its complement.

A *side* is ``(Sub, sector, swizzle)``: the (parent) subspace, 0 or the XParity sector +-1, and the XOR-swizzle shift of
a Full / Parity vector in memory (element i lies at position vec_pos(i, swizzle)).  Vectors are handed over and
returned AS THEY LIE.  Amplitudes are pairs (re, im) of int64 arrays; every function asserts that each intermediate it
forms is an integer of modulus below 2^53, so that a double holds it whatever the order of the operations.
"""
import functools
from math import comb

import numpy as np

U64 = np.uint64
KAPPA = 0.70710678118654752440          # the constant of csrc/submap_rank.h: SUBMAP_KAPPA
LIMIT = 1 << 53
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def below_2_53(*arrays):
    """every array holds integers of modulus < 2^53 (int64 arrays, or Python integers); returns its arguments"""
    for a in arrays:
        if isinstance(a, (int, np.integer)):
            assert abs(int(a)) < LIMIT
        else:
            assert a.dtype == np.int64, a.dtype
            assert a.size == 0 or max(int(a.max()), -int(a.min())) < LIMIT, "an intermediate reaches 2^53"
    return arrays if len(arrays) > 1 else arrays[0]


def popcount(c):
    c = np.ascontiguousarray(c, dtype=U64)
    return _POP8[c.view(np.uint8).reshape(-1, 8)].sum(axis=1)


def all_sites(L):
    return U64((1 << L) - 1)


def vec_pos(i, S):
    """the position of element i of a vector in the XOR-swizzled layout of shift S (an involution; 0: index order):
    the S - 4 index bits from bit S up are folded onto the bits from 4 up"""
    i = np.asarray(i, dtype=np.int64)
    if not S:
        return i
    return i ^ (((i >> S) & ((1 << (S - 4)) - 1)) << 4)


@functools.lru_cache(maxsize=16)
def _ascending(L, k):
    """the configurations of L sites with k set bits in ascending order (read-only uint64)"""
    if k < 0 or k > L:
        out = np.zeros(0, dtype=U64)
    elif 2 * k > L:                      # the complements of the others: complementing reverses the order
        out = (all_sites(L) ^ _ascending(L, L - k))[::-1].copy()
    else:
        # level[s] after site p: the configurations of the sites 0..p with s set bits -- those with bit p clear come
        # first (they are smaller), then those with it set
        level = [np.zeros(1, dtype=U64)] + [np.zeros(0, dtype=U64) for _ in range(k)]
        for p in range(L):
            b = U64(1 << p)
            level = [level[0]] + [np.concatenate([level[s], level[s - 1] | b]) for s in range(1, k + 1)]
        out = level[k]
    assert out.size == (comb(L, k) if 0 <= k <= L else 0)
    assert out.size < 2 or np.all(out[1:] > out[:-1])
    out.setflags(write=False)
    return out


def colex_rank(c, L):
    """sum_i C(p_i, i + 1) over the set bits p_0 < p_1 < ... of every configuration (int64), from math.comb"""
    c = np.ascontiguousarray(c, dtype=U64)
    rank = np.zeros(c.size, dtype=np.int64)
    seen = np.zeros(c.size, dtype=np.int64)
    for p in range(L):
        b = ((c >> U64(p)) & U64(1)).astype(np.int64)
        seen += b
        row = np.array([comb(p, s) if comb(p, s) < LIMIT else 0 for s in range(L + 2)], dtype=np.int64)
        rank += b * row[seen]
    return rank


class Sub:
    """A subspace by its definition.  kind: 'full', 'parity', 'sc' (SpinConserve(L, k)) or 'explicit' (``states``: the
    list, in list order, any integers below 2^64)."""

    def __init__(self, kind, L, k=0, space=0, states=None):
        assert kind in ("full", "parity", "sc", "explicit") and 1 <= L <= 64
        assert kind in ("sc", "explicit") or L <= 24, "Full and Parity are enumerated: small L only"
        self.kind, self.L = kind, L
        self.k = k if kind == "sc" else 0
        self.space = space if kind == "parity" else 0
        if kind == "explicit":
            self.states = np.array([int(s) for s in states], dtype=U64)
            self.states.setflags(write=False)
            self._order = np.argsort(self.states, kind="stable")
            self._sorted = self.states[self._order]
            assert self.states.size >= 1 and np.all(self._sorted[1:] > self._sorted[:-1]), "a list of distinct states"
            self.dim = self.states.size
        else:
            self.states = None
            self.dim = comb(L, k) if kind == "sc" else 1 << (L - (kind == "parity"))

    def __repr__(self):
        return {"full": "Full(%d)" % self.L, "parity": "Parity(%d, %d)" % (self.L, self.space),
                "sc": "SpinConserve(%d, %d)" % (self.L, self.k),
                "explicit": "Explicit(%d states, L=%d)" % (self.dim, self.L)}[self.kind]

    def configs(self):
        """the configuration of every index, in index order (read-only uint64)"""
        if self.kind == "explicit":
            return self.states
        return _configs(self.kind, self.L, self.k, self.space)

    def index(self, c):
        """the index of every configuration, -1 where it is not in the subspace (int64)"""
        c = np.ascontiguousarray(c, dtype=U64).reshape(-1)
        inside = (c & ~all_sites(self.L)) == U64(0)
        if self.kind == "full":
            i = c.astype(np.int64)
        elif self.kind == "parity":
            inside &= (popcount(c) & 1) == self.space
            i = (c >> U64(1)).astype(np.int64)
        elif self.kind == "sc":
            inside &= popcount(c) == self.k
            i = colex_rank(np.where(inside, c, U64(0)), self.L)
        else:
            # (a listed state of more than L bits is in no subspace of L spins: never found)
            at = np.minimum(np.searchsorted(self._sorted, c), self.dim - 1)
            inside &= self._sorted[at] == c
            i = self._order[at].astype(np.int64)
        return np.where(inside, i, -1)

    def carries_flip(self):
        """the complement of every configuration of the subspace lies in it, by its form"""
        return self.kind == "full" or (self.kind == "parity" and self.L % 2 == 0) or \
            (self.kind == "sc" and self.L == 2 * self.k)


@functools.lru_cache(maxsize=8)
def _configs(kind, L, k, space):
    if kind == "sc":
        return _ascending(L, k)
    if kind == "full":
        out = np.arange(1 << L, dtype=U64)
    else:
        idx = np.arange(1 << (L - 1), dtype=U64)
        out = (idx << U64(1)) | ((popcount(idx) & 1) ^ space).astype(U64)
    out.setflags(write=False)
    return out


def rows_of(side):
    """the elements of the vector of a side"""
    sub, sector, _ = side
    assert sector in (0, 1, -1) and (sector == 0 or sub.dim % 2 == 0)
    return sub.dim // 2 if sector else sub.dim


def row_configs(side, positions=None):
    """the configuration of the row at every position of the vector as it lies (all positions when None)"""
    sub, sector, swz = side
    n = rows_of(side)
    if positions is None:
        positions = np.arange(n, dtype=np.int64)
    positions = np.asarray(positions, dtype=np.int64)
    assert positions.size == 0 or (positions.min() >= 0 and positions.max() < n)
    cfg = sub.configs()[vec_pos(positions, swz)]
    if sector:
        assert not np.any((cfg >> U64(sub.L - 1)) & U64(1)), "a representative has spin L - 1 down"
    return cfg


def amplitude_of(side, cfg):
    """(position in the vector as it lies or -1, factor): the amplitude psi(c) of every configuration c is factor *
    x[position] (times kappa under a sector), 0 where the position is -1"""
    sub, sector, swz = side
    cfg = np.ascontiguousarray(cfg, dtype=U64).reshape(-1)
    factor = np.ones(cfg.size, dtype=np.int64)
    if sector:
        top = ((cfg >> U64(sub.L - 1)) & U64(1)) == U64(1)
        top &= (cfg & ~all_sites(sub.L)) == U64(0)
        cfg = np.where(top, cfg ^ all_sites(sub.L), cfg)
        factor = np.where(top, sector, 1).astype(np.int64)
    i = sub.index(cfg)
    have = (i >= 0) & (i < rows_of(side))
    return np.where(have, vec_pos(np.maximum(i, 0), swz), -1), np.where(have, factor, 0)


# ---------------------------------------------------------------- site permutations (csrc/perm_kernels.hip)

def perm_source(cfg, perm):
    """P_pi moves the spin at site i to site pi(i): (P_pi x)(c') = x(c) where bit i of c = bit pi(i) of c'"""
    cfg = np.ascontiguousarray(cfg, dtype=U64)
    src = np.zeros_like(cfg)
    assert sorted(int(p) for p in perm) == list(range(len(perm)))
    for i, p in enumerate(perm):
        src |= ((cfg >> U64(int(p))) & U64(1)) << U64(i)
    return src


def perm_gather(side, perm, positions=None):
    """(p_g(r), s_g(r)) for the row at every position: where the source amplitude lies, and its factor"""
    sub = side[0]
    assert len(perm) == sub.L and sub.kind != "explicit"
    pos, factor = amplitude_of(side, perm_source(row_configs(side, positions), perm))
    assert np.all(pos >= 0) and np.all(factor != 0), "a permutation keeps a row inside its subspace"
    return pos, factor


def perm_apply(x, side, perms, coef, y=None):
    """y[r] = (y[r] if given else 0) + sum_g c_g s_g(r) x[p_g(r)]; x, y and the result are (re, im) int64 pairs, coef a
    list of Gaussian integers (re, im)"""
    xr, xi = below_2_53(*x)
    assert xr.size == rows_of(side)
    if y is None:
        yr, yi = np.zeros(xr.size, dtype=np.int64), np.zeros(xr.size, dtype=np.int64)
    else:
        yr, yi = (a.copy() for a in below_2_53(*y))
    assert len(perms) == len(coef)
    for perm, (cr, ci) in zip(perms, coef):
        pos, s = perm_gather(side, perm)
        vr, vi = below_2_53(s * xr[pos], s * xi[pos])
        tr, ti = below_2_53(int(cr) * vr - int(ci) * vi, int(cr) * vi + int(ci) * vr)
        yr, yi = below_2_53(yr + tr, yi + ti)
    return yr, yi


def perm_dots(phi, psi, side, perms):
    """out[g] = sum_r conj(phi[r]) s_g(r) psi[p_g(r)]: a list of (re, im) Python integers"""
    fr, fi = below_2_53(*phi)
    pr, pi = below_2_53(*psi)
    assert fr.size == pr.size == rows_of(side)
    out = []
    for perm in perms:
        pos, s = perm_gather(side, perm)
        vr, vi = s * pr[pos], s * pi[pos]
        tr, ti = below_2_53(fr * vr + fi * vi, fr * vi - fi * vr)
        # (every partial sum of either part is bounded by the sum of the moduli)
        assert int(np.abs(tr).sum()) < LIMIT and int(np.abs(ti).sum()) < LIMIT
        out.append((int(tr.sum()), int(ti.sum())))
    return out


# ---------------------------------------------------------------- subspace maps (csrc/submap_kernels.hip)

COPY, FROM_SECTOR, TO_SECTOR = "copy", "from sector", "to sector"


def map_mode(src, dst):
    """plain -> plain and sector -> sector copy bits; sector -> plain is one multiply by +-kappa; plain -> sector one
    add and one multiply by kappa"""
    if src[1]:
        return COPY if dst[1] else FROM_SECTOR
    return TO_SECTOR if dst[1] else COPY


def map_terms(src, dst, positions=None):
    """(idx (n, 2), sign (n, 2), scale): y[r] = scale * sum_m sign[r, m] * x[idx[r, m]] for the target row at every
    position; idx -1 and sign 0 where there is no such amplitude.  The map is the orthogonal projection onto the span
    of the target of the source state seen as a vector of the whole 2^L space."""
    assert src[0].L == dst[0].L
    L = dst[0].L
    cfg = row_configs(dst, positions)
    n = cfg.size
    idx = np.full((n, 2), -1, dtype=np.int64)
    sign = np.zeros((n, 2), dtype=np.int64)
    mode = map_mode(src, dst)
    if src[1] and dst[1] and src[1] != dst[1]:
        return idx, sign, 1.0                                    # the two sectors are orthogonal
    idx[:, 0], sign[:, 0] = amplitude_of(src, cfg)               # psi(c)
    if mode == TO_SECTOR:                                        # (psi(c) + t psi(cbar)) kappa
        inside = (cfg & ~all_sites(L)) == U64(0)
        p, f = amplitude_of(src, np.where(inside, cfg ^ all_sites(L), cfg))
        idx[:, 1] = np.where(inside, p, -1)
        sign[:, 1] = np.where(inside, f, 0) * dst[1]
    return idx, sign, (1.0 if mode == COPY else KAPPA)


def map_apply(x, src, dst):
    """The target vector as it lies (complex128) from the source vector as it lies (complex128).  A copy moves bits,
    whatever they are.  In the two kappa modes the amplitudes must be Gaussian integers: the quantity multiplied by
    kappa -- x, or psi(c) +- psi(cbar) -- is asserted to be an integer below 2^53, and kappa * integer is rounded
    once, with the constant of the kernel."""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    assert x.size == rows_of(src)
    idx, sign, scale = map_terms(src, dst)
    mode = map_mode(src, dst)
    have = idx >= 0
    if mode == COPY:
        bits = x.view(np.uint64).reshape(-1, 2)
        out = np.where(have[:, :1], bits[np.maximum(idx[:, 0], 0)], np.uint64(0))
        return np.ascontiguousarray(out).view(np.complex128).reshape(-1)
    parts = x.view(np.float64).reshape(-1, 2)
    ints = np.rint(parts).astype(np.int64)
    assert np.array_equal(ints.astype(np.float64), parts), "the kappa modes take Gaussian integers"
    below_2_53(ints)
    a = np.where(have[:, :1], ints[np.maximum(idx[:, 0], 0)], 0)
    if mode == FROM_SECTOR:
        # one multiply per component by +-kappa (a sign times an integer: -0.0 where the kernel gives it)
        y = a.astype(np.float64) * (np.where(sign[:, 0] < 0, -KAPPA, KAPPA))[:, None]
    else:
        b = np.where(have[:, 1:], ints[np.maximum(idx[:, 1], 0)], 0)
        assert set(np.unique(sign[:, 1])) <= {0, dst[1]} and set(np.unique(sign[:, 0])) <= {0, 1}
        total = below_2_53(a + dst[1] * b)
        y = total.astype(np.float64) * KAPPA
    return np.ascontiguousarray(y).view(np.complex128).reshape(-1)


# ---------------------------------------------------------------- sector weights (csrc/submap_kernels.hip)

def weights_branch(side):
    """which of its three branches the kernel takes: pairs (the flip sums come with the bins), sector, plain"""
    sub, sector, _ = side
    if sector:
        return "sector"
    return "pairs" if sub.carries_flip() and sub.kind != "explicit" and sub.dim % 2 == 0 else "plain"


def sector_weights(x, side):
    """(mag2, flip2): TWICE the L + 1 sums of |psi(c)|^2 over the configurations with k set bits, and TWICE (F+, F-),
    F+- = sum over the pairs {c, cbar} of |psi(c) +- psi(cbar)|^2 / 2 (None where the subspace does not carry the flip)
    -- Python integers, doubled because a representative of a sector adds |x|^2 / 2 to bin k and to bin L - k."""
    sub, sector, swz = side
    L = sub.L
    xr, xi = below_2_53(*x)
    n = rows_of(side)
    assert xr.size == n
    cfg = row_configs(side)                                       # by position: x[p] belongs to cfg[p]
    k = popcount(cfg & all_sites(L))                              # (spins beyond L in a listed state are ignored)
    w = below_2_53(xr * xr + xi * xi)
    assert int(w.sum()) * 2 < LIMIT
    # (bincount adds in double: every partial sum is an integer below 2^53, as just asserted, so it is exact)
    per_k = [int(v) for v in np.bincount(k, weights=w.astype(np.float64), minlength=L + 1)]
    assert sum(per_k) == int(w.sum())
    if sector:
        mag2 = [per_k[kk] + per_k[L - kk] for kk in range(L + 1)]
        total = 2 * int(w.sum())
        return mag2, ([total, 0] if sector > 0 else [0, total])
    mag2 = [2 * v for v in per_k]
    if weights_branch(side) != "pairs":
        return mag2, None
    first = ((cfg >> U64(L - 1)) & U64(1)) == U64(0)
    mate, f = amplitude_of(side, cfg[first] ^ all_sites(L))
    assert np.all(f == 1) and 2 * int(first.sum()) == n
    ar, ai, br, bi = xr[first], xi[first], xr[mate], xi[mate]
    plus = below_2_53((ar + br) ** 2 + (ai + bi) ** 2)
    minus = below_2_53((ar - br) ** 2 + (ai - bi) ** 2)
    assert int(plus.sum()) < LIMIT and int(minus.sum()) < LIMIT
    return mag2, [int(plus.sum()), int(minus.sum())]             # (twice the halves)


# ---------------------------------------------------------------- products of site operators (site_ops_kernels.hip)

def gaussian_matrix(M):
    """a 2 x 2 complex matrix with Gaussian-integer entries as ((re, im) per entry) Python integers"""
    M = np.asarray(M, dtype=np.complex128)
    assert M.shape == (2, 2)
    re, im = np.rint(M.real).astype(np.int64), np.rint(M.imag).astype(np.int64)
    assert np.array_equal(re + 1j * im, M), "matrix entries must be Gaussian integers"
    return [[(int(re[a, b]), int(im[a, b])) for b in range(2)] for a in range(2)]


def _add_scaled(acc, c, v):
    """acc += c * v for a Python integer c (nothing to do for 0)"""
    if c == 1:
        acc += v
    elif c == -1:
        acc -= v
    elif c:
        acc += c * v


def site_product(x, mats, swz=0):
    """y(c') = sum_c prod_j M_j[c'_j][c_j] x(c) with spin j = index bit j, on a Full-space vector as it lies in the
    layout ``swz``; x and the result are (re, im) int64 pairs, mats[j] Gaussian-integer matrices.  With B the largest
    modulus of a part of the vector before a site and m that of a part of an entry of its matrix, a product of parts
    is at most m B, a part of a complex product 2 m B and a part of the sum of two 4 m B -- in any order of the
    additions -- so 4 m B < 2^53 is asserted site by site, for every intermediate of that site at once."""
    xr, xi = below_2_53(*x)
    n = xr.size
    L = n.bit_length() - 1
    assert n == 1 << L and len(mats) == L
    pos = vec_pos(np.arange(n, dtype=np.int64), swz)
    yr, yi = xr[pos], xi[pos]                                     # index order
    for j, M in enumerate(mats):
        m = gaussian_matrix(M)
        if m == [[(1, 0), (0, 0)], [(0, 0), (1, 0)]]:
            continue
        B = max(int(np.abs(yr).max()), int(np.abs(yi).max()))
        assert 4 * max(abs(p) for row in m for e in row for p in e) * B < LIMIT, "an intermediate reaches 2^53"
        vr, vi = yr.reshape(-1, 2, 1 << j), yi.reshape(-1, 2, 1 << j)
        outr, outi = np.zeros_like(vr), np.zeros_like(vi)
        for a in range(2):
            for b in range(2):
                mr, mi = m[a][b]                                  # (mr + i mi)(vr + i vi)
                _add_scaled(outr[:, a, :], mr, vr[:, b, :])
                _add_scaled(outr[:, a, :], -mi, vi[:, b, :])
                _add_scaled(outi[:, a, :], mr, vi[:, b, :])
                _add_scaled(outi[:, a, :], mi, vr[:, b, :])
        yr, yi = below_2_53(outr.reshape(-1), outi.reshape(-1))
    outr, outi = np.empty_like(yr), np.empty_like(yi)
    outr[pos], outi[pos] = yr, yi
    return outr, outi
