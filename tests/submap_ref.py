"""
A numpy restatement of the subspace maps (dnm_subspace_map_apply, dnm_subspace_map_indices, dnm_sector_weights) from
``idx_to_state`` and ``state_to_idx`` of the Python subspaces alone -- written from the definition, independently of
csrc/submap_rank.h.

The map is the orthogonal projection, onto the span of the target subspace, of the source state seen as a vector of the
whole 2^L space.  psi(c) is the amplitude of configuration c in the source: x[i_src(c)] or 0; on the XParity sector s
over a parent, KAPPA x[i(c)] for c in the parent with bit L - 1 clear and KAPPA s x[i(cbar)] with it set.  For the
target row of configuration c (the representative under a target sector t):

    plain     -> plain       x[i_src(c)] or 0
    XParity s -> plain       x[.] * KAPPA with the sign s on the flipped half, or 0
    plain     -> XParity t   (psi(c) + t psi(cbar)) * KAPPA
    XParity s -> XParity t   x[i(c)] if s == t and c lies in the source's parent, else 0

A *side* is ``(subspace, sector, swizzle)``: a Full / Parity / SpinConserve / Explicit subspace, 0 or the XParity sector
+-1 whose representatives (the first half of the subspace's rows) the vector holds, and the XOR-swizzle shift of the
vector in memory (Full / Parity; 0 = index order).
"""
import numpy as np

KAPPA = 0.70710678118654752440


def vec_pos(i, S):
    """Position of element i in the XOR-swizzled layout of shift S (an involution; S = 0: index order)."""
    i = np.asarray(i, dtype=np.int64)
    if not S:
        return i
    return i ^ (((i >> S) & ((1 << (S - 4)) - 1)) << 4)


def side_of(subspace, swizzle=0):
    """(base subspace, sector, swizzle) of a Python subspace: XParity gives its parent and its sector."""
    from dynamite_amd.subspaces import XParity
    if type(subspace) is XParity:
        return subspace.parent, int(subspace.sector), swizzle
    return subspace, 0, swizzle


def rows_of(side):
    sub, sector, _ = side
    return sub.get_dimension() // 2 if sector else sub.get_dimension()


def _lookup(side, cfg):
    """(position in the source vector or -1, sign) of psi(cfg) / KAPPA^[sector != 0]."""
    sub, sector, swz = side
    L = sub.L
    cfg = np.asarray(cfg, dtype=np.int64)
    if sector == 0:
        i = np.asarray(sub.state_to_idx(cfg))
        return np.where(i >= 0, vec_pos(np.maximum(i, 0), swz), -1), np.where(i >= 0, 1, 0)
    flipped = ((cfg >> (L - 1)) & 1) == 1
    rep = np.where(flipped, cfg ^ ((1 << L) - 1), cfg)
    i = np.asarray(sub.state_to_idx(rep))
    ok = (i >= 0) & (i < rows_of(side))
    return np.where(ok, vec_pos(np.maximum(i, 0), swz), -1), np.where(ok, np.where(flipped, sector, 1), 0)


def map_indices(src, dst, rows=None):
    """``(idx, sign, scale)`` of dnm_subspace_map_indices for the target positions ``rows`` (all of them when None):
    int64 (n, 2), int8 (n, 2), float."""
    ssub, ssec, _ = src
    dsub, dsec, dswz = dst
    L = dsub.L
    if rows is None:
        rows = np.arange(rows_of(dst), dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    cfg = np.asarray(dsub.idx_to_state(vec_pos(rows, dswz)), dtype=np.int64).reshape(-1)
    idx = np.full((rows.size, 2), -1, dtype=np.int64)
    sign = np.zeros((rows.size, 2), dtype=np.int8)
    if ssec and dsec:
        scale = 1.0
        if ssec == dsec:
            idx[:, 0], sign[:, 0] = _lookup(src, cfg)
    elif ssec:
        scale = KAPPA
        idx[:, 0], sign[:, 0] = _lookup(src, cfg)
    elif dsec:
        scale = KAPPA
        idx[:, 0], sign[:, 0] = _lookup(src, cfg)
        idx[:, 1], s1 = _lookup(src, cfg ^ ((1 << L) - 1))
        sign[:, 1] = s1 * dsec
    else:
        scale = 1.0
        idx[:, 0], sign[:, 0] = _lookup(src, cfg)
    return idx, sign, scale


def map_apply(x, src, dst):
    """The target vector as it lies, from the source vector ``x`` as it lies -- with the operations of the table in
    their order (a copy; one multiply; one add, then one multiply), so that it holds the bits the device must give."""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    assert x.size == rows_of(src)
    idx, sign, scale = map_indices(src, dst)
    xr = x.view(np.float64).reshape(-1, 2)

    def term(m):
        have = idx[:, m] >= 0
        return np.where(have[:, None], xr[np.maximum(idx[:, m], 0)], 0.0), have

    a, have = term(0)
    if src[1] == 0 and dst[1] != 0:
        b, _ = term(1)
        y = (a + b if dst[1] > 0 else a - b) * KAPPA
    elif src[1] != 0 and dst[1] == 0:
        y = a * (sign[:, 0].astype(np.float64) * KAPPA)[:, None]
    else:
        y = a
    assert scale == (1.0 if (src[1] != 0) == (dst[1] != 0) else KAPPA)
    return np.ascontiguousarray(y).view(np.complex128).reshape(-1)


def carries_flip(sub):
    """The closed-form subspaces whose rows i and dim - 1 - i are complements of each other."""
    from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve
    if isinstance(sub, Explicit):
        return False
    if isinstance(sub, Full):
        return True
    if isinstance(sub, Parity):
        return sub.L % 2 == 0
    if isinstance(sub, SpinConserve):
        return sub.L == 2 * sub.k
    return False


def sector_weights(x, side):
    """``(magnetization (L + 1,), flip (2,) or None)`` of dnm_sector_weights for the vector ``x`` as it lies."""
    sub, sector, swz = side
    L = sub.L
    n = rows_of(side)
    x = np.ascontiguousarray(x, dtype=np.complex128)
    assert x.size == n
    nat = x[vec_pos(np.arange(n, dtype=np.int64), swz)]          # index order
    w = nat.real ** 2 + nat.imag ** 2
    cfg = np.asarray(sub.idx_to_state(np.arange(n, dtype=np.int64)), dtype=np.int64)
    k = np.array([bin(int(c)).count("1") for c in cfg], dtype=np.int64)
    if sector:
        mag = np.bincount(k, weights=w / 2, minlength=L + 1) + np.bincount(L - k, weights=w / 2, minlength=L + 1)
        flip = np.array([w.sum(), 0.0]) if sector > 0 else np.array([0.0, w.sum()])
        return mag, flip
    mag = np.bincount(k, weights=w, minlength=L + 1)
    if not carries_flip(sub):
        return mag, None
    first = cfg[((cfg >> (L - 1)) & 1) == 0]
    a = nat[np.asarray(sub.state_to_idx(first))]
    b = nat[np.asarray(sub.state_to_idx(first ^ ((1 << L) - 1)))]
    plus, minus = a + b, a - b
    flip = np.array([np.sum((plus.real ** 2 + plus.imag ** 2) / 2), np.sum((minus.real ** 2 + minus.imag ** 2) / 2)])
    return mag, flip


def gaussian_integers(n, seed):
    """complex128 amplitudes with integer components in [-8, 8]: sums of a few thousand of their products are exact."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-8, 9, size=n) + 1j * rng.integers(-8, 9, size=n)).astype(np.complex128)
