"""Host references for the sweeps that visit every row or column and reduce to a small answer (the infinity norm, the
cached diagonal, CheckConserves, the column window / chunk map / local rows of a window partition), restated in numpy
from the MSC definition and the subspace maps (Subspace.idx_to_state / state_to_idx) in integer and double arithmetic,
and the operators with a planted row that make one row decide the answer.

Every operator built here has dyadic coefficients (small integers times a power of two): every partial sum is exact in
double whatever the order of summation, so these references are bit-exact expectations.
tests/test_row_sweep_ref.py pins them against the oracle."""
import numpy as np

from dynamite_amd import msc_tools
from dynamite_amd.operators import sigmax, sigmay, sigmaz, identity, op_sum
from dynamite_amd.subspaces import Explicit

ROWS_PER_WG = 256          # rows of a workgroup of the one-thread-per-row kernels


def marshal(H, L):
    """(masks, mask_offsets, signs, coeffs) of an operator, as build_mat receives them."""
    H.L = L
    H.reduce_msc()
    masks, offs = msc_tools.get_mask_offsets(H.msc)
    return (np.ascontiguousarray(masks, dtype=np.int64), np.ascontiguousarray(offs, dtype=np.int64),
            np.ascontiguousarray(H.msc['signs'], dtype=np.int64), np.ascontiguousarray(H.msc['coeffs'], dtype=np.complex128))


def parity(v):
    if hasattr(np, "bitwise_count"):
        return (np.bitwise_count(np.asarray(v, dtype=np.int64)) & 1).astype(np.int64)
    v = np.asarray(v, dtype=np.uint64).copy()
    for s in (32, 16, 8, 4, 2, 1):
        v ^= v >> np.uint64(s)
    return (v & np.uint64(1)).astype(np.int64)


def real_coeffs(coeffs):
    """One double per term: the real part if non-zero, else the imaginary part."""
    return np.where(coeffs.real != 0, coeffs.real, coeffs.imag)


def elements(arrs, left, right, row0, m):
    """The matrix elements of rows [row0, row0 + m), one per (row, mask): cols[m, nmasks] (the column
    s2i_R(i2s_L(row) ^ mask), -1 outside the right subspace) and re / im [m, nmasks], the sum of +-c_t over the mask's
    terms with the sign taken on bra = ket ^ mask and the split by parity(mask & sign)."""
    masks, offs, signs, coeffs = arrs
    rc = real_coeffs(coeffs)
    ket = np.asarray(left.idx_to_state(np.arange(row0, row0 + m, dtype=np.int64)), dtype=np.int64).reshape(-1)
    cols = np.empty((m, masks.size), dtype=np.int64)
    re = np.zeros((m, masks.size))
    im = np.zeros((m, masks.size))
    for i, mask in enumerate(masks):
        bra = ket ^ mask
        cols[:, i] = right.state_to_idx(bra)
        for t in range(offs[i], offs[i + 1]):
            v = (1 - 2 * parity(bra & signs[t])) * rc[t]
            if parity(np.array([mask & signs[t]]))[0]:
                im[:, i] += v
            else:
                re[:, i] += v
    return cols, re, im


def row_sums(arrs, left, right, row0=0, m=None):
    """sum_m |sum_t +-c_t| of rows [row0, row0 + m) (MatNorm_CPU's row sums); their maximum is the norm of these rows."""
    m = left.get_dimension() - row0 if m is None else m
    cols, re, im = elements(arrs, left, right, row0, m)
    return np.where(cols >= 0, np.hypot(re, im), 0.0).sum(axis=1)


def diagonal(arrs, sub, row0=0, m=None):
    """The diagonal of rows [row0, row0 + m): the terms of mask 0 on the row's own state."""
    masks, offs, signs, coeffs = arrs
    assert masks.size and masks[0] == 0
    m = sub.get_dimension() - row0 if m is None else m
    rc = real_coeffs(coeffs)
    st = np.asarray(sub.idx_to_state(np.arange(row0, row0 + m, dtype=np.int64)), dtype=np.int64).reshape(-1)
    d = np.zeros(m)
    for t in range(offs[1]):
        d += (1 - 2 * parity(st & signs[t])) * rc[t]
    return d


def conserves(arrs, left, right, xparity=False):
    """(verdict, violating columns): a column violates when some mask takes its state out of the left subspace with a
    non-zero (complex) sum of its terms.  xparity: only the first half of the columns is looked at."""
    masks, offs, signs, coeffs = arrs
    n = right.get_dimension() // (2 if xparity else 1)
    bra = np.asarray(right.idx_to_state(np.arange(n, dtype=np.int64)), dtype=np.int64).reshape(-1)
    bad = np.zeros(n, dtype=bool)
    for i, mask in enumerate(masks):
        out = np.asarray(left.state_to_idx(bra ^ mask)).reshape(-1) == -1
        v = np.zeros(n, dtype=np.complex128)
        for t in range(offs[i], offs[i + 1]):
            v += (1 - 2 * parity(bra & signs[t])) * coeffs[t]
        bad |= out & (v != 0)
    cols = np.nonzero(bad)[0]
    return cols.size == 0, cols


def column_sets(arrs, left, right, row0, m):
    """(reach, need, cols) of the rows [row0, row0 + m): every column some mask reaches, those among them whose summed
    coefficient is non-zero (both sorted, unique), and the per-(row, mask) columns they were taken from."""
    cols, re, im = elements(arrs, left, right, row0, m)
    inside = cols >= 0
    return np.unique(cols[inside]), np.unique(cols[inside & ((re != 0) | (im != 0))]), cols


def hull(*sets):
    """[min, max] of the union of integer sets / (lo, hi) pairs; None when all are empty."""
    allv = np.concatenate([np.asarray(s, dtype=np.int64).reshape(-1) for s in sets])
    return (int(allv.min()), int(allv.max())) if allv.size else None


def coarsen(byte_map, lo, shift):
    """The chunk map at 2^shift columns per chunk that the one-column map over [lo, lo + len) amounts to."""
    col = lo + np.nonzero(byte_map)[0]
    out = np.zeros(((lo + byte_map.size - 1) >> shift) - (lo >> shift) + 1, dtype=np.uint8)
    out[(col >> shift) - (lo >> shift)] = 1
    return out


def local_runs(cols, col_lo, col_hi, per=ROWS_PER_WG):
    """Runs [b0, b1) of consecutive workgroups (``per`` rows each) none of whose rows reaches a column outside
    [col_lo, col_hi)."""
    m = cols.shape[0]
    nb = (m + per - 1) // per
    ok = []
    for b in range(nb):
        c = cols[b * per:(b + 1) * per]
        c = c[c >= 0]
        ok.append(c.size == 0 or (c.min() >= col_lo and c.max() < col_hi))
    runs, b = [], 0
    while b < nb:
        if not ok[b]:
            b += 1
            continue
        e = b
        while e < nb and ok[e]:
            e += 1
        runs.append((b, e))
        b = e
    return runs


def select_runs(runs, m, max_ranges, min_blocks, per=ROWS_PER_WG):
    """The row ranges dnm_mat_window_local_rows hands out: runs of at least min_blocks workgroups, the max_ranges
    longest, in ascending order.  None where runs of equal length meet at the cut: which of them stays is not defined."""
    runs = [r for r in runs if r[1] - r[0] >= max(1, min_blocks)]
    by_len = sorted(runs, key=lambda r: r[0] - r[1])
    if len(by_len) > max_ranges:
        if by_len[max_ranges - 1][1] - by_len[max_ranges - 1][0] == by_len[max_ranges][1] - by_len[max_ranges][0]:
            return None
        by_len = by_len[:max_ranges]
    return [(b0 * per, min(m, b1 * per)) for b0, b1 in sorted(by_len)]


# ---------------------------------------------------------------------------------------------------------------------
# operators with a planted row
# ---------------------------------------------------------------------------------------------------------------------

def planted_fields(L, rstar):
    """1 + sum_i h_i Z_i with h_i = +-2^-(i+1), signed so that D(r) = 1 + sum_i h_i (-1)^{r_i} has its unique maximum
    2 - 2^-L at r = rstar; a state that differs from rstar in the bits S has D lower by sum_{i in S} 2^-i (at least
    2^(1-L)), and every D(r) >= 2^-L is non-zero."""
    return identity() + op_sum((-1.0 if (rstar >> i) & 1 else 1.0) * 2.0 ** -(i + 1) * sigmaz(i) for i in range(L))


def planted_operator(L, rstar, variant):
    """Variant 'A' (real): the planted fields, 0.25 X_3 and the bond 0.125 (X_0 X_1 + Y_0 Y_1) (an element 0.25 where
    spins 0 and 1 differ).  Variant 'B': A plus 0.375 X_5 + 0.5 Y_5, one element of magnitude 5/8 with both parts."""
    H = planted_fields(L, rstar) + 0.25 * sigmax(3) + 0.125 * (sigmax(0) * sigmax(1) + sigmay(0) * sigmay(1))
    if variant == 'B':
        H = H + 0.375 * sigmax(5) + 0.5 * sigmay(5)
    else:
        assert variant == 'A'
    return marshal(H, L)


PARTNER_MASKS = (3, 1 << 3, 1 << 5)      # the off-diagonal masks of the planted operators
_PARTNER_BITS = 3 | 1 << 3 | 1 << 5


def explicit_with_planted(L, n, index, seed):
    """(sorted states, rstar): n random states of L spins with rstar at position ``index``.  rstar's partners under
    the planted operators' masks are in the basis too (all above it, or all below it in the upper half), so that no
    other row gains more from the off-diagonal terms than rstar does and rstar keeps the largest row sum."""
    rs = np.random.RandomState(seed)
    base = np.unique(rs.randint(0, 1 << L, size=n + n // 4 + 64).astype(np.int64))
    assert base.size >= n + 64
    # (the candidate sits a little further up than ``index``: clearing or setting its mask bits moves it past a few
    # neighbours, and the surplus below and above it is dropped afterwards)
    if index < n // 2:      # partners above: the mask bits of rstar clear
        rstar = int(base[index + (16 if index else 0)]) & ~_PARTNER_BITS
    else:                   # partners below: the mask bits set
        rstar = int(base[index + 16]) | _PARTNER_BITS
    special = np.array(sorted({rstar} | {rstar ^ p for p in PARTNER_MASKS}), dtype=np.int64)
    rest = base[~np.isin(base, special)]
    below, above = rest[rest < rstar], rest[rest > rstar]
    nsb = int((special < rstar).sum())
    nsa = special.size - 1 - nsb
    kb, ka = index - nsb, n - 1 - index - nsa
    assert 0 <= kb <= below.size and 0 <= ka <= above.size, (index, kb, below.size, ka, above.size)
    states = np.sort(np.concatenate([below[below.size - kb:], special, above[:ka]]))
    assert states.size == n and states[index] == rstar
    return states, rstar


def outsider_at(sector_states, j, L):
    """A state of L spins outside the (sorted) sector that sorts to position j among its states, or None."""
    lo = int(sector_states[j - 1]) + 1 if j > 0 else 0
    hi = int(sector_states[j]) if j < sector_states.size else 1 << L
    return lo if lo < hi else None


def states_of(sub):
    return np.asarray(sub.idx_to_state(np.arange(sub.get_dimension(), dtype=np.int64)), dtype=np.int64).reshape(-1)


def explicit(states, L):
    return Explicit(np.ascontiguousarray(states, dtype=np.int64), L=L)


# ---------------------------------------------------------------------------------------------------------------------
# the cases the CPU and the GPU tests share
# ---------------------------------------------------------------------------------------------------------------------

TRIP = 4096 * ROWS_PER_WG      # rows one trip of norm_kernel's grid-stride loop covers (the grid is capped at 4096)

NORM_SHAPES = ('full', 'parity', 'sc', 'explicit')      # the smallest of each type with a second trip
NORM_DIMS = {'full': 1 << 21, 'parity': 1 << 21, 'sc': 1352078, 'explicit': TRIP + 777}


def norm_placements(M):
    """Where the planted row goes: first workgroup (both ends), second workgroup, both sides of the trip boundary, wave 3
    lane 37 of the first workgroup of the second trip, a row of the last workgroup (ragged where M is no multiple of 256)
    and the last row."""
    tail = M - 1 - (M % ROWS_PER_WG or ROWS_PER_WG) // 2
    return [0, 255, 256, TRIP - 1, TRIP, TRIP + 3 * 64 + 37, tail, M - 1]


def norm_case(shape, index, variant):
    """(subspace, operator arrays, planted state) of a norm shape with the planted row at ``index``."""
    from dynamite_amd.subspaces import Full, Parity, SpinConserve
    if shape == 'explicit':
        states, rstar = explicit_with_planted(22, NORM_DIMS[shape], index, seed=7)
        sub = explicit(states, 22)
    else:
        sub = {'full': lambda: Full(L=21), 'parity': lambda: Parity('odd', L=22), 'sc': lambda: SpinConserve(23, 11)}[shape]()
        rstar = int(sub.idx_to_state(index))
    assert sub.get_dimension() == NORM_DIMS[shape]
    return sub, planted_operator(sub.L, rstar, variant), rstar


def pair_subspaces(L=13):
    """One subspace of each type that all hold the state ``rstar`` (and, the Explicit one, its partners under the
    planted masks), for the 16 (left, right) pairs."""
    from dynamite_amd.subspaces import Full, Parity, SpinConserve
    sc = SpinConserve(L, 6)
    rstar = int(sc.idx_to_state(777))                  # six spins down: even parity
    rs = np.random.RandomState(13)
    st = np.unique(np.concatenate([rs.randint(0, 1 << L, size=3000), [rstar] + [rstar ^ p for p in PARTNER_MASKS]]))
    return {'full': Full(L=L), 'parity': Parity('even', L=L), 'sc': sc, 'explicit': explicit(st, L)}, rstar


def conserves_sector(kind, L, alt=0):
    from dynamite_amd.subspaces import Full, Parity, SpinConserve
    if kind == 'full':
        return Full(L=L)
    if kind == 'parity':
        return Parity(alt, L=L)
    if kind == 'sc':
        return SpinConserve(L, L // 2 - alt)
    rs = np.random.RandomState(5)
    return explicit(np.unique(rs.randint(0, 1 << L, size=6000)), L)


def conserves_columns(N, sliced=False):
    """Planted columns: both ends of the first workgroup, the second, the last column, one in the ragged tail (where
    there is one); with launches of 2^10 columns also both sides of the first slice boundary."""
    cols = [0, 255, 256, N - 1]
    if N % ROWS_PER_WG:
        cols.append(N - 1 - (N % ROWS_PER_WG) // 2)
    if sliced:
        cols += [1023, 1024]
    return sorted(set(c for c in cols if 0 <= c < N))


def minus_one(right, j):
    """left = Explicit(states of right without the one at column j): column j alone leaves the left subspace."""
    return explicit(np.delete(states_of(right), j), right.L)


def plus_outsider(kind, j, L):
    """(left, right): left a Parity / SpinConserve sector, right = Explicit(its states and one outsider that sorts to
    column j).  Of the two sectors of the kind, the first that has room for an outsider at that place."""
    for alt in (0, 1):
        left = conserves_sector(kind, L, alt)
        st = states_of(left)
        o = outsider_at(st, j, L)
        if o is not None:
            right = explicit(np.insert(st, j, o), L)
            assert right.rmap_indices is None and right.state_map[j] == o
            return left, right
    raise AssertionError("no outsider sorts to column %d" % j)


def window_operator(L):
    """Nearest-neighbour and third-neighbour hops (elements that vanish where the two spins agree: reached but not
    needed) and ZZ couplings, dyadic coefficients."""
    hop = lambda i, j: sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j)
    H = op_sum(0.5 * hop(i, i + 1) for i in range(L - 1)) + op_sum(0.25 * hop(i, i + 3) for i in range(0, L - 3, 2))
    H = H + op_sum(2.0 ** -(i % 5) * sigmaz(i) * sigmaz(i + 1) for i in range(L - 1))
    return marshal(H, L)


def far_column_case(pos, with_partner=True, L=16, n_low=3000):
    """(subspace, operator arrays): X_{L-1} plus a diagonal on n_low states below 2^(L-1) (no partner of theirs is in
    the basis) and, with_partner, the partner p ^ 2^(L-1) of the state p at position ``pos`` -- it sorts last."""
    rs = np.random.RandomState(16)
    low = np.unique(rs.randint(0, 1 << (L - 1), size=2 * n_low))[:n_low].astype(np.int64)
    assert low.size == n_low
    states = np.concatenate([low, [low[pos] | 1 << (L - 1)]]) if with_partner else low
    return explicit(states, L), marshal(planted_fields(L, 0) + sigmax(L - 1), L)
