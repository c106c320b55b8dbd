"""The case table of tests/test_gpu_sc_rows_exact.py -- the SpinConserve multiply in REFERENCE order: sc_block_kernel<10, 64>,
sc_block_kernel<13, 512>, sc_matvec_kernel and sc_matvec_fused_kernel -- and what each case reaches, derived from L, k and
the block width alone.

The exact reference itself is tests/sc3_exact_ref.py (``Ref``, ``Product``, ``fused_sums8`` and their 2^53 assertions):
reference order is its native order, so it is imported, not copied.  Added here:

  * three operators the block form needs (``far_small``: non-fast masks on the per-row path at ordinary L; ``graph70``:
    more masks than the block form takes), handed to ``sc3_exact_ref.Ref`` as arrays (``get`` / ``product`` here);
  * a restatement of csrc/mat.cpp: setup_sc_block -- which block form a handle chooses, its range of high parts, the
    swizzle, the block order of DNM_SC_ORDER / DNM_SC_CHUNK with its 0xffffffff holes -- and of the workgroup-to-block
    map of sc_block_kernel, so that the GPU file can hold dnm_mat_export_sc_block against it and the CPU file can prove
    which register rows, block orders and early returns the table reaches;
  * the arms of every mask class a case takes (high bond up / down, low bond up / down, boundary bond up / down, per-row
    path inside and leaving the subspace, complemented mask inside and leaving).

tests/test_sc_rows_exact_ref.py pins every reference used here to the oracle and asserts ``NEEDS`` on the table."""
from math import comb

import numpy as np

import sc3_exact_ref as ref
import wide_ref
from dynamite_amd.operators import sigmax, sigmay, sigmaz, sigma_plus, sigma_minus, op_product

NT = {10: 64, 13: 512}           # threads of a workgroup of the two instances (csrc/matvec_kernels.hip: launch_sc_block)
RPT = 4                          # register rows: ceil(C(10, 5) / 64) = ceil(C(13, 6) / 512) = 4
MAXM = 64                        # masks the block form takes (SCB_MAXM)
HOLE = 0xffffffff


# ---------------------------------------------------------------------------------------------------------------------
# operators
# ---------------------------------------------------------------------------------------------------------------------

def far_small(L, lb):
    """wide_ref.chain plus a hop between sites 0 and L-1, a hop between lb-2 and lb+1 (not adjacent, across the block
    boundary), ZZ between 0 and L-1 and sigma+ sigma- sigma+ sigma- + h.c. on (0, lb-1, lb, L-1): the couplings of
    wide_ref.far on sites that exist at ordinary L.  All real, all eighths."""
    assert 0 < lb - 2 and lb + 1 <= L - 1 and lb < L - 1
    hop = lambda i, j: sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j)
    a, b, c, d = 0, lb - 1, lb, L - 1
    quad = op_product([sigma_plus(a), sigma_minus(b), sigma_plus(c), sigma_minus(d)])
    quad = quad + op_product([sigma_minus(a), sigma_plus(b), sigma_minus(c), sigma_plus(d)])
    return (wide_ref.chain(L) + 0.625 * hop(0, L - 1) + 1.75 * hop(lb - 2, lb + 1) + (-1.375) * sigmaz(0) * sigmaz(L - 1)
            + 0.125 * quad)


OPERATORS = {
    'far10': lambda L: far_small(L, 10), 'far13': lambda L: far_small(L, 13),
    # 70 bonds: 71 masks with the diagonal, more than the block form's 64
    'graph70': lambda L: ref.pair_graph(L, seed=70, nbonds=70, complex_hops=False, fields=True),
}
REAL_OPS = ref.REAL_OPS + tuple(OPERATORS)
_own = {}


def get(op, L, k, sector=None):
    """sc3_exact_ref.get, and the same for the operators of this module (handed to Ref as arrays)"""
    if op not in OPERATORS:
        return ref.get(op, L, k, sector)
    assert sector is None
    if (op, L, k) not in _own:
        r = ref.Ref(op, L, k, arrs=wide_ref.marshal(OPERATORS[op](L), L))
        _own[op, L, k] = (r, ref.Product(r, False))
    return _own[op, L, k][0]


def product(op, L, k, sector=None):
    if op not in OPERATORS:
        return ref.product(op, L, k, sector, False)
    get(op, L, k)
    return _own[op, L, k][1]


# ---------------------------------------------------------------------------------------------------------------------
# csrc/mat.cpp: setup_sc_block and csrc/matvec_kernels.hip: the block id -> high part map, restated
# ---------------------------------------------------------------------------------------------------------------------

def is_fast(mask, ts):
    """csrc/kernels.h: ScMask::fast -- a bond of two adjacent spins whose sign masks all lie inside the bond"""
    lo = (mask & -mask).bit_length() - 1
    return mask != 0 and mask == 3 << lo and all(sg & ~mask == 0 for sg, _, _ in ts)


def chosen_block(r, knob):
    """The low bits per block a handle of Ref ``r`` runs on under DNM_SC_BLOCK=``knob`` (None: unset), 0: the row kernel."""
    if knob == 0:
        return 0
    lb = 13 if knob is None else knob
    assert lb in (10, 13)
    nmasks = len(r.terms)
    if nmasks > MAXM or r.L <= lb or r.L - lb > 48:
        return 0
    if knob is None:
        if (r.N >> (r.L - lb)) < 256:
            return 0
        if 2 * sum(is_fast(m, ts) for m, ts in r.terms) < nmasks:
            return 0
    return lb


def block_order(k, lb, hf, hl, g, chunk):
    """The block order of DNM_SC_ORDER = g > 0 (setup_sc_block): the high parts with rows sorted by (chunk, popcount,
    bits above g, value), runs of equal (bits above g, popcount) dealt round-robin to eight lists, the lists
    interleaved and padded with holes."""
    if chunk is None or chunk <= 0 or chunk > 40:
        chunk = 62
    ent = [e for e in range(hl - hf + 1) if 0 <= k - bin(hf + e).count('1') <= lb]
    ent.sort(key=lambda e: ((hf + e) >> chunk, bin(hf + e).count('1'), (hf + e) >> g, hf + e))
    lists = [[] for _ in range(8)]
    i = q = 0
    while i < len(ent):
        h0 = hf + ent[i]
        j = i
        while j < len(ent) and (hf + ent[j]) >> g == h0 >> g and bin(hf + ent[j]).count('1') == bin(h0).count('1'):
            j += 1
        lists[q & 7] += ent[i:j]
        q += 1
        i = j
    longest = max(len(l) for l in lists)
    perm = np.full(longest * 8, HOLE, dtype=np.uint32)
    for x, l in enumerate(lists):
        perm[x:8 * len(l):8] = l
    return perm


class BlockPlan:
    """What setup_sc_block decides for the rows [row0, row0 + m) of SpinConserve(L, k) (XParity: of its first half) at
    ``lb`` low bits under DNM_SC_ORDER=``order`` / DNM_SC_CHUNK=``chunk`` (None: unset), and what the launch then does:
    ``visits`` -- workgroup -> high part or -1 where the workgroup returns before it reads a row."""

    def __init__(self, states, L, k, lb, order=None, chunk=None, row0=0, m=None):
        m = states.size - row0 if m is None else m
        self.L, self.k, self.lb, self.row0, self.m = L, k, lb, row0, m
        hf, hl = int(states[row0]) >> lb, int(states[row0 + m - 1]) >> lb
        self.swizzle = 0
        if hl - (hf & ~511) + 1 >= 1024:
            self.swizzle, hf = 1, hf & ~511
        self.h_first, self.h_last = hf, hl
        span = hl - hf + 1
        g = 6 if span >= 1024 else 0
        if order is not None:
            g = order
        self.perm = block_order(k, lb, hf, hl, g, chunk) if g > 0 else None
        self.nperm = 0 if self.perm is None else int(self.perm.size)
        self.kind = 'permutation' if self.perm is not None else ('swizzle' if self.swizzle else 'ascending')
        self.grid = self.nperm if self.perm is not None else ((span + 511) & ~511 if self.swizzle else span)
        # the launch: block id -> high part, early returns
        first = (states >> lb)
        self.visits = np.full(self.grid, -1, dtype=np.int64)
        for b in range(self.grid):
            if self.perm is not None:
                if self.perm[b] == HOLE:
                    continue
                hrel = int(self.perm[b])
            elif self.swizzle:
                seq, xcd = b >> 3, b & 7
                hrel = ((seq >> 6) << 9) | (xcd << 6) | (seq & 63)
            else:
                hrel = b
            H = hf + hrel
            kl = k - bin(H).count('1')
            if H > hl or kl < 0 or kl > lb:
                continue
            self.visits[b] = H
        # the blocks with rows of this share: (high part, first local row, rows, whole?)
        Hs = first[row0:row0 + m]
        self.blocks = {}
        for H in np.unique(Hs).tolist():
            n = comb(lb, k - bin(H).count('1'))
            mine = int(np.count_nonzero(Hs == H))
            self.blocks[H] = (n, mine)

    def fields(self):
        """what dnm_mat_export_sc_block returns"""
        return [self.lb, self.h_first, self.h_last, self.swizzle, self.nperm, self.grid]

    def sizes(self):
        """the sizes of the blocks that hold rows of the share, in ascending order of the high part"""
        return [self.blocks[H][0] for H in sorted(self.blocks)]

    def register_rows(self):
        """the register rows r // NT that hold a row of some block"""
        return sorted({r // NT[self.lb] for n in self.sizes() for r in (0, n - 1)} |
                      {i for n in self.sizes() for i in range((n + NT[self.lb] - 1) // NT[self.lb])})

    def ragged(self):
        """some block ends inside the LAST register row, short of its end"""
        return any(n > (RPT - 1) * NT[self.lb] and n % NT[self.lb] for n in self.sizes())

    def partial(self):
        """blocks of which the share holds only a part (r_lo > 0 or r_hi < nrows)"""
        return [H for H, (n, mine) in self.blocks.items() if mine < n]

    def early(self):
        """workgroups that return before they read a row (a hole, a high part past the last, kl out of range)"""
        return int(np.count_nonzero(self.visits < 0))

    def check(self):
        """every block with rows is visited exactly once, nothing else is"""
        seen = self.visits[self.visits >= 0]
        assert np.unique(seen).size == seen.size
        with_rows = {H for H in range(self.h_first, self.h_last + 1) if 0 <= self.k - bin(H).count('1') <= self.lb}
        assert set(seen.tolist()) == with_rows and set(self.blocks) <= with_rows


def plan_of(r, lb, order=None, chunk=None, row0=0, m=None):
    return BlockPlan(r.states, r.L, r.k, lb, order, chunk, row0, m)


def arms(r, lb):
    """The arms of every mask class the rows of Ref ``r`` take, as a set of words.  lb > 0: sc_block_kernel (classes 0,
    1, 2 of its ballots); lb == 0: the row kernels."""
    out = set()
    st = r.states
    for mask, ts in r.terms:
        if mask == 0:
            out.add('diagonal')
            continue
        if is_fast(mask, ts):
            lo = (mask & -mask).bit_length() - 1
            pair = (st >> lo) & 3
            where = 'fast' if lb == 0 else ('high' if lo >= lb else ('boundary' if lo == lb - 1 else 'low'))
            if (pair == 1).any():
                out.add(where + ' up')
            if (pair == 2).any():
                out.add(where + ' down')
            if ((pair == 0) | (pair == 3)).any():
                out.add(where + ' idle')
            continue
        stays = np.bitwise_count(st ^ np.int64(mask)) == r.k
        what = 'complemented' if mask & (mask + 1) == 0 else 'general'
        if stays.any():
            out.add(what + ' inside')
        if (~stays).any():
            out.add(what + ' leaves')
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------

def case(op, L, k, sector=None, block=None, order=None, chunk=None, fuse=True):
    """block: DNM_SC_BLOCK (None: unset, 0: the row kernel), order: DNM_SC_ORDER, chunk: DNM_SC_CHUNK (None: unset),
    fuse False: DNM_ROW_FUSE=0"""
    return dict(op=op, L=L, k=k, sector=sector, block=block, order=order, chunk=chunk, fuse=fuse)


def name_of(c):
    s = '%s-%d-%d%s' % (c['op'], c['L'], c['k'], c['sector'] or '')
    s += {None: '-default', 0: '-rows'}.get(c['block'], '-b%s' % c['block'])
    if c['order'] is not None:
        s += '-o%d' % c['order']
    if c['chunk'] is not None:
        s += '-c%d' % c['chunk']
    return s + ('' if c['fuse'] else '-unfused')


BLOCK_SHAPES = {10: (14, 6), 13: (17, 7)}
BLOCK_OPS = ('chain', 'dm', 'nnn', 'long', 'hops_dm', 'far', 'graph_c', 'graph_cf')     # far: far10 / far13 by the width

_cases = []
for _lb, (_L, _k) in BLOCK_SHAPES.items():
    for _o in BLOCK_OPS:
        for _ord in (0, 3):
            _cases.append(case(_o + str(_lb) if _o == 'far' else _o, _L, _k, block=_lb, order=_ord))
# edge sectors of the 10-bit instance: blocks of 1 and 10 rows, dimension 1
for _L, _k in ((14, 1), (14, 13), (12, 0), (12, 12)):
    _cases.append(case('dm', _L, _k, block=10, order=0))
# the XCD swizzle: exactly 1024 high parts; span 2047 (grid 2048, the last workgroup has no block); 1024 high parts of
# which nearly all return early ((23, 3) ends at high part 896 and so runs ascending: (24, 3) is its swizzled twin)
SWIZZLE = [case('dm', 20, 10, block=10, order=0), case('dm', 21, 10, block=10, order=0),
           case('dm', 23, 3, block=13, order=0), case('dm', 23, 20, block=13, order=0),
           case('dm', 24, 3, block=13, order=0)]
# the default permutation (g = 6 from 1024 high parts on), DNM_SC_CHUNK once, and the production instance with no knob
DEFAULT_ORDER = [case('dm', 20, 10, block=10), case('dm', 20, 10, block=10, chunk=4)]
PRODUCTION = case('dm', 23, 11)
# XParity: the complemented-mask branch, in both block forms and in the row kernels
XPARITY = [case(_o, _L, _L // 2, sector=_s, block=_b, order=0 if _b else None)
           for _L in (16, 14) for _s in '+-' for _o in ('chain_xp', 'graph_xp') for _b in (10, 13, 0)]
# what falls back to one row per thread although the knob asks for a block form
FALLBACK = [case('graph70', 14, 6, block=10), case('dm', 13, 6, block=13), case('dm', 10, 5, block=10)]
# the row kernel and its fused twin
ROW_SHAPES = [(12, 6), (16, 8), (17, 7), (20, 10)]
ROWS = [case({'far': 'far10' if _L < 16 else 'far13'}.get(_o, _o), _L, _k, block=0, fuse=_f)
        for _L, _k in ROW_SHAPES for _o in ('chain', 'dm', 'far', 'graph_cf') for _f in (True, False)]
_cases += SWIZZLE + DEFAULT_ORDER + [PRODUCTION] + XPARITY + FALLBACK + ROWS
CASES = {name_of(c): c for c in _cases}
assert len(CASES) == len(_cases)

# planted columns, shares, row ranges, rounding: (operator, L, k, sector, DNM_SC_BLOCK)
PLANTED = [('dm', 14, 6, None, 10), ('far10', 14, 6, None, 10), ('dm', 17, 7, None, 13), ('far13', 17, 7, None, 13),
           ('dm', 14, 6, None, 0), ('far13', 17, 7, None, 0), ('chain_xp', 16, 8, '-', 10), ('chain_xp', 16, 8, '-', 0)]
# (operator, L, k, DNM_SC_BLOCK, DNM_SC_ORDER, rank counts).  No third of (20, 10) spans 1024 high parts, so its shares
# run ascending although the whole subspace swizzles; the last share of (24, 3) and the first of (21, 18) end or begin
# at a high part beyond 1024 with few rows before it: those are the shares under the swizzle, at both widths.
SHARES = [('dm', 14, 6, 10, None, (2, 3, 5)), ('dm', 17, 7, 13, None, (2, 3, 5)), ('dm', 20, 10, 10, 0, (3,)),
          ('dm', 24, 3, 13, 0, (2, 3)), ('dm', 21, 18, 10, 0, (3,))]
SWIZZLED_SHARES = {(24, 3), (21, 18)}
ROUNDING = [('block 10', 'dm', 14, 6, None, 10), ('block 13', 'dm', 17, 7, None, 13),
            ('per-row path in the block form', 'graph_cf', 14, 6, None, 10), ('row kernel', 'dm', 16, 8, None, 0),
            ('XParity', 'chain_xp', 16, 8, '-', 13)]

# What every kernel instance needs of the table as a whole (tests/test_sc_rows_exact_ref.py asserts it).
BLOCK_ARMS = {'diagonal', 'high up', 'high down', 'high idle', 'low up', 'low down', 'low idle', 'boundary up',
              'boundary down', 'boundary idle', 'general inside', 'general leaves', 'complemented inside',
              'complemented leaves'}
NEEDS = {
    10: dict(register_rows=[0, 1, 2, 3], ragged=True, full_block=252, orders={'ascending', 'swizzle', 'permutation'},
             early_returns=True, no_block_for_last_workgroup=True, holes=True, sizes_one_and_lb=True, arms=BLOCK_ARMS),
    13: dict(register_rows=[0, 1, 2, 3], ragged=True, full_block=1716, orders={'ascending', 'swizzle', 'permutation'},
             early_returns=True, no_block_for_last_workgroup=False, holes=True, sizes_one_and_lb=False, arms=BLOCK_ARMS),
    0: dict(arms={'diagonal', 'fast up', 'fast down', 'fast idle', 'general inside', 'general leaves',
                  'complemented inside', 'complemented leaves'},
            walk_steps={0, 1, 4},            # steps of the unranking walk above bit 16: L = 12 / 16, 17, 20
            ragged_last_workgroup=True, fused_and_plain=True),
}


def pairs_used():
    """every (operator, L, k, sector) a GPU test takes a reference for"""
    out = {(c['op'], c['L'], c['k'], c['sector']) for c in CASES.values()}
    out |= {p[:4] for p in PLANTED} | {(s[0], s[1], s[2], None) for s in SHARES} | {q[1:5] for q in ROUNDING}
    out |= {('dm', 14, 6, None)}                 # the row ranges
    return sorted(out, key=str)
