"""
The diagonal of a pass as tables (dynamite_amd/csrc/plan.h: DevPass::dblock; passes.cpp: build_diag_tables) without a
GPU: one double per workgroup for the terms outside the tile, sections of 2^B doubles for the terms that see the tile.
The operators have dyadic coefficients (J = 0.25, anisotropy 0.5, fields in multiples of 1/8), so every partial sum of a
diagonal is exact in double whatever its order, and the tables are compared with the diagonal of the MSC bit for bit:

    dblock[block(r)] + dtile[section(r)][t(r)]  ==  sum_t c_t (-1)^popcount(state(r) & sign_t)  -  sum_bonds c [bits agree]

for every row r of the rank -- the second sum is what the exchanges of the flip-flop form (plan.h: DevFlip) take back
from the diagonal: the coefficient c of every bond that runs as a tile record, on the rows whose two bits agree (none
with DNM_FLIPFLOP=0).
"""
import ctypes as C

import numpy as np
import pytest

from dynamite_amd import _lib, models
from dynamite_amd.operators import sigmax, sigmay, sigmaz, op_sum
from dynamite_amd.subspaces import Full, Parity
import plan_emulator as pe
from test_flipflop import FlipPass, _host, _cfg, _pairs


def _fields(L):
    return [((7 * i + 3) % 17 - 8) / 8.0 for i in range(L)]


def dy_mbl(L):
    """isotropic bonds and fields"""
    H = op_sum(0.25 * op_sum(s(i) * s(i + 1) for s in (sigmax, sigmay, sigmaz)) for i in range(L - 1))
    H = H + op_sum(h * sigmaz(i) for i, h in enumerate(_fields(L)) if h)
    H.L = L
    return H


def dy_aniso(L, extra=()):
    """anisotropy 0.5: every exchange leaves a ZZ term behind; with fields"""
    H = op_sum(0.25 * (sigmax(i) * sigmax(i + 1) + sigmay(i) * sigmay(i + 1)) + 0.125 * sigmaz(i) * sigmaz(i + 1)
               for i in range(L - 1))
    H = H + op_sum(h * sigmaz(i) for i, h in enumerate(_fields(L)) if h)
    for t in extra:
        H = H + t
    H.L = L
    return H


def dy_xxz(L):
    return models.xxz(L, 0.5)


def dy_cross(L):
    """ZZ couplings (8,11), (7,12), (6,13) on top of the chain: across the boundary of a tile [0,10) they and the chain's own
    (9,10) have four distinct outside parts and four distinct parts inside -- no three of them form a group (a plain
    next-nearest ZZ chain has at most three outside parts at this boundary, and three terms on spin 9 once it reaches
    further: a group)"""
    assert L >= 14
    return dy_aniso(L, [0.125 * sigmaz(8) * sigmaz(11), 0.375 * sigmaz(7) * sigmaz(12), 0.125 * sigmaz(6) * sigmaz(13)])


DYADIC = {"mbl": dy_mbl, "aniso": dy_aniso, "xxz": dy_xxz}


class DiagTables:
    """dnm_mat_export_diag_tables of one pass of a handle: ``on`` False when the pass evaluates its diagonal from records"""

    def __init__(self, handle, idx, remote=0):
        L = _lib.lib()
        nb, nt, nm = C.c_int64(), C.c_int64(), C.c_int()
        _lib.check(L.dnm_mat_export_diag_tables(handle, remote, idx, None, 0, C.byref(nb), None, 0, C.byref(nt), None,
                                                C.byref(nm)))
        self.on = nb.value > 0
        if not self.on:
            assert nt.value == 0 and nm.value == 0
            return
        self.dblock, self.dtile = np.empty(nb.value), np.empty(nt.value)
        masks = (C.c_uint64 * 3)()
        _lib.check(L.dnm_mat_export_diag_tables(handle, remote, idx, self.dblock.ctypes.data_as(_lib.f64p), nb.value,
                                                C.byref(nb), self.dtile.ctypes.data_as(_lib.f64p), nt.value, C.byref(nt),
                                                masks, C.byref(nm)))
        self.masks = [int(masks[i]) for i in range(nm.value)]
        assert all(self.masks) and len(set(self.masks)) == nm.value <= 3 and not any(masks[i] for i in range(nm.value, 3))

    def rows(self, desc):
        """the diagonal the kernel reads for every row of the pass: what tile_pass_body forms from the tables"""
        B, n = desc.tile_bits, 1 << desc.n_eff
        assert self.dblock.size == n >> B and self.dtile.size == (1 << B) << len(self.masks)
        r = np.arange(n, dtype=np.uint64)
        tb, t, b = 0, np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        for j in range(desc.nseg):
            tb |= ((1 << desc.seg_len[j]) - 1) << desc.seg_pos[j]
            t |= ((r >> np.uint64(desc.seg_pos[j])) & np.uint64((1 << desc.seg_len[j]) - 1)).astype(np.int64) << desc.seg_off[j]
        for j in range(desc.nbseg):
            b |= ((r >> np.uint64(desc.bseg_pos[j])) & np.uint64((1 << desc.bseg_len[j]) - 1)).astype(np.int64) << desc.bseg_off[j]
        sbase = (r & ~np.uint64(tb)) | np.uint64(desc.sign_base)
        sec = np.zeros(n, dtype=np.int64)
        for i, m in enumerate(self.masks):
            assert m & tb == 0
            sec |= (pe._popc(sbase & np.uint64(m)) & 1) << i
        return self.dblock[b] + self.dtile[(sec << B) + t]


def msc_diagonal(arrs, sub, rows):
    """the diagonal of the MSC at the given rows of the subspace (index space: Full the state, Parity state >> 1)"""
    masks, offs, signs, coeffs = arrs
    rows = np.asarray(rows, dtype=np.uint64)
    if isinstance(sub, Parity):
        states = (rows << np.uint64(1)) | ((pe._popc(rows) & 1) ^ int(sub.space)).astype(np.uint64)
    else:
        states = rows
    d = np.zeros(rows.size)
    for mi, m in enumerate(masks):
        if m != 0:
            continue
        for t in range(offs[mi], offs[mi + 1]):
            assert coeffs[t].imag == 0
            d += np.where(pe._popc(states & np.uint64(signs[t])) & 1, -coeffs[t].real, coeffs[t].real)
    return d


def kernel_passes(hm):
    """(description, flip-flop form or None) of what the kernel runs on, per local pass"""
    out = []
    for i, (desc, _) in enumerate(hm.local):
        fp = FlipPass(hm, i)
        out.append((fp.desc if fp.on else desc, fp if fp.on else None))
    return out


def exchange_part(hm, n_loc, rank):
    """sum over the bonds that run as exchanges of c on the rows whose two bits agree"""
    rows = (np.arange(1 << n_loc, dtype=np.uint64)) | np.uint64(rank << n_loc)
    out = np.zeros(rows.size)
    for desc, fp in kernel_passes(hm):
        if fp is None:
            continue
        for F in fp.flips[:fp.loop[2]]:
            m = 0
            for k in range(desc.nseg):
                m |= ((F.mask_tile >> desc.seg_off[k]) & ((1 << desc.seg_len[k]) - 1)) << desc.seg_pos[k]
            # known answers, independent of the export: every bond of these chains is 0.25 (XX + YY) + d ZZ, so an
            # exchange has c = 0.5 and sits on two index bits that are neighbours (Parity: one step down)
            assert bin(m).count("1") == 2 and m % 3 == 0 and bin(m // 3).count("1") == 1 and F.c == 0.5
            out += np.where(pe._popc(rows & np.uint64(m)) & 1, 0.0, F.c)
    return out


def outside_parts(desc, quads):
    """the distinct outside parts of the diagonal terms that see the tile and bits outside it (the bucket lists)"""
    out = set()
    for q in range(desc.dbucket[0], desc.dbucket[_lib.MAXR]):
        out |= {int(quads[q].sign_ext[j]) for j in range(quads[q].nslots)}
    return out - {0}


SPACES = {"full": lambda L: Full(L=L), "parity0": lambda L: Parity(0, L=L), "parity1": lambda L: Parity(1, L=L)}


@pytest.mark.parametrize("rank,nranks", [(0, 1), (1, 2), (3, 4)])
@pytest.mark.parametrize("space", sorted(SPACES))
def test_tables_equal_the_msc_diagonal(monkeypatch, space, rank, nranks):
    L = 14
    sub = SPACES[space](L)
    kinds, nchecked = set(), 0
    for name in sorted(DYADIC):
        for B, logR in ((8, 2), (8, 3), (10, 2), (10, 3)):
            if B == 8 and logR == 3:
                continue            # (no kernel instance of 32 threads: tile_config_supported)
            for flip in ("1", "0"):
                for where in ("first", "last"):
                    _cfg(monkeypatch, B, logR, 2, 3)
                    monkeypatch.setenv("DNM_FLIPFLOP", flip)
                    monkeypatch.setenv("DNM_DIAG_PASS", where)
                    hm, arrs = _host(DYADIC[name](L), sub, rank=rank, nranks=nranks)
                    assert hm.tiled == 1, hm.describe()
                    n_loc = hm.n_loc
                    want = msc_diagonal(arrs, sub, np.arange(1 << n_loc, dtype=np.uint64) | np.uint64(rank << n_loc))
                    want -= exchange_part(hm, n_loc, rank)
                    seen = 0
                    for i, (desc, fp) in enumerate(kernel_passes(hm)):
                        T = DiagTables(hm.h, i)
                        # (Parity folds the dropped bit into the sign masks: a term that saw it spreads over the whole
                        # index, and a pass may then have more than three outside parts -- it keeps its lists)
                        quads = fp.quads if fp is not None else hm.local[i][1]
                        plain = desc.tab_loop[2] == 0 and desc.gbucket[_lib.MAXR] == desc.gbucket[0]
                        assert T.on == bool(desc.has_diag and plain and len(outside_parts(desc, quads)) <= 3), \
                            (name, B, logR, flip, where, hm.describe())
                        if space == "full":
                            assert T.on == bool(desc.has_diag)
                        if desc.has_diag and not T.on:
                            seen += 1
                        assert ("diag_tables=1" in hm.describe().splitlines()[1 + i]) == T.on
                        if not T.on:
                            continue
                        seen += 1
                        kinds.add(desc.nseg > 1)
                        assert rank == 0 or desc.sign_base != 0
                        got = T.rows(desc)
                        assert np.array_equal(got, want), (name, B, logR, flip, where, np.abs(got - want).max())
                        nchecked += 1
                    assert seen == 1
                    for i in range(hm.n_remote_passes):
                        assert not DiagTables(hm.h, i, remote=1).on
    # 36 plans per case; all of them have tables but five of the Parity plans of rank 1 of 2, whose diagonal pass has more
    # than three outside parts (counted above from the exported records)
    assert nchecked == (31 if space != "full" and nranks == 2 else 36), nchecked
    # the diagonal sat in a contiguous pass and in a window pass (a quarter of the Parity space, 2^11 rows, has no window
    # pass that qualifies)
    assert kinds == ({False, True} if space == "full" or nranks < 4 else {False})


def test_knob_restores_the_lists(monkeypatch):
    L = 14
    _cfg(monkeypatch, 10, 2, 2, 3)
    monkeypatch.setenv("DNM_DIAG_BLOCK_TABLE", "0")
    hm, _ = _host(dy_mbl(L))
    assert not any(DiagTables(hm.h, i).on for i in range(hm.n_local_passes))
    assert "diag_tables" not in hm.describe()
    off = [(bytes(d), [bytes(q) for q in qs]) for d, qs in hm.local]
    monkeypatch.setenv("DNM_DIAG_BLOCK_TABLE", "1")
    hm1, _ = _host(dy_mbl(L))
    assert any(DiagTables(hm1.h, i).on for i in range(hm1.n_local_passes))
    # what dnm_mat_export_pass hands out -- description and records -- is the same with and without the tables
    assert off == [(bytes(d), [bytes(q) for q in qs]) for d, qs in hm1.local]
    for fl in ("0", "1"):                        # ... and so is the flip-flop form's description (dnm_mat_export_flip_pass)
        monkeypatch.setenv("DNM_DIAG_BLOCK_TABLE", fl)
        h, _ = _host(dy_aniso(L))
        fps = [FlipPass(h, i) for i in range(h.n_local_passes)]
        assert all(fp.on for fp in fps)
        got = [(bytes(fp.desc), [bytes(q) for q in fp.quads], fp.quads.dtile.tobytes() if fp.quads.dtile is not None else b"")
               for fp in fps]
        if fl == "0":
            first = got
    assert got == first
    monkeypatch.setenv("DNM_DIAG_BLOCK_TABLE", "1")
    monkeypatch.setenv("DNM_DIAG_TABLE", "0")          # no in-tile table: none of the others either
    hm2, _ = _host(dy_mbl(L))
    assert not any(DiagTables(hm2.h, i).on for i in range(hm2.n_local_passes))


def _bucket_terms(desc):
    return desc.dbucket[_lib.MAXR] - desc.dbucket[0]


def test_too_many_outside_parts_keeps_the_lists(monkeypatch):
    """Four ZZ couplings across the tile boundary with four distinct outside parts and no group among them: no tables, the
    bucket lists stay -- on both staging paths (the planner groups nothing under DNM_MAT_USE_GLDS)."""
    L = 14
    _cfg(monkeypatch, 10, 2, 1, 3)          # one pass, tile [0, 10)
    for flags in (0, _lib.MAT_USE_GLDS):
        hm, arrs = _host(dy_cross(L), flags=flags)
        assert hm.tiled == 1
        dp = [(i, desc, fp) for i, (desc, fp) in enumerate(kernel_passes(hm)) if desc.has_diag]
        assert len(dp) == 1
        i, desc, fp = dp[0]
        assert desc.gbucket[_lib.MAXR] == desc.gbucket[0] and desc.tab_loop[2] == 0
        parts = outside_parts(desc, fp.quads if fp is not None else hm.local[i][1])
        assert parts == {1 << 10, 1 << 11, 1 << 12, 1 << 13}
        assert not DiagTables(hm.h, i).on and _bucket_terms(desc) > 0
        assert "diag_tables" not in hm.describe()


@pytest.mark.parametrize("make,L,B", [(models.long_range, 14, 10), (models.syk, 12, 8)])
def test_grouped_terms_and_table_records_keep_the_lists(monkeypatch, make, L, B):
    """A pass with grouped diagonal terms (long_range) or table records (SYK) runs on the kernel instance that keeps the
    lists: no tables."""
    _cfg(monkeypatch, B, 2, 2, 3)
    hm, _ = _host(make(L))
    assert hm.tiled == 1
    special = 0
    for i, (desc, _) in enumerate(hm.local):
        special += desc.tab_loop[2] + desc.gbucket[_lib.MAXR] - desc.gbucket[0]
        if desc.tab_loop[2] or desc.gbucket[_lib.MAXR] > desc.gbucket[0]:
            assert not DiagTables(hm.h, i).on
    assert special > 0
    assert not any(DiagTables(hm.h, i).on for i in range(hm.n_local_passes) if hm.local[i][0].has_diag)
