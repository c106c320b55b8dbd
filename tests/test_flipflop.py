"""
Flip-flop records (dynamite_amd/csrc/plan.h: DevFlip) without a GPU: which masks the host code takes as such, what it
leaves of the diagonal, and a numpy emulation of the records' arithmetic (the exchange of the tile records, the liveness
of the gathered ones, the reduced diagonal and its constant) against ``plan_emulator``'s result for the generic pass the
same handle exports.
"""
import ctypes as C

import numpy as np
import pytest

from dynamite_amd import _lib, models, msc_tools
from dynamite_amd.operators import sigmax, sigmay, sigmaz, op_sum
from dynamite_amd.subspaces import Full, Parity
from oracle import oracle as orc
import plan_emulator as pe
from plan_emulator import HostMat

EPS = 2.2e-16


def _arrs(H):
    H.establish_L()
    H.reduce_msc()
    masks, offs = msc_tools.get_mask_offsets(H.msc)
    return masks, offs, np.ascontiguousarray(H.msc["signs"]), np.ascontiguousarray(H.msc["coeffs"])


def tol_for(arrs, x):       # tests/test_gpu_matvec.py
    return 8 * len(arrs[0]) * EPS * max(1.0, np.abs(arrs[3]).max()) * max(1.0, np.abs(x).max())


def _cfg(monkeypatch, B, logR, mode=2, amin=3, gbits=3):
    monkeypatch.setenv("DNM_GBITS", str(gbits))
    monkeypatch.setenv("DNM_TILE_BITS", str(B))
    monkeypatch.setenv("DNM_LOG_ROWS", str(logR))
    monkeypatch.setenv("DNM_PLAN_MODE", str(mode))
    monkeypatch.setenv("DNM_AMIN", str(amin))


def _rand(n, seed=0):
    rs = np.random.RandomState(seed)
    return rs.standard_normal(n) + 1j * rs.standard_normal(n)


def xx_chain(L):
    return models.bench_xx(L)


def dm_chain(L):
    """Heisenberg bonds with a Dzyaloshinskii-Moriya term: the bond masks carry an imaginary part."""
    H = op_sum(0.25 * op_sum(s(i) * s(i + 1) for s in (sigmax, sigmay, sigmaz))
               + 0.1 * (sigmax(i) * sigmay(i + 1) - sigmay(i) * sigmax(i + 1)) for i in range(L - 1))
    H.L = L
    return H


def aniso_chain(L):
    """d != a, with a field"""
    H = op_sum(0.25 * (sigmax(i) * sigmax(i + 1) + sigmay(i) * sigmay(i + 1)) + 0.425 * sigmaz(i) * sigmaz(i + 1)
               + 0.3 * sigmaz(i) for i in range(L - 1))
    H.L = L
    return H


def alternating_chain(L):
    """couplings of alternating sign"""
    H = op_sum((-1) ** i * (0.25 + 0.01 * i) * op_sum(s(i) * s(i + 1) for s in (sigmax, sigmay, sigmaz))
               for i in range(L - 1))
    H.L = L
    return H


class FlipPass:
    """What the kernel reads for one pass of a handle: None when the pass runs on its generic records."""

    def __init__(self, hm, idx, remote=0):
        L = _lib.lib()
        n = C.c_int()
        loops = (C.c_uint32 * (_lib.FL_COUNT + 1))()
        dconst = C.c_double()
        _lib.check(L.dnm_mat_export_flip(hm.h, remote, idx, None, 0, 0, C.byref(n), loops, C.byref(dconst)))
        self.on = n.value >= 0
        if not self.on:
            return
        recs = (_lib.DevFlip * max(1, n.value))()
        _lib.check(L.dnm_mat_export_flip(hm.h, remote, idx, recs, C.sizeof(_lib.DevFlip), n.value, C.byref(n), loops,
                                         C.byref(dconst)))
        self.flips = [recs[i] for i in range(n.value)]
        self.loop = list(loops)
        self.dconst = dconst.value
        nq, nd = C.c_int(), C.c_int64()
        _lib.check(L.dnm_mat_export_flip_pass(hm.h, remote, idx, None, 0, None, 0, 0, C.byref(nq), None, 0, C.byref(nd)))
        self.desc = _lib.DevPass()
        quads = (_lib.DevQuad * max(1, nq.value))()
        dt = np.zeros(max(1, nd.value))
        _lib.check(L.dnm_mat_export_flip_pass(hm.h, remote, idx, C.byref(self.desc), C.sizeof(self.desc), quads,
                                              C.sizeof(_lib.DevQuad), nq.value, C.byref(nq),
                                              dt.ctypes.data_as(_lib.f64p), dt.size, C.byref(nd)))
        self.quads = pe._Quads(quads[i] for i in range(nq.value))
        self.quads.dtile = dt if nd.value else None
        assert self.desc.nquads == nq.value and nd.value in (0, 1 << self.desc.tile_bits)

    def diag_signs(self):
        """(sign mask in index space, coefficient) of every term of the pass's diagonal lists"""
        d, out = self.desc, []
        if not d.has_diag:
            return out
        for q in list(range(d.dext_begin, d.dext_end)) + list(range(d.dbucket[0], d.dbucket[_lib.MAXR])):
            Q = self.quads[q]
            for j in range(Q.nslots):
                st, s = Q.sign_tile[j], Q.sign_ext[j]
                for k in range(d.nseg):
                    s |= ((st >> d.seg_off[k]) & ((1 << d.seg_len[k]) - 1)) << d.seg_pos[k]
                out.append((s, Q.coeff[j]))
        return out


def _natural(desc):
    nat = type(desc).from_buffer_copy(desc)
    nat.swz_shift = 0
    return nat


def run_flip_pass(hm, fp, x, y):
    """One pass as the flip-flop kernel instance runs it, on vectors in index order: the remaining generic records and
    the reduced diagonal by plan_emulator, then the flip-flop records and the constant as flip_tile / flip_gathers do."""
    desc = fp.desc
    pe.run_pass(hm, (_natural(desc), fp.quads), x, y)
    B, logR, n_loc = desc.tile_bits, desc.log_rows, desc.n_eff
    lognt = B - logR
    rows = np.arange(1 << n_loc, dtype=np.uint64)
    tile_bits = 0
    for j in range(desc.nseg):
        tile_bits |= ((1 << desc.seg_len[j]) - 1) << desc.seg_pos[j]

    def compress(v):
        out = np.zeros(v.shape, dtype=np.uint64)
        for j in range(desc.nseg):
            out |= ((v >> np.uint64(desc.seg_pos[j])) & np.uint64((1 << desc.seg_len[j]) - 1)) << np.uint64(desc.seg_off[j])
        return out

    def deposit(t):
        out = np.zeros(t.shape, dtype=np.uint64)
        for j in range(desc.nseg):
            out |= ((t >> np.uint64(desc.seg_off[j])) & np.uint64((1 << desc.seg_len[j]) - 1)) << np.uint64(desc.seg_pos[j])
        return out

    tt = compress(rows)
    base = rows & ~np.uint64(tile_bits)
    sbase = base | np.uint64(desc.sign_base)
    one = np.uint64(1)
    acc = np.zeros(1 << n_loc, dtype=np.complex128)
    for q, F in enumerate(fp.flips):
        cls = max(c for c in range(_lib.FL_COUNT) if fp.loop[c] <= q)
        assert F.c != 0.0
        if cls in (0, 1):
            assert F.p0 < F.p1 < B and F.mask_tile == (1 << F.p0) | (1 << F.p1)
            assert (F.p1 < lognt) == (cls == 0) and desc.need_tile
            differ = ((tt >> np.uint64(F.p0)) ^ (tt >> np.uint64(F.p1))) & one
            partner = base | deposit(tt ^ (np.uint64(F.mask_tile) & (np.uint64(0) - differ)))
            acc += F.c * x[partner.astype(np.int64)]
            continue
        if cls == 2:
            mloc = (1 << F.p0) | (1 << F.p1)
            assert F.p0 < F.p1 < n_loc and not (mloc & tile_bits)
            live = ((sbase >> np.uint64(F.p0)) ^ (sbase >> np.uint64(F.p1))) & one
        else:
            assert F.p0 < B and not ((tile_bits >> F.p1) & 1) and F.p1 < n_loc
            mloc = int(deposit(np.array([1 << F.p0], dtype=np.uint64))[0]) | (1 << F.p1)
            live = ((tt >> np.uint64(F.p0)) ^ (sbase >> np.uint64(F.p1))) & one
        assert F.mask_pos == int(pe.vec_pos(mloc, desc.swz_shift))
        acc += np.where(live == one, F.c * x[(rows ^ np.uint64(mloc)).astype(np.int64)], 0.0)
    if desc.has_diag:
        acc += fp.dconst * x
    else:
        assert fp.dconst == 0.0
    y += acc


def count_flips(handle, n_passes):
    """flip-flop records over the local passes of a handle (host-only or not)"""
    n = C.c_int()
    tot = 0
    for i in range(n_passes):
        _lib.check(_lib.lib().dnm_mat_export_flip(handle, 0, i, None, 0, 0, C.byref(n), None, None))
        tot += max(0, n.value)
    return tot


def flip_multiply(hm, x):
    y = np.zeros(1 << hm.n_loc, dtype=np.complex128)
    fps = [FlipPass(hm, i) for i in range(hm.n_local_passes)]
    for p, fp in zip(hm.local, fps):
        if fp.on:
            run_flip_pass(hm, fp, x, y)
        else:
            pe.run_pass(hm, (_natural(p[0]), p[1]), x, y)
    return y, fps


def generic_multiply(hm, x):
    y = np.zeros(1 << hm.n_loc, dtype=np.complex128)
    for desc, quads in hm.local:
        pe.run_pass(hm, (_natural(desc), quads), x, y)
    return y


def _host(H, sub=None, **kw):
    arrs = _arrs(H)
    sub = Full(L=H.L) if sub is None else sub
    return HostMat(*arrs, sub._c(), sub._c(), **kw), arrs


def _pairs(hm, fps, tile_only):
    """index-space masks of the flip-flop records of a handle"""
    out = []
    for fp in fps:
        if not fp.on:
            continue
        d = fp.desc
        for q, F in enumerate(fp.flips):
            if q < fp.loop[2]:
                m = 0
                for k in range(d.nseg):
                    m |= ((F.mask_tile >> d.seg_off[k]) & ((1 << d.seg_len[k]) - 1)) << d.seg_pos[k]
                out.append(m)
            elif not tile_only:
                out.append(None)
    return out


@pytest.mark.parametrize("name", ["heisenberg", "mbl"])
def test_all_bonds_taken(monkeypatch, name):
    """Every bond of the isotropic chains is a flip-flop record, no generic off-diagonal record is left, and the ZZ
    term of every bond that runs as an exchange is gone from what the kernel reads of the diagonal (-a per bond in
    the constant instead); the generic export still describes the whole pass."""
    L = 14
    _cfg(monkeypatch, 10, 2)
    hm, arrs = _host(models.BY_NAME[name](L))
    assert hm.tiled == 1
    fps = [FlipPass(hm, i) for i in range(hm.n_local_passes)]
    assert all(fp.on for fp in fps) and len(fps) >= 2
    assert sum(len(fp.flips) for fp in fps) == L - 1
    exch = [m for m in _pairs(hm, fps, True)]
    assert len(exch) >= 2 and {fp.loop[2] - fp.loop[0] > 0 for fp in fps} == {True}
    nz_generic = 0
    for (desc, quads), fp in zip(hm.local, fps):
        assert fp.desc.loop[_lib.LP_COUNT] == fp.desc.loop[0]            # nothing but flip-flop records off the diagonal
        nz_generic += desc.loop[_lib.LP_COUNT] - desc.loop[0]
        signs = fp.diag_signs()
        assert not [s for s, c in signs if s in exch]
        if fp.desc.has_diag:
            assert fp.dconst == -0.25 * len(exch)
            # the tabulated part: no component on the pair of an exchanged bond inside this tile
            tc = np.arange(1 << fp.desc.tile_bits, dtype=np.uint64)
            for F in fp.flips[:fp.loop[2]]:
                chi = 1.0 - 2.0 * (pe._popc(tc & np.uint64(F.mask_tile)) & 1)
                assert abs(np.dot(chi, fp.quads.dtile)) <= 1e-12 * tc.size
    assert nz_generic >= L - 1
    monkeypatch.setenv("DNM_FLIPFLOP", "0")
    hm0, _ = _host(models.BY_NAME[name](L))
    assert not any(FlipPass(hm0, i).on for i in range(hm0.n_local_passes))
    assert hm0.describe() == hm.describe()            # the plan's text speaks of passes and tiles, not of record kinds


def test_xxz_keeps_residual_zz(monkeypatch):
    L, delta = 14, 0.5
    _cfg(monkeypatch, 10, 2)
    hm, arrs = _host(models.xxz(L, delta))
    fps = [FlipPass(hm, i) for i in range(hm.n_local_passes)]
    assert sum(len(fp.flips) for fp in fps if fp.on) == L - 1
    exch = _pairs(hm, fps, True)
    dp = [fp for fp in fps if fp.on and fp.desc.has_diag]
    assert len(dp) == 1 and dp[0].dconst == -0.25 * len(exch)
    tc = np.arange(1 << dp[0].desc.tile_bits, dtype=np.uint64)
    resid = {s: c for s, c in dp[0].diag_signs()}
    for F in dp[0].flips[:dp[0].loop[2]]:             # in the tile of the diagonal pass: tabulated
        chi = 1.0 - 2.0 * (pe._popc(tc & np.uint64(F.mask_tile)) & 1)
        assert abs(np.dot(chi, dp[0].quads.dtile) / tc.size - 0.25 * (delta - 1)) <= 1e-14
    for m in exch:
        if m in resid:
            assert resid[m] == 0.25 * delta - 0.25


@pytest.mark.parametrize("make", [xx_chain, dm_chain, models.long_range, models.syk])
def test_none_taken(monkeypatch, make):
    L = 9 if make is models.syk else 13
    _cfg(monkeypatch, 8 if make is models.syk else 10, 2)
    H = make(L)
    hm, arrs = _host(H)
    assert hm.tiled == 1
    assert not any(FlipPass(hm, i).on for i in range(hm.n_local_passes))


@pytest.mark.parametrize("space", [0, 1])
def test_parity_takes_the_clean_bonds(monkeypatch, space):
    """Parity drops state bit 0 and folds it into the sign masks: the bond (0, 1) flips one index bit only, and every
    other bond's sign masks stay clear of the folded bit -- L - 2 records; the emulation agrees with the generic pass."""
    L = 14
    _cfg(monkeypatch, 10, 2)
    H = models.mbl(L)
    hm, arrs = _host(H, Parity(space, L=L))
    x = _rand(1 << hm.n_loc, 5)
    y, fps = flip_multiply(hm, x)
    assert sum(len(fp.flips) for fp in fps if fp.on) == L - 2
    assert np.max(np.abs(y - generic_multiply(hm, x))) <= tol_for(arrs, x)


CHAINS = {"mbl": models.mbl, "heisenberg": models.heisenberg, "xxz": models.xxz, "aniso": aniso_chain,
          "alternating": alternating_chain}


SHAPES14 = [(14, 10, 2, 2, 3), (14, 12, 2, 2, 4), (14, 10, 3, 0, 3)]
SHAPES20 = [(20, 10, 4, 2, 4), (20, 11, 3, 2, 3), (20, 12, 3, 2, 4), (20, 12, 2, 2, 4)]      # one isotropic, one anisotropic chain


@pytest.mark.parametrize("name,L,B,logR,mode,amin", [(n,) + s for n in sorted(CHAINS) for s in SHAPES14] +
                         [(n,) + s for n in ("mbl", "aniso") for s in SHAPES20])
def test_emulation_equals_generic(monkeypatch, name, L, B, logR, mode, amin):
    """The records the kernel runs on give what the exported generic pass gives (and the oracle at L = 14)."""
    _cfg(monkeypatch, B, logR, mode, amin, gbits=3 if L == 14 else 6)
    H = CHAINS[name](L)
    hm, arrs = _host(H)
    assert hm.tiled == 1
    x = _rand(1 << L, L)
    y, fps = flip_multiply(hm, x)
    assert sum(len(fp.flips) for fp in fps if fp.on) == L - 1, hm.describe()
    assert np.max(np.abs(y - generic_multiply(hm, x))) <= tol_for(arrs, x), hm.describe()
    if L == 14:
        ref = orc.matvec_general(orc.Msc(*arrs), orc.full(L), orc.full(L), x)
        assert np.max(np.abs(y - ref)) <= tol_for(arrs, x)


def test_partitioned_local_passes(monkeypatch):
    """Partitioned: the bonds inside a rank's block are flip-flop records of its local passes, the bond across the rank
    bit stays a generic partner pass; both emulations agree rank by rank."""
    L, P = 14, 2
    _cfg(monkeypatch, 10, 2)
    H = models.mbl(L)
    for r in range(P):
        hm, arrs = _host(H, rank=r, nranks=P)
        x = _rand(1 << hm.n_loc, 7 + r)
        y, fps = flip_multiply(hm, x)
        assert sum(len(fp.flips) for fp in fps if fp.on) == L - 2
        assert all(not FlipPass(hm, i, remote=1).on for i in range(hm.n_remote_passes))
        assert np.max(np.abs(y - generic_multiply(hm, x))) <= tol_for(arrs, x)


# ---- flip-flop bonds WITHOUT a ZZ term on their pair: an exchange would add a term to the diagonal per bond (and, three
# of them on one spin across the tile boundary of the diagonal pass, a group of terms, which another kernel instance
# runs) -- such bonds keep their generic tile records, only their gathered form is a flip-flop record

def xy_field_chain(L):
    from random import seed, uniform
    seed(3)
    H = op_sum(0.25 * (sigmax(i) * sigmax(i + 1) + sigmay(i) * sigmay(i + 1)) for i in range(L - 1))
    H = H + op_sum(uniform(-1, 1) * sigmaz(i) for i in range(L))
    H.L = L
    return H


def long_range_xy(L):
    """sum_{i<j} 0.25 / |i - j|^1.5 (XX + YY)_ij + sum_i h_i Z_i: every spin has partners all over the index"""
    from random import seed, uniform
    seed(4)
    H = op_sum(0.25 / (j - i) ** 1.5 * (sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j))
               for i in range(L) for j in range(i + 1, L))
    H = H + op_sum(uniform(-1, 1) * sigmaz(i) for i in range(L))
    H.L = L
    return H


NO_ZZ = {"xy_field": xy_field_chain, "long_range_xy": long_range_xy}


def assert_launchable(fps):
    """a pass with flip-flop records runs on the instance that knows them and nothing else: no table records, no
    grouped diagonal terms (matvec_kernels.hip: launch_cfg refuses such a pass)"""
    for fp in fps:
        if fp.on:
            assert fp.desc.tab_loop[2] == 0 and fp.desc.gbucket[_lib.MAXR] == fp.desc.gbucket[0]


@pytest.mark.parametrize("L,B,logR,mode,amin", [(14, 8, 2, 2, 3), (14, 10, 2, 2, 3), (15, 10, 3, 2, 4), (14, 10, 2, 0, 3)])
@pytest.mark.parametrize("name", sorted(NO_ZZ))
def test_bonds_without_zz(monkeypatch, name, L, B, logR, mode, amin):
    _cfg(monkeypatch, B, logR, mode, amin)
    H = NO_ZZ[name](L)
    hm, arrs = _host(H)
    assert hm.tiled == 1
    x = _rand(1 << L, L)
    y, fps = flip_multiply(hm, x)
    assert_launchable(fps)
    nbonds = len(arrs[0]) - 1                       # every mask but the diagonal is a flip-flop bond
    ngather = sum(d.loop[_lib.LP_COUNT] - d.loop[_lib.LP_GATHER[0]] for d, _ in hm.local)
    nflip = sum(len(fp.flips) for fp in fps if fp.on)
    # the gathered bonds, all of them and nothing else: no tile record, no constant, the diagonal as it was
    assert nflip == ngather and (ngather == 0 or 0 < nflip < nbonds), hm.describe()
    for (desc, quads), fp in zip(hm.local, fps):
        if fp.on:
            assert fp.loop[2] == 0 and fp.dconst == 0.0
            assert fp.desc.loop[_lib.LP_GATHER[0]] == fp.desc.loop[_lib.LP_COUNT]
            assert (fp.desc.dext_end - fp.desc.dext_begin, list(fp.desc.dbucket)) == \
                   (desc.dext_end - desc.dext_begin, list(desc.dbucket))
    assert np.max(np.abs(y - generic_multiply(hm, x))) <= tol_for(arrs, x), hm.describe()
    ref = orc.matvec_general(orc.Msc(*arrs), orc.full(L), orc.full(L), x)
    assert np.max(np.abs(y - ref)) <= tol_for(arrs, x)


def test_mixed_bonds(monkeypatch):
    """A chain whose even bonds carry ZZ and whose odd bonds do not: exchanges for the former, generic tile records
    for the latter, one diagonal that both agree on."""
    L = 14
    _cfg(monkeypatch, 10, 2)
    H = op_sum(0.25 * (sigmax(i) * sigmax(i + 1) + sigmay(i) * sigmay(i + 1))
               + (0.3 * sigmaz(i) * sigmaz(i + 1) if i % 2 == 0 else 0.2 * sigmaz(i)) for i in range(L - 1))
    H.L = L
    hm, arrs = _host(H)
    x = _rand(1 << L, 2)
    y, fps = flip_multiply(hm, x)
    assert_launchable(fps)
    exch = _pairs(hm, fps, True)
    assert exch and all((m & -m).bit_length() % 2 == 1 for m in exch)          # lowest bit of the pair: an even site
    assert sum(fp.desc.loop[_lib.LP_GATHER[0]] - fp.desc.loop[0] for fp in fps if fp.on) > 0
    assert np.max(np.abs(y - generic_multiply(hm, x))) <= tol_for(arrs, x)
    ref = orc.matvec_general(orc.Msc(*arrs), orc.full(L), orc.full(L), x)
    assert np.max(np.abs(y - ref)) <= tol_for(arrs, x)
