"""tests/tiled_exact_ref.py -- the int64 reference of the tiled multiply that tests/test_gpu_tiled_exact.py compares the
kernels with -- pinned to the oracle on every (operator, subspace, arithmetic) triple the GPU file uses, and to
tests/plan_emulator.py on a handful of the smallest cases; and the COVERAGE PROOF of the GPU file's case table: for
every case a DNM_MAT_HOST_ONLY handle is opened with the case's knobs and flags, and from what it exports
(dnm_mat_export_pass, _export_tabs, _export_flip, _export_flip_pass, _export_diag_tables, dnm_mat_plan_counts)
``derive`` works out, pass by pass, which kernel instance matvec_kernels.hip: launch_cfg picks and which record
classes and diagonal forms the pass carries.  The union over the table must hold every instance, (B, logR) pair, record
class and diagonal form; the GPU file asserts the same derivation, case by case, on the handle it multiplies with."""
import ctypes as C

import numpy as np
import pytest

import tiled_exact_ref as ref
from dynamite_amd import _lib, backend
from oracle import oracle as orc
import plan_emulator as pe
from test_diag_tables import DiagTables
from test_flipflop import FlipPass

FULL, PARITY = 0, 1          # dnm_subspace.type (include/dynamite_amd.h)
INSTANCES = ("plain-late", "plain-early", "GLDS", "PACK", "TAB", "DT", "DT+GLDS", "FLIP", "FLIP+GLDS", "FLIP+DT",
             "FLIP+DT+GLDS")
PAIRS = ((8, 2), (10, 2), (11, 2), (12, 2), (10, 3), (10, 4), (11, 3), (11, 4), (12, 3), (12, 4), (13, 3), (13, 4))
LP = ["LP_TILE_REAL_K0", "LP_TILE_REAL", "LP_TILE_CPLX", "LP_TILE_KVAR_REAL", "LP_TILE_KVAR_CPLX", "LP_GATHER_REAL",
      "LP_GATHER_KVAR_REAL", "LP_GATHER_CPLX", "LP_GATHER_KVAR_CPLX"]
FL = ["FL_TILE_T", "FL_TILE_K", "FL_GATHER_U", "FL_GATHER_B"]
MAXDSEL = 3
KNOBS = ("DNM_TILE_BITS", "DNM_LOG_ROWS", "DNM_PLAN_MODE", "DNM_AMIN", "DNM_GBITS", "DNM_FLIPFLOP", "DNM_DIAG_TABLE",
         "DNM_DIAG_BLOCK_TABLE", "DNM_DIAG_GROUPS", "DNM_TAB_RECORDS", "DNM_TAB_LOG_ROWS", "DNM_CACHE_POLICY")


def descriptor(sub, L, S):
    d = _lib.Subspace()
    d.type, d.L = (FULL if sub[0] == 'full' else PARITY), L
    if sub[0] == 'parity':
        d.space = sub[1]
    d.vec_swizzle = S
    return d


def set_knobs(monkeypatch, case):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.knobs.items():
        monkeypatch.setenv(k, str(v))


def open_raw(case, flags=0, rank=0, nranks=1):
    """dnm_mat_create of a case (the knobs are in the environment already): (handle, descriptors to keep alive)"""
    left, right = descriptor(case.left, case.L, case.S), descriptor(case.right, case.L, case.S)
    h = backend.create_mat(*ref.arrays(case.op, case.L), left, right, False, case.flags | flags, rank, nranks)
    return h, (left, right)


def plan_counts(h):
    vals = [C.c_int() for _ in range(6)]
    _lib.check(_lib.lib().dnm_mat_plan_counts(h, *[C.byref(v) for v in vals]))
    return [v.value for v in vals]         # local passes, remote passes, tiled, B, logR, n_loc


class _H:
    """what plan_emulator.HostMat's exporters need of a handle"""

    def __init__(self, h):
        self.h = h

    _export = pe.HostMat._export


def derive(h, flags, remote=0):
    """Per pass of the handle (local ones; remote=1: the partner passes), what the kernel would run: a dict with
    ``instance`` (launch_cfg's choice), ``pair`` (B, logR), ``classes`` (the non-empty record classes), ``diag`` (the form
    of the diagonal), ``accumulate``, ``window`` (the tile has more than one segment), ``swz`` (non-zero swz_xor_y /
    swz_xor_src)."""
    counts = plan_counts(h)
    assert counts[2] == 1, "not a tiled handle"
    out = []
    for i in range(counts[remote]):
        whole, quads = _H(h)._export(remote, i)
        fp = FlipPass(_H(h), i, remote)
        d = fp.desc if fp.on else whole
        qs = fp.quads if fp.on else quads
        dt = DiagTables(h, i, remote)
        R = 1 << d.log_rows
        pack = bool(d.cache_policy & 256)
        tab = d.tab_loop[2] > 0 or d.gbucket[_lib.MAXR] > d.gbucket[0]
        isdt = bool(d.has_diag) and dt.on
        gv = 1 if d.cache_policy & 32 else 0
        glds = bool(flags & _lib.MAT_USE_GLDS)
        # matvec_kernels.hip: launch_cfg
        assert not isdt or (not pack and not tab and gv == 1)
        if fp.on:
            assert not pack and not tab and gv == 1
            inst = "FLIP" + ("+DT" if isdt else "") + ("+GLDS" if glds else "")
        elif pack:
            inst = "PACK"
        elif tab:
            inst = "TAB"
        elif isdt:
            inst = "DT+GLDS" if glds else "DT"
        elif glds:
            inst = "GLDS"
        else:
            inst = "plain-early" if gv else "plain-late"
        classes = {LP[c] for c in range(_lib.LP_COUNT) if d.loop[c + 1] > d.loop[c]}
        if d.tab_loop[1] > d.tab_loop[0]:
            classes.add("TAB_TILE")
        if d.tab_loop[2] > d.tab_loop[1]:
            classes.add("TAB_GATHER")
        if fp.on:
            classes |= {FL[c] for c in range(_lib.FL_COUNT) if fp.loop[c + 1] > fp.loop[c]}
        diag = set()
        if not d.has_diag:
            diag.add("none")
        elif isdt:
            diag.add("DT%d" % len(dt.masks))
        else:
            slots = [j for j in range(R) if d.dbucket[j + 1] > d.dbucket[j]]
            if d.dext_end > d.dext_begin and not slots and qs.dtile is None and not d.gbucket[_lib.MAXR] > d.gbucket[0]:
                diag.add("dext-only")
            if d.dext_end > d.dext_begin:
                diag.add("dext")
            if slots:
                diag.add("dbucket%d" % min(len(slots), 4))
                if len(slots) > 4:
                    diag.add("dbucket>4")
            if qs.dtile is not None and slots:
                diag.add("dtile+lists")
            if qs.dtile is not None:
                diag.add("dtile")
            if d.gbucket[_lib.MAXR] > d.gbucket[0]:
                diag.add("gbucket")
            if fp.on and fp.dconst != 0.0:
                diag.add("dconst")
        out.append(dict(instance=inst, pair=(d.tile_bits, d.log_rows), classes=classes, diag=diag,
                        accumulate=bool(d.accumulate), window=d.nseg > 1, swz=bool(d.swz_xor_y or d.swz_xor_src),
                        need_tile=bool(d.need_tile), nwg=1 << (d.n_eff - d.tile_bits)))
    return out


def signature(passes):
    """what a case pins of its handle: per pass (instance, pair, sorted classes, sorted diagonal forms)"""
    return [(p["instance"], p["pair"], tuple(sorted(p["classes"])), tuple(sorted(p["diag"]))) for p in passes]


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------

def _orc_sub(sub, L):
    return orc.full(L) if sub[0] == 'full' else orc.parity(L, sub[1])


def test_subspace_states():
    for sub in (('full',), ('parity', 0), ('parity', 1)):
        st = ref.sub_states(sub, 9)
        assert np.array_equal(st, _orc_sub(sub, 9).i2s(np.arange(st.size, dtype=np.int64)))
        assert np.array_equal(ref.sub_index(sub, 9, st), np.arange(st.size))


@pytest.mark.parametrize("triple", ref.triples_used(), ids=str)
def test_reference_is_the_oracle(triple):
    """H x, H x - b z and H x - b z + c z2 of the case's own vectors against the oracle; the fused sums against a
    longdouble sum of the oracle's exact products."""
    op, L, left, right, real = triple
    r = ref.get(op, L, left, right)
    p = ref.product(op, L, left, right, real)
    assert p.amp == 8 and not ref.FALLBACK          # (no case had to fall back to [-2, 2])
    assert op in ref.REAL_OPS or not real
    hx = orc.matvec(orc.Msc(*r.arrs), _orc_sub(left, L), _orc_sub(right, L), np.array(p.x),
                    nthreads=min(8, orc.max_threads()))
    assert np.array_equal(p.y, hx)
    if real:
        assert not r.arrs[3].imag.any() and not p.y.imag.any()
    if not r.square:
        return
    assert np.array_equal(p.y_z, hx - ref.B * p.z)
    assert np.array_equal(p.y_z2, (hx - ref.B * p.z) + p.c * p.z2)
    for y, sums in ((p.y, p.sums), (p.y_z, p.sums_z)):
        d = np.sum(np.conj(p.x).astype(np.clongdouble) * y.astype(np.clongdouble))
        n2 = np.sum(y.real.astype(np.longdouble) ** 2 + y.imag.astype(np.longdouble) ** 2)
        assert (float(d.real), float(d.imag), float(n2)) == tuple(sums.tolist())
    if r.M > 1 << 18:
        ref.release()


def test_columns_are_the_products_of_unit_vectors():
    for op, L, sub in (("dm", 10, ('full',)), ("syk", 9, ('parity', 1)), ("xstring", 10, ('full',))):
        r = ref.get(op, L, sub)
        for j in (0, r.N // 3, r.N - 1):
            e = np.zeros(r.N, dtype=np.complex128)
            e[j] = 1
            want = orc.matvec(orc.Msc(*r.arrs), _orc_sub(sub, L), _orc_sub(sub, L), e)
            assert np.array_equal(r.column(j), want)


def test_operators_are_what_their_names_say():
    for name in ref.OPERATORS:
        arrs = ref.arrays(name, 13)
        assert (not arrs[3].imag.any()) == (name in ref.REAL_OPS), name
        assert np.all(np.diff(arrs[0]) > 0)
    assert ref.arrays("hops", 13)[0][0] != 0                       # no diagonal at all
    masks = ref.arrays("pk_flip0", 13)[0].tolist()
    assert 1 in masks and all(m in (0, 1) for m in masks)          # site 0 flipped alone
    assert all(m == 0 or (m & 1 and bin(m).count('1') == 2) for m in ref.arrays("pk_flip0x", 13)[0].tolist())
    a = ref.arrays("pk_sign0", 13)
    assert not (a[0] & 1).any() and (a[2] & 1).any()
    assert max(np.diff(ref.arrays("syk", 13)[1])) >= 8


# ---------------------------------------------------------------------------------------------------------------------
# coverage of the GPU file's case table, from HOST_ONLY handles
# ---------------------------------------------------------------------------------------------------------------------

_DERIVED = {}


def derived(monkeypatch, name):
    if name not in _DERIVED:
        case = ref.CASES[name]
        set_knobs(monkeypatch, case)
        h, keep = open_raw(case, _lib.MAT_HOST_ONLY)
        try:
            _DERIVED[name] = derive(h, case.flags)
        finally:
            _lib.lib().dnm_mat_destroy(h)
    return _DERIVED[name]


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_case_runs_what_it_is_named_for(monkeypatch, name):
    """the instance(s) a case names are the ones its handle runs on (the GPU file asserts the same on the real handle)"""
    case = ref.CASES[name]
    passes = derived(monkeypatch, name)
    got = [p["instance"] for p in passes]
    assert got == list(case.instances), (name, signature(passes))
    assert all(p["pair"] == case.pair for p in passes), signature(passes)


def _union(monkeypatch):
    return [(n, p) for n in sorted(ref.CASES) for p in derived(monkeypatch, n)]


def test_every_instance_is_reached(monkeypatch):
    seen = {p["instance"] for _, p in _union(monkeypatch)}
    assert seen == set(INSTANCES), set(INSTANCES) - seen


def test_every_tile_configuration_is_reached(monkeypatch):
    """each of the twelve (B, logR) pairs of tile_config_supported, on the plain and on the FLIP instances at least"""
    u = _union(monkeypatch)
    for fam in ("plain", "FLIP"):
        seen = {p["pair"] for _, p in u if p["instance"].startswith(fam)}
        assert seen >= set(PAIRS), (fam, sorted(set(PAIRS) - seen))


def test_every_record_class_is_reached(monkeypatch):
    seen = set()
    for _, p in _union(monkeypatch):
        seen |= p["classes"]
    want = set(LP) | set(FL) | {"TAB_TILE", "TAB_GATHER"}
    assert seen >= want, sorted(want - seen)


def test_every_diagonal_form_is_reached(monkeypatch):
    seen = set()
    for _, p in _union(monkeypatch):
        seen |= p["diag"]
    want = {"none", "dext-only", "dbucket1", "dbucket2", "dbucket3", "dbucket4", "dtile+lists", "gbucket", "dconst",
            "DT0", "DT1", "DT2", "DT%d" % MAXDSEL}
    assert seen >= want, sorted(want - seen)


def test_pass_structures_are_reached(monkeypatch):
    """plans of one pass and of several (the later ones accumulate), plans with a window pass"""
    by_case = {n: derived(monkeypatch, n) for n in ref.CASES}
    assert any(len(ps) == 1 for ps in by_case.values())
    multi = [ps for ps in by_case.values() if len(ps) > 1]
    assert multi and all(not ps[0]["accumulate"] and all(p["accumulate"] for p in ps[1:]) for ps in by_case.values())
    assert any(p["window"] for ps in by_case.values() for p in ps)
    assert any(p["nwg"] == 1 for ps in by_case.values() for p in ps) and any(p["nwg"] > 1 for ps in by_case.values() for p in ps)


def test_sub_block_passes_carry_the_swizzle_of_their_offset(monkeypatch):
    """partner passes of a partitioned handle in a swizzled layout: non-zero swz_xor_y / swz_xor_src"""
    hit = False
    for name, P in ref.SHARES:
        case = ref.CASES[name]
        set_knobs(monkeypatch, case)
        for rank in range(P):
            h, keep = open_raw(case, _lib.MAT_HOST_ONLY, rank, P)
            if plan_counts(h)[1]:
                hit = hit or any(p["swz"] for p in derive(h, case.flags, remote=1))
            _lib.lib().dnm_mat_destroy(h)
    assert hit


# ---------------------------------------------------------------------------------------------------------------------
# the emulator and the reference agree
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ref.EMULATED)
def test_emulator_equals_reference(monkeypatch, name):
    """plan_emulator.multiply (the generic records of every pass, in numpy doubles) on the exact inputs of the smallest
    cases: with dyadic coefficients and integer amplitudes its doubles are exact too."""
    case = ref.CASES[name]
    set_knobs(monkeypatch, case)
    left, right = descriptor(case.left, case.L, case.S), descriptor(case.right, case.L, case.S)
    hm = pe.HostMat(*ref.arrays(case.op, case.L), left, right, flags=case.flags)
    assert hm.tiled == 1
    p = ref.product(case.op, case.L, case.left, case.right, case.real)
    n = 1 << hm.n_loc
    pos = pe.vec_pos(np.arange(n), case.S)
    if case.real:
        xe = np.array(p.x.real).view(np.complex128)
        img = np.zeros(n, dtype=np.complex128)
        img[pos] = xe
        y = pe.multiply(hm, img)[pos]
        assert np.array_equal(y.view(np.float64), p.y.real)
    else:
        img = np.zeros(n, dtype=np.complex128)
        img[pos] = p.x
        y = pe.multiply(hm, img)[pos]
        assert np.array_equal(y, p.y)
