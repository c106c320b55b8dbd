"""
The SpinConserve multiply in REFERENCE order -- sc_block_kernel<10, 64>, sc_block_kernel<13, 512>, sc_matvec_kernel
(csrc/matvec_kernels.hip), sc_matvec_fused_kernel (csrc/row_fused_kernels.hip) and their launchers in csrc/mat_mult.cpp --
through the C ABI, one call at a time, on device buffers of the test's own, in exact arithmetic.

Method (that of tests/test_gpu_sc3_exact.py): coefficients are multiples of 1/8, amplitudes Gaussian integers in [-8, 8],
b = 3/8, c = -1/4 + 5/8 i.  tests/sc3_exact_ref.py works in int64 eighths and asserts on the numbers of every case that
sums of moduli stay below 2^53 in units of 1/64, so any order of summation, with or without fma, gives the same VALUE;
the comparisons are array_equal.  tests/test_sc_rows_exact_ref.py pins every reference used here to the oracle.

Buffers: reference order has no padding, a vector is dim elements (dim / 2 under XParity) between two guards of 64
complex128 elements.  The guards of x, z, z2 hold NaN; y and its guards hold a sentinel before every call.  After every
call: y equals the reference, both guards of y hold their bits, no NaN and no sentinel is in y, the inputs with their
guards are bit-identical to a device copy taken at upload, the fused sums equal the reference's, and the slots of dot an
entry does not own still hold the sentinel.

Every case asserts the route words of dnm_mat_plan_describe and, through dnm_mat_export_sc_block, the block width, the
range of high parts, the swizzle and the block order against what tests/sc_rows_exact_ref.py derives from L, k and the
knobs -- so no case silently runs another instance or another order.
"""
import ctypes as C

import numpy as np
import pytest

import sc3_exact_ref as ref
import sc_rows_exact_ref as t
from dynamite_amd import _lib, backend
from dynamite_amd.config import config
from dynamite_amd.subspaces import Explicit
from test_gpu_row_sweeps import chunks_of, local_rows_of
from test_gpu_sc3_exact import DBuf, ENTRIES
from test_gpu_vec import NAN, SENT, gamma

pytestmark = pytest.mark.gpu

BLOCK_WORDS, ROW_WORDS = "SpinConserve kernel, block form (%d low bits", "one row per thread"


@pytest.fixture(autouse=True)
def no_layout():
    """SpinConserve in reference order, whatever the dimension."""
    old = config.sc_layout
    config.sc_layout = None
    yield
    config.sc_layout = old


# ---------------------------------------------------------------- handles

def knobs_of(block=None, order=None, chunk=None, fuse=True):
    k = {}
    if block is not None:
        k["DNM_SC_BLOCK"] = str(block)
    if order is not None:
        k["DNM_SC_ORDER"] = str(order)
    if chunk is not None:
        k["DNM_SC_CHUNK"] = str(chunk)
    if not fuse:
        k["DNM_ROW_FUSE"] = "0"
    return k


def exported(mat):
    """(fields, block order or None) of dnm_mat_export_sc_block"""
    f = (C.c_int64 * 6)()
    _lib.check(_lib.lib().dnm_mat_export_sc_block(mat.handle, f, None, 0))
    f = list(f)
    if not f[4]:
        return f, None
    perm = np.full(f[4], 7, dtype=np.uint32)
    g = (C.c_int64 * 6)()
    _lib.check(_lib.lib().dnm_mat_export_sc_block(mat.handle, g, perm.ctypes.data_as(C.POINTER(C.c_uint32)), perm.size))
    assert list(g) == f
    return f, perm


def open_handle(monkeypatch, r, block=None, order=None, chunk=None, fuse=True, rank=0, nranks=1, sub=None):
    """A handle of Ref ``r`` under the knobs, with every assertion on what it says of itself: the route words, the
    exported block form against the derived plan, dnm_mat_fuses_init.  Returns (handle, derived plan or None)."""
    knobs = knobs_of(block, order, chunk, fuse)
    for k_, v_ in knobs.items():
        monkeypatch.setenv(k_, v_)
    explicit = sub is not None
    sub = r.subspace() if sub is None else sub
    desc = sub._to_c()
    d = desc['data']
    config._initialize()
    h = backend.create_mat(*r.arrs, d, d, r.sector is not None, 0, rank, nranks)
    mat = backend.ShellMat(h, d, d, nranks, rank)
    for k_ in knobs:
        monkeypatch.delenv(k_)
    mat._sub = (sub, desc)
    row0, m = backend.split_ownership(r.N, nranks, rank)
    assert (mat.swz_left, mat.swz_right, mat.M, mat.N, mat.row0, mat.m_local) == (0, 0, r.N, r.N, row0, m)
    says = mat.describe()
    fields, perm = exported(mat)
    fuses = _lib.lib().dnm_mat_fuses_init(mat.handle)
    if explicit:
        assert "row-gather" in says and fields == [0] * 6, says
        return mat, None
    lb = t.chosen_block(r, block)
    if not lb:
        assert ROW_WORDS in says and "block form" not in says and fields == [0] * 6 and perm is None, (says, fields)
        assert fuses == (1 if fuse and nranks == 1 else 0)
        return mat, None
    assert BLOCK_WORDS % lb in says and ROW_WORDS not in says, says
    plan = t.plan_of(r, lb, order, chunk, row0, m)
    assert fields == plan.fields(), (fields, plan.fields())
    assert (perm is None) == (plan.perm is None) and (perm is None or np.array_equal(perm, plan.perm)), plan.kind
    assert fuses == (1 if nranks == 1 else 0)
    return mat, plan


# ---------------------------------------------------------------- one call and everything asserted after it

def fresh_y(n):
    return DBuf(np.full(n, SENT), SENT)


def check_y(Y, want, what):
    """y == want, guards intact (DBuf.payload asserts it), no NaN, no sentinel; returns y"""
    now = Y.payload()
    assert not np.isnan(now).any(), what + ": NaN in y"
    y = now.view(np.complex128)
    bad = np.flatnonzero(y != want)
    if bad.size:
        i = int(bad[0])
        left = int(np.sum(now == SENT.real))
        raise AssertionError("%s: %d of %d rows differ (%d doubles still hold the sentinel), the first is row %d: got %r, "
                             "reference %r" % (what, bad.size, y.size, left, i, y[i], want[i]))
    assert np.array_equal(y, want)
    assert not (now == SENT.real).any() and not (now == SENT.imag).any(), what + ": the sentinel is left in y"
    return y


def run_entries(mat, r, p, what, entries=ENTRIES):
    Lb, h = _lib.lib(), mat.handle
    X, Z, Z2 = DBuf(p.x, NAN), DBuf(p.z, NAN), DBuf(p.z2, NAN)
    for name in entries:
        Y = fresh_y(r.N)
        dot = (C.c_double * 3)(SENT.real, SENT.real, SENT.real)
        sums = None
        if name == "mult":
            _lib.check(Lb.dnm_mat_mult(h, X.ptr, Y.ptr, None))
            want = p.y
        elif name == "mult_dot":
            _lib.check(Lb.dnm_mat_mult_dot(h, X.ptr, Y.ptr, dot, None))
            want, sums = p.y, p.sums[:2]
        elif name == "lanczos":
            _lib.check(Lb.dnm_mat_mult_lanczos(h, X.ptr, Y.ptr, None, 0.0, dot, None))
            want, sums = p.y, p.sums
        elif name == "lanczos_z":
            _lib.check(Lb.dnm_mat_mult_lanczos(h, X.ptr, Y.ptr, Z.ptr, ref.B, dot, None))
            want, sums = p.y_z, p.sums_z
        elif name == "sub":
            _lib.check(Lb.dnm_mat_mult_sub(h, X.ptr, Y.ptr, Z.ptr, ref.B, None))
            want = p.y_z
        elif name == "sub2":
            _lib.check(Lb.dnm_mat_mult_sub2(h, X.ptr, Y.ptr, Z.ptr, ref.B, None, 0.0, 0.0, None))
            want = p.y_z
        else:
            _lib.check(Lb.dnm_mat_mult_sub2(h, X.ptr, Y.ptr, Z.ptr, ref.B, Z2.ptr, p.c.real, p.c.imag, None))
            want = p.y_z2
        tag = "%s %s" % (what, name)
        check_y(Y, want, tag)
        assert X.untouched() and Z.untouched() and Z2.untouched(), tag + ": an input vector or its guard was written"
        if sums is not None:
            got = np.array(dot[:len(sums)])
            assert np.array_equal(got, sums), "%s: fused sums %r, reference %r" % (tag, got.tolist(), sums.tolist())
            assert all(v == SENT.real for v in dot[len(sums):])


def run_case(monkeypatch, c):
    """Every entry with the diagonal on the fly, then after precompute_diagonal."""
    r, p = t.get(c['op'], c['L'], c['k'], c['sector']), t.product(c['op'], c['L'], c['k'], c['sector'])
    mat, plan = open_handle(monkeypatch, r, c['block'], c['order'], c['chunk'], c['fuse'])
    what = t.name_of(c)
    run_entries(mat, r, p, what + " diagonal on the fly")
    mat.precompute_diagonal()
    run_entries(mat, r, p, what + " diagonal cached")
    mat.destroy()
    return plan


def cases(group):
    return pytest.mark.parametrize("c", group, ids=[t.name_of(c) for c in group])


BLOCKS = [c for c in t.CASES.values() if c['block'] in (10, 13) and c['sector'] is None and c not in t.FALLBACK
          and c not in t.SWIZZLE + t.DEFAULT_ORDER]


# ---------------------------------------------------------------- the block form

@cases(BLOCKS)
def test_block_form(monkeypatch, c):
    """(14, 6) at 10 bits and (17, 7) at 13: every register row of both instances, the last one ragged; fast bonds in the
    high part, in the low part and across the boundary; far hops, the four-site term and bond graphs on the per-row
    path; ascending order and the DNM_SC_ORDER=3 permutation with its holes.  The edge sectors: blocks of 1 and 10 rows,
    dimension 1."""
    plan = run_case(monkeypatch, c)
    assert plan.kind == ('permutation' if c['order'] else 'ascending')
    if (c['L'], c['k']) in t.BLOCK_SHAPES.values():
        assert plan.register_rows() == [0, 1, 2, 3] and plan.ragged()


@cases(t.SWIZZLE)
def test_swizzled_order(monkeypatch, c):
    """DNM_SC_ORDER=0 from 1024 high parts on: the XCD swizzle of the workgroup-to-block map; a grid rounded up past the
    last high part; high parts without rows, whose workgroups return early and whose sum slots must stay zero."""
    plan = run_case(monkeypatch, c)
    assert plan.kind == ('ascending' if (c['L'], c['k']) == (23, 3) else 'swizzle')
    assert plan.early() > 0 or (c['L'], c['k']) == (20, 10)


@cases(t.DEFAULT_ORDER)
def test_default_permutation(monkeypatch, c):
    """No DNM_SC_ORDER: g = 6 from 1024 high parts on, and once inside chunks of 16 high parts (DNM_SC_CHUNK=4)."""
    plan = run_case(monkeypatch, c)
    assert plan.kind == 'permutation' and plan.swizzle == 1


def test_production_instance(monkeypatch):
    """dm on SpinConserve(23, 11), 1 352 078 rows, no knob at all: the handle chooses 13 bits and a permutation (asserted
    from the export inside open_handle, and here)."""
    c = t.PRODUCTION
    r = t.get(c['op'], c['L'], c['k'])
    assert r.N == 1352078
    plan = run_case(monkeypatch, c)
    assert (plan.lb, plan.kind) == (13, 'permutation') and plan.register_rows() == [0, 1, 2, 3]
    del r
    ref.release()


@cases(t.XPARITY)
def test_xparity(monkeypatch, c):
    """XParity(SpinConserve(L, L / 2), +-) on the first half of the states: the terms that flip spin L-1 come composed
    with the global flip, the bond (L-2, L-1) as a mask of every spin below L-2 -- the complemented-mask branch of the
    per-row path, in both block forms and in both row kernels (chain_xp; the bonds of graph_xp from spin L-1 come as
    masks of every spin but two, on the general arm)."""
    r = t.get(c['op'], c['L'], c['k'], c['sector'])
    want = 'complemented' if c['op'] == 'chain_xp' else 'general'
    assert {want + ' inside', want + ' leaves'} <= t.arms(r, c['block'])
    run_case(monkeypatch, c)


@cases(t.FALLBACK)
def test_what_falls_back(monkeypatch, c):
    """More than 64 masks, L = 13 at 13 bits, L = 10 at 10 bits: the knob asks for a block form, the handle says one row
    per thread (open_handle asserts it) and is exact."""
    assert run_case(monkeypatch, c) is None


@cases(t.ROWS)
def test_row_kernels(monkeypatch, c):
    """DNM_SC_BLOCK=0: sc_matvec_kernel and, for the entries with start vectors or sums, its fused twin; under
    DNM_ROW_FUSE=0 the plain kernel and sweeps.  (12, 6): the 16-bit table alone; (17, 7): one step of the walk above
    bit 16; dimensions that are no multiple of 256."""
    assert run_case(monkeypatch, c) is None


# ---------------------------------------------------------------- planted columns

def planted_states(r, lb):
    """At most 40 rows where a wrong offset would show."""
    st, nt = r.states, t.NT[lb]
    H = st >> lb
    starts = np.flatnonzero(np.r_[True, H[1:] != H[:-1]])
    ends = np.r_[starts[1:], st.size]
    size = ends - starts
    picks = [0, st.size - 1, int(starts[0]), int(ends[0]) - 1, int(starts[-1]), int(ends[-1]) - 1]
    for n in np.unique(size).tolist():                       # the first and last row of a block of every size
        b = int(np.flatnonzero(size == n)[len(np.flatnonzero(size == n)) // 2])
        picks += [int(starts[b]), int(ends[b]) - 1]
    full = int(np.argmax(size))                              # the register-row boundaries of a full block
    picks += [int(starts[full]) + q for q in (nt - 1, nt, 2 * nt - 1, 2 * nt, 3 * nt) if q < size[full]]
    pair = (st >> (lb - 1)) & 3                              # the boundary bond: the partner lies in another block
    for v in (1, 2):
        w = np.flatnonzero(pair == v)
        picks += [int(w[0]), int(w[w.size // 2]), int(w[-1])] if w.size else []
    top = (st >> (r.L - 2)) & 3                              # the highest bond
    for v in (1, 2):
        w = np.flatnonzero(top == v)
        picks += [int(w[0]), int(w[-1])] if w.size else []
    out = sorted(set(picks))
    assert 8 <= len(out) <= 40
    return out


@pytest.mark.parametrize("which", range(len(t.PLANTED)),
                         ids=["%s-%d-%d%s-%s" % (q[0], q[1], q[2], q[3] or "", q[4] or "rows") for q in t.PLANTED])
def test_planted_columns(monkeypatch, which):
    """x = 3 - 2i at one state and zero elsewhere: y is (3 - 2i) times that column of H, exactly, and exactly zero at
    every other row, between untouched guards."""
    op, L, k, sector, block = t.PLANTED[which]
    r = t.get(op, L, k, sector)
    mat, _ = open_handle(monkeypatch, r, block, 0 if block else None)
    amp = 3 - 2j
    for cached in (False, True):
        if cached:
            mat.precompute_diagonal()
        for j in planted_states(r, block or 10):
            x = np.zeros(r.N, dtype=np.complex128)
            x[j] = amp
            rows, vals = r.column(j)
            want = np.zeros(r.N, dtype=np.complex128)
            want[rows] = amp * vals                      # (small dyadic numbers: the product is exact)
            X, Y = DBuf(x, NAN), fresh_y(r.N)
            _lib.check(_lib.lib().dnm_mat_mult(mat.handle, X.ptr, Y.ptr, None))
            check_y(Y, want, "%s column %d (state %#x)" % (op, j, int(r.states[j])))
            assert X.untouched()
    mat.destroy()


# ---------------------------------------------------------------- shares of a partition, on one GPU

def window_of(mat, x):
    """(first column, the window with NaN at every column the chunk map does not mark)"""
    lo, hi = mat.column_window()
    cmap = chunks_of(mat, 0)
    assert cmap.size == hi - lo + 1 and set(np.unique(cmap).tolist()) <= {0, 1}
    xw = np.array(x[lo:hi + 1])
    xw[cmap == 0] = NAN
    return lo, xw


@pytest.mark.parametrize("op,L,k,lb,order,P", [s[:5] + (P,) for s in t.SHARES for P in s[5]],
                         ids=lambda v: str(v))
def test_shares(monkeypatch, op, L, k, lb, order, P):
    """Ranks 0 .. P-1 in one process: the ownership boundaries cut blocks (live, r_lo, r_hi, whole == false); the window
    holds NaN wherever dnm_mat_column_chunks(shift 0) marks nothing; dnm_mat_mult_window gives the reference's rows of
    the share exactly, with the diagonal on the fly and cached, between untouched sentinel guards."""
    r, p = t.get(op, L, k), t.product(op, L, k)
    cut, kinds = 0, set()
    for q in range(P):
        mat, plan = open_handle(monkeypatch, r, lb, order, rank=q, nranks=P)
        cut += len(plan.partial())
        kinds.add(plan.kind)
        row0, m = mat.row0, mat.m_local
        lo, xw = window_of(mat, p.x)
        Wn = DBuf(xw, NAN)
        for cached in (False, True):
            if cached:
                mat.precompute_diagonal()
            Y = fresh_y(m)
            _lib.check(_lib.lib().dnm_mat_mult_window(mat.handle, Wn.ptr, lo, xw.size, Y.ptr, None))
            check_y(Y, p.y[row0:row0 + m], "rank %d of %d, %s" % (q, P, "cached" if cached else "on the fly"))
            assert Wn.untouched()
        # the fused Lanczos step is refused on a partitioned handle, before anything is written
        Y = fresh_y(m)
        dot = (C.c_double * 3)()
        assert _lib.lib().dnm_mat_mult_lanczos(mat.handle, Wn.ptr, Y.ptr, None, 0.0, dot, None) != 0
        assert Y.untouched()
        mat.destroy()
    assert cut >= P and ('swizzle' in kinds) == ((L, k) in t.SWIZZLED_SHARES)


# ---------------------------------------------------------------- dnm_mat_mult_window_rows

def row_ranges(mat, r, kind):
    """The covers (lists of ranges whose union is the share) and the single ranges to run."""
    m, row0 = mat.m_local, mat.row0
    lo, hi = mat.column_window()
    covers = [[(0, m)]]
    # the rows that read only the rank's own block of x, and those that read nothing below the window's first quarter
    for col_lo, col_hi in ((row0, row0 + m), (lo + (hi - lo) // 4, hi + 1)):
        local = local_rows_of(mat, col_lo, col_hi, 8, 1)
        assert all(0 <= a < b <= m for a, b in local)
        covers.append(local + backend.complement_ranges(local, m))
    H = r.states[row0:row0 + m] >> 10
    starts = np.flatnonzero(np.r_[True, H[1:] != H[:-1]])
    assert starts.size >= 5
    mid = lambda b: int(starts[b] + starts[b + 1]) // 2
    singles = [(m // 2, m // 2 + 1), (1, m - 1), (mid(1), mid(3)), (0, 1), (m - 1, m)]
    covers.append([(0, mid(0)), (mid(0), mid(2)), (mid(2), m)])          # a cover whose cuts lie inside blocks
    return covers, singles


@pytest.mark.parametrize("kind", ["block", "rows", "explicit"])
def test_window_rows(monkeypatch, kind):
    """dnm_mat_mult_window_rows narrows the ScBlock to a row range and offsets y and the cached diagonal: on a block
    handle, a row-kernel handle and an Explicit handle holding SpinConserve(14, 6)'s states (the gather kernel), rank 1
    of 3.  After each call the positions of y_local outside [r0, r1) hold the sentinel and those inside the final value;
    the calls of a cover equal dnm_mat_mult_window bit for bit; with the diagonal on the fly and cached."""
    r, p = t.get('dm', 14, 6), t.product('dm', 14, 6)
    sub = Explicit(np.array(r.states), L=14) if kind == "explicit" else None
    mat, _ = open_handle(monkeypatch, r, {"block": 10, "rows": 0, "explicit": None}[kind], 0 if kind == "block" else None,
                         rank=1, nranks=3, sub=sub)
    Lb, m, row0 = _lib.lib(), mat.m_local, mat.row0
    lo, xw = window_of(mat, p.x)
    Wn = DBuf(xw, NAN)
    want = p.y[row0:row0 + m]
    covers, singles = row_ranges(mat, r, kind)
    for cached in (False, True):
        if cached:
            mat.precompute_diagonal()
        Y = fresh_y(m)
        _lib.check(Lb.dnm_mat_mult_window(mat.handle, Wn.ptr, lo, xw.size, Y.ptr, None))
        whole = check_y(Y, want, "%s whole share" % kind).copy()
        for cover in covers:
            assert sorted(cover)[0][0] == 0 and sorted(cover)[-1][1] == m
            Y = fresh_y(m)
            done = np.zeros(m, dtype=bool)
            for r0, r1 in cover:
                _lib.check(Lb.dnm_mat_mult_window_rows(mat.handle, Wn.ptr, lo, xw.size, Y.ptr, r0, r1, None))
                done[r0:r1] = True
                y = Y.payload().view(np.complex128)
                assert np.array_equal(y[done], want[done]), (kind, cached, r0, r1)
                assert (y[~done] == SENT).all(), (kind, cached, r0, r1)
            assert done.all()
            assert np.array_equal(check_y(Y, want, "%s cover" % kind).view(np.uint64), whole.view(np.uint64))
        for r0, r1 in singles:
            Y = fresh_y(m)
            _lib.check(Lb.dnm_mat_mult_window_rows(mat.handle, Wn.ptr, lo, xw.size, Y.ptr, r0, r1, None))
            y = Y.payload().view(np.complex128)
            inside = np.zeros(m, dtype=bool)
            inside[r0:r1] = True
            assert np.array_equal(y[inside], want[inside]), (kind, cached, r0, r1)
            assert (y[~inside] == SENT).all() and not np.isnan(y[inside].view(np.float64)).any(), (kind, cached, r0, r1)
        assert Wn.untouched()
        # a range outside the share is refused
        Y = fresh_y(m)
        for r0, r1 in ((-1, 1), (0, m + 1), (5, 5)):
            assert Lb.dnm_mat_mult_window_rows(mat.handle, Wn.ptr, lo, xw.size, Y.ptr, r0, r1, None) != 0
        assert Y.untouched()
    mat.destroy()


# ---------------------------------------------------------------- refusals

@pytest.mark.parametrize("block", [10, 0])
def test_aliasing_is_refused(monkeypatch, block):
    """x, z or z2 aliasing y, in every entry: an error, y untouched."""
    r, p = t.get('dm', 14, 6), t.product('dm', 14, 6)
    mat, _ = open_handle(monkeypatch, r, block, 0 if block else None)
    Lb, h = _lib.lib(), mat.handle
    X, Z = DBuf(p.x, NAN), DBuf(p.z, NAN)
    Y = DBuf(p.z2, SENT)
    dot = (C.c_double * 3)()
    y = Y.ptr
    calls = [lambda: Lb.dnm_mat_mult(h, y, y, None), lambda: Lb.dnm_mat_mult_dot(h, y, y, dot, None),
             lambda: Lb.dnm_mat_mult_lanczos(h, y, y, None, 0.0, dot, None),
             lambda: Lb.dnm_mat_mult_lanczos(h, X.ptr, y, y, ref.B, dot, None),
             lambda: Lb.dnm_mat_mult_sub(h, y, y, Z.ptr, ref.B, None), lambda: Lb.dnm_mat_mult_sub(h, X.ptr, y, y, ref.B, None),
             lambda: Lb.dnm_mat_mult_sub2(h, y, y, Z.ptr, ref.B, None, 0.0, 0.0, None),
             lambda: Lb.dnm_mat_mult_sub2(h, X.ptr, y, y, ref.B, None, 0.0, 0.0, None),
             lambda: Lb.dnm_mat_mult_sub2(h, X.ptr, y, Z.ptr, ref.B, y, 0.5, 0.25, None)]
    for i, call in enumerate(calls):
        assert call() != 0, i
        assert b"alias" in Lb.dnm_last_error() or b"different vectors" in Lb.dnm_last_error(), Lb.dnm_last_error()
        assert Y.untouched() and X.untouched() and Z.untouched(), i
    mat.destroy()


# ---------------------------------------------------------------- rounding

@pytest.mark.parametrize("what,op,L,k,sector,block", t.ROUNDING, ids=[q[0] for q in t.ROUNDING])
def test_rounding(monkeypatch, what, op, L, k, sector, block):
    """Normal deviates against numpy.longdouble (Ref.rounding_reference).  A component of an entry of y is a chain of
    products and fused multiply-adds, each rounded once, in some order: the diagonal's product (matvec_kernels.hip
    1096-1097 in sc_matvec_kernel, 1391-1392 in sc_block_kernel; on the fly: the fmas of the per-row path) and, for every
    hop, one fma with the real part of the element and one with the imaginary part (sc_matvec_kernel 1119-1122,
    1182-1185; sc_block_kernel 1440-1443 high bonds, 1468-1471 low bonds, 1532-1535 per-row path).  An fma whose
    coefficient is zero -- the imaginary part of a real element, a high bond that does not act -- returns its accumulator
    unchanged.  So with n the row's non-zero elements (twice that where the operator has complex elements),
    |got - ref| <= gamma(n) * sum |products| per row and component (Higham, Accuracy and Stability, (3.5)); the elements
    themselves -- sums of dyadic coefficients -- are exact.  The reference's own error, gamma_64(n) of the same sum, is
    added.  The bound was fixed before the first run."""
    r = t.get(op, L, k, sector)
    mat, _ = open_handle(monkeypatch, r, block, 0 if block else None)
    rs = np.random.RandomState(len(what))
    x = rs.standard_normal(r.N) + 1j * rs.standard_normal(r.N)
    yr, yi, mr, mi, cnt = r.rounding_reference(x)
    n = cnt if op in t.REAL_OPS else 2 * cnt
    bound_r = (gamma(n) + n * 2.0 ** -63) * mr
    bound_i = (gamma(n) + n * 2.0 ** -63) * mi
    for cached in (False, True):
        if cached:
            mat.precompute_diagonal()
        X, Y = DBuf(x, NAN), fresh_y(r.N)
        _lib.check(_lib.lib().dnm_mat_mult(mat.handle, X.ptr, Y.ptr, None))
        now = Y.payload()
        assert not np.isnan(now).any()
        got = now.view(np.complex128)
        er = np.abs(got.real.astype(np.longdouble) - yr)
        ei = np.abs(got.imag.astype(np.longdouble) - yi)
        ok = bound_r > 0
        ratio = float(max((er[ok] / bound_r[ok]).max(), (ei[ok] / bound_i[ok]).max()))
        print("rounding %s (%s): n up to %d, worst |got - ref| / bound = %.3f, worst error %.3e"
              % (what, "cached" if cached else "on the fly", int(n.max()), ratio, float(max(er.max(), ei.max()))))
        assert np.all(er <= bound_r) and np.all(ei <= bound_i), ratio
    mat.destroy()
