"""
The multiply kernels of the SpinConserve internal layout (csrc/sc3_kernels.hip: sc3_lo_pass, sc3_lo_pass_r,
sc3_win_pass, sc3_row_kernel; csrc/sc3g_kernels.hip: sc3g_lo_pass, sc3g_lo_pass_r, sc3g_win_pass; their launcher
csrc/sc3_launch.h) through the C ABI, one call at a time, on device buffers of the test's own, in exact arithmetic.

Exact cases: coefficients are multiples of 1/8, amplitudes Gaussian integers in [-8, 8], b = 3/8, c = -1/4 + 5/8 i
(tests/sc3_exact_ref.py, which asserts on the numbers of every case that all partial sums stay below 2^53 in units of
1/64).  Any order of summation, with or without fma, then gives the same VALUE, and the tests assert equality with the
int64 reference -- of values, not of bits: -0.0 is allowed.  tests/test_sc3_exact_ref.py pins that reference to the
oracle on every pair used here.

Buffers: every vector lies at its internal length (dnm_vec_layout_size; the first half of the layout under XParity)
between two guards of 64 complex128 elements (128 doubles on real-packed handles).  x, z and z2 are laid out on the
host through dnm_vec_layout_positions_host, their padding zero -- the contract of csrc/sc3.h -- and their guards NaN;
y and its guards are filled with a sentinel before every call.  After every call: y at the rows' positions equals the
reference, every padding position of y is exactly zero, both guards of y hold their bits, no NaN is anywhere in y,
x / z / z2 with their guards are bit-identical to what was uploaded, and the fused sums equal the reference's.

Every case asserts what dnm_mat_plan_describe says of its handle, so that none silently runs another kernel.
"""
import ctypes as C

import numpy as np
import pytest

import sc3_exact_ref as ref
from dynamite_amd import _lib, backend
from dynamite_amd.config import config
from test_gpu_vec import NAN, SENT, gamma

pytestmark = pytest.mark.gpu

GD = 128                         # guard doubles on each side: 64 complex128 elements
ENTRIES = ("mult", "mult_dot", "lanczos", "lanczos_z", "sub", "sub2", "sub2_z2")
KNOBS = {"tiled": {}, "cached": {"DNM_SC3_DIAG": "cached"}, "rows": {"DNM_SC3_TILED": "0"},
         "noptab": {"DNM_SC3G_PTAB": "0"}}


@pytest.fixture
def layout64():
    """(6, 4) field split for every SpinConserve subspace with L >= 11, whatever its dimension."""
    old = (config.sc_layout, config.sc_layout_min_dim)
    config.sc_layout, config.sc_layout_min_dim = (6, 4), 0
    yield (6, 4)
    config.sc_layout, config.sc_layout_min_dim = old


@pytest.fixture
def layout1410():
    """The production instances at any dimension."""
    old = (config.sc_layout, config.sc_layout_min_dim)
    config.sc_layout, config.sc_layout_min_dim = (14, 10), 0
    yield (14, 10)
    config.sc_layout, config.sc_layout_min_dim = old


# ---------------------------------------------------------------- buffers

class DBuf:
    """``payload`` (doubles) in device memory between two guards of GD doubles holding the parts of ``guard`` in turn;
    a device copy of the whole is kept to compare with."""

    def __init__(self, payload, guard):
        import torch
        payload = np.ascontiguousarray(payload).view(np.float64).reshape(-1)
        g = np.full(GD // 2, guard, dtype=np.complex128).view(np.float64)
        self.n = payload.size
        self.host = np.concatenate([g, payload, g])
        self.t = torch.from_numpy(self.host).cuda()
        self.orig = self.t.clone()
        self.ptr = C.c_void_p(self.t.data_ptr() + 8 * GD)

    def untouched(self):
        import torch
        return torch.equal(self.t.view(torch.int64), self.orig.view(torch.int64))

    def payload(self):
        """The payload as it is now; asserts that both guards still hold their bits."""
        now = self.t.cpu().numpy()
        for sl in (slice(0, GD), slice(GD + self.n, None)):
            assert np.array_equal(now[sl].view(np.uint64), self.host[sl].view(np.uint64)), "guard of y overwritten"
        return now[GD:GD + self.n]


def positions(d, idx, part=None):
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    out = np.empty_like(idx)
    _lib.check(_lib.lib().dnm_vec_layout_positions_host(C.byref(d), C.byref(part) if part is not None else None, idx.size,
                                                        _lib.p64(idx), _lib.p64(out)))
    return out


class Layout:
    """Where the N rows of a handle's vectors lie: internal length, positions of the rows, the padding."""

    def __init__(self, mat, N, half):
        d = mat._keep[0]
        if half:                   # XParity: the layout's first half, what rank 0 of 2 would own
            istart, self.nint, nstart, nlen = backend.layout_partition(d, 2, 0)
            assert (istart, nstart, nlen) == (0, 0, N)
            self.pos = positions(d, np.arange(N), _lib.Partition(0, 2))
        else:
            n = C.c_int64()
            _lib.check(_lib.lib().dnm_vec_layout_size(C.byref(d), C.byref(n)))
            self.nint = n.value
            self.pos = positions(d, np.arange(N))
        self.set_rows(self.pos)
        assert mat.m_local * (2 if mat.real_packed else 1) == self.nint and mat.M == N, (mat.m_local, self.nint)

    def set_rows(self, pos):
        self.pos = pos
        assert pos.min() >= 0 and pos.max() < self.nint and np.unique(pos).size == pos.size
        self.pad = np.ones(self.nint, dtype=bool)
        self.pad[pos] = False

    def lay(self, v, real, guard=NAN):
        """v (reference order) at the rows' positions, zeros in the padding, between guards"""
        a = np.zeros(self.nint, dtype=np.float64 if real else np.complex128)
        a[self.pos] = v.real if real else v
        return DBuf(a, guard)

    def fresh_y(self, real):
        return DBuf(np.full(self.nint, SENT.real if real else SENT), SENT)

    def check_y(self, Y, want, real, what):
        """y at the rows' positions == want, padding exactly zero, guards intact, no NaN"""
        now = Y.payload()
        assert not np.isnan(now).any(), what + ": NaN in y"
        y = now if real else now.view(np.complex128)
        got, want = y[self.pos], (want.real if real else want)
        bad = np.flatnonzero(got != want)
        if bad.size:
            i = int(bad[0])
            left = int(np.sum(got.view(np.float64) == SENT.real))
            raise AssertionError("%s: %d of %d rows differ (%d still hold the sentinel), the first is row %d at position "
                                 "%d: got %r, reference %r" % (what, bad.size, got.size, left, i, int(self.pos[i]),
                                                               got[i], want[i]))
        assert np.array_equal(got, want)
        padding = y[self.pad]
        nz = np.flatnonzero(padding != 0)
        assert nz.size == 0, "%s: %d of %d padding positions of y are not zero, the first at position %d holds %r" % (
            what, nz.size, padding.size, int(np.flatnonzero(self.pad)[nz[0]]), padding[nz[0]])


# ---------------------------------------------------------------- handles

def open_handle(r, monkeypatch, knobs=(), real=False, site_perm=None, order=0):
    """(handle, what it says of itself, the subspace object that keeps its descriptor alive)"""
    for k_, v_ in dict(knobs).items():
        monkeypatch.setenv(k_, v_)
    sub = r.subspace()
    desc = sub._to_c()
    if order:
        d = type(desc['data']).from_buffer_copy(desc['data'])
        d.vec_swizzle = int(d.vec_swizzle) | (order << 16)
        desc = {'type': desc['type'], 'data': d, '_keep': desc}
        site_perm = False
    config._initialize()
    mat = backend.build_mat(*r.arrs, desc, desc, xparity=r.sector is not None,
                            flags=_lib.MAT_REAL_PACKED if real else 0, site_perm=site_perm)
    for k_ in dict(knobs):
        monkeypatch.delenv(k_)
    mat._sub = (sub, desc)
    d = mat.describe()
    assert mat.real_packed == real
    if mat.uses_cached_diagonal():
        mat.precompute_diagonal()
    return mat, d


def say(d, aw, L):
    """the field split the handle must name"""
    assert "internal layout [T %d | W %d | Lo %d]" % (L - aw[0] - aw[1], aw[1], aw[0]) in d, d


def diagonal_word(d):
    for w in ("diagonal none", "diagonal cached", "diagonal on the fly"):
        if w in d:
            return w.split(" ", 1)[1]
    return None


def mixed_patterns(r, mat, a):
    """(the operator has diagonal terms, the distinct Lo patterns of those that see Lo AND a spin above it): from the
    MSC arrays and the handle's relabelling alone -- what csrc/sc3_tables.cpp: split_diagonal decides by (at most four
    such patterns are evaluated on the fly, more need the cached diagonal)."""
    masks, offs, signs, _ = r.arrs
    if not (masks.size and masks[0] == 0):
        return False, set()
    perm, lom, groups = mat.perm_left, (1 << a) - 1, set()
    for sg in signs[offs[0]:offs[1]].tolist():
        if perm is not None:
            sg = sum(1 << perm[i] for i in range(r.L) if (sg >> i) & 1)
        if sg & ~lom and sg & lom:
            groups.add(sg & lom)
    return True, groups


def check_plan(mat, d, r, a, kind="tiled", want=None):
    """The handle of a two-pass route runs the kernel instances the case is named for: the diagonal word of
    dnm_mat_plan_describe is EXACTLY what the operator's arrays and the knobs imply (``want``: and what the case
    pins), the handle's own record of its passes (dnm_mat_export_sc3 "op") agrees, an on-the-fly diagonal has the
    number of mixed patterns counted here, and a bond graph's lo pass has its partner table exactly when the knob
    leaves it and the LDS hops fit.  Returns (word, mixed patterns)."""
    has, groups = mixed_patterns(r, mat, a)
    word = "none" if not has else ("cached" if kind == "cached" or len(groups) > 4 else "on the fly")
    assert diagonal_word(d) == word, (d, sorted(groups))
    assert want is None or word == want, (word, want, sorted(groups))
    f = backend.sc3_op_fields(mat.handle)
    assert f["tiled"] == 1 and f["diag_mode"] == {"none": 0, "cached": 1, "on the fly": 2}[word], f
    assert bool(f["graph"]) == ("bond graph" in d) and bool(f["real"]) == mat.real_packed
    if word == "on the fly":
        assert f["ngroups"] == len(groups), (f, sorted(groups))
    if f["graph"]:
        assert (f["nhp"] > 0) == (kind != "noptab" and 0 < f["nldsA"] <= 32), (kind, f)
    return word, len(groups)


def run_entries(mat, r, p, real, entries=ENTRIES, what=""):
    """Every entry of ``entries`` once, on buffers between guards, with all of the module's assertions."""
    Lb, h = _lib.lib(), mat.handle
    lay = Layout(mat, r.N, r.sector is not None)
    X, Z, Z2 = lay.lay(p.x, real), lay.lay(p.z, real), lay.lay(p.z2, real)
    for name in entries:
        Y = lay.fresh_y(real)
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
        lay.check_y(Y, want, real, tag)
        assert X.untouched() and Z.untouched() and Z2.untouched(), tag + ": an input vector or its guard was written"
        if sums is not None:
            got = np.array(dot[:len(sums)])
            assert np.array_equal(got, sums), "%s: fused sums %r, reference %r" % (tag, got.tolist(), sums.tolist())
            assert all(v == SENT.real for v in dot[len(sums):])
    return lay


def case(name):
    op, L, k, sector, real = ref.CASES[name]
    return ref.get(op, L, k, sector), ref.product(op, L, k, sector, real), real


# ---------------------------------------------------------------- chains: sc3_lo_pass, sc3_lo_pass_r, sc3_win_pass, sc3_row_kernel

SHAPES = [(11, 5), (12, 6), (13, 4), (14, 7), (12, 1), (12, 11)]     # t = 1; ...; classes of one row, rows of one state
WANT_DIAG = {"hops": "none", "hops_dm": "none", "long": "cached"}


# (DNM_SC3_DIAG=cached changes the handle only where the diagonal would be evaluated on the fly)
CHAIN_KINDS = [(o, kd) for o in ref.CHAIN_OPS for kd in ("tiled", "cached", "rows") if kd != "cached" or o not in WANT_DIAG]


@pytest.mark.parametrize("op,kind", CHAIN_KINDS)
@pytest.mark.parametrize("L,k", SHAPES)
def test_chain_complex(layout64, monkeypatch, L, k, op, kind):
    """The two tiled passes on complex vectors (on-the-fly, cached and no diagonal; symmetric and direction-dependent
    hops) and the row kernel."""
    r, p, _ = case("%s-%d-%d" % (op, L, k))
    mat, d = open_handle(r, monkeypatch, KNOBS[kind])
    say(d, layout64, L)
    assert "bond graph" not in d and ("row kernel" in d) == (kind == "rows") and ("two-pass" in d) == (kind != "rows"), d
    if kind != "rows":
        assert ("real symmetric" in d) == (op in ref.REAL_OPS), d
        check_plan(mat, d, r, 6, kind, want=WANT_DIAG.get(op, "cached" if kind == "cached" else "on the fly"))
    run_entries(mat, r, p, False, what=d.split(",")[0])
    mat.destroy()


@pytest.mark.parametrize("op,kind", [(o, kd) for o, kd in CHAIN_KINDS if o in ref.REAL_OPS and kd != "rows"])
@pytest.mark.parametrize("L,k", SHAPES)
def test_chain_real(layout64, monkeypatch, L, k, op, kind):
    """DNM_MAT_REAL_PACKED on a chain: sc3_lo_pass_r and the window pass on the halved tables, one double per position."""
    r, p, real = case("%s-%d-%d-real" % (op, L, k))
    mat, d = open_handle(r, monkeypatch, KNOBS[kind], real=True)
    say(d, layout64, L)
    assert "bond graph" not in d and "two-pass" in d and "real symmetric" in d, d
    check_plan(mat, d, r, 6, kind, want=WANT_DIAG.get(op, "cached" if kind == "cached" else "on the fly"))
    run_entries(mat, r, p, True, what="real " + d.split(",")[0])
    mat.destroy()


def test_real_packed_refuses_imaginary_hops(layout64, monkeypatch):
    """No real form for direction-dependent complex hops, on a chain or on a graph: dnm_mat_create refuses."""
    for name in ("dm-13-4", "hops_dm-13-4", "graph_c-13-4"):
        r, _, _ = case(name)
        with pytest.raises(_lib.BackendError, match="no real-packed form in this layout"):
            open_handle(r, monkeypatch, real=True)


@pytest.mark.parametrize("op", ["chain", "dm", "graph_cf"])
@pytest.mark.parametrize("L,k", [(12, 0), (12, 12)])
def test_dimension_one(layout64, monkeypatch, L, k, op):
    """A subspace of one state: the handle names the two tiled passes (chain or bond graph) and multiplies through every
    entry -- one row of one state in one class of one T block."""
    r, p, _ = case("%s-%d-%d" % (op, L, k))
    assert r.N == 1
    mat, d = open_handle(r, monkeypatch)
    say(d, layout64, L)
    assert "two-pass" in d and "row kernel" not in d and ("bond graph" in d) == (op == "graph_cf"), d
    check_plan(mat, d, r, 6)
    run_entries(mat, r, p, False, what=d.split(",")[0])
    mat.destroy()


# ---------------------------------------------------------------- bond graphs: sc3g_lo_pass, sc3g_lo_pass_r, sc3g_win_pass

@pytest.mark.parametrize("kind,perm", [("tiled", "auto"), ("tiled", "off"), ("cached", "auto"), ("noptab", "auto")])
@pytest.mark.parametrize("op", ref.GRAPHS)
@pytest.mark.parametrize("L,k", SHAPES)
def test_graph_complex(layout64, monkeypatch, L, k, op, kind, perm):
    """The bond-graph passes on complex vectors: with and without the lo pass's partner table, with and without fields,
    symmetric and direction-dependent hops, in the relabelled layout the chooser picks and in the subspace's own."""
    r, p, _ = case("%s-%d-%d" % (op, L, k))
    mat, d = open_handle(r, monkeypatch, KNOBS[kind], site_perm=None if perm == "auto" else False)
    say(d, layout64, L)
    assert "bond graph" in d and "two-pass" in d and ("real symmetric" in d) == (op in ref.REAL_OPS), d
    assert (mat.perm_left is None) == (perm == "off")        # (the chooser relabels every graph of this family)
    check_plan(mat, d, r, 6, kind)
    run_entries(mat, r, p, False, what=d.split(",")[0])
    mat.destroy()


@pytest.mark.parametrize("kind,perm", [("tiled", "auto"), ("tiled", "off"), ("cached", "auto"), ("noptab", "auto")])
@pytest.mark.parametrize("op", ["graph", "graph_f"])
@pytest.mark.parametrize("L,k", SHAPES)
def test_graph_real(layout64, monkeypatch, L, k, op, kind, perm):
    """DNM_MAT_REAL_PACKED on a bond graph: sc3g_lo_pass_r (partner table and rank tables) and the window pass on pairs."""
    r, p, _ = case("%s-%d-%d-real" % (op, L, k))
    mat, d = open_handle(r, monkeypatch, KNOBS[kind], real=True, site_perm=None if perm == "auto" else False)
    say(d, layout64, L)
    assert "bond graph" in d and "two-pass" in d and "real symmetric" in d, d
    assert (mat.perm_left is None) == (perm == "off")
    check_plan(mat, d, r, 6, kind)
    run_entries(mat, r, p, True, what="real " + d.split(",")[0])
    mat.destroy()


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("kind", ["tiled", "noptab"])
@pytest.mark.parametrize("name,L,k", [("kagome12", 12, 6), ("kagome15", 15, 7)])
def test_kagome(layout64, monkeypatch, name, L, k, kind, real):
    r, p, _ = case("%s-%d-%d%s" % (name, L, k, "-real" if real else ""))
    mat, d = open_handle(r, monkeypatch, KNOBS[kind], real=real)
    say(d, layout64, L)
    assert "bond graph" in d and "real symmetric" in d and mat.perm_left is not None, d
    check_plan(mat, d, r, 6, kind, want="cached")             # (ZZ on every bond of the torus: more than four patterns)
    run_entries(mat, r, p, real, what=d.split(",")[0])
    mat.destroy()


FLY_CASES = [(o, real) for o in sorted(ref.FLY) for real in (False, True) if not real or o in ref.REAL_OPS]


@pytest.mark.parametrize("kind", ["tiled", "noptab"])
@pytest.mark.parametrize("op,real", FLY_CASES)
@pytest.mark.parametrize("L,k", ref.FLY_SHAPES)
def test_graph_diagonal_on_the_fly(request, monkeypatch, L, k, op, real, kind):
    """The DIAGM 2 instances of the bond-graph passes: graphs with fields whose ZZ bonds cross out of Lo from two, three
    or four Lo spins only (sc3_exact_ref.fly_graph), in the subspace's own labelling, complex and real arithmetic, with
    and without the partner table, on (6, 4) shapes and on the (14, 10) instance.  Every case asserts ``diagonal on the
    fly`` and the number of mixed patterns."""
    aw = request.getfixturevalue("layout1410" if L == 25 else "layout64")
    r, p, _ = case("%s-%d-%d%s" % (op, L, k, "-real" if real else ""))
    mat, d = open_handle(r, monkeypatch, KNOBS[kind], real=real, site_perm=False)
    say(d, aw, L)
    assert "bond graph" in d and "two-pass" in d and ("real symmetric" in d) == (op in ref.REAL_OPS), d
    assert "diagonal on the fly" in d and mat.perm_left is None, d
    assert check_plan(mat, d, r, aw[0], kind, want="on the fly") == ("on the fly", ref.FLY[op])
    run_entries(mat, r, p, real, what=("real " if real else "") + d.split(",")[0])
    mat.destroy()


# ---------------------------------------------------------------- block orders, XParity

@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", ["dm-16-8", "chain-16-8", "chain-16-8-real", "graph_cf-16-8"])
def test_block_orders(layout64, monkeypatch, name, order):
    """(16, 8): 64 T blocks; in block order 1 they lie in another order than the reference's, and a handle finds them
    through the ibase table all the same."""
    r, p, real = case(name)
    mat, d = open_handle(r, monkeypatch, real=real, order=order, site_perm=False)
    say(d, layout64, 16)
    assert mat.swz_left >> 16 == order and ("bond graph" in d) == name.startswith("graph"), d
    check_plan(mat, d, r, 6, want="cached" if name.startswith("graph") else "on the fly")
    lay = run_entries(mat, r, p, real, what="order %d %s" % (order, d.split(",")[0]))
    if order == 1:
        base = positions(r.subspace()._c(), np.arange(r.N))
        assert not np.array_equal(base, lay.pos)              # (the blocks really lie elsewhere)
    mat.destroy()


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("sector", ['+', '-'])
@pytest.mark.parametrize("op,L,perm", [("chain_xp", 14, "auto"), ("graph_xp", 14, "auto"), ("graph_xp", 14, "off"),
                                       ("chain_xp", 22, "auto"), ("graph_xp", 22, "auto"), ("graph_xp", 22, "off")])
def test_xparity(layout64, monkeypatch, op, L, perm, sector, real):
    """XParity(SpinConserve(L, L / 2)) in the layout's first half: the hops that touch spin L-1 come composed with the
    global flip, as gathered hops of the bond-graph passes.  L = 22: t = 12, the blocks T = 0 and T = 0xfff are empty.
    Without a relabelling the graph's bonds from spin L-1 into Lo and into W stay where the operator puts them: flip-
    composed hops gathered by the lo pass and by the window pass."""
    r, p, _ = case("%s-%d-%d%s%s" % (op, L, L // 2, sector, "-real" if real else ""))
    mat, d = open_handle(r, monkeypatch, real=real, site_perm=None if perm == "auto" else False)
    assert perm == "auto" or mat.perm_left is None
    say(d, layout64, L)
    assert "bond graph" in d and "two-pass" in d and "real symmetric" in d, d
    # (the chain's ZZ bond across the Lo / W boundary is its one mixed pattern; the graph has more than four)
    check_plan(mat, d, r, 6, want="on the fly" if op == "chain_xp" else "cached")
    run_entries(mat, r, p, real, what="XParity %s %s" % (sector, d.split(",")[0]))
    mat.destroy()


# ---------------------------------------------------------------- the (14, 10) production instances

@pytest.mark.parametrize("name", ["dm-25-3", "dm-25-22", "chain-25-3-real", "chain-25-22-real", "graph_cf-25-3",
                                  "graph_cf-25-22", "graph_f-25-3-real", "graph_f-25-22-real", "dense_lo-25-3",
                                  "dense_lo-25-22", "dm-25-12", "graph_f-25-12-real"])
def test_production_instances(layout1410, monkeypatch, name):
    """(a, w) = (14, 10), 1024 threads: at 2300 states, where nearly every class is empty or tiny, and at 5.2 million."""
    r, p, real = case(name)
    dense = name.startswith("dense_lo")
    mat, d = open_handle(r, monkeypatch, real=real, site_perm=False if dense else None)
    say(d, layout1410, 25)
    assert "two-pass" in d and ("bond graph" in d) == (not name.startswith(("dm", "chain"))), d
    if dense:
        assert "91 hops in LDS" in d, d
    chain = name.startswith(("dm", "chain"))
    check_plan(mat, d, r, 14, want="on the fly" if chain or dense else "cached")
    run_entries(mat, r, p, real, what=d.split(",")[0])
    mat.destroy()
    if r.N > 1 << 20:
        del r, p
        ref.release()                # (nothing else uses these; the small cases are rebuilt in milliseconds)


# ---------------------------------------------------------------- planted columns

def planted_states(r, a, w):
    """At most 40 states of the subspace where a wrong offset would show: the ends of the subspace, of the first and
    last non-empty T block, of the first and last row of every class of a middle T block, and runs of k set bits that
    end or begin at the Lo/W and at the W/T boundary (the boundary bond is then one of the two bonds with a hop)."""
    st = r.states
    T, W = st >> (a + w), (st >> a) & ((1 << w) - 1)
    picks = [int(st[0]), int(st[-1])]
    blocks = np.unique(T)
    for tb in (blocks[0], blocks[-1]):
        s = st[T == tb]
        picks += [int(s[0]), int(s[-1])]
    mid = blocks[blocks.size // 2]
    inb = T == mid
    cw = np.bitwise_count(W)
    for c in np.unique(cw[inb]).tolist():
        rows = np.unique(W[inb & (cw == c)])
        for wv in (rows[0], rows[-1]):
            s = st[inb & (W == wv)]
            picks += [int(s[0]), int(s[-1])]
    run = (1 << r.k) - 1
    for b in (a, a + w):
        for lo in (b - r.k, b):
            if lo >= 0 and lo + r.k <= r.L:
                picks.append(run << lo)
    out = []
    for s in picks:
        j = int(np.searchsorted(st, s))
        if j < st.size and int(st[j]) == s and j not in out:
            out.append(j)
    assert 4 <= len(out) <= 40
    return out


@pytest.mark.parametrize("which", range(len(ref.PLANTED)), ids=["%s-%d-%d%s" % (q[0], q[1], q[2], q[3] or "") for q in ref.PLANTED])
def test_planted_columns(request, monkeypatch, which):
    """x = 3 - 2i at one state and zero elsewhere: y is (3 - 2i) times that column of H, exactly, and zero everywhere
    else -- at every other row, in the padding, between untouched guards."""
    op, L, k, sector = ref.PLANTED[which]
    aw = request.getfixturevalue("layout1410" if L == 25 else "layout64")
    r = ref.get(op, L, k, sector)
    mat, d = open_handle(r, monkeypatch, site_perm=False)
    say(d, aw, L)
    assert ("bond graph" in d) == (op == "graph_c" or sector is not None) and "two-pass" in d, d
    check_plan(mat, d, r, aw[0], want="cached" if op == "graph_c" else "on the fly")
    lay = Layout(mat, r.N, sector is not None)
    amp = 3 - 2j
    for j in planted_states(r, *aw):
        x = np.zeros(r.N, dtype=np.complex128)
        x[j] = amp
        rows, vals = r.column(j)
        want = np.zeros(r.N, dtype=np.complex128)
        want[rows] = amp * vals                      # (small dyadic numbers: the product is exact)
        X, Y = lay.lay(x, False), lay.fresh_y(False)
        _lib.check(_lib.lib().dnm_mat_mult(mat.handle, X.ptr, Y.ptr, None))
        lay.check_y(Y, want, False, "%s column %d (state %#x)" % (op, j, int(r.states[j])))
        assert X.untouched()
    mat.destroy()


# ---------------------------------------------------------------- shares of a partition, on one GPU

@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("L,k", [(15, 7), (16, 8)])
def test_shares(layout64, L, k, P, order):
    """Rank r of P: the window holds x at the positions the rank reads (dnm_mat_column_ranges) and NaN everywhere else;
    dnm_mat_mult_window, and dnm_mat_mult_window_local + _remote where the handle splits, give the reference's rows of
    the share exactly, zero padding inside the share, untouched guards."""
    from test_gpu_layout_handles import Shares, descriptor, handle
    r = ref.get("dm", L, k)
    p = ref.product("dm", L, k)
    sub = r.subspace()
    d = descriptor(sub, order)
    sh = Shares(sub, d, P)
    Lb = _lib.lib()
    for q in range(P):
        istart, ilen, _, nlen = sh.parts[q]
        mat = handle(r.arrs, d, q, P)
        desc = mat.describe()
        assert "two-pass" in desc and "bond graph" not in desc and (mat.row0, mat.m_local) == (istart, ilen), desc
        assert "diagonal on the fly" in desc, desc
        lo, hi = mat.column_window()
        n = C.c_int64()
        _lib.check(Lb.dnm_mat_column_ranges(mat.handle, 0, None, C.byref(n)))
        rg = (C.c_int64 * (2 * n.value))()
        _lib.check(Lb.dnm_mat_column_ranges(mat.handle, n.value, rg, C.byref(n)))
        marked = np.zeros(hi - lo + 1, dtype=bool)
        for i in range(n.value):
            assert lo <= rg[2 * i] < rg[2 * i + 1] <= hi + 1
            marked[rg[2 * i] - lo:rg[2 * i + 1] - lo] = True
        inside = (sh.gpos >= lo) & (sh.gpos <= hi)
        xw = np.zeros(hi - lo + 1, dtype=np.complex128)
        xw[sh.gpos[inside] - lo] = p.x[inside]
        xw[~marked] = NAN
        share = Layout.__new__(Layout)
        share.nint = ilen
        share.set_rows(sh.gpos[sh.rows[q]] - istart)
        assert sh.rows[q].size == nlen
        split = C.c_int()
        _lib.check(Lb.dnm_mat_window_split(mat.handle, C.byref(split)))
        assert split.value == 1
        Wn = DBuf(xw, NAN)
        Xl = DBuf(xw[istart - lo:istart - lo + ilen], NAN)
        for parts in (False, True):
            Y = share.fresh_y(False)
            if parts:
                _lib.check(Lb.dnm_mat_mult_window_local(mat.handle, Xl.ptr, Y.ptr, None))
                _lib.check(Lb.dnm_mat_mult_window_remote(mat.handle, Wn.ptr, lo, xw.size, Y.ptr, None))
            else:
                _lib.check(Lb.dnm_mat_mult_window(mat.handle, Wn.ptr, lo, xw.size, Y.ptr, None))
            share.check_y(Y, p.y[sh.rows[q]], False, "rank %d of %d, order %d, %s" % (q, P, order, "two calls" if parts else "one call"))
            assert Wn.untouched() and Xl.untouched()
        mat.destroy()


# ---------------------------------------------------------------- rounding

ROUNDING = [("lo pass complex", "dm-13-4", "tiled"), ("lo pass real", "chain-13-4-real", "tiled"),
            ("window pass (k = 1)", "dm-12-1", "tiled"), ("graph without the partner table", "graph_f-14-7", "noptab"),
            ("XParity", "chain_xp-14-7-", "tiled")]


@pytest.mark.parametrize("what,name,kind", ROUNDING, ids=[q[0] for q in ROUNDING])
def test_rounding(layout64, monkeypatch, what, name, kind):
    """Normal deviates against numpy.longdouble.  A component of an entry of y is a sum of n products in some order,
    with or without fma: n = the row's non-zero elements (real arithmetic; real-symmetric elements on complex vectors)
    or twice that (complex elements: two products per component).  Each product is rounded at most once and the sum
    takes n - 1 additions, so |got - ref| <= gamma(n) * sum |products| (Higham, Accuracy and Stability, (3.5)); the
    elements themselves -- sums of dyadic coefficients, times the sector sign -- are exact.  The reference's own error,
    gamma_64(n) of the same sum, is three orders below and added to the bound."""
    op, L, k, sector, real = ref.CASES[name]
    r = ref.get(op, L, k, sector)
    mat, d = open_handle(r, monkeypatch, KNOBS[kind], real=real)
    check_plan(mat, d, r, 6, kind, want="cached" if op == "graph_f" else "on the fly")
    lay = Layout(mat, r.N, sector is not None)
    rs = np.random.RandomState(len(name))
    x = rs.standard_normal(r.N) + (0 if real else 1j) * rs.standard_normal(r.N)
    yr, yi, mr, mi, cnt = r.rounding_reference(x)
    X, Y = lay.lay(x, real), lay.fresh_y(real)
    _lib.check(_lib.lib().dnm_mat_mult(mat.handle, X.ptr, Y.ptr, None))
    now = Y.payload()
    y = now if real else now.view(np.complex128)
    assert not y[lay.pad].any() and not np.isnan(now).any()
    got = y[lay.pos]
    n = cnt if (real or op in ref.REAL_OPS) else 2 * cnt
    bound_r = (gamma(n) + n * 2.0 ** -63) * mr
    bound_i = (gamma(n) + n * 2.0 ** -63) * mi
    er = np.abs(got.real.astype(np.longdouble) - yr)
    ei = np.abs(got.imag.astype(np.longdouble) - yi) if not real else np.zeros_like(er)
    ok = bound_r > 0
    ratio = float(max((er[ok] / bound_r[ok]).max(), (ei[ok] / bound_i[ok]).max() if not real else 0))
    print("rounding %s: %s, n up to %d, worst |got - ref| / bound = %.3f, worst error %.3e"
          % (what, d.split(",")[0], int(n.max()), ratio, float(max(er.max(), ei.max()))))
    assert np.all(er <= bound_r) and np.all(ei <= bound_i), ratio
    mat.destroy()
