"""
The tiled multiply of Full and Parity subspaces (csrc/matvec_kernels.hip: tile_pass_body, tile_pass_kernel,
tile_pass_flip_kernel; their launcher launch_cfg) through the C ABI, one call at a time, on device buffers of the test's
own, in exact arithmetic.

Exact cases: coefficients are multiples of 1/8, amplitudes Gaussian integers in [-8, 8], b = 3/8, c = -1/4 + 5/8 i
(tests/tiled_exact_ref.py, which asserts on the numbers of every case that all partial sums stay below 2^53 in units of
1/64).  Any order of summation, any grouping of terms into records and tables, with or without fma, then gives the same
VALUE, and the tests assert equality with the int64 reference -- of values, not of bits: -0.0 is allowed.
tests/test_tiled_exact_ref.py pins that reference to the oracle on every triple used here and proves from host-only
handles that the case table reaches every kernel instance, tile configuration, record class and diagonal form.

Buffers: every vector lies between two guards of 64 complex128 elements, element i at vec_pos(i, S).  The guards of x, z
and z2 hold NaN; y and its guards are filled with a sentinel before every call.  After every call: y equals the
reference, both guards of y hold their bits, no NaN is anywhere in y, x / z / z2 with their guards are bit-identical to
what was uploaded, the fused sums equal the reference's, and the slots of ``dot`` an entry does not own still hold the
sentinel.  On real-packed handles (two real amplitudes to an element) include/dynamite_amd.h says what dot[0] = <x, y>
and dot[2] = |y|^2 are and is silent on what dot[1] holds in real arithmetic: slots 0 and 2 are asserted.

Every case asserts, on the handle it multiplies with, the kernel instance of every pass, its (B, logR), its record
classes and the form of its diagonal -- the derivation of tests/test_tiled_exact_ref.py, equal to what the host-only
handle of the same case gave -- so that none silently runs another kernel.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import tiled_exact_ref as ref
from dynamite_amd import _lib, backend
from dynamite_amd.config import config
from plan_emulator import vec_pos
from test_gpu_sc3_exact import DBuf, GD
from test_flipflop import FlipPass
from test_gpu_vec import NAN, SENT, gamma
from test_tiled_exact_ref import _H, derive, descriptor, open_raw, plan_counts, set_knobs, signature

pytestmark = pytest.mark.gpu

ENTRIES = ("mult", "mult_dot", "lanczos", "lanczos_z", "sub", "sub2", "sub2_z2")


@pytest.fixture(autouse=True)
def own_layout():
    """Every handle here is made in the vector layout of its case (0, 5, 6, 8; 16 under the default_layout marker):
    ``Handle`` sets config.vec_swizzle to it, next to the descriptors it fills in by hand, and this puts back what the
    test found."""
    old = config.vec_swizzle
    yield
    config.vec_swizzle = old


class Handle:
    """A case's handle and where its vectors lie: ``nel`` elements (complex128; two real amplitudes each on a
    real-packed handle), element i at position pos[i]."""

    def __init__(self, case, monkeypatch, rank=0, nranks=1, check=True):
        set_knobs(monkeypatch, case)
        config.vec_swizzle = case.S
        self.case = case
        self.h, self._keep = open_raw(case, 0, rank, nranks)
        counts = plan_counts(self.h)
        assert counts[2] == 1, "not a tiled handle"
        self.nel = 1 << counts[5]
        self.pos = vec_pos(np.arange(self.nel), case.S)
        assert np.array_equal(np.sort(self.pos), np.arange(self.nel))
        l, r = C.c_int(), C.c_int()
        _lib.check(_lib.lib().dnm_mat_layouts(self.h, C.byref(l), C.byref(r)))
        assert (l.value, r.value) == (case.S, case.S)
        pk = C.c_int()
        _lib.check(_lib.lib().dnm_mat_is_real_packed(self.h, C.byref(pk)))
        assert bool(pk.value) == case.real
        if check and nranks == 1:
            self.passes = derive(self.h, case.flags)
            assert tuple(p["instance"] for p in self.passes) == case.instances, signature(self.passes)
            assert all(p["pair"] == case.pair for p in self.passes), signature(self.passes)
            hh, keep = open_raw(case, _lib.MAT_HOST_ONLY)
            try:
                assert signature(derive(hh, case.flags)) == signature(self.passes)
            finally:
                _lib.lib().dnm_mat_destroy(hh)

    def elements(self, v):
        """a vector in index order as the elements of the handle"""
        if self.case.real:
            assert not np.asarray(v).imag.any()
            return np.ascontiguousarray(np.asarray(v).real).view(np.complex128)
        return np.asarray(v, dtype=np.complex128)

    def lay(self, v, guard=NAN):
        a = np.empty(self.nel, dtype=np.complex128)
        a[self.pos] = self.elements(v)
        return DBuf(a, guard)

    def fresh_y(self, n=None):
        return DBuf(np.full(self.nel if n is None else n, SENT), SENT)

    def read_y(self, Y, what):
        """y in index order (real handles: the real amplitudes as complex numbers); guards intact, no NaN"""
        now = Y.payload()
        assert not np.isnan(now).any(), what + ": NaN in y"
        y = now.view(np.complex128)[self.pos]
        return y.view(np.float64) + 0j if self.case.real else y

    def check_y(self, Y, want, what):
        got = self.read_y(Y, what)
        bad = np.flatnonzero(got != want)
        if bad.size:
            i = int(bad[0])
            left = int(np.sum(got.real == SENT.real))
            raise AssertionError("%s: %d of %d rows differ (%d still hold the sentinel), the first is row %d: got %r, "
                                 "reference %r" % (what, bad.size, got.size, left, i, got[i], want[i]))
        assert np.array_equal(got, want)

    def destroy(self):
        _lib.lib().dnm_mat_destroy(self.h)


def run_entries(H, p, entries=ENTRIES, what=""):
    """Every entry of ``entries`` once, on buffers between guards, with all of the module's assertions."""
    Lb, h, real = _lib.lib(), H.h, H.case.real
    X, Z, Z2 = H.lay(p.x), H.lay(p.z), H.lay(p.z2)
    for name in entries:
        Y = H.fresh_y()
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
        H.check_y(Y, want, tag)
        assert X.untouched() and Z.untouched() and Z2.untouched(), tag + ": an input vector or its guard was written"
        if sums is not None:
            got = np.array(dot[:len(sums)])
            own = [0] if real and len(sums) == 2 else ([0, 2] if real else list(range(len(sums))))
            assert np.array_equal(got[own], sums[own]), "%s: fused sums %r, reference %r" % (tag, got.tolist(), sums.tolist())
            assert all(v == SENT.real for v in dot[len(sums):]), tag + ": a slot of dot the entry does not own was written"


def product(case):
    return ref.product(case.op, case.L, case.left, case.right, case.real)


# ---------------------------------------------------------------- every case of the table, every entry

SQUARE = sorted(n for n, c in ref.CASES.items() if c.square and c.S != 16)
PAIRS = sorted(n for n, c in ref.CASES.items() if not c.square)


@pytest.mark.parametrize("name", SQUARE)
def test_entries(monkeypatch, name):
    case = ref.CASES[name]
    H = Handle(case, monkeypatch)
    run_entries(H, product(case), what=name)
    H.destroy()


@pytest.mark.default_layout
def test_entries_production_layout(monkeypatch):
    """L = 18 in the production layout (shift 16: amplitudes beyond 2^16 move)"""
    case = ref.CASES["chain-18-prod"]
    assert config.vec_swizzle == case.S == 16
    H = Handle(case, monkeypatch)
    assert not np.array_equal(H.pos, np.arange(H.nel))
    run_entries(H, product(case), what="chain-18-prod")
    H.destroy()


@pytest.mark.parametrize("name", PAIRS)
def test_parity_pairs(monkeypatch, name):
    """Rectangular handles between the two Parity sectors: dnm_mat_mult exactly; the entries with sums refuse."""
    case = ref.CASES[name]
    H = Handle(case, monkeypatch)
    p = product(case)
    X, Y = H.lay(p.x), H.fresh_y()
    _lib.check(_lib.lib().dnm_mat_mult(H.h, X.ptr, Y.ptr, None))
    H.check_y(Y, p.y, name)
    assert X.untouched()
    dot = (C.c_double * 3)(SENT.real, SENT.real, SENT.real)
    Y = H.fresh_y()
    before = Y.t.clone()
    for call in (lambda: _lib.lib().dnm_mat_mult_lanczos(H.h, X.ptr, Y.ptr, None, 0.0, dot, None),
                 lambda: _lib.lib().dnm_mat_mult_dot(H.h, X.ptr, Y.ptr, dot, None)):
        with pytest.raises(_lib.BackendError, match="same subspace on both sides"):
            _lib.check(call())
    assert torch.equal(Y.t.view(torch.int64), before.view(torch.int64)) and all(v == SENT.real for v in dot)
    H.destroy()


# ---------------------------------------------------------------- refusals

def test_refusals(monkeypatch):
    case = ref.CASES["dm-10"]
    set_knobs(monkeypatch, case)
    with pytest.raises(_lib.BackendError):          # imaginary coefficients have no real-packed form
        open_raw(case, _lib.MAT_REAL_PACKED)
    # a Parity pair of two different vector layouts
    pc = ref.CASES["long_range-11-p01"]
    set_knobs(monkeypatch, pc)
    with pytest.raises(_lib.BackendError):
        backend.create_mat(*ref.arrays(pc.op, pc.L), descriptor(pc.left, pc.L, 6), descriptor(pc.right, pc.L, 5), False, 0)
    # x aliasing y (and, last, z aliasing y): every entry refuses and writes nothing
    H = Handle(case, monkeypatch)
    p = product(case)
    X, Z = H.lay(p.x), H.lay(p.z)
    Lb = _lib.lib()
    dot = (C.c_double * 3)(SENT.real, SENT.real, SENT.real)
    for call in (lambda: Lb.dnm_mat_mult(H.h, X.ptr, X.ptr, None),
                 lambda: Lb.dnm_mat_mult_dot(H.h, X.ptr, X.ptr, dot, None),
                 lambda: Lb.dnm_mat_mult_lanczos(H.h, X.ptr, X.ptr, None, 0.0, dot, None),
                 lambda: Lb.dnm_mat_mult_lanczos(H.h, X.ptr, X.ptr, Z.ptr, ref.B, dot, None),
                 lambda: Lb.dnm_mat_mult_sub(H.h, X.ptr, X.ptr, Z.ptr, ref.B, None),
                 lambda: Lb.dnm_mat_mult_sub2(H.h, X.ptr, X.ptr, Z.ptr, ref.B, None, 0.0, 0.0, None),
                 lambda: Lb.dnm_mat_mult_sub2(H.h, X.ptr, X.ptr, Z.ptr, ref.B, Z.ptr, -0.25, 0.625, None),
                 lambda: Lb.dnm_mat_mult_local(H.h, X.ptr, X.ptr, None),
                 lambda: Lb.dnm_mat_mult_local_part(H.h, X.ptr, X.ptr, 0, 2, None),
                 lambda: Lb.dnm_mat_mult_sub2(H.h, X.ptr, Z.ptr, Z.ptr, ref.B, None, 0.0, 0.0, None)):
        with pytest.raises(_lib.BackendError):
            _lib.check(call())
    assert X.untouched() and Z.untouched() and all(v == SENT.real for v in dot)
    H.destroy()


# ---------------------------------------------------------------- planted columns

def planted_indices(H):
    """Element indices where a wrong offset would show: the ends, around 2^B and 2^S, one with bits in [S, 2S - 4), the
    first and last index of the first and last workgroup of every window pass."""
    c, n = H.case, H.nel
    B, S = c.pair[0], c.S
    idx = {0, n - 1, (1 << B) - 1, 1 << B}
    if S:
        idx |= {(1 << S) - 1, 1 << S, (1 << S) | (1 << (2 * S - 5)) | 5}
    for i in range(len(H.passes)):
        d, _ = _H(H.h)._export(0, i)
        if d.nseg > 1:
            tb = 0
            for j in range(d.nseg):
                tb |= ((1 << d.seg_len[j]) - 1) << d.seg_pos[j]
            idx |= {0, tb, n - 1 - tb, n - 1}
    return sorted(i for i in idx if 0 <= i < n)


@pytest.mark.parametrize("name", ref.PLANTED)
def test_planted_columns(monkeypatch, name):
    """x = 3 - 2i at one index (real-packed handles: 3 in one lane of an element) and zero elsewhere: y is (3 - 2i) times
    that column of H, exactly, and exactly zero everywhere else, between untouched guards."""
    case = ref.CASES[name]
    H = Handle(case, monkeypatch)
    r = ref.get(case.op, case.L, case.left, case.right)
    amp = 3.0 if case.real else 3 - 2j
    if case.real:       # both lanes of the elements 0 and nel - 1, and of the elements picked above
        cols = sorted({2 * e + lane for e in planted_indices(H) for lane in (0, 1)})
        assert {0, 1, r.N - 2, r.N - 1} <= set(cols)
    else:
        cols = planted_indices(H)
    for j in cols:
        x = np.zeros(r.N, dtype=np.complex128)
        x[j] = amp
        want = amp * r.column(j)          # (small dyadic numbers: the product is exact)
        X, Y = H.lay(x), H.fresh_y()
        _lib.check(_lib.lib().dnm_mat_mult(H.h, X.ptr, Y.ptr, None))
        H.check_y(Y, want, "%s column %d" % (name, j))
        assert X.untouched()
    H.destroy()


# ---------------------------------------------------------------- ranges of one pass

def free_bits(H, top, logp):
    """the logp index bits ending at ``top`` lie outside the tile of every local pass"""
    for i in range(len(H.passes)):
        d, _ = _H(H.h)._export(0, i)
        tb = 0
        for j in range(d.nseg):
            tb |= ((1 << d.seg_len[j]) - 1) << d.seg_pos[j]
        if any((tb >> b) & 1 for b in range(top - logp + 1, top + 1)):
            return False
    return True


@pytest.mark.parametrize("name", ref.PARTS)
def test_ranges_of_one_pass(monkeypatch, name):
    """dnm_mat_mult_local_part for nparts = 2, 4: the parts together write, bit for bit, what dnm_mat_mult_local writes.
    Where dnm_mat_local_part_bits names the top free bit and no gathers, and the log2(nparts) index bits ending there are
    outside every tile, every position outside a part's range still holds the sentinel after that part's call and every
    position inside it the final value.  A plan of several passes whose ranges are not the same amplitudes in every pass
    (low12-13-m0 at nparts = 4: the window tile of the second pass holds bit 11) is refused and nothing is written."""
    case = ref.CASES[name]
    H = Handle(case, monkeypatch)
    Lb = _lib.lib()
    top, gathers = C.c_int(), C.c_int()
    _lib.check(Lb.dnm_mat_local_part_bits(H.h, C.byref(top), C.byref(gathers)))
    p = product(case)
    X, Yw = H.lay(p.x), H.fresh_y()
    _lib.check(Lb.dnm_mat_mult_local(H.h, X.ptr, Yw.ptr, None))
    H.check_y(Yw, p.y, name)
    whole = Yw.payload().view(np.complex128)[H.pos]
    sent = H.fresh_y().payload().view(np.complex128)
    refused = 0
    for nparts in (2, 4):
        logp = nparts.bit_length() - 1
        own = top.value >= 0 and gathers.value == 0 and free_bits(H, top.value, logp)
        if len(H.passes) > 1 and not own:
            Y = H.fresh_y()
            for part in range(nparts):
                with pytest.raises(_lib.BackendError, match="are not the amplitudes of the ranges of its first pass"):
                    _lib.check(Lb.dnm_mat_mult_local_part(H.h, X.ptr, Y.ptr, part, nparts, None))
            assert np.array_equal(Y.payload().view(np.uint64), sent.view(np.uint64))
            refused += 1
            continue
        Y = H.fresh_y()
        for part in range(nparts):
            _lib.check(Lb.dnm_mat_mult_local_part(H.h, X.ptr, Y.ptr, part, nparts, None))
            if own:
                mine = ((np.arange(H.nel) >> (top.value + 1 - logp)) & (nparts - 1)) == part
                Y1 = H.fresh_y()
                _lib.check(Lb.dnm_mat_mult_local_part(H.h, X.ptr, Y1.ptr, part, nparts, None))
                now = Y1.payload().view(np.complex128)[H.pos]
                assert np.array_equal(now[~mine].view(np.uint64), sent[:np.count_nonzero(~mine)].view(np.uint64)), (name, nparts, part)
                assert np.array_equal(now[mine].view(np.uint64), whole[mine].view(np.uint64)), (name, nparts, part)
        assert np.array_equal(Y.payload().view(np.complex128)[H.pos].view(np.uint64), whole.view(np.uint64)), (name, nparts)
        assert X.untouched()
    assert refused == (1 if name == "low12-13-m0" else 0)
    H.destroy()


# ---------------------------------------------------------------- shares of a partition, on one GPU

@pytest.mark.parametrize("name,P", ref.SHARES)
def test_shares(monkeypatch, name, P):
    """Ranks 0 .. P-1 of P, each on this one GPU: dnm_mat_mult_local on the rank's block, then dnm_mat_mult_remote with
    the partner slices the exchange plan names (device memory as it lies).  Exact; every remote call leaves y outside
    [y_off, y_off + count) bit for bit as it was; the fused entries refuse a handle with partner passes."""
    case = ref.CASES[name]
    p = product(case)
    Lb = _lib.lib()
    nloc = p.x.size // P
    handles = [Handle(case, monkeypatch, q, P) for q in range(P)]
    assert all(H.nel == nloc for H in handles)
    xs = [handles[q].lay(p.x[q * nloc:(q + 1) * nloc]) for q in range(P)]
    remote = 0
    for q, H in enumerate(handles):
        Y = H.fresh_y()
        _lib.check(Lb.dnm_mat_mult_local(H.h, xs[q].ptr, Y.ptr, None))
        sends, recvs = backend.exchange_plan(H.h)
        counts = plan_counts(H.h)
        assert counts[1] == len(recvs)
        for i, (partner, off, cnt) in enumerate(recvs):
            d, _ = _H(H.h)._export(1, i)
            y_off = int(d.sign_base) & (nloc - 1)
            assert cnt == 1 << d.n_eff and 0 <= off and off + cnt <= nloc and y_off + cnt <= nloc
            XR = DBuf(xs[partner].host[GD + 2 * off:GD + 2 * (off + cnt)], NAN)
            before = Y.t.clone()
            _lib.check(Lb.dnm_mat_mult_remote(H.h, i, XR.ptr, Y.ptr, None))
            keep = torch.ones(Y.t.numel(), dtype=torch.bool, device=Y.t.device)
            keep[GD + 2 * y_off:GD + 2 * (y_off + cnt)] = False
            assert torch.equal(Y.t.view(torch.int64)[keep], before.view(torch.int64)[keep]), "written outside the pass's block"
            assert XR.untouched()
            remote += 1
        H.check_y(Y, p.y[q * nloc:(q + 1) * nloc], "%s rank %d of %d" % (name, q, P))
        assert xs[q].untouched()
        if recvs:
            dot = (C.c_double * 3)(SENT.real, SENT.real, SENT.real)
            Z = H.lay(p.z[q * nloc:(q + 1) * nloc])
            with pytest.raises(_lib.BackendError, match="couples different ranks"):
                _lib.check(Lb.dnm_mat_mult_lanczos(H.h, xs[q].ptr, Y.ptr, None, 0.0, dot, None))
            with pytest.raises(_lib.BackendError, match="couples different ranks"):
                _lib.check(Lb.dnm_mat_mult_sub2(H.h, xs[q].ptr, Y.ptr, Z.ptr, ref.B, None, 0.0, 0.0, None))
            assert all(v == SENT.real for v in dot)
    assert remote >= P          # (every rank has a partner pass)
    for H in handles:
        H.destroy()


# ---------------------------------------------------------------- rounding

def exchanges(H):
    """[(mask in index space, 8 c)] of the bonds the handle runs as flip-flop exchanges (the tile records of its passes)"""
    out = []
    for i in range(len(H.passes)):
        fp = FlipPass(_H(H.h), i)
        if not fp.on:
            continue
        d = fp.desc
        for F in fp.flips[:fp.loop[2]]:
            m = 0
            for k in range(d.nseg):
                m |= ((F.mask_tile >> d.seg_off[k]) & ((1 << d.seg_len[k]) - 1)) << d.seg_pos[k]
            assert F.c * 8 == int(F.c * 8)
            out.append((m, int(F.c * 8)))
    assert len({m for m, _ in out}) == len(out)
    return out


@pytest.mark.parametrize("what,name", ref.ROUNDING, ids=[q[0] for q in ref.ROUNDING])
def test_rounding(monkeypatch, what, name):
    """Normal deviates against numpy.longdouble.  The coefficients stay dyadic, so everything the kernel adds up BEFORE it
    multiplies by an amplitude -- slot amplitudes a0 + a1 (matvec_kernels.hip: accum_record), table entries, the dext
    butterfly, D[] and its Walsh-Hadamard levels, the flip-flop constant -- is exact; what rounds is the chain of fmas
    into a component of an accumulator: one for the diagonal (diag_part2: D(row) times the row's amplitude), one per real
    term off the diagonal and two per imaginary one (a real record of one or two terms does one fma per component, a
    complex record and a table record two: accum_record, apply_tabs; a flip-flop record one for its two terms: flip_fma),
    and the late add of y of every pass after the first (late_y).  n is counted per row from the terms that reach it,
    and |got - ref| <= gamma(n) * sum |products| per row and component (Higham, Accuracy and Stability, (3.5)): the
    diagonal's one product, the moduli of the terms' products off the diagonal (which bounds every grouping of them),
    and for the bonds a handle runs as exchanges the products of that form -- c x_partner where the bond's bits
    differ, c x_row where they agree, and the diagonal D - c there (tiled_exact_ref.Ref.rounding_reference).  The
    reference's own error, n 2^-63 of the same sum, is added to the bound."""
    case = ref.CASES[name]
    H = Handle(case, monkeypatch)
    r = ref.get(case.op, case.L, case.left, case.right)
    rs = np.random.RandomState(len(name))
    x = rs.standard_normal(r.N) + (0 if case.real else 1j) * rs.standard_normal(r.N)
    ex = exchanges(H)
    assert bool(ex) == any(p["classes"] & {"FL_TILE_T", "FL_TILE_K"} for p in H.passes)
    yr, yi, mr, mi, n = r.rounding_reference(x, ex)
    n = n + (len(H.passes) - 1)
    X, Y = H.lay(x), H.fresh_y()
    _lib.check(_lib.lib().dnm_mat_mult(H.h, X.ptr, Y.ptr, None))
    got = H.read_y(Y, name)
    bound_r = (gamma(n) + n * 2.0 ** -63) * mr
    bound_i = (gamma(n) + n * 2.0 ** -63) * mi
    er = np.abs(got.real.astype(np.longdouble) - yr)
    ei = np.abs(got.imag.astype(np.longdouble) - yi)
    ok = bound_r > 0
    ratio = float(max((er[ok] / bound_r[ok]).max(), 0 if case.real else (ei[ok] / bound_i[ok]).max()))
    print("rounding %s: %s, n up to %d, worst |got - ref| / bound = %.4f, worst error %.3e"
          % (what, name, int(n.max()), ratio, float(max(er.max(), ei.max()))))
    assert np.all(er <= bound_r) and (case.real or np.all(ei <= bound_i)), ratio
    H.destroy()
