"""The sweeps that visit every row or column and reduce to a small answer -- ||H||_inf, the cached diagonal,
CheckConserves, the column window, the chunk map and the local rows of a window partition -- against the host references
of tests/row_sweep_ref.py (which tests/test_row_sweep_ref.py pins against the oracle), on operators with a PLANTED row:
one row, column or matrix element decides the answer, so a dropped lane, wavefront, workgroup, grid-stride trip or launch
slice changes it.  All coefficients are dyadic, every sum is exact in double: the comparisons are == / array_equal; the
one tolerance is 4 ulp where an element of the norm goes through hypot."""
import ctypes as C

import numpy as np
import pytest

import row_sweep_ref as ref
from dynamite_amd import _lib, backend
from dynamite_amd.config import config
from dynamite_amd.subspaces import Parity, SpinConserve
from oracle import oracle as orc
from gpu_util import orc_sub, vec_from, rand_state
from test_gpu_matvec import tol_for

pytestmark = pytest.mark.gpu


def handle(arrs, left, right=None, rank=0, nranks=1):
    right = left if right is None else right
    config._initialize()
    h = backend.create_mat(*arrs, left._c(), right._c(), flags=0, rank=rank, nranks=nranks)
    return backend.ShellMat(h, left._c(), right._c(), nranks, rank)


def norm_of(mat):
    """This handle's own maximum (a partitioned handle: of its rows; the caller reduces)."""
    v = C.c_double()
    _lib.check(_lib.lib().dnm_mat_norm_inf(mat.handle, C.byref(v), None))
    return v.value


def diagonal_of(mat):
    mat.precompute_diagonal()
    d = np.full(mat.m_local, np.nan)
    _lib.check(_lib.lib().dnm_mat_get_diagonal(mat.handle, _lib.pf64(d), None))
    return d


# ---- 1. norm: a planted maximum -------------------------------------------------------------------------------------

@pytest.mark.parametrize("place", range(8))
@pytest.mark.parametrize("shape", ref.NORM_SHAPES)
def test_norm_planted_maximum(shape, place):
    """The smallest shapes whose rows take a second trip of norm_kernel's grid-stride loop (4096 workgroups of 256
    rows), the planted row at both ends of a workgroup, on both sides of the trip boundary, in the last wavefront of a
    second-trip workgroup, in the (ragged) last workgroup and last of all.  A missed planted row lowers the norm by at
    least 2^(1-L) ~ 1e-6.  Variant A is exact; variant B has one element that goes through hypot: 4 ulp."""
    index = ref.norm_placements(ref.NORM_DIMS[shape])[place]
    for variant in ('A', 'B'):
        sub, arrs, _ = ref.norm_case(shape, index, variant)
        s = ref.row_sums(arrs, sub, sub)
        want = s.max()
        assert np.flatnonzero(s == want).tolist() == [index] and np.sort(s)[-2] <= want - 2.0 ** (1 - sub.L)
        mat = handle(arrs, sub)                 # (a fresh handle: the norm is cached in it)
        got = norm_of(mat)
        mat.destroy()
        print(shape, index, variant, repr(got), repr(want))
        if variant == 'A':
            assert got == want
        else:
            assert abs(got - want) <= 4 * 2.0 ** -52 * want


def test_norm_all_sixteen_pairs():
    """Every (left, right) pair of subspace types at L = 13: the contains(bra, right) filter of each right type under
    the maps of each left type.  Exact."""
    subs, rstar = ref.pair_subspaces()
    arrs = ref.planted_operator(13, rstar, 'A')
    for ln, left in subs.items():
        for rn, right in subs.items():
            s = ref.row_sums(arrs, left, right)
            assert np.flatnonzero(s == s.max()).tolist() == [int(left.state_to_idx(rstar))]
            mat = handle(arrs, left, right)
            got = norm_of(mat)
            mat.destroy()
            assert got == s.max(), (ln, rn, got, s.max())


@pytest.mark.parametrize("shape,P", [('sc', 3), ('explicit', 3), ('full', 2)])
def test_norm_partitioned(shape, P):
    """Each rank's own maximum is the reference restricted to its rows: the rank that holds the planted row (not rank 0)
    returns the norm, the others the lower value of their rows."""
    M = ref.NORM_DIMS[shape]
    index = backend.split_ownership(M, P, P - 1)[0] + 3 * 64 + 37
    sub, arrs, _ = ref.norm_case(shape, index, 'A')
    s = ref.row_sums(arrs, sub, sub)
    assert np.flatnonzero(s == s.max()).tolist() == [index]
    got = []
    for r in range(P):
        mat = handle(arrs, sub, rank=r, nranks=P)
        row0, m = backend.split_ownership(M, P, r)
        got.append(norm_of(mat))
        mat.destroy()
        assert got[-1] == s[row0:row0 + m].max(), (r, got[-1])
    assert got[P - 1] == s.max() and max(got[:P - 1]) <= s.max() - 2.0 ** (1 - sub.L)


# ---- 2. diagonal ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ref.NORM_SHAPES)
def test_diagonal_in_slices(monkeypatch, shape):
    """diag_kernel in launches of 2^20 rows (at least two per shape, the last one ragged for SpinConserve and Explicit):
    every row's diagonal, exact."""
    monkeypatch.setenv("DNM_LAUNCH_SLICE_LOG2", "20")
    sub, arrs, _ = ref.norm_case(shape, ref.TRIP + 229, 'B')
    mat = handle(arrs, sub)
    got = diagonal_of(mat)
    mat.destroy()
    assert np.array_equal(got, ref.diagonal(arrs, sub))


def test_diagonal_partitioned(monkeypatch):
    """Rank 1 of 3, SpinConserve in reference order: the rows [row0, row0 + m) only, in slices of 2^10."""
    monkeypatch.setenv("DNM_LAUNCH_SLICE_LOG2", "10")
    monkeypatch.setattr(config, "sc_layout", None)
    sub = SpinConserve(16, 8)
    arrs = ref.planted_operator(16, int(sub.idx_to_state(5000)), 'B')
    mat = handle(arrs, sub, rank=1, nranks=3)
    row0, m = backend.split_ownership(sub.get_dimension(), 3, 1)
    assert (mat.row0, mat.m_local) == (row0, m)
    got = diagonal_of(mat)
    mat.destroy()
    assert np.array_equal(got, ref.diagonal(arrs, sub, row0, m))


# ---- 3. conserves: a planted violation ------------------------------------------------------------------------------

def _fields(L, zero_at=None):
    from dynamite_amd.operators import identity
    H = ref.planted_fields(L, 0x1234)
    if zero_at is not None:
        H = H + (-zero_at) * identity()
    return ref.marshal(H, L)


def gpu_conserves(arrs, left, right, xparity=False):
    return backend.check_conserves(*arrs, left._to_c(), right._to_c(), xparity=xparity)


@pytest.mark.parametrize("slice_log2", [None, 10])
@pytest.mark.parametrize("kind", ['full', 'parity', 'sc', 'explicit'])
def test_conserves_one_column_leaves_the_left_subspace(monkeypatch, kind, slice_log2):
    """A diagonal operator, non-zero on every column; right = a subspace of each type, left = Explicit(its states without
    the one at column j): that single column decides.  With the state put back, or with a diagonal that is exactly zero
    at that column (the reference forgives a zero element), the verdict is True."""
    if slice_log2:
        monkeypatch.setenv("DNM_LAUNCH_SLICE_LOG2", str(slice_log2))
    L = 14
    arrs = _fields(L)
    right = ref.conserves_sector(kind, L)
    assert gpu_conserves(arrs, ref.explicit(ref.states_of(right), L), right) is True
    for j in ref.conserves_columns(right.get_dimension(), sliced=bool(slice_log2)):
        left = ref.minus_one(right, j)
        assert ref.conserves(arrs, left, right)[1].tolist() == [j]
        assert gpu_conserves(arrs, left, right) is False, j
        z = _fields(L, zero_at=ref.diagonal(arrs, right, j, 1)[0])
        assert ref.conserves(z, left, right)[0] is True
        assert gpu_conserves(z, left, right) is True, j


@pytest.mark.parametrize("slice_log2", [None, 10])
@pytest.mark.parametrize("kind", ['parity', 'sc'])
def test_conserves_one_outsider_among_the_columns(monkeypatch, kind, slice_log2):
    """left = a Parity / SpinConserve sector, right = Explicit(its states plus one outsider that sorts to column j)."""
    if slice_log2:
        monkeypatch.setenv("DNM_LAUNCH_SLICE_LOG2", str(slice_log2))
    L = 14
    arrs = _fields(L)
    n = ref.conserves_sector(kind, L).get_dimension() + 1
    for j in ref.conserves_columns(n, sliced=bool(slice_log2)):
        left, right = ref.plus_outsider(kind, j, L)
        assert ref.conserves(arrs, left, right)[1].tolist() == [j]
        assert gpu_conserves(arrs, left, right) is False, j
        assert gpu_conserves(arrs, left, ref.explicit(ref.states_of(left), L)) is True


def test_conserves_imaginary_only_and_cancelling():
    """X_i Y_j + Y_i X_j on SpinConserve leaves the sector with the element 2i (real part zero): False.
    X_i X_j + Y_i Y_j cancels exactly on the columns that would leave it: True."""
    from dynamite_amd.operators import sigmax, sigmay
    L = 14
    sub = SpinConserve(L, 7)
    imag = ref.marshal(sigmax(2) * sigmay(9) + sigmay(2) * sigmax(9), L)
    assert np.all(imag[3].real == 0) and ref.conserves(imag, sub, sub)[0] is False
    assert gpu_conserves(imag, sub, sub) is False
    real = ref.marshal(sigmax(2) * sigmax(9) + sigmay(2) * sigmay(9), L)
    assert ref.conserves(real, sub, sub)[0] is True
    assert gpu_conserves(real, sub, sub) is True


def test_conserves_xparity_looks_at_half_the_columns():
    L = 14
    arrs = _fields(L)
    right = SpinConserve(L, 7)
    half = right.get_dimension() // 2
    for j, with_flag in ((half, True), (2 * half - 1, True), (half - 1, False), (0, False)):
        left = ref.minus_one(right, j)
        assert ref.conserves(arrs, left, right, xparity=True)[0] is with_flag
        assert gpu_conserves(arrs, left, right, xparity=True) is with_flag, j
        assert gpu_conserves(arrs, left, right) is False, j


# ---- 4. column window, chunk map, local rows ------------------------------------------------------------------------

def window_of(mat):
    return mat.column_window()


def chunks_of(mat, shift):
    lo, hi = mat.column_window()
    n = (hi >> shift) - (lo >> shift) + 1
    cmap = np.full(n, 7, dtype=np.uint8)
    _lib.check(_lib.lib().dnm_mat_column_chunks(mat.handle, shift, cmap.ctypes.data_as(C.POINTER(C.c_uint8)), n, None))
    return cmap


def local_rows_of(mat, col_lo, col_hi, max_ranges, min_blocks):
    buf = (C.c_int64 * (2 * max_ranges))()
    n = C.c_int()
    _lib.check(_lib.lib().dnm_mat_window_local_rows(mat.handle, col_lo, col_hi, max_ranges, min_blocks, buf, C.byref(n),
                                                    None))
    return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(n.value)]


def mult_window(mat, xw, lo, n):
    xv, yl = vec_from(xw), vec_from(np.full(n, 777.0 + 0j))
    _lib.check(_lib.lib().dnm_mat_mult_window(mat.handle, xv.ptr, lo, xw.size, yl.ptr, None))
    return yl.local_numpy()


def window_pair(kind):
    """(left, right, operator arrays, gather kernel?) of the partitions whose maps come from a device sweep."""
    if kind in ('sc_row', 'sc_block'):
        sub = SpinConserve(16, 8)                                   # 12870 rows
        return sub, sub, ref.window_operator(16), False
    if kind == 'explicit':
        rs = np.random.RandomState(44)
        sub = ref.explicit(np.unique(rs.randint(0, 1 << 15, size=9000)), 15)    # ~ 7900 of 32768 states
        return sub, sub, ref.window_operator(15), True
    if kind == 'explicit_64k':
        rs = np.random.RandomState(45)
        sub = ref.explicit(np.sort(rs.choice(1 << 18, size=1 << 16, replace=False)), 18)
        return sub, sub, ref.window_operator(18), True
    assert kind == 'projection'
    return Parity('odd', L=14), SpinConserve(14, 7), ref.window_operator(14), True     # (seven spins down: odd)


@pytest.fixture
def index_order(monkeypatch):
    """A window partition works in index order: no swizzled Parity vectors, SpinConserve in reference order."""
    monkeypatch.setattr(config, "sc_layout", None)
    monkeypatch.setattr(config, "vec_swizzle", 0)


@pytest.mark.parametrize("P", [2, 3, 5])
@pytest.mark.parametrize("kind", ['sc_row', 'sc_block', 'explicit', 'explicit_64k', 'projection'])
def test_window_maps_and_unmarked_columns(index_order, monkeypatch, kind, P):
    """For every rank: hull(need) within [cmin, cmax] within hull(reach + own block) (the gather kernel: hull(reach)
    exactly); the one-byte-per-column map between need and reach + own block (gather: reach exactly), the coarser maps its
    exact coarsening; the local rows exactly the runs of workgroups that reach nothing outside the own block; and a
    multiply whose window holds NaN at every unmarked column bit-identical to the one on the whole window (and within
    the usual bar of the oracle): what is not marked is not read."""
    if kind == 'sc_block':
        monkeypatch.setenv("DNM_SC_BLOCK", "10")
    left, right, arrs, gather = window_pair(kind)
    M, N = left.get_dimension(), right.get_dimension()
    x = rand_state(N, seed=P)
    yref = orc.matvec(orc.Msc(*arrs), orc_sub(left), orc_sub(right), x)
    for r in range(P):
        mat = handle(arrs, left, right, rank=r, nranks=P)
        if kind == 'sc_block':
            assert "block form" in mat.describe()
        row0, m = backend.split_ownership(M, P, r)
        assert (mat.row0, mat.m_local) == (row0, m)
        reach, need, cols = ref.column_sets(arrs, left, right, row0, m)
        own = np.arange(row0, row0 + m)
        lo, hi = window_of(mat)
        assert reach.size and need.size
        if gather:
            assert (lo, hi) == ref.hull(reach), (r, lo, hi)
        else:
            nlo, nhi = ref.hull(need)
            olo, ohi = ref.hull(reach, own)
            assert olo <= lo <= nlo and nhi <= hi <= ohi, (r, lo, hi)
        cmap = chunks_of(mat, 0)
        assert set(np.unique(cmap).tolist()) <= {0, 1}
        marked = lo + np.flatnonzero(cmap)
        if gather:
            assert np.array_equal(marked, reach), r
        else:
            assert np.isin(need, marked).all() and np.isin(marked, np.union1d(reach, own)).all(), r
        for shift in (3, 7):
            assert np.array_equal(chunks_of(mat, shift), ref.coarsen(cmap, lo, shift)), (r, shift)
        # rows that read only the rank's own block of x (columns [row0, row0 + m) of a square operator)
        c0, c1 = backend.split_ownership(N, P, r)
        c1 += c0
        runs = ref.local_runs(cols, c0, c1)
        assert local_rows_of(mat, c0, c1, 4096, 1) == ref.select_runs(runs, m, 4096, 1), r
        one = ref.select_runs(runs, m, 1, 2)
        if one is not None:
            assert local_rows_of(mat, c0, c1, 1, 2) == one, r
        # unmarked means unread
        xw = x[lo:hi + 1].copy()
        y_full = mult_window(mat, xw, lo, m)
        xw[cmap == 0] = complex(np.nan, np.nan)
        y_nan = mult_window(mat, xw, lo, m)
        mat.destroy()
        assert np.array_equal(y_full.view(np.uint64), y_nan.view(np.uint64)), (r, int(np.isnan(y_nan).sum()))
        assert np.max(np.abs(y_full - yref[row0:row0 + m])) <= tol_for(arrs, x), r


FAR_POSITIONS = [0, 64 + 37, 128 + 5, 255, 256, 900, 1000]      # every wavefront of workgroup 0, workgroup 1, the ragged
#                                                                 last workgroup (rows 768..1000) and the last row


@pytest.mark.parametrize("pos", FAR_POSITIONS)
def test_window_planted_far_column(index_order, pos):
    """Explicit, L = 16, X_15 plus a diagonal on 3000 states below 2^15 (none of their partners is in the basis) and the
    partner of the state at position ``pos`` of rank 0, which sorts last: that single row decides rank 0's cmax (the
    partner's index) and the last rank's cmin (``pos``); without the partner the window falls back to the own block."""
    P = 3
    sub, arrs = ref.far_column_case(pos)
    n = sub.get_dimension()
    m0 = backend.split_ownership(n, P, 0)[1]
    assert n == 3001 and m0 == 1001 and pos < m0
    mat = handle(arrs, sub, rank=0, nranks=P)
    reach, _, cols = ref.column_sets(arrs, sub, sub, 0, m0)
    assert reach.tolist() == list(range(m0)) + [n - 1]
    assert window_of(mat) == (0, n - 1)
    assert np.array_equal(np.flatnonzero(chunks_of(mat, 0)), reach)
    # every workgroup but the one that holds the planted row reads nothing but the own block
    b = pos // ref.ROWS_PER_WG
    runs = [(b0, b1) for b0, b1 in ((0, b), (b + 1, 4)) if b1 > b0]
    assert ref.local_runs(cols, 0, m0) == runs
    assert local_rows_of(mat, 0, m0, 16, 1) == ref.select_runs(runs, m0, 16, 1)
    longest = ref.select_runs(runs, m0, 1, 2)
    assert longest is not None and local_rows_of(mat, 0, m0, 1, 2) == longest
    mat.destroy()
    row0, m = backend.split_ownership(n, P, P - 1)
    mat = handle(arrs, sub, rank=P - 1, nranks=P)
    assert window_of(mat) == (pos, n - 1) == ref.hull(ref.column_sets(arrs, sub, sub, row0, m)[0])
    mat.destroy()
    sub, arrs = ref.far_column_case(pos, with_partner=False)
    m0 = backend.split_ownership(n - 1, P, 0)[1]
    mat = handle(arrs, sub, rank=0, nranks=P)
    assert window_of(mat) == (0, m0 - 1) == ref.hull(ref.column_sets(arrs, sub, sub, 0, m0)[0])
    assert local_rows_of(mat, 0, m0, 16, 1) == [(0, m0)]
    mat.destroy()


# ---- ... and the internal SpinConserve layout: what lies outside dnm_mat_column_ranges is not read -------------------

@pytest.fixture
def small_layout():
    old = (config.sc_layout, config.sc_layout_min_dim)
    config.sc_layout, config.sc_layout_min_dim = (6, 4), 0
    yield
    config.sc_layout, config.sc_layout_min_dim = old


def chain_operator(L):
    from dynamite_amd.operators import sigmax, sigmay, sigmaz, op_sum
    hop = lambda i, j: sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j)
    return ref.marshal(op_sum(0.5 * hop(i, i + 1) + 2.0 ** -(i % 4) * sigmaz(i) * sigmaz(i + 1) for i in range(L - 1)), L)


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("kind", ['chain', 'graph'])
def test_internal_layout_reads_only_its_column_ranges(small_layout, kind, P):
    """Partitioned SpinConserve in the internal layout (windows are ranges of the layout, the needed positions come from
    host tables: dnm_mat_column_ranges): NaN at every position of the window outside those ranges leaves y bit-identical,
    in one call and -- where the multiply splits -- as the local part on the rank's own block plus the remote part on the
    window; y is within the usual bar of the oracle."""
    L, k = 16, 8
    sub = SpinConserve(L, k)
    d = sub._c()
    assert d.vec_swizzle == (6 | (4 << 8))
    arrs = chain_operator(L) if kind == 'chain' else ref.window_operator(L)
    N = sub.get_dimension()
    x = rand_state(N, seed=P)
    yref = orc.matvec(orc.Msc(*arrs), orc_sub(sub), orc_sub(sub), x)
    Lb = _lib.lib()

    def positions(idx, part):
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        out = np.empty_like(idx)
        _lib.check(Lb.dnm_vec_layout_positions_host(C.byref(d), C.byref(part) if part is not None else None, idx.size,
                                                    _lib.p64(idx), _lib.p64(out)))
        return out
    gpos = positions(np.arange(N), None)
    for r in range(P):
        istart, ilen, nstart, nlen = backend.layout_partition(d, P, r)
        config._initialize()
        h = backend.create_mat(*arrs, d, d, flags=0, rank=r, nranks=P)
        mat = backend.ShellMat(h, d, d, P, r)
        assert (mat.row0, mat.m_local) == (istart, ilen) and mat.swz_right == d.vec_swizzle
        lo, hi = mat.column_window()
        assert lo <= istart and istart + ilen - 1 <= hi
        n = C.c_int64()
        _lib.check(Lb.dnm_mat_column_ranges(mat.handle, 0, None, C.byref(n)))
        rg = (C.c_int64 * (2 * n.value))()
        _lib.check(Lb.dnm_mat_column_ranges(mat.handle, n.value, rg, C.byref(n)))
        marked = np.zeros(hi - lo + 1, dtype=bool)
        for i in range(n.value):
            assert lo <= rg[2 * i] < rg[2 * i + 1] <= hi + 1
            marked[rg[2 * i] - lo:rg[2 * i + 1] - lo] = True
        assert marked[istart - lo:istart - lo + ilen].all()          # the own block is always read
        inside = (gpos >= lo) & (gpos <= hi)
        xw = np.zeros(hi - lo + 1, dtype=np.complex128)              # (padding positions: zero)
        xw[gpos[inside] - lo] = x[inside]
        xnan = xw.copy()
        xnan[~marked] = complex(np.nan, np.nan)
        split = C.c_int()
        _lib.check(Lb.dnm_mat_window_split(mat.handle, C.byref(split)))

        def run(w, parts):
            wv, yv = vec_from(w), vec_from(np.full(ilen, 777.0 + 0j))
            if parts:
                xl = vec_from(w[istart - lo:istart - lo + ilen])
                _lib.check(Lb.dnm_mat_mult_window_local(mat.handle, xl.ptr, yv.ptr, None))
                _lib.check(Lb.dnm_mat_mult_window_remote(mat.handle, wv.ptr, lo, w.size, yv.ptr, None))
            else:
                _lib.check(Lb.dnm_mat_mult_window(mat.handle, wv.ptr, lo, w.size, yv.ptr, None))
            return yv.local_numpy()
        lpos = positions(np.arange(nlen), _lib.Partition(r, P))
        print(kind, P, r, "splits" if split.value else "one call", "unmarked positions:", int((~marked).sum()))
        for parts in ([False, True] if split.value else [False]):
            y_full, y_nan = run(xw, parts), run(xnan, parts)
            assert np.array_equal(y_full[lpos].view(np.uint64), y_nan[lpos].view(np.uint64)), \
                (r, parts, int(np.isnan(y_nan[lpos]).sum()), int((~marked).sum()))
            assert np.max(np.abs(y_full[lpos] - yref[nstart:nstart + nlen])) <= tol_for(arrs, x), (r, parts)
        mat.destroy()
