"""Handles of PARTITIONED SpinConserve operators in the internal three-field layout (csrc/sc3.h), in both block orders,
and the XParity handle on top of a layout with empty blocks: what a handle's block range means.

A handle covers the blocks [T0, T1) of the layout's block sequence -- PLACES in Sc3Layout::tseq, not values of T.  In
block order 0 that is a range of the reference order too; in block order 1 (the solver's partition, Operator.
get_solver_mat) it is not, and whatever sweeps a handle's rows in reference order -- the norm, the cached diagonal, the
host's position map -- has to walk the share's own rows or refuse.  The rows of rank r are told here WITHOUT the
handle: the reference indices whose position in the whole vector (dnm_vec_layout_positions_host, no partition) lies
in the rank's range of the layout (dnm_vec_layout_partition).  The method is that of test_gpu_row_sweeps.py: operators
with a planted row, dyadic coefficients, exact comparisons against tests/row_sweep_ref.py."""
import ctypes as C

import numpy as np
import pytest

import row_sweep_ref as ref
from dynamite_amd import _lib, backend, msc_tools
from dynamite_amd.config import config
from dynamite_amd.subspaces import SpinConserve, XParity
from oracle import oracle as orc
from gpu_util import orc_sub, vec_from, rand_state
from test_gpu_matvec import tol_for
from test_gpu_row_sweeps import norm_of, diagonal_of, chain_operator

pytestmark = pytest.mark.gpu

SHAPES = [(16, 8), (15, 7)]        # 64 and 32 T blocks in the (6, 4) layout: block order 1 really permutes them
RANKS = [2, 3, 4]


@pytest.fixture
def small_layout():
    old = (config.sc_layout, config.sc_layout_min_dim)
    config.sc_layout, config.sc_layout_min_dim = (6, 4), 0
    yield
    config.sc_layout, config.sc_layout_min_dim = old


def descriptor(sub, order):
    """The subspace's descriptor with its T blocks in block order ``order`` (vec_swizzle bits 16-19)."""
    d = _lib.Subspace.from_buffer_copy(sub._c())
    assert d.vec_swizzle == (6 | (4 << 8))
    d.vec_swizzle = int(d.vec_swizzle) | (order << 16)
    return d


def handle(arrs, d, rank, nranks, flags=0):
    config._initialize()
    h = backend.create_mat(*arrs, d, d, flags=flags, rank=rank, nranks=nranks)
    return backend.ShellMat(h, d, d, nranks, rank)


def positions(d, idx, part=None):
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    out = np.empty_like(idx)
    _lib.check(_lib.lib().dnm_vec_layout_positions_host(C.byref(d), C.byref(part) if part is not None else None, idx.size,
                                                        _lib.p64(idx), _lib.p64(out)))
    return out


class Shares:
    """The shares of P ranks of a descriptor's layout, from the whole-vector position map and the partition alone."""

    def __init__(self, sub, d, P):
        N = sub.get_dimension()
        self.gpos = positions(d, np.arange(N))
        self.parts = [backend.layout_partition(d, P, r) for r in range(P)]
        self.rows = [np.flatnonzero((self.gpos >= p[0]) & (self.gpos < p[0] + p[1])) for p in self.parts]
        assert [r.size for r in self.rows] == [p[3] for p in self.parts]
        assert np.array_equal(np.sort(np.concatenate(self.rows)), np.arange(N))       # disjoint, all of the subspace
        _, ib = backend.layout_blocks(d)
        # per rank: its blocks in the order they lie in memory, each as (first, last) reference index -- a block of
        # equal top bits is a range of the reference order
        self.blocks = []
        for p in self.parts:
            mine = []
            for j in np.flatnonzero((ib[:-1] >= p[0]) & (ib[:-1] < p[0] + p[1])):
                br = np.flatnonzero((self.gpos >= ib[j]) & (self.gpos < ib[j + 1]))
                assert br.size and br[-1] - br[0] + 1 == br.size and ib[j + 1] <= p[0] + p[1]
                mine.append((int(br[0]), int(br[-1])))
            self.blocks.append(mine)

    def present_code_could_pass(self, s):
        """Block order 1: does some rank r > 0 get its right answer from the reference rows [0, nlen_r) or
        [-1, nlen_r - 1) -- what a sweep of [row0, row0 + rows_local) with sc3_range's nstart looks at?"""
        for r in range(1, len(self.parts)):
            nlen = self.parts[r][3]
            if s[self.rows[r]].max() in (s[:nlen].max(), s[:nlen - 1].max()):
                return True
        return False


def tiled_operator(L, rstar, scale):
    """A chain of pair hops (element 1/2) and ZZ couplings plus ``scale`` times the planted fields: two tiled passes.
    With scale = 2^(L+3) the planted row keeps the largest row sum: the fields separate it from every other row by at
    least 2^(1-L) scale = 16, hops and couplings move a row sum by less than (L-1) (1/2 + 1/4) < 12."""
    from dynamite_amd.operators import sigmax, sigmay, sigmaz, op_sum
    hop = lambda i, j: sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j)
    H = op_sum(0.25 * hop(i, i + 1) + 2.0 ** -(2 + i % 4) * sigmaz(i) * sigmaz(i + 1) for i in range(L - 1))
    return ref.marshal(H + scale * ref.planted_fields(L, rstar), L)


def norm_operators(L, rstar):
    """(name, arrays, create flags, tiled?): the planted operators on the row kernel (their single-spin flips leave the
    subspace, what is left is a chain: DNM_SC3_TILED=0 keeps it off the tiled passes) and the tiled handle in complex
    and in real arithmetic (what the solver runs by default)."""
    t = tiled_operator(L, rstar, 2.0 ** (L + 3))
    return [('A', ref.planted_operator(L, rstar, 'A'), 0, False), ('B', ref.planted_operator(L, rstar, 'B'), 0, False),
            ('tiled', t, 0, True), ('tiled real', t, _lib.MAT_REAL_PACKED, True)]


def planted_rows(sub, sh, order):
    """Where the planted row goes: the first and the last state of the first and of the last block of every rank's share.
    In block order 1 the case must be able to fail (Shares.present_code_could_pass): where a block does not qualify
    -- an early block of the reference order lies inside the rows the old sweep looked at anyway -- the next block of
    the share from that end takes its place."""
    out = []
    for q, blocks in enumerate(sh.blocks):
        for seq in (blocks, blocks[::-1]):
            for end in (0, 1):
                for b in seq:
                    if order == 0:
                        break
                    s = ref.row_sums(ref.planted_operator(sub.L, int(sub.idx_to_state(b[end])), 'A'), sub, sub)
                    if not sh.present_code_could_pass(s):
                        break
                else:
                    raise AssertionError("no block of rank %d's share can show a wrong sweep" % q)
                out.append((q, b[end]))
    return sorted(set(out))


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("P", RANKS)
@pytest.mark.parametrize("L,k", SHAPES)
def test_norm_of_a_share_planted(small_layout, monkeypatch, L, k, P, order):
    """Every rank's handle returns the maximum row sum over ITS rows, exactly (4 ulp where variant B's element goes
    through hypot), and the largest of them is the planted row's.  In block order 1 every placement is one where, for
    every rank beyond the first, that value differs from the maxima over the reference rows [0, nlen_r) and
    [0, nlen_r - 1): a sweep that takes the share for a range of the reference order cannot pass."""
    sub = SpinConserve(L, k)
    d = descriptor(sub, order)
    sh = Shares(sub, d, P)
    places = planted_rows(sub, sh, order)
    assert {q for q, _ in places} == set(range(P)) and len(places) >= 2 * P
    for q, index in places:
        rstar = int(sub.idx_to_state(index))
        for name, arrs, flags, tiled in norm_operators(L, rstar):
            s = ref.row_sums(arrs, sub, sub)
            assert np.flatnonzero(s == s.max()).tolist() == [index] and index in sh.rows[q]
            if order == 1:
                assert not sh.present_code_could_pass(s), (name, q, index)
            got = []
            monkeypatch.setenv("DNM_SC3_TILED", "1" if tiled else "0")
            for r in range(P):
                mat = handle(arrs, d, r, P, flags)           # (a fresh handle: the norm is cached in it)
                assert ("two-pass" in mat.describe()) == tiled and mat.real_packed == bool(flags)
                got.append(norm_of(mat))
                mat.destroy()
                want = s[sh.rows[r]].max()
                print((L, k), P, order, name, (q, index), r, repr(got[-1]), repr(want))
                if name == 'B':
                    assert abs(got[-1] - want) <= 4 * 2.0 ** -52 * want, (name, q, index, r)
                else:
                    assert got[-1] == want, (name, q, index, r)
            assert int(np.argmax(got)) == q and sorted(got)[-2] < got[q]
            if name != 'B':
                assert max(got) == s.max()


def chain_with_fields(L):
    """The chain of ``tiled_operator`` with unscaled fields: a tiled handle with a diagonal, all coefficients <= 1."""
    return tiled_operator(L, 0x2b67 & ((1 << L) - 1), 1.0)


@pytest.mark.parametrize("P", RANKS)
@pytest.mark.parametrize("L,k", SHAPES)
def test_cached_diagonal_of_a_share(small_layout, monkeypatch, L, k, P):
    """Block order 0, rank r of P, the diagonal cached (DNM_SC3_DIAG=c): handed out in reference order it is the
    reference's rows [nstart, nstart + nlen), exactly; and the window multiply that reads it is within the usual bar
    of the oracle's rows."""
    monkeypatch.setenv("DNM_SC3_DIAG", "c")
    sub = SpinConserve(L, k)
    d = descriptor(sub, 0)
    sh = Shares(sub, d, P)
    arrs = chain_with_fields(L)
    N = sub.get_dimension()
    x = rand_state(N, seed=10 * P + L)
    yref = orc.matvec(orc.Msc(*arrs), orc_sub(sub), orc_sub(sub), x)
    Lb = _lib.lib()
    for r in range(P):
        istart, ilen, nstart, nlen = sh.parts[r]
        assert np.array_equal(sh.rows[r], np.arange(nstart, nstart + nlen))       # order 0: a range of the reference order
        mat = handle(arrs, d, r, P)
        assert "two-pass" in mat.describe() and "diagonal cached" in mat.describe() and mat.uses_cached_diagonal()
        assert (mat.row0, mat.m_local) == (istart, ilen)
        got = diagonal_of(mat)
        assert np.array_equal(got[:nlen], ref.diagonal(arrs, sub, nstart, nlen)), r
        lo, hi = mat.column_window()
        inside = (sh.gpos >= lo) & (sh.gpos <= hi)
        xw = np.zeros(hi - lo + 1, dtype=np.complex128)              # (padding positions: zero)
        xw[sh.gpos[inside] - lo] = x[inside]
        wv, yv = vec_from(xw), vec_from(np.full(ilen, 777.0 + 0j))
        _lib.check(Lb.dnm_mat_mult_window(mat.handle, wv.ptr, lo, xw.size, yv.ptr, None))
        y = yv.local_numpy()
        lpos = positions(d, np.arange(nlen), _lib.Partition(r, P))
        assert np.array_equal(lpos + istart, sh.gpos[nstart:nstart + nlen])
        mat.destroy()
        assert np.max(np.abs(y[lpos] - yref[nstart:nstart + nlen])) <= tol_for(arrs, x), r


@pytest.mark.parametrize("P", RANKS)
def test_cached_diagonal_of_a_share_without_a_reference_side_is_refused(small_layout, monkeypatch, P):
    """Block order 1: the cached diagonal is computed row by row in reference order, and no share of P > 1 ranks is a range
    of that order -- precompute_diagonal refuses EVERY rank's handle (rank 0 too: it starts the sequence, but its blocks
    are not the first rows either), naming the block order, before anything is launched; the handle stays usable and
    keeps no diagonal.  (One rank computes: test_gpu_sc3.py::test_block_order_for_partitions_on_one_rank.)"""
    monkeypatch.setenv("DNM_SC3_DIAG", "c")
    L, k = 16, 8
    sub = SpinConserve(L, k)
    d = descriptor(sub, 1)
    arrs = chain_with_fields(L)
    for r in range(P):
        mat = handle(arrs, d, r, P)
        assert mat.uses_cached_diagonal()
        with pytest.raises(_lib.BackendError, match="block order 1"):
            mat.precompute_diagonal()
        with pytest.raises(_lib.BackendError, match="no precomputed diagonal"):
            _lib.check(_lib.lib().dnm_mat_get_diagonal(mat.handle, _lib.pf64(np.zeros(mat.m_local)), None))
        with pytest.raises(_lib.BackendError, match="block order 1"):
            positions(d, np.arange(4), _lib.Partition(r, P))
        mat.destroy()


# ---- XParity on top of a layout with empty blocks --------------------------------------------------------------------

def _chain22():
    from dynamite_amd.operators import sigmax, sigmay, sigmaz, op_sum
    hop = lambda i, j: sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j)
    H = op_sum(0.5 * hop(i, i + 1) + 2.0 ** -(i % 4) * sigmaz(i) * sigmaz(i + 1) for i in range(21))
    H.L = 22
    return H


def _graph22():
    from dynamite_amd.operators import sigmax, sigmay, sigmaz, op_sum
    hop = lambda i, j: sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j)
    H = op_sum(0.5 * hop(i, i + 1) for i in range(21)) + op_sum(0.25 * hop(i, i + 3) for i in range(0, 19, 2))
    H = H + op_sum(2.0 ** -(i % 5) * sigmaz(i) * sigmaz(i + 1) for i in range(21))
    H.L = 22
    return H


_XP = {}


def _xparity_reference(kind, sector):
    """(operator, XParity subspace, x, the oracle's reduced operator applied to x, its norm): computed once."""
    if (kind, sector) not in _XP:
        H = _chain22() if kind == 'chain' else _graph22()
        # (the chain_operator of test_gpu_row_sweeps.py and ref.window_operator, as operators)
        same = ref.window_operator(22) if kind == 'graph' else chain_operator(22)
        assert all(np.array_equal(u, v) for u, v in zip(ref.marshal(H.copy(), 22), same))
        parent = SpinConserve(22, 11)
        sub = XParity(parent, sector)
        H.reduce_msc()
        m = sub.reduce_msc(H.msc)
        masks, offs = msc_tools.get_mask_offsets(m)
        red, osub = orc.Msc(masks, offs, m['signs'], m['coeffs']), orc.xparity(orc_sub(parent))
        x = rand_state(sub.get_dimension(), seed=22 + (sector == '-'))
        _XP[(kind, sector)] = (H, sub, x, orc.matvec(red, osub, osub, x, nthreads=8),
                               orc.matvec(red, osub, osub, x.real + 0j, nthreads=8), orc.infnorm(red, osub, osub))
    return _XP[(kind, sector)]


@pytest.mark.parametrize("sector", ['+', '-'])
@pytest.mark.parametrize("kind", ['chain', 'graph'])
def test_xparity_over_a_layout_with_empty_blocks(small_layout, kind, sector):
    """XParity(SpinConserve(22, 11)) in the (6, 4) layout: t = 12 and k = 11 > a + w, so the blocks T = 0 and T = 0xfff are
    empty and the half whose top bit is clear is the PLACES [0, 2047) of the block sequence, not [0, 2048).  The handle
    and the vector agree on that half (352 716 representatives), and H.dot(x) is the oracle's reduced operator at the
    bar of the XParity tests of test_gpu_sc3_graph.py."""
    from dynamite_amd.states import State
    H, sub, x, want, _, nrm = _xparity_reference(kind, sector)
    dim = sub.parent.get_dimension()
    assert sub.get_dimension() == dim // 2 == 352716 and sub.vec_swizzle == (6 | (4 << 8))
    Hc = H.copy()
    Hc.add_subspace(sub)
    xs = State(L=22, subspace=sub)
    assert xs.vec.internal and xs.vec.half
    xs.vec.set_local_from_numpy(x)
    xs.set_initialized()
    mat = Hc.get_mat(subspaces=(sub, sub))
    assert "internal layout [T 12 | W 4 | Lo 6]" in mat.describe()
    assert (mat.M, mat.N) == (dim // 2, dim // 2)
    assert mat.m_local == mat.n_local == xs.vec.local_size == backend.layout_partition(sub.parent._c(), 2, 0)[1]
    y = Hc.dot(xs).to_numpy()
    assert np.abs(y - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), mat.describe()
    # the norm sweeps the handle's rows in reference order: dim / 2 of them, none of the other half
    assert abs(mat.norm() - nrm) <= 1e-12 * nrm
    Hc.destroy_mat()


@pytest.mark.parametrize("sector", ['+', '-'])
def test_xparity_over_a_layout_with_empty_blocks_real_arithmetic(small_layout, sector):
    """The real-symmetric chain on a real vector: the complex handle and the real-packed one (one double per position of
    the same half) against the oracle."""
    import torch
    H, sub, x, _, want, _ = _xparity_reference('chain', sector)
    Hc = H.copy()
    Hc.add_subspace(sub)
    cmat, rmat = Hc.get_mat(subspaces=(sub, sub)), Hc.get_real_packed_mat(sub)
    assert rmat is not None and rmat.real_packed and rmat.perm_left == cmat.perm_left
    assert 2 * rmat.m_local == cmat.m_local == backend.layout_partition(sub.parent._c(), 2, 0)[1]
    xv, yv = cmat.createVecs()
    assert xv.half and xv.local_size == cmat.n_local
    xv.set_local_from_numpy(x.real + 0j)
    cmat.mult(xv, yv)
    bar = 1e-12 * max(1.0, np.abs(want).max())
    assert np.abs(yv.local_numpy() - want).max() <= bar
    xd = xv.array.real.contiguous()
    yd = torch.full_like(xd, 3.0)
    _lib.check(_lib.lib().dnm_mat_mult(rmat.handle, C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr()), None))
    torch.cuda.synchronize()
    out = backend.Vec(sub.get_dimension(), swz=cmat.swz_left, sub_c=cmat._keep[0])
    torch.view_as_real(out.array)[:, 0] = yd
    assert np.abs(out.local_numpy() - want).max() <= bar, rmat.describe()
    Hc.destroy_mat()
