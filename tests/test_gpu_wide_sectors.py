"""The row kernels on subspaces of 33 to 63 spins and a few hundred to two thousand states, against the exact
plain-Python reference of tests/wide_ref.py (pinned to the oracle by tests/test_wide_ref.py).  Every coefficient is a
multiple of 1/8 and every amplitude a Gaussian integer in [-8, 8]: all products and partial sums are exact in double in
any order and with or without fma, so every comparison is ``np.array_equal`` / ``==`` unless it says otherwise (the one
test with random floats, at the end).  A ``1u <<``, a 32-bit popcount or an ``int`` that holds a state breaks these rows
and no others.  tests/test_wide_sectors_host.py asserts, on host-only handles, the route of every handle built here.

Which case runs which branch:
  binomial table in global memory (sc_matvec_kernel<false> and its fused twin) ... test_row_kernel / test_fused_twins
                                                                                   on sc63_61 (and sc63_62)
  mixed LDS / global staging (stage_sub) ......................................... gather-sc40_38-* of test_gather_kernel,
                                                                                   test_row_sweeps[sc40_38]
  both tables global / both in LDS ............................................... gather-sc63_61-*, gather-sc63_2-*
  unranking above bit 16, the join with the 16-bit table ......................... every sc* case (47 steps at L = 63)
  general-mask path (span up to bit 62, ffs / clz on 63-bit words) ............... the 'far' operator on every sc* case
  complemented-mask branch, c = 34 ............................................... 'far' on sc34_*, sc40_38 (no row of these
                                                                                   sectors has a partner under it: the branch
                                                                                   must drop them all), block-* cases do not
                                                                                   carry it
  sign parities over 63-bit words ................................................ every case (ZZ and fields up to site 62)
  Explicit with wide states, buckets, unsorted lists ............................. gather-exp63*, two-buckets
No reduced density matrix is computed on a wide subspace anywhere: its kernel walks 2^(L - k) configurations per row."""
import ctypes as C

import numpy as np
import pytest

import wide_ref as w
from dynamite_amd import _lib, backend
from dynamite_amd.config import config
from dynamite_amd.operators import sigmax, sigmay, op_sum
from dynamite_amd.states import State
from dynamite_amd.subspaces import Explicit, Full, SpinConserve
from oracle import oracle as orc
from gpu_util import mult_numpy, orc_msc, orc_sub, rand_state, shell, vec_from
from test_gpu_interior import EPS, heisenberg
from test_gpu_row_sweeps import chunks_of, mult_window

pytestmark = pytest.mark.gpu

B, CZ = 0.375, complex(-0.5, 0.75)      # dyadic: y = H x - B z + CZ z2 stays exact


@pytest.fixture(autouse=True)
def no_layout():
    """SpinConserve in reference order (these subspaces are too small for the internal layout anyway)."""
    old = config.sc_layout
    config.sc_layout = None
    yield
    config.sc_layout = old


def make(c, flags=0, rank=0, nranks=1):
    config._initialize()
    left, right = c.subspaces()
    lc, rc = left._c(), right._c()
    mat = backend.ShellMat(backend.create_mat(*c.arrs, lc, rc, False, flags, rank, nranks), lc, rc, nranks, rank)
    mat._subspaces = (left, right)          # (the descriptors point into their tables)
    assert (mat.swz_left, mat.swz_right) == (0, 0)
    return mat


def handle_of(monkeypatch, name):
    left, right, op, flags, knobs, route = w.HANDLES[name]
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    c = w.case(left, op, right)
    mat = make(c, flags)
    assert route in mat.describe(), mat.describe()
    x, want = w.product(left, op, right)
    return c, mat, (np.array(x), want)          # (the shared vectors are read-only; the device copy wants a writable x)


def check_multiply(mat, x, want, diagonal):
    """The plain multiply into a y that holds 777, on the fly and (diagonal) with the diagonal cached."""
    assert np.array_equal(mult_numpy(mat, x), want), mat.describe()
    if diagonal:
        mat.precompute_diagonal()
        assert np.array_equal(mult_numpy(mat, x), want), mat.describe()


class Fused:
    """x, z, z2 of a square handle on the device and the two fused entry points."""

    def __init__(self, mat, x, M):
        self.mat, self.x = mat, x
        self.z, self.z2 = w.int_vector(M, seed=11), w.int_vector(M, seed=12)
        self.xv, self.yv = mat.createVecs()
        self.xv.set_local_from_numpy(np.array(x))
        self.zv, self.z2v = vec_from(self.z), vec_from(self.z2)

    def fuses_init(self):
        return _lib.lib().dnm_mat_fuses_init(self.mat.handle)

    def sub2(self, with_z2):
        self.yv.set(777.0)
        _lib.check(_lib.lib().dnm_mat_mult_sub2(self.mat.handle, self.xv.ptr, self.yv.ptr, self.zv.ptr, B,
                                                self.z2v.ptr if with_z2 else None, CZ.real if with_z2 else 0.0,
                                                CZ.imag if with_z2 else 0.0, backend._stream()))
        return self.yv.local_numpy()

    def lanczos(self, with_z):
        self.yv.set(777.0)
        dot = (C.c_double * 3)()
        _lib.check(_lib.lib().dnm_mat_mult_lanczos(self.mat.handle, self.xv.ptr, self.yv.ptr,
                                                   self.zv.ptr if with_z else None, B if with_z else 0.0, dot,
                                                   backend._stream()))
        return self.yv.local_numpy(), np.array(dot)

    def check(self, Hx):
        """Both entry points with and without their optional vectors; exact."""
        for with_z2 in (True, False):
            want = Hx - B * self.z + (CZ * self.z2 if with_z2 else 0.0)
            assert np.array_equal(self.sub2(with_z2), want), (with_z2, self.mat.describe())
        for with_z in (True, False):
            want = Hx - (B * self.z if with_z else 0.0)
            y, dot = self.lanczos(with_z)
            assert np.array_equal(y, want), (with_z, self.mat.describe())
            assert np.array_equal(dot, w.fused_sums(self.x, want)), (with_z, dot, self.mat.describe())


# ---- 1. the SpinConserve row kernel ----------------------------------------------------------------------------------

@pytest.mark.parametrize("op", ['chain', 'dm', 'far'])
@pytest.mark.parametrize("s", w.SC_NAMES)
def test_row_kernel(monkeypatch, s, op):
    """One row per thread.  sc63_61 and sc63_62 are the instances whose binomial table (3968 and 4032 entries) stays
    in global memory: sc_matvec_kernel<IN_LDS = false>; all others stage it in LDS."""
    c, mat, (x, want) = handle_of(monkeypatch, 'rows-%s-%s' % (s, op))
    assert ((w.SC[s][1] + 1) * (w.SC[s][0] + 1) > 2048) == (s in w.GLOBAL_TABLE)
    check_multiply(mat, x, want, diagonal=True)
    mat.destroy()


# ---- 2. its fused twins ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fuse", ['fused', 'unfused'])
@pytest.mark.parametrize("s", w.FUSED_SUBS)
def test_fused_twins(monkeypatch, s, fuse):
    """dnm_mat_mult_sub2 (z, z2) and dnm_mat_mult_lanczos (three sums) on the fused row kernel (sc63_61: its
    global-table instance) and, under DNM_ROW_FUSE=0, as the plain kernel followed by sweeps."""
    c, mat, (x, Hx) = handle_of(monkeypatch, ('rows-%s-dm' if fuse == 'fused' else 'unfused-%s-dm') % s)
    f = Fused(mat, x, c.M)
    assert f.fuses_init() == (1 if fuse == 'fused' else 0)
    f.check(Hx)
    mat.precompute_diagonal()
    f.check(Hx)
    mat.destroy()


# ---- 3. the gather kernel --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(n for n in w.HANDLES if n.startswith('gather-')))
def test_gather_kernel(monkeypatch, name):
    """DNM_MAT_FORCE_GATHER on SpinConserve pairs (sc40_38: the left table in LDS, the right one global; sc63_61: both
    global; sc63_2: both in LDS), Explicit lists with states up to bit 62 (sorted, unsorted -- through rmap_indices --
    and with DNM_BUCKET_BITS=1, two buckets), and the rectangular pair SpinConserve(40, 2) / the same states plus
    outsiders, both ways: rows whose partner is not in the right subspace contribute nothing."""
    c, mat, (x, want) = handle_of(monkeypatch, name)
    square = c.left == c.right
    assert (mat.M, mat.N) == (c.M, c.N)
    check_multiply(mat, x, want, diagonal=square)
    if square:
        Fused(mat, x, c.M).check(want)
    mat.destroy()


# ---- 4. the sweeps that reduce over rows or columns ------------------------------------------------------------------

def norm_of(mat):
    v = C.c_double()
    _lib.check(_lib.lib().dnm_mat_norm_inf(mat.handle, C.byref(v), None))
    return v.value


def gpu_conserves(c):
    left, right = c.subspaces()
    return backend.check_conserves(*c.arrs, left._to_c(), right._to_c())


@pytest.mark.parametrize("s", w.SWEEP_SUBS)
def test_row_sweeps(s):
    """dnm_mat_norm_inf, dnm_mat_get_diagonal and dnm_check_conserves; exact (every complex element of 'dm' is a
    (3, 4) multiple: its modulus is exact whether it is taken by sqrt or by hypot)."""
    for op in ('dm', 'farx' if s.startswith('exp') else 'far'):
        c = w.case(s, op)
        mat = make(c)
        assert norm_of(mat) == w.infnorm(c), (s, op)
        mat.precompute_diagonal()
        d = np.full(c.M, np.nan)
        _lib.check(_lib.lib().dnm_mat_get_diagonal(mat.handle, _lib.pf64(d), None))
        assert np.array_equal(d, w.diagonal(c)), (s, op)
        mat.destroy()
        assert gpu_conserves(c) is w.conserves(c)[0], (s, op)
    plain, broken = w.case(s, 'chain'), w.case(s, 'chain', extra='xtop')      # xtop: sigma-x on site L - 1 (62 at L = 63)
    if s.startswith('sc'):
        assert w.conserves(plain)[0] is True
    assert w.conserves(broken)[0] is False
    assert gpu_conserves(plain) is w.conserves(plain)[0]
    assert gpu_conserves(broken) is False


def test_row_sweeps_rectangular():
    for left, right in (w.RECT, w.RECT[::-1]):
        for op in ('chain', 'dm', 'far'):
            c = w.case(left, op, right)
            mat = make(c)
            assert norm_of(mat) == w.infnorm(c), (left, op)
            mat.destroy()
            assert gpu_conserves(c) is w.conserves(c)[0], (left, op)
    # the outsiders are columns that leave SpinConserve(40, 2); the other way round every column stays
    assert w.conserves(w.case(w.RECT[0], 'chain', w.RECT[1]))[0] is False
    assert w.conserves(w.case(w.RECT[1], 'chain', w.RECT[0]))[0] is True


# ---- 5. a partitioned share ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", ['sc63_2', 'sc50_2'])
def test_partitioned_share(s):
    """Three ranks in one process: each rank's column window and one-byte-per-column map from the colrange sweep of the
    row kernel are exactly the columns the reference says its rows reach (the general masks of 'far' reach columns
    whose element is zero: reached, not needed), and the windowed multiply gives the reference's rows -- also with NaN
    at every column that is not marked."""
    P = 3
    c = w.case(s, 'far')
    x, want = w.product(s, 'far')
    for r in range(P):
        mat = make(c, rank=r, nranks=P)
        assert w.ROWS in mat.describe()
        row0, m = backend.split_ownership(c.M, P, r)
        assert (mat.row0, mat.m_local) == (row0, m)
        reach, need = w.column_sets(c, row0, m)
        lo, hi = mat.column_window()
        assert (lo, hi) == (reach[0], reach[-1]), (r, lo, hi)
        cmap = chunks_of(mat, 0)
        assert np.array_equal(lo + np.flatnonzero(cmap), np.array(reach)), r
        xw = np.array(x[lo:hi + 1])
        assert np.array_equal(mult_window(mat, xw, lo, m), want[row0:row0 + m]), r
        xw[cmap == 0] = complex(np.nan, np.nan)
        assert np.array_equal(mult_window(mat, xw, lo, m), want[row0:row0 + m]), r
        mat.precompute_diagonal()
        assert np.array_equal(mult_window(mat, xw, lo, m), want[row0:row0 + m]), r
        mat.destroy()


# ---- 6. the block kernel, at the one width where its grid is affordable ------------------------------------------------

@pytest.mark.parametrize("name", sorted(n for n in w.HANDLES if n.startswith('block-')))
def test_block_kernel(monkeypatch, name):
    """DNM_SC_BLOCK=13 at L = 34: 2^21 high parts, of which the 232 with at most two set bits (sc34_2) or at least 19
    (sc34_32) hold rows.  34 masks: within the block kernel's 64."""
    c, mat, (x, want) = handle_of(monkeypatch, name)
    assert c.nmasks <= 64
    check_multiply(mat, x, want, diagonal=True)
    Fused(mat, x, c.M).check(want)
    mat.destroy()


# ---- 7. end to end, with random floats -------------------------------------------------------------------------------

def test_two_free_fermions_on_63_sites():
    """0.25 sum (XX + YY) on SpinConserve(63, 2) is two free fermions hopping with amplitude 0.5: the lowest energy is
    the sum of the two lowest levels of the 63 x 63 hopping matrix.  Tolerance: the solver's tol times |H|_inf.
    evolve keeps the norm to the bar of smoke()."""
    L, tol = 63, 1e-9
    sub = SpinConserve(L, 2)
    H = op_sum(0.25 * (sigmax(i) * sigmax(i + 1) + sigmay(i) * sigmay(i + 1)) for i in range(L - 1))
    H.L = L
    H.add_subspace(sub)
    T = np.zeros((L, L))
    for i in range(L - 1):
        T[i, i + 1] = T[i + 1, i] = 0.5
    levels = np.linalg.eigvalsh(T)
    ev = H.eigsolve(nev=1, tol=tol, subspace=sub)
    norm = H.infinity_norm(subspaces=(sub, sub))
    print("E0 = %.12f, free fermions %.12f, |H|_inf = %g" % (ev[0], levels[0] + levels[1], norm))
    assert norm == 2.0                      # two magnons apart from each other and from the ends: four hops of 0.5
    assert abs(ev[0] - (levels[0] + levels[1])) <= tol * norm
    psi = State(L=L, subspace=sub, state='random', seed=3)
    out = H.evolve(psi, t=0.5)
    print("|exp(-iHt) psi| - 1 = %.2e" % (out.norm() - 1))
    assert abs(out.norm() - 1) < 1e-9


@pytest.mark.parametrize("route", ['rows', 'fused', 'gather'])
def test_random_complex_state_against_the_oracle(route):
    """Non-dyadic coefficients (the random-field Heisenberg chain of tests/test_gpu_interior.py at L = 63) and a random
    complex state on SpinConserve(63, 2), one per route of parts 1 to 3, against oracle.matvec; the suite's bar for that
    comparison: number of masks * eps * 100, relative."""
    L = 63
    H = heisenberg(L)
    sub = SpinConserve(L, 2)
    mat = shell(H, sub, flags=_lib.MAT_FORCE_GATHER if route == 'gather' else 0)
    assert (w.GATHER if route == 'gather' else w.ROWS) in mat.describe(), mat.describe()
    n = sub.get_dimension()
    x = rand_state(n, seed=63)
    want = orc.matvec(orc_msc(H), orc_sub(sub), orc_sub(sub), x)
    bar = len(np.unique(H.msc['masks'])) * EPS * 100
    if route == 'fused':
        z, z2 = rand_state(n, seed=64), rand_state(n, seed=65)
        xv, yv = mat.createVecs()
        xv.set_local_from_numpy(x)
        zv, z2v = vec_from(z), vec_from(z2)
        yv.set(777.0)
        assert _lib.lib().dnm_mat_fuses_init(mat.handle) == 1
        _lib.check(_lib.lib().dnm_mat_mult_sub2(mat.handle, xv.ptr, yv.ptr, zv.ptr, 0.37, z2v.ptr, -0.4, 0.9,
                                                backend._stream()))
        got, want = yv.local_numpy(), want - 0.37 * z + complex(-0.4, 0.9) * z2
    else:
        got = mult_numpy(mat, x)
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print("%s: %.2e of %.2e" % (route, err, bar))
    assert err <= bar
    mat.destroy()


# ---- the dense reduced density matrix refuses what it could not finish -------------------------------------------------

def test_dense_rdm_refuses_wide_subspaces_and_serves_the_others():
    """dnm_reduced_density_matrix walks 2^(L - k) traced configurations per kept one, whatever the dimension: more than
    40 spins are refused (before any launch: the refusal is all that is tested on a wide subspace); Full(12) is served."""
    from dynamite_amd.computations import reduced_density_matrix
    for sub in (SpinConserve(63, 2), Explicit(np.array([3, 1 << 20, 1 << 40], dtype=np.int64), L=41)):
        psi = State(L=sub.L, subspace=sub, state='random', seed=1)
        with pytest.raises((ValueError, _lib.BackendError), match="traced configurations"):
            reduced_density_matrix(psi, [0, 1, 5])
    sub = Full(L=12)
    psi = State(L=12, subspace=sub, state='random', seed=2)
    rho = reduced_density_matrix(psi, [0, 1, 5])
    want = orc.rdm(orc.full(12), psi.to_numpy(), [0, 1, 5])
    assert np.max(np.abs(rho - want)) <= 1e-14
