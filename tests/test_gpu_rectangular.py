"""Operators whose left and right subspaces differ, on the one-thread-per-row "gather" kernels that serve them:
gather_matvec_kernel<LT, RT>, norm_kernel<LT, RT>, conserves_kernel<LT, RT> (csrc/matvec_kernels.hip) and the fused twin
gather_matvec_fused_kernel<LT, RT> (csrc/row_fused_kernels.hip), each instantiated for the 4 x 4 pairs of subspace types.

Seven subspaces at L = 10 -- Full, both Parity sectors, SpinConserve(10, 5) and (10, 4), a sorted Explicit list of 300
states and an unsorted one of 210 that holds states 0 and 2^L - 1 -- in all 49 ordered (left, right) pairs: every one of
the sixteen instances of each kernel runs, with a right map that has to turn away states of the wrong parity or
magnetisation and a left layout that differs from the right one (the suite's test swizzle, shift 6, permutes the Full and
Parity vectors of this size).  Every handle is built with DNM_MAT_FORCE_GATHER so that the like pairs (Full / Full,
Parity / Parity, SpinConserve(k) / SpinConserve(k)) run the same family.

The reference is the dense matrix of tests/test_rectangular_ref.py, which that file checks against the oracle without a
GPU.  Coefficients are multiples of 1/8 and amplitudes Gaussian integers, so every multiply is compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

import test_rectangular_ref as ref
from dynamite_amd import _lib, backend, models
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve
from gpu_util import marshal, mult_numpy, orc_msc, orc_sub, vec_from
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

B, CZ = 0.5, complex(0.25, -0.5)
PLANT = complex(1, 2)
OPS = ("pauli", "heisenberg")

_SUBS = {}


def sub(name):
    if name not in _SUBS:
        _SUBS[name] = ref.make_subspace(name)
    return _SUBS[name]


def handle(arrs, left, right, flags=_lib.MAT_FORCE_GATHER):
    """The native handle of (left <- right); on the row-gather kernel, whatever the pair."""
    mat = backend.build_mat(*arrs, left._to_c(), right._to_c(), flags=flags)
    assert "row-gather kernel" in mat.describe(), mat.describe()
    return mat


def planted(n, j):
    x = np.zeros(n, dtype=np.complex128)
    x[j] = PLANT
    return x


def check_sub2(mat, D, tag):
    """dnm_mat_mult_sub2 with and without z2: y = A x - b z + c z2, z and z2 in the left space, exactly"""
    x, z, z2 = ref.gauss_ints(mat.N, 5), ref.gauss_ints(mat.M, 6), ref.gauss_ints(mat.M, 7)
    xv, yv = mat.createVecs()
    xv.set_local_from_numpy(x)
    zv, z2v = vec_from(z, mat.swz_left), vec_from(z2, mat.swz_left)
    for with_z2 in (True, False):
        yv.set(777.0)
        _lib.check(_lib.lib().dnm_mat_mult_sub2(mat.handle, xv.ptr, yv.ptr, zv.ptr, B, z2v.ptr if with_z2 else None,
                                                CZ.real if with_z2 else 0.0, CZ.imag if with_z2 else 0.0,
                                                backend._stream()))
        want = D @ x - B * z + (CZ * z2 if with_z2 else 0.0)
        y = yv.local_numpy()
        bad = np.flatnonzero(y != want)
        assert bad.size == 0, (tag, with_z2, "first differing row", int(bad[0]), y[bad[0]], want[bad[0]])


@pytest.mark.parametrize("ln", ref.NAMES)
def test_product_norm_and_planted_columns(ln):
    """One left subspace against the seven right ones, both operators: the product of a vector without a zero component
    (rows without a partner must come out as exact zeros over the 777 the result vector held), single columns at both
    ends of the right subspace and at a right state the left subspace does not hold, the infinity norm, and -- the fused
    twin of the multiply, all sixteen instances over the seven calls -- the product with start vectors."""
    left = sub(ln)
    zero = []
    for opname in OPS:
        arrs, A = ref.operator_arrays(opname), ref.dense_of(opname)
        exact_norm = not ref.mixes_real_and_imaginary(arrs)
        for rn in ref.NAMES:
            D = ref.block(A, ln, rn)
            mat = handle(arrs, left, sub(rn))
            assert (mat.M, mat.N) == D.shape
            x = ref.gauss_ints(mat.N, 17)
            want = D @ x
            y = mult_numpy(mat, x)
            bad = np.flatnonzero(y != want)
            assert bad.size == 0, (opname, ln, rn, "first differing row", int(bad[0]), y[bad[0]], want[bad[0]])
            if not want.any():
                zero.append((ln, rn))
            cols = [0, mat.N - 1] + [j for j in [ref.absent_column(ln, rn)] if j is not None]
            for j in cols:
                y = mult_numpy(mat, planted(mat.N, j))
                assert np.array_equal(y, PLANT * D[:, j]), (opname, ln, rn, "column", j)
            nrm, want_nrm = mat.norm(), ref.infnorm_dense(D)
            if exact_norm:
                assert nrm == want_nrm, (opname, ln, rn, nrm, want_nrm)
            else:
                assert abs(nrm - want_nrm) <= 1e-12 * max(1.0, nrm), (opname, ln, rn, nrm, want_nrm)
            if opname == "pauli":
                assert _lib.lib().dnm_mat_fuses_init(mat.handle) == 1
                check_sub2(mat, D, (ln, rn))
            mat.destroy()
    # the Pauli sum couples every pair; Heisenberg all but the parity- and magnetisation-mismatched ones
    assert zero == [p for p in ref.HEISENBERG_ZERO_PAIRS if p[0] == ln]


# one orientation of each pair of types that differ or of two different subspaces of one type
FUSED_PAIRS = [("full", "odd"), ("expB", "full"), ("sc4", "odd"), ("even", "expB"), ("expA", "sc5"), ("expA", "expB"),
               ("sc5", "sc4")]


@pytest.mark.parametrize("row_fuse", ["1", "0"])
@pytest.mark.parametrize("ln,rn", FUSED_PAIRS)
def test_fused_start_vectors(monkeypatch, ln, rn, row_fuse):
    """dnm_mat_mult_sub2 on an unlike pair: y = A x - b z + c z2 with z and z2 in the LEFT space, exactly -- on the fused
    twin of the gather kernel and, under DNM_ROW_FUSE=0, as the plain kernel followed by two sweeps."""
    monkeypatch.setenv("DNM_ROW_FUSE", row_fuse)
    arrs, A = ref.operator_arrays("pauli"), ref.dense_of("pauli")
    D = ref.block(A, ln, rn)
    mat = handle(arrs, sub(ln), sub(rn))
    assert _lib.lib().dnm_mat_fuses_init(mat.handle) == int(row_fuse)      # (both ways to the same result are taken)
    check_sub2(mat, D, (ln, rn))
    mat.destroy()


@pytest.mark.parametrize("slice_log2", [None, "8"])
def test_check_conserves_every_pair(monkeypatch, slice_log2):
    """CheckConserves against the dense verdict -- the rows of A outside the left subspace, restricted to the columns in
    the right one, are all zero -- on the 49 pairs with both operators, and at L = 6 with the projector onto one
    configuration, which vanishes off every left subspace that holds it: every pair of types is seen with the verdict
    True, and with False wherever it can be (a Full left subspace has no rows outside it).  In one launch and in
    launches of 2^8 columns."""
    if slice_log2:
        monkeypatch.setenv("DNM_LAUNCH_SLICE_LOG2", slice_log2)
    seen = {}
    for opname in OPS:
        arrs, A = ref.operator_arrays(opname), ref.dense_of(opname)
        for ln, rn in ref.PAIRS:
            got = backend.check_conserves(*arrs, sub(ln)._to_c(), sub(rn)._to_c())
            assert got == ref.conserves_dense(A, ln, rn), (opname, ln, rn)
            seen.setdefault((ref.TYPE[ln], ref.TYPE[rn]), set()).add(got)
    arrs = ref.projector_arrays(ref.PBITS, ref.CONFIG)
    psubs = {n: ref.projector_subspace(n, "lib") for n in ref.PNAMES}
    for ln in ref.PNAMES:
        for rn in ref.PNAMES:
            got = backend.check_conserves(*arrs, psubs[ln]._to_c(), psubs[rn]._to_c())
            assert got == ref.projector_verdict(ln, rn), ("projector", ln, rn)
            seen.setdefault((ref.PTYPE[ln], ref.PTYPE[rn]), set()).add(got)
    ref.assert_verdicts_cover(seen)


@pytest.mark.parametrize("ln,rn", [("expB", "sc5"), ("odd", "full"), ("sc4", "expA")])
def test_operator_level(ln, rn):
    """Operator.add_subspace(left, right) with allow_projection: dot() and to_numpy() are the dense block."""
    from dynamite_amd.states import State
    H = ref.pauli_operator()
    left, right = sub(ln), sub(rn)
    H.allow_projection = True
    H.add_subspace(left, right)
    D = ref.block(ref.dense_of("pauli"), ln, rn)
    x = ref.gauss_ints(D.shape[1], 23)
    xs = State(L=ref.L, subspace=right)
    xs.vec.set_local_from_numpy(x)
    xs.set_initialized()
    y = H.dot(xs, result=State(L=ref.L, subspace=left))       # (the operator keeps its default pair, Full <- Full)
    assert y.subspace.identical(left)
    assert np.array_equal(y.to_numpy(), D @ x)
    assert np.array_equal(H.to_numpy(subspaces=(left, right), sparse=False), D)
    H.destroy_mat()


@pytest.mark.default_layout
def test_production_swizzle():
    """The production layout (shift 16) at L = 18, the smallest size at which it moves a Parity vector, against the
    oracle bit for bit.  long_range has coefficients that are no dyadic fractions, so the comparison is exact only where
    kernel and oracle round alike: the amplitudes are +-1, 2, 4, 8, all real in one vector and all imaginary in a second
    one.  Every product coefficient x amplitude is then exact (the kernel's fma and the oracle's multiply-then-add round
    the same sum once), the other part of the amplitude adds exact zeros, and both sum a mask's terms and a row's masks
    in ascending order."""
    L = 18
    H = models.long_range(L)
    full, sc, even, odd = Full(L=L), SpinConserve(L, 9), Parity(0, L=L), Parity(1, L=L)
    assert full.vec_swizzle == 16 and odd.vec_swizzle == 16
    arrs = marshal(H)
    for left, right in ((full, sc), (sc, odd), (even, full)):
        mat = handle(arrs, left, right)
        rs = np.random.RandomState(31)
        for unit in (1.0, 1j):
            x = rs.choice([1.0, 2.0, 4.0, 8.0], size=mat.N) * rs.choice([-1.0, 1.0], size=mat.N) * unit
            want = orc.matvec(orc_msc(H), orc_sub(left), orc_sub(right), x)
            assert want.any()
            y = mult_numpy(mat, x)
            bad = np.flatnonzero(y != want)
            assert bad.size == 0, (left, right, unit, "first differing row", int(bad[0]), y[bad[0]], want[bad[0]])
        mat.destroy()


def test_cached_diagonal_refused_between_two_subspaces():
    """Equal dimensions do not make a handle square in the sense the cached diagonal needs: between two different
    subspaces the identity mask pairs a row with the column of the SAME state, not with the column of its own index.
    dnm_mat_precompute_diagonal refuses such a handle, and its product stays the dense one.  Two Explicit objects that
    hold the same list are one subspace: accepted, and the product with the cached diagonal is exact as well."""
    arrs, A = ref.operator_arrays("pauli"), ref.dense_of("pauli")
    assert arrs[0][0] == 0
    a, b = ref.explicit_lists()
    cases = [(SpinConserve(ref.L, 4), ref.states_of("sc4"), SpinConserve(ref.L, 6), ref.states_of("sc6")),
             (Explicit(a[:210], L=ref.L), a[:210], sub("expB"), b),
             (sub("even"), ref.states_of("even"), sub("odd"), ref.states_of("odd"))]
    for left, lst, right, rst in cases:
        mat = handle(arrs, left, right)
        assert mat.M == mat.N
        D = ref.block(A, lst, rst)
        x = ref.gauss_ints(mat.N, 29)
        assert np.array_equal(mult_numpy(mat, x), D @ x), (left, right)
        with pytest.raises(_lib.BackendError, match="same subspace"):
            mat.precompute_diagonal()
        assert np.array_equal(mult_numpy(mat, x), D @ x), (left, right)
        mat.destroy()
    mat = handle(arrs, sub("expA"), Explicit(a.copy(), L=ref.L))
    mat.precompute_diagonal()
    d = np.empty(a.size)
    _lib.check(_lib.lib().dnm_mat_get_diagonal(mat.handle, d.ctypes.data_as(_lib.f64p), None))
    assert np.array_equal(d, A[a, a].real)
    x = ref.gauss_ints(a.size, 29)
    assert np.array_equal(mult_numpy(mat, x), ref.block(A, a, a) @ x)
    mat.destroy()


@pytest.mark.parametrize("row_fuse", ["1", "0"])
def test_lanczos_sums_refused_between_two_subspaces(monkeypatch, row_fuse):
    """<x, y> pairs x_i with y_i: dnm_mat_mult_lanczos and dnm_mat_mult_dot refuse Full <- SpinConserve, with the fused
    twin and without it.  (Every vector here has max(M, N) elements: no sweep over M elements of x could leave it.)"""
    monkeypatch.setenv("DNM_ROW_FUSE", row_fuse)
    arrs = ref.operator_arrays("pauli")
    mat = handle(arrs, sub("full"), sub("sc5"))
    n = max(mat.M, mat.N)
    assert mat.M > mat.N
    xv, zv, yv = backend.Vec(n, swz=mat.swz_right), backend.Vec(n, swz=mat.swz_left), backend.Vec(n, swz=mat.swz_left)
    xv.set(1.0)
    zv.set(1.0)
    d3, d2 = (C.c_double * 3)(), (C.c_double * 2)()
    lib = _lib.lib()
    for z in (zv.ptr, None):
        with pytest.raises(_lib.BackendError, match="same subspace"):
            _lib.check(lib.dnm_mat_mult_lanczos(mat.handle, xv.ptr, yv.ptr, z, 0.5 if z else 0.0, d3, backend._stream()))
    with pytest.raises(_lib.BackendError, match="same subspace"):
        _lib.check(lib.dnm_mat_mult_dot(mat.handle, xv.ptr, yv.ptr, d2, backend._stream()))
    # the handle still multiplies
    x = ref.gauss_ints(mat.N, 3)
    assert np.array_equal(mult_numpy(mat, x), ref.block(ref.dense_of("pauli"), "full", "sc5") @ x)
    mat.destroy()
