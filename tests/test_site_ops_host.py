"""
The host side of the site-operator product and of evolve(algo='exact') -- no GPU needed: the plan of
dnm_site_ops_plan (classes of the sites, passes, workgroups), what dnm_site_ops_plan / _apply and
dnm_mat_expm_diagonal refuse before any device call, the classification of operators (computations.
product_operator_fields), the single-site exponentials against eigh, and the rotations of the measurement bases.
"""
import ctypes as C

import numpy as np
import pytest

import site_ops_ref as ref
from dynamite_amd import _lib, backend
from dynamite_amd.computations import basis_rotations, product_operator_fields, site_exponentials
from dynamite_amd.operators import identity, index_sum, op_sum, sigmax, sigmay, sigmaz
from dynamite_amd.subspaces import Full, Parity, SpinConserve

EPS = np.finfo(float).eps


def _desc(sub, swz=0):
    d = _lib.Subspace.from_buffer_copy(sub._c())
    d.vec_swizzle = swz
    d._keep = sub
    return d


def _raw_full(L):
    d = _lib.Subspace()
    d.type, d.L = 0, L
    return d


def _mp(mats):
    mats = np.ascontiguousarray(mats, dtype=np.complex128)
    return mats, mats.view(np.float64).ctypes.data_as(C.POINTER(C.c_double))


def _message(rc):
    assert rc != 0
    msg = _lib.lib().dnm_last_error().decode()
    assert msg
    return msg


# ---- the plan -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 3, 4, 5, 12, 13, 14, 22, 30, 33])
def test_plan_partitions_the_sites(L):
    d = _desc(Full(L=L))
    for seed in range(6):
        rng = np.random.default_rng(100 * L + seed)
        classes = rng.integers(0, 3, L) if seed else np.full(L, 2)
        mats = ref.exact_matrices(L, seed, classes=classes)
        tb, npasses, site_pass, nwg, lds = backend.site_ops_plan(d, mats)
        assert tb in (12, 13)
        general = [j for j in range(L) if classes[j] == 2]
        n_hi = sum(j >= 4 for j in general)
        assert npasses == max(1, -(-n_hi // (tb - 4)))
        for j in range(L):
            if classes[j] == 0:
                assert site_pass[j] == -1
            elif classes[j] == 1:
                assert site_pass[j] == -2
            else:
                assert 0 <= site_pass[j] < npasses
                if j < 4:
                    assert site_pass[j] == 0
        for p in range(npasses):
            assert sum(1 for j in general if j >= 4 and site_pass[j] == p) <= tb - 4
        assert 1 <= nwg <= 2 ** 31 - 1 and nwg <= max(1, 1 << max(0, L - tb))
        assert lds == 16 << min(tb, L) and lds <= 160 * 1024


def test_workgroups_at_33_spins_fit_a_grid():
    d = _desc(Full(L=33))
    mats = ref.exact_matrices(33, 0, classes=[2] * 33)
    tb, npasses, _, nwg, _ = backend.site_ops_plan(d, mats)
    assert npasses == -(-29 // (tb - 4))
    assert 1 <= nwg <= 65536


def test_classes_are_decided_on_bits():
    d = _desc(Full(L=6))
    mats = np.broadcast_to(np.eye(2, dtype=complex), (6, 2, 2)).copy()
    mats[2] = [[1, 0], [0, np.nextafter(1, 2)]]   # not the identity: diagonal
    mats[3] = [[1, 1e-300], [0, 1]]               # not diagonal: general
    mats[5] = [[0, 1], [1, 0]]
    _, npasses, site_pass, _, _ = backend.site_ops_plan(d, mats)
    assert list(site_pass) == [-1, -1, -2, 0, -1, 0] and npasses == 1


def test_refusals():
    lib = _lib.lib()
    ok = _desc(Full(L=8))
    good, gp = _mp(ref.exact_matrices(8, 1))

    def plan(d, mp):
        return _message(lib.dnm_site_ops_plan(C.byref(d) if d is not None else None, mp, None, None, None, None, None))

    def apply(d, mp, x=16, y=16):
        return _message(lib.dnm_site_ops_apply(C.c_void_p(x), C.c_void_p(y), C.byref(d) if d is not None else None, mp,
                                               None))

    for call in (plan, apply):
        assert "null" in call(None, gp)
        assert "null" in call(ok, None)
        assert "Full" in call(_desc(Parity('even', L=8)), gp)
        assert "Full" in call(_desc(SpinConserve(8, 4)), gp)
        perm = np.arange(8, dtype=np.int8)
        d = _desc(Full(L=8))
        d.site_perm = perm.ctypes.data_as(C.POINTER(C.c_int8))
        assert "site_perm" in call(d, gp)
        for L in (0, 63, -1):
            big, bp = _mp(np.broadcast_to(np.eye(2, dtype=complex), (max(L, 1), 2, 2)).copy())
            assert "outside [1, 62]" in call(_raw_full(L), bp)
        for swz in (1, 4, 25, -3):
            assert "swizzle" in call(_desc(Full(L=8), swz), gp)
        for bad_value in (np.nan, np.inf, -np.inf):
            for where in ((0, 0, 0), (7, 1, 1)):
                bad = good.copy()
                bad[where] = bad_value if where[0] == 0 else 1j * bad_value
                b, bp = _mp(bad)
                assert "site %d" % where[0] in call(ok, bp) and "finite" in call(ok, bp)
    assert "null" in apply(ok, gp, x=0)
    assert "null" in apply(ok, gp, y=0)


def test_python_layer_checks_shapes():
    d = _desc(Full(L=8))
    with pytest.raises(ValueError, match='shape'):
        backend.site_ops_plan(d, np.zeros((7, 2, 2)))


def _host_handle(op, sub, flags=0):
    from dynamite_amd import msc_tools
    op.L = sub.L
    op.reduce_msc()
    masks, offs = msc_tools.get_mask_offsets(op.msc)
    return backend.create_mat(masks, offs, np.ascontiguousarray(op.msc['signs']), np.ascontiguousarray(op.msc['coeffs']),
                              sub._c(), sub._c(), False, _lib.MAT_HOST_ONLY | flags)


def test_expm_diagonal_refusals_on_the_host():
    lib = _lib.lib()
    sub = Full(L=10)
    heis = index_sum(op_sum(s(0) * s(1) for s in (sigmax, sigmay, sigmaz)), size=10)
    h = _host_handle(heis, sub)
    msg = _message(lib.dnm_mat_expm_diagonal(h, C.c_void_p(16), C.c_void_p(16), 0.0, 1.0, None))
    assert "operator is not diagonal" in msg
    lib.dnm_mat_destroy(h)
    zz = index_sum(sigmaz(0) * sigmaz(1), size=10)
    h = _host_handle(zz, sub)
    assert "null" in _message(lib.dnm_mat_expm_diagonal(h, C.c_void_p(0), C.c_void_p(16), 0.0, 1.0, None))
    assert "finite" in _message(lib.dnm_mat_expm_diagonal(h, C.c_void_p(16), C.c_void_p(16), np.nan, 1.0, None))
    assert "host-only" in _message(lib.dnm_mat_expm_diagonal(h, C.c_void_p(16), C.c_void_p(16), 0.0, 1.0, None))
    lib.dnm_mat_destroy(h)
    big = Full(L=20)
    zz = index_sum(sigmaz(0) * sigmaz(1), size=20)
    h = _host_handle(zz, big, _lib.MAT_REAL_PACKED)
    assert "real-packed" in _message(lib.dnm_mat_expm_diagonal(h, C.c_void_p(16), C.c_void_p(16), 0.0, 1.0, None))
    lib.dnm_mat_destroy(h)


# ---- classification -------------------------------------------------------------------------------------------------
def test_classification_diagonal():
    L = 8
    H = index_sum(sigmaz(0) * sigmaz(1), size=L) + 0.5 * index_sum(sigmaz(0), size=L) + 3 * identity()
    H.L = L
    kind, a, c0 = product_operator_fields(H)
    assert kind == 'diagonal' and a is None


def test_classification_single_site_and_constant():
    L = 6
    rng = np.random.default_rng(3)
    f = rng.normal(size=(L, 3))
    f[2] = 0                      # a site without a field
    f[4, 0] = f[4, 1] = 0         # a site with a sigma-z field alone
    H = op_sum(f[j, 0] * sigmax(j) + f[j, 1] * sigmay(j) + f[j, 2] * sigmaz(j) for j in range(L) if j != 2)
    H = H + 1.25 * identity()
    H.L = L
    kind, a, c0 = product_operator_fields(H)
    assert kind == 'single-site'
    assert np.array_equal(a, f.astype(complex))
    assert c0 == 1.25
    # the sigma-y sign and bit <-> site against to_numpy: h rebuilt from the fields is the operator
    paulis = [np.array([[0, 1], [1, 0]]), np.array([[0, -1j], [1j, 0]]), np.array([[1, 0], [0, -1]])]
    dense = 1.25 * np.eye(1 << L, dtype=complex)
    for j in range(L):
        hj = sum(a[j, k] * paulis[k] for k in range(3))
        mats = np.broadcast_to(np.eye(2, dtype=complex), (L, 2, 2)).copy()
        mats[j] = hj
        dense += ref.dense(mats)
    assert np.max(np.abs(H.to_numpy(sparse=False) - dense)) <= 8 * EPS * np.max(np.abs(f))


def test_classification_mixed_is_refused():
    L = 6
    heis = index_sum(op_sum(s(0) * s(1) for s in (sigmax, sigmay, sigmaz)), size=L)
    heis.L = L
    assert product_operator_fields(heis)[0] is None
    tfim = index_sum(sigmaz(0) * sigmaz(1), size=L) + 0.7 * index_sum(sigmax(0), size=L)
    tfim.L = L
    assert product_operator_fields(tfim)[0] is None
    xx = sigmax(0) * sigmax(3)
    xx.L = L
    assert product_operator_fields(xx)[0] is None
    zx = sigmaz(1) * sigmax(2)          # one-bit mask, one-bit sign, different bits
    zx.L = L
    assert product_operator_fields(zx)[0] is None


# ---- the single-site exponentials ---------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0.3, -1.7, 0.9, 0.4 - 0.3j, 1.1 + 0.9j, -2j], ids=str)
def test_site_exponentials_against_eigh(t):
    """Allowed error: 8 eps max(1, e^{|Im t| |a|}) -- one sincos, a division and the products.  The times are of order
    one: the phase t |a| is rounded once on either side, which moves exp(-i t |a|) by up to |t| |a| eps / 2, a term the
    bound does not carry (at t = 12.5 and |a| = 2.3 it alone is 14 eps)."""
    rng = np.random.default_rng(5)
    a = rng.normal(size=(12, 3))
    a[3] = 0
    a[5, :2] = 0
    a[7, 1:] = 0
    U = site_exponentials(a, t)
    paulis = [np.array([[0, 1], [1, 0]]), np.array([[0, -1j], [1j, 0]]), np.array([[1, 0], [0, -1]])]
    worst = 0.0
    for j in range(len(a)):
        h = sum(a[j, k] * paulis[k] for k in range(3))
        w, V = np.linalg.eigh(h)
        want = (V * np.exp(-1j * complex(t) * w)) @ V.conj().T
        norm_a = np.sqrt(np.sum(a[j] ** 2))
        bound = 8 * EPS * max(1.0, np.exp(abs(complex(t).imag) * norm_a))
        err = np.max(np.abs(U[j] - want))
        worst = max(worst, err / bound)
        print("t=%s site %d: error %.3e, bound %.3e" % (t, j, err, bound))
        assert err <= bound
    assert U[3].tobytes() == np.eye(2, dtype=complex).tobytes()          # |a| = 0: the exact identity
    assert U[5][0, 1] == 0 and U[5][1, 0] == 0                           # a sigma-z field alone: diagonal


def test_site_exponentials_of_an_operator_match_its_dense_exponential():
    L, t = 4, 0.37 + 0.2j
    rng = np.random.default_rng(8)
    f = rng.normal(size=(L, 3))
    H = op_sum(f[j, 0] * sigmax(j) + f[j, 1] * sigmay(j) + f[j, 2] * sigmaz(j) for j in range(L))
    H.L = L
    kind, a, c0 = product_operator_fields(H)
    U = ref.dense(site_exponentials(a, t))
    w, V = np.linalg.eigh(H.to_numpy(sparse=False))
    want = (V * np.exp(-1j * t * w)) @ V.conj().T
    assert np.max(np.abs(U - want)) <= 64 * EPS * L * np.exp(abs(t.imag) * np.max(np.abs(w)))


# ---- measurement bases ----------------------------------------------------------------------------------------------
def test_basis_rotations():
    paulis = {'x': np.array([[0, 1], [1, 0]]), 'y': np.array([[0, -1j], [1j, 0]]), 'z': np.array([[1, 0], [0, -1]])}
    for ch, P in paulis.items():
        V = basis_rotations(ch, 3)
        assert V.shape == (3, 2, 2) and np.array_equal(V[0], V[2])
        V = V[0]
        assert np.max(np.abs(V @ V.conj().T - np.eye(2))) <= 4 * EPS
        w, vec = np.linalg.eigh(P)
        plus, minus = vec[:, 1], vec[:, 0]              # eigenvalues -1, +1 in ascending order
        assert abs((V @ plus)[1]) <= 4 * EPS and abs(abs((V @ plus)[0]) - 1) <= 4 * EPS
        assert abs((V @ minus)[0]) <= 4 * EPS
        # V P V^H = sigma-z: outcome bit b is eigenvalue (-1)^b
        assert np.max(np.abs(V @ P @ V.conj().T - paulis['z'])) <= 4 * EPS
    mixed = basis_rotations('xyz', 3)
    assert np.array_equal(mixed[0], basis_rotations('x', 1)[0]) and np.array_equal(mixed[2], np.eye(2))
    own = np.array([np.eye(2), paulis['x'], basis_rotations('y', 1)[0]])
    assert np.array_equal(basis_rotations(own, 3), own)
    for bad in ('xy', 'q', np.zeros((3, 2, 2)), np.eye(2)):
        with pytest.raises(ValueError):
            basis_rotations(bad, 3)
