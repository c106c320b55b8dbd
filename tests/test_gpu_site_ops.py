"""
Products of single-site operators on a state and the exponential of a diagonal operator on the device
(csrc/site_ops_kernels.hip, csrc/site_ops.h, csrc/site_ops.cpp: dnm_site_ops_apply, dnm_mat_expm_diagonal;
backend.site_ops_apply, backend.expm_diagonal, computations.apply_site_operators, evolve(algo='exact'),
sample(bases=...)).

The product kernel is compared bit for bit with tests/site_ops_ref.py: matrix entries from {0, +-1, +-i, +-1+-i} and
Gaussian-integer amplitudes up to 8 grow at most fourfold per site, 8 * 4^24 < 2^53, so every intermediate is an exact
integer for L <= 24 in any order.  The diagonal exponential is held element by element to 16 eps |ref| against numpy's
e^{s_re d} (cos theta + i sin theta) x, theta = s_im d, with d exact (coefficients are multiples of 1/8): two ulp each
for the device's sin and cos and one for exp are assumed, the products add about two, a margin of 2.5 on the sum of 6.
"""

import numpy as np
import pytest
import torch

import site_ops_ref as ref
from dynamite_amd import _lib, backend
from dynamite_amd.computations import apply_site_operators, basis_rotations, evolve, sample
from dynamite_amd.config import config
from dynamite_amd.operators import identity, index_sum, op_sum, sigmax, sigmay, sigmaz
from dynamite_amd.states import State
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve, XParity
from test_gpu_zz_moments import state_from

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


def _desc(L, swz):
    d = _lib.Subspace.from_buffer_copy(Full(L=L)._c())
    d.vec_swizzle = swz
    return d


def tile_bits():
    return backend.site_ops_plan(_desc(6, 0), np.broadcast_to(np.eye(2, dtype=complex), (6, 2, 2)))[0]


def device_vec(lies, swz):
    config._initialize()          # (config.device is None until then, and .to(None) leaves a tensor on the host)
    assert config.device is not None and config.device.type == 'cuda'
    return backend.Vec(lies.size, array=torch.from_numpy(np.ascontiguousarray(lies)).to(config.device), swz=swz)


def product(L, mats, x, swz, in_place):
    """The kernel on x (index order) lying in the layout swz; the result in index order."""
    pos = ref.positions(1 << L, swz)
    lies = np.empty_like(x)
    lies[pos] = x
    xv = device_vec(lies, swz)
    yv = xv if in_place else device_vec(np.full_like(lies, np.nan), swz)
    backend.site_ops_apply(xv, {'data': _desc(L, swz)}, mats, yv)
    if not in_place:
        assert np.array_equal(xv.array.cpu().numpy(), lies)         # the input is left alone
    return yv.array.cpu().numpy()[pos]


def swizzles(L):
    return [0] + [s for s in (5, 6, 12) if L > s]


# ---- the product of site operators: exact ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["1", "2", "3", "4", "5", "8", "12", "tb", "tb+1", "three-passes"])
def test_product_exact(size):
    """L in {1, 2, 3, 4, 5, 8, 12, tb, tb + 1, 4 + 2 (tb - 4) + 1} with tb read from the plan, every swizzle the size
    allows, in place and out of place, random mixes of identity, diagonal and general sites; the largest size has every
    site general, which takes three passes."""
    tb = tile_bits()
    L = {"tb": tb, "tb+1": tb + 1, "three-passes": 4 + 2 * (tb - 4) + 1}.get(size) or int(size)
    three = size == "three-passes"
    seeds = [0] if three else [0, 1, 2]
    for seed in seeds:
        classes = [2] * L if three or seed == 0 else None
        mats = ref.exact_matrices(L, 10 * L + seed, classes=classes)
        if three:
            assert backend.site_ops_plan(_desc(L, 0), mats)[1] == 3
        x = ref.gaussian_integers(1 << L, 7 * L + seed)
        want = ref.apply_product(x, mats)
        assert np.max(np.abs(want.real)) < 2.0 ** 53 and np.max(np.abs(want.imag)) < 2.0 ** 53
        for swz in swizzles(L):
            for in_place in (False, True):
                got = product(L, mats, x, swz, in_place)
                assert np.array_equal(got, want), (L, seed, swz, in_place, np.flatnonzero(got != want)[:8])


def test_free_bits_need_not_be_adjacent():
    tb = tile_bits()
    L = 4 + 2 * (tb - 4) + 1
    classes = np.zeros(L, dtype=int)
    classes[[5, 9, 17, 20]] = 2
    mats = ref.exact_matrices(L, 3, classes=classes)
    assert backend.site_ops_plan(_desc(L, 0), mats)[1] == 1
    x = ref.gaussian_integers(1 << L, 4)
    want = ref.apply_product(x, mats)
    for swz in (0, 12):
        assert np.array_equal(product(L, mats, x, swz, True), want)
    # with diagonal sites around them: some in the tile, the others a factor per tile
    classes[[0, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 18, 19]] = 1
    mats = ref.exact_matrices(L, 5, classes=classes)
    want = ref.apply_product(x, mats)
    for swz in (0, 6):
        assert np.array_equal(product(L, mats, x, swz, False), want)


def test_each_site_alone_with_a_non_symmetric_matrix():
    """M = [[1, 2], [3i, 4]] on site j alone: a transposed matrix, a swapped partner or a wrong bit shows."""
    L = tile_bits() + 1
    x = ref.gaussian_integers(1 << L, 9)
    for j in range(L):
        mats = np.broadcast_to(np.eye(2, dtype=complex), (L, 2, 2)).copy()
        mats[j] = [[1, 2], [3j, 4]]
        want = ref.apply_site(x, j, mats[j])
        for swz in (0, 6):
            got = product(L, mats, x, swz, j % 2 == 0)
            assert np.array_equal(got, want), (j, swz)


def test_union_equals_sequence_and_calls_repeat():
    L = tile_bits() + 1
    rng = np.random.default_rng(2)
    mats = ref.exact_matrices(L, 21, classes=rng.integers(1, 3, L))
    in_a = rng.integers(0, 2, L).astype(bool)
    eye = np.eye(2, dtype=complex)
    A = np.where(in_a[:, None, None], mats, eye)
    B = np.where(in_a[:, None, None], eye, mats)
    x = ref.gaussian_integers(1 << L, 22)
    for swz in (0, 6):
        both = product(L, mats, x, swz, False)
        assert np.array_equal(both, product(L, mats, x, swz, False))           # two calls: the same bits
        assert np.array_equal(product(L, B, product(L, A, x, swz, False), swz, True), both)
    # the same with amplitudes that round: two calls still return the same bits
    y = rng.normal(size=1 << L) + 1j * rng.normal(size=1 << L)
    U = basis_rotations('xyz' * L, 3 * L)[:L]
    assert product(L, U, y, 6, False).tobytes() == product(L, U, y, 6, False).tobytes()


def test_all_identity_returns_x():
    L = 9
    mats = np.broadcast_to(np.eye(2, dtype=complex), (L, 2, 2)).copy()
    x = ref.gaussian_integers(1 << L, 1) * (1 + 1e-3)
    for swz in (0, 6):
        for in_place in (False, True):
            assert product(L, mats, x, swz, in_place).tobytes() == x.tobytes()


def test_state_method_and_sites_argument():
    L = 10
    st = State(subspace=Full(L=L), state='random', seed=3)
    x = st.to_numpy()
    M = np.array([[1, 2], [3j, 4]])
    out = st.apply_site_operators(M, sites=[7])
    assert np.array_equal(st.to_numpy(), x)
    mats = np.broadcast_to(np.eye(2, dtype=complex), (L, 2, 2)).copy()
    mats[7] = M
    want = ref.apply_product(x, mats)
    assert np.max(np.abs(out.to_numpy() - want)) <= 16 * EPS * np.max(np.abs(want))
    same = apply_site_operators(st, [M, M.T], sites=[7, 2], result=st)
    assert same is st
    mats[2] = M.T
    want = ref.apply_product(x, mats)
    assert np.max(np.abs(st.to_numpy() - want)) <= 32 * EPS * np.max(np.abs(want))
    for sub, word in ((Parity('even', L=L), 'add_subspace'), (SpinConserve(L, 5), 'add_subspace'),
                      (XParity(Full(L=L), '+'), 'convert_state')):
        with pytest.raises(ValueError, match=word):
            State(subspace=sub, state='random', seed=1).apply_site_operators(M)
    with pytest.raises(ValueError, match='sites'):
        State(subspace=Full(L=L), state='random', seed=1).apply_site_operators(M, sites=[1, 1])


# ---- the exponential of a diagonal operator ---------------------------------------------------------------------------
def eighths(rng, n):
    return rng.integers(-16, 17, n) / 8.0


def diagonal_operator(L, seed, fields=True):
    """ZZ chain, all-to-all ZZ and z fields with coefficients that are multiples of 1/8."""
    rng = np.random.default_rng(seed)
    c = eighths(rng, L)
    H = op_sum(c[i] * sigmaz(i) * sigmaz(i + 1) for i in range(L - 1))
    H = H + 0.125 * op_sum(sigmaz(i) * sigmaz(j) for i in range(L) for j in range(i + 1, L))
    if fields:
        h = eighths(rng, L)
        H = H + op_sum(h[i] * sigmaz(i) for i in range(L))
    H.L = L
    return H


def expm_case(sub, H, s, x=None, in_place=False):
    """(got, want, x): backend.expm_diagonal through the handle of H on sub against numpy, in the order of the subspace."""
    H.add_subspace(sub)
    st = State(subspace=sub, state='random', seed=5)
    if x is not None:
        lo, hi = st.vec.getOwnershipRange()
        st.vec.set_local_from_numpy(x[lo:hi])
    x = st.to_numpy()
    mat = H.get_mat(subspaces=(sub, sub))
    xin = mat.vec_in(st.vec)
    yout = xin if in_place else backend.Vec(xin.size, swz=xin.swz, sub_c=xin.sub_c)
    backend.expm_diagonal(mat, xin, yout, s)
    res = State(subspace=sub)
    res._vec = yout
    res.set_initialized()
    d = np.real(H.to_numpy(subspaces=(sub, sub), sparse=True).diagonal())
    assert np.array_equal(d * 8, np.round(d * 8))
    s = complex(s)
    with np.errstate(over='ignore', invalid='ignore'):
        f = np.exp(s.real * d) * (np.cos(s.imag * d) + 1j * np.sin(s.imag * d))
        want = f * x
    return res.to_numpy(), want, x, d


def explicit12():
    rng = np.random.default_rng(5)
    states = np.unique(rng.integers(0, 1 << 12, 900, dtype=np.int64))[:500]
    rng.shuffle(states)
    return Explicit(states, L=12)


SUBSPACES = [
    pytest.param(lambda: Full(L=12), 0, False, id="full-swz0"),
    pytest.param(lambda: Full(L=12), 6, False, id="full-swz6"),
    pytest.param(lambda: Parity('even', L=12), 6, False, id="parity-even"),
    pytest.param(lambda: Parity('odd', L=12), 6, False, id="parity-odd"),
    pytest.param(lambda: SpinConserve(12, 6), 6, False, id="sc-reference"),
    pytest.param(lambda: SpinConserve(12, 6), 6, True, id="sc-internal"),
    pytest.param(explicit12, 6, False, id="explicit"),
    pytest.param(lambda: XParity(SpinConserve(12, 6), '+'), 6, False, id="xparity-sc"),
]


@pytest.mark.parametrize("make,swz,internal", SUBSPACES)
def test_expm_diagonal(make, swz, internal):
    old = (config.sc_layout, config.sc_layout_min_dim)
    config.vec_swizzle = swz
    if internal:
        config.sc_layout, config.sc_layout_min_dim = (6, 4), 0
    try:
        sub = make()
        flip_even = isinstance(sub, XParity)
        if internal:
            assert sub.vec_swizzle >= 256
        for s in (-0.7j, 0.31 + 1.3j, -0.2 + 0.05j):
            H = diagonal_operator(12, 1, fields=not flip_even)
            got, want, x, d = expm_case(sub, H, s)
            err = np.abs(got - want)
            worst = np.max(err / np.abs(want))
            print("s=%s: largest error %.2f eps |ref|" % (s, worst / EPS))
            assert np.all(err <= 16 * EPS * np.abs(want))
            # in place: the same bits
            again, _, _, _ = expm_case(sub, diagonal_operator(12, 1, fields=not flip_even), s, x=x, in_place=True)
            assert again.tobytes() == got.tobytes()
        # s = 0 returns x bit for bit
        got, _, x, _ = expm_case(sub, diagonal_operator(12, 1, fields=not flip_even), 0.0)
        assert got.tobytes() == x.tobytes()
        # rows with x = 0 stay exactly 0, also where exp overflows
        H = diagonal_operator(12, 1, fields=not flip_even)
        H.add_subspace(sub)
        d = np.real(H.to_numpy(subspaces=(sub, sub), sparse=True).diagonal())
        s_re = 800.0 / np.max(d)
        x = State(subspace=sub, state='random', seed=6).to_numpy()
        x[s_re * d > 600.0] = 0
        x[::3] = 0
        assert np.any(s_re * d > 710.0)
        got, want, _, _ = expm_case(sub, H, s_re, x=x)
        assert np.all(np.isfinite(got.view(float)))
        assert np.all(got[x == 0] == 0)
        live = x != 0
        assert np.all(np.abs(got - want)[live] <= 16 * EPS * np.abs(want)[live])
    finally:
        config.sc_layout, config.sc_layout_min_dim = old


def test_expm_diagonal_refusals():
    L = 20
    sub = Full(L=L)
    heis = index_sum(op_sum(0.25 * s(0) * s(1) for s in (sigmax, sigmay, sigmaz)), size=L)
    heis.add_subspace(sub)
    v = backend.Vec(1 << L, swz=sub.vec_swizzle)
    with pytest.raises(_lib.BackendError, match="operator is not diagonal"):
        backend.expm_diagonal(heis.get_mat(subspaces=(sub, sub)), v, v, 1j)
    zz = index_sum(sigmaz(0) * sigmaz(1), size=L)
    zz.add_subspace(sub)
    packed = zz.get_real_packed_mat(sub)
    assert packed is not None
    rc = _lib.lib().dnm_mat_expm_diagonal(packed.handle, v.ptr, v.ptr, 0.0, 1.0, None)
    assert rc != 0 and "real-packed" in _lib.lib().dnm_last_error().decode()


# ---- evolve(algo='exact') ---------------------------------------------------------------------------------------------
def dense_evolve(H, sub, t, x):
    w, V = np.linalg.eigh(H.to_numpy(subspaces=(sub, sub), sparse=False))
    return (V * np.exp(-1j * complex(t) * w)) @ (V.conj().T @ x), np.max(np.abs(w))


def field_operator(L, seed):
    rng = np.random.default_rng(seed)
    f = rng.normal(size=(L, 3))
    H = op_sum(f[j, 0] * sigmax(j) + f[j, 1] * sigmay(j) + f[j, 2] * sigmaz(j) for j in range(L)) + 0.3 * identity()
    H.L = L
    return H


@pytest.mark.parametrize("L,t", [(8, 0.83), (9, -1.9), (10, 0.4 - 0.25j), (9, 0.2 + 0.1j)], ids=str)
def test_evolve_exact_site_dependent_field(L, t):
    """All three components on every site, real and complex t; allowed error 64 eps L e^{|Im t| ||H||} of the norm."""
    sub = Full(L=L)
    H = field_operator(L, L)
    H.add_subspace(sub)
    st = State(subspace=sub, state='random', seed=L)
    x = st.to_numpy()
    out = evolve(H, st, t, algo='exact')
    assert evolve.last_stats['matvecs'] == 0 and evolve.last_stats['its'] == 0 and evolve.last_stats['err_est'] == 0.0
    assert evolve.last_stats['reason'] > 0
    want, nrm = dense_evolve(H, sub, t, x)
    err = np.linalg.norm(out.to_numpy() - want)
    bound = 64 * EPS * L * np.exp(abs(complex(t).imag) * nrm) * np.linalg.norm(x)
    print("L=%d t=%s: error %.3e, bound %.3e" % (L, t, err, bound))
    assert err <= bound
    assert np.array_equal(st.to_numpy(), x)
    # in place
    evolve(H, st, t, result=st, algo='exact')
    assert st.to_numpy().tobytes() == out.to_numpy().tobytes()


@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=10), id="full"),
                                  pytest.param(lambda: SpinConserve(10, 5), id="sc"),
                                  pytest.param(lambda: XParity(Full(L=10), '-'), id="xparity")])
def test_evolve_exact_diagonal(make):
    L = 10
    sub = make()
    # (a sigma-z field anticommutes with the global flip: the XParity sector gets the flip-even part alone)
    H = diagonal_operator(L, 4, fields=not isinstance(sub, XParity))
    H.add_subspace(sub)
    st = State(subspace=sub, state='random', seed=2)
    x = st.to_numpy()
    for t in (1.7, 0.3 - 0.05j):
        out = evolve(H, st, t, algo='exact')
        assert evolve.last_stats['matvecs'] == 0
        want, nrm = dense_evolve(H, sub, t, x)
        err = np.linalg.norm(out.to_numpy() - want)
        bound = 64 * EPS * L * np.exp(abs(complex(t).imag) * nrm) * np.linalg.norm(x)
        print("%r t=%s: error %.3e, bound %.3e" % (sub, t, err, bound))
        assert err <= bound


def test_kicked_ising_cycles():
    L, T, theta, cycles = 9, 0.8, np.pi / 2 - 0.1, 5
    sub = Full(L=L)
    D = diagonal_operator(L, 9)
    X = index_sum(sigmax(0), size=L)
    X.L = L
    X.add_subspace(sub)
    D.add_subspace(sub)
    st = State(subspace=sub, state='random', seed=4)
    want = st.to_numpy()
    nrm = 0.0
    for _ in range(cycles):
        want, n1 = dense_evolve(X, sub, theta, want)
        want, n2 = dense_evolve(D, sub, T, want)
        nrm = n1 + n2
    for _ in range(cycles):
        evolve(X, st, theta, result=st, algo='exact')
        evolve(D, st, T, result=st, algo='exact')
        assert evolve.last_stats['matvecs'] == 0
    err = np.linalg.norm(st.to_numpy() - want)
    bound = 2 * cycles * 64 * EPS * L * np.linalg.norm(want)
    print("kicked Ising, %d cycles (||H|| T about %.1f): error %.3e, bound %.3e" % (cycles, nrm, err, bound))
    assert err <= bound


def test_evolve_exact_refusals():
    L = 8
    heis = index_sum(op_sum(0.25 * s(0) * s(1) for s in (sigmax, sigmay, sigmaz)), size=L)
    st = State(subspace=Full(L=L), state='random', seed=1)
    heis.add_subspace(st.subspace)
    with pytest.raises(ValueError, match="diagonal.*single-site"):
        evolve(heis, st, 0.5, algo='exact')
    sc = SpinConserve(L, 4)
    X = index_sum(sigmax(0), size=L)
    X.add_subspace(st.subspace)
    X.add_subspace(sc)
    with pytest.raises(ValueError, match="Full"):
        evolve(X, State(subspace=sc, state='random', seed=1), 0.5, algo='exact')
    with pytest.raises(ValueError, match="algo must be"):
        evolve(X, st, 0.5, algo='exactly')


# ---- sampling in another basis ----------------------------------------------------------------------------------------
def test_sample_z_is_todays_path():
    st = State(subspace=Full(L=10), state='random', seed=8)
    a = sample(st, 300, seed=11)
    assert np.array_equal(sample(st, 300, seed=11, bases='z'), a)
    assert np.array_equal(st.sample(300, seed=11, bases='z' * 10), a)
    assert np.array_equal(st.sample(300, seed=11, bases=None), a)


@pytest.mark.parametrize("bases", ['x', 'y', 'xyzzyxxyzy'])
def test_sample_in_a_basis_is_rotate_then_sample(bases):
    L = 10
    st = State(subspace=Full(L=L), state='random', seed=9)
    x = st.to_numpy()
    got = st.sample(400, seed=5, bases=bases)
    assert np.array_equal(st.to_numpy(), x)                  # a copy was rotated
    rotated = apply_site_operators(st, basis_rotations(bases, L))
    assert np.array_equal(got, rotated.sample(400, seed=5))
    own = basis_rotations(bases, L).copy()
    assert np.array_equal(st.sample(400, seed=5, bases=own), got)


def test_uniform_state_in_x_returns_only_zero():
    """x0 - x1 of equal amplitudes is exactly 0 at every site, and a row of weight zero is never returned."""
    st = State(subspace=Full(L=10))
    st.set_uniform()
    assert np.array_equal(st.sample(500, seed=3, bases='x'), np.zeros(500, dtype=np.int64))


def test_cat_state_in_x_has_even_parity():
    """(|0...0> + |1...1>) / sqrt 2: the two paths cancel exactly at the last site for every odd outcome."""
    L = 9
    amps = np.zeros(1 << L, dtype=np.complex128)
    amps[0] = amps[-1] = 1 / np.sqrt(2)
    st = state_from(Full(L=L), amps)
    shots = st.sample(600, seed=2, bases='x')
    pop = np.array([bin(int(s)).count('1') for s in shots])
    assert np.all(pop % 2 == 0) and len(set(shots.tolist())) > 20


def test_sample_spin_conserve_state_is_expanded():
    L = 10
    sub = SpinConserve(L, 5)
    st = State(subspace=sub, state='random', seed=12)
    got = st.sample(300, seed=7, bases='x')
    full = Full(L=L)
    expand = identity()
    expand.L = L
    expand.add_subspace(full, sub)
    by_hand = expand.dot(st)
    apply_site_operators(by_hand, basis_rotations('x', L), result=by_hand)
    assert np.array_equal(got, by_hand.sample(300, seed=7))


def test_sample_xparity_in_a_basis_raises():
    st = State(subspace=XParity(Full(L=8), '+'), state='random', seed=1)
    with pytest.raises(ValueError, match='convert_state'):
        st.sample(10, seed=1, bases='x')
    assert st.sample(10, seed=1, bases='z').shape == (10,)
