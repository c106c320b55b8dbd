"""
A state moved between subspaces on the device and its weights per sector (csrc/submap_kernels.hip, csrc/submap_rank.h,
csrc/observables.cpp: dnm_subspace_map_apply, dnm_sector_weights; backend.subspace_map / sector_weights;
computations.to_subspace / sector_weights).

The reference is tests/submap_ref.py: numpy on the host, from idx_to_state and state_to_idx and the table of the four
(source, target) cases, with the operations of the table in their order.  Amplitudes are Gaussian integers with
components in [-8, 8]: a copy rounds nothing, x * kappa and (a +- b) * kappa are one rounding of an exact operand on
either side, and every sum of |x|^2 or |a +- b|^2 / 2 over at most 2^14 rows is an integer or half-integer far below
2^53 -- so every comparison against the reference is ``np.array_equal``, with no tolerance.

Two bounds are not exact, with u = 2^-53.  XParity -> parent -> XParity computes ((x kappa) + (x kappa)) kappa: one
rounding for each multiply, none for the sum of two equal numbers, and kappa itself is 1 / sqrt 2 rounded once, which
enters twice: four relative errors of u, 4 u = 2^-51 <= 2^-50 per component.  ``XParity.convert_state`` divides by
np.sqrt(2) (one rounding of the root, one of the division) where the pass multiplies by kappa (one rounding of kappa,
one of the product): again four, the same bound.
"""
import ctypes as C

import numpy as np
import pytest

import submap_ref
from dynamite_amd import _lib, backend
from dynamite_amd.computations import sector_weights, sigmaz_correlations, to_subspace
from dynamite_amd.config import config
from dynamite_amd.operators import op_sum, sigmax, sigmay
from dynamite_amd.states import State
from dynamite_amd.subspaces import Auto, Explicit, Full, Parity, SpinConserve, XParity

pytestmark = pytest.mark.gpu

REL = 2.0 ** -50


def _desc(sub, swz=0):
    d = _lib.Subspace.from_buffer_copy(sub._c())
    d.vec_swizzle = swz
    d._keep = sub
    return d


def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_map(src, dst, x, fill=777.0):
    """dnm_subspace_map_apply on raw buffers: the target vector as it lies.  A side is (subspace, sector, swizzle)."""
    import torch
    config._initialize()
    xd = _device(x)
    y = torch.full((submap_ref.rows_of(dst),), fill, dtype=torch.complex128, device=xd.device)
    _lib.check(_lib.lib().dnm_subspace_map_apply(C.c_void_p(xd.data_ptr()), C.byref(_desc(src[0], src[2])), src[1],
                                                 C.c_void_p(y.data_ptr()), C.byref(_desc(dst[0], dst[2])), dst[1],
                                                 backend._stream()))
    return y.cpu().numpy()


def check_map(src, dst, seed=1):
    x = submap_ref.gaussian_integers(submap_ref.rows_of(src), seed)
    got = run_map(src, dst, x)
    want = submap_ref.map_apply(x, src, dst)
    assert np.array_equal(got, want), (src, dst, int(np.flatnonzero(got != want)[0]))
    return got


# ---- through the ABI with raw buffers -------------------------------------------------------------------------------
@pytest.mark.parametrize('ssec,dsec', [(0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)])
def test_spin_conserve_and_full_with_every_sector(ssec, dsec):
    """3432 rows: runs of four and workgroups of 1024 rows have ragged ends; the sectors s != t give all zeros."""
    sc, full = SpinConserve(14, 7), Full(L=14)
    up = check_map((sc, ssec, 0), (full, dsec, 0), seed=2)
    down = check_map((full, ssec, 0), (sc, dsec, 0), seed=3)
    if ssec and dsec and ssec != dsec:
        assert not up.any() and not down.any()
    else:
        assert np.count_nonzero(up) > 1500 and np.count_nonzero(down) > 1500


@pytest.mark.parametrize('s_src', [0, 5])
@pytest.mark.parametrize('s_dst', [0, 5])
def test_parity_and_full_with_independent_swizzles(s_src, s_dst):
    par, full = Parity('odd', L=13), Full(L=13)
    check_map((par, 0, s_src), (full, 0, s_dst))
    check_map((full, 0, s_src), (par, 0, s_dst))
    check_map((par, 0, s_src), (full, -1, s_dst))
    check_map((full, 1, s_src), (par, 0, s_dst))


@pytest.mark.parametrize('order', ['sorted', 'unsorted'])
def test_explicit_lists(order):
    rng = np.random.default_rng(14)
    states = rng.choice(1 << 14, size=1000, replace=False).astype(np.int64)
    ex = Explicit(np.sort(states) if order == 'sorted' else states, L=14)
    full, sc = Full(L=14), SpinConserve(14, 7)
    up = check_map((ex, 0, 0), (full, 0, 6))
    assert np.count_nonzero(up) > 900
    check_map((full, 0, 6), (ex, 0, 0))
    check_map((ex, 0, 0), (full, 1, 0))
    check_map((full, -1, 0), (ex, 0, 0))
    check_map((sc, 0, 0), (ex, 0, 0))
    check_map((ex, 0, 0), (sc, 0, 0))
    check_map((ex, 0, 0), (sc, -1, 0))
    check_map((sc, 1, 0), (ex, 0, 0))


def test_flip_closed_explicit_list_in_a_sector():
    rng = np.random.default_rng(15)
    reps = rng.choice(1 << 13, size=500, replace=False).astype(np.int64)
    ex = Explicit(np.concatenate([reps, (reps ^ ((1 << 14) - 1))[rng.permutation(500)]]), L=14)
    full = Full(L=14)
    for sec in (1, -1):
        check_map((ex, sec, 0), (full, 0, 0))
        check_map((full, 0, 0), (ex, sec, 0))
        check_map((ex, sec, 0), (full, sec, 5))
        check_map((ex, 0, 0), (ex, sec, 0))
        check_map((ex, sec, 0), (ex, 0, 0))


def test_a_second_workgroup_on_the_spin_conserve_side():
    sc, full = SpinConserve(16, 8), Full(L=16)          # 12870 rows
    check_map((sc, 0, 0), (full, 0, 0))
    check_map((full, 0, 5), (sc, 0, 0))
    check_map((full, 0, 0), (sc, 1, 0))


def test_disjoint_sectors_give_zeros_and_one_row_embeds():
    out = check_map((SpinConserve(12, 5), 0, 0), (SpinConserve(12, 6), 0, 0))
    assert out.size == 924 and not out.any()
    x = np.array([3 - 5j])
    got = run_map((SpinConserve(9, 0), 0, 0), (Full(L=9), 0, 0), x)
    want = np.zeros(512, dtype=np.complex128)
    want[0] = 3 - 5j
    assert np.array_equal(got, want)
    assert np.array_equal(run_map((Full(L=9), 0, 0), (SpinConserve(9, 0), 0, 0), want), x)


def test_a_copy_keeps_every_bit():
    """Between two plain subspaces nothing is computed: signed zeros, subnormals and NaN payloads arrive as they are."""
    sc, full = SpinConserve(10, 5), Full(L=10)
    bits = np.random.default_rng(3).integers(0, 1 << 63, size=2 * 252, dtype=np.int64)
    bits[:4] = [np.int64(-1 << 63), 1, 0x7ff8000000000123, np.int64(-1 << 63) | 5]
    x = bits.view(np.complex128)
    up = run_map((sc, 0, 0), (full, 0, 0), x)
    back = run_map((full, 0, 0), (sc, 0, 0), up)
    assert np.array_equal(back.view(np.int64), bits)
    at = sc.idx_to_state(np.arange(252))
    assert np.array_equal(up[at].view(np.int64), bits)


def test_refusals_leave_the_output_untouched():
    import torch
    config._initialize()
    L = _lib.lib()
    full, sc = _desc(Full(L=10)), _desc(SpinConserve(10, 5))
    x = _device(submap_ref.gaussian_integers(1024, 1))
    y = torch.full((1024,), 777.0, dtype=torch.complex128, device=x.device)
    before = x.clone()

    def refused(rc, word):
        assert rc != 0 and word in L.dnm_last_error().decode()
        assert bool((y == 777.0).all()) and torch.equal(x, before)

    px, py = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())
    refused(L.dnm_subspace_map_apply(px, C.byref(full), 0, px, C.byref(full), 0, backend._stream()), 'same vector')
    refused(L.dnm_subspace_map_apply(px, C.byref(full), 0, py, C.byref(_desc(Full(L=9))), 0, backend._stream()), 'L=9')
    refused(L.dnm_subspace_map_apply(px, C.byref(full), 2, py, C.byref(sc), 0, backend._stream()), 'sector 2')
    refused(L.dnm_subspace_map_apply(px, C.byref(full), 0, py, C.byref(_desc(SpinConserve(10, 4))), 1, backend._stream()),
            'k = L / 2')
    refused(L.dnm_subspace_map_apply(px, C.byref(_desc(Full(L=10), 3)), 0, py, C.byref(sc), 0, backend._stream()),
            'vec_swizzle')
    refused(L.dnm_subspace_map_apply(px, C.byref(full), 0, py, C.byref(_desc(SpinConserve(10, 5), 2 | (2 << 8))), 0,
                                     backend._stream()), 'reference order')
    refused(L.dnm_subspace_map_apply(px, None, 0, py, C.byref(sc), 0, backend._stream()), 'null')


# ---- through the Python layer ---------------------------------------------------------------------------------------
def integer_state(subspace, seed):
    s = State(subspace=subspace)
    lo, hi = s.vec.getOwnershipRange()
    s.vec.set_local_from_numpy(submap_ref.gaussian_integers(subspace.get_dimension(), seed)[lo:hi])
    s.set_initialized()
    return s


def _auto(L):
    H = op_sum([sigmax(i) * sigmax(i + 1) + sigmay(i) * sigmay(i + 1) for i in range(L - 1)])
    H.L = L
    return Auto(H, 'U' * (L // 2) + 'D' * (L // 2), sort=False)


@pytest.fixture(params=['reference order', 'internal layout'])
def sc12(request):
    old = (config.sc_layout, config.sc_layout_min_dim)
    if request.param == 'internal layout':
        config.sc_layout, config.sc_layout_min_dim = (6, 4), 0
    sub = SpinConserve(12, 6)
    assert (sub.vec_swizzle >= 256) == (request.param == 'internal layout')
    yield sub
    config.sc_layout, config.sc_layout_min_dim = old


def test_round_trip_through_full_spin_conserve(sc12):
    s = integer_state(sc12, 4)
    assert s.vec.internal == (sc12.vec_swizzle >= 256)
    up = s.to_subspace(Full(L=12))
    assert type(up.subspace) is Full and up.vec.swz == Full(L=12).vec_swizzle
    want = np.zeros(4096, dtype=np.complex128)
    want[sc12.idx_to_state(np.arange(924))] = s.to_numpy()
    assert np.array_equal(up.to_numpy(), want)
    back = up.to_subspace(s.subspace)
    assert back.vec.internal == s.vec.internal
    assert np.array_equal(back.to_numpy(), s.to_numpy())
    # ... and into a result that exists
    again = State(subspace=sc12)
    assert to_subspace(up, sc12, result=again) is again and np.array_equal(again.to_numpy(), s.to_numpy())


def test_backend_takes_the_layout_from_the_vector(sc12):
    """A vector in reference order under a descriptor that names the internal layout (and back): the backend hands the
    kernel a descriptor of the layout the vector is in."""
    x = submap_ref.gaussian_integers(924, 20)
    full = Full(L=12)
    v = backend.Vec(924, swz=0)
    v.set_local_from_numpy(x)
    out = backend.Vec(4096, swz=0)
    backend.subspace_map(v, sc12._to_c(), out, full._to_c())
    want = submap_ref.map_apply(x, (sc12, 0, 0), (full, 0, 0))
    assert np.array_equal(out.array.cpu().numpy(), want)
    back = backend.Vec(924, swz=0)
    backend.subspace_map(out, full._to_c(), back, sc12._to_c())
    assert np.array_equal(back.array.cpu().numpy(), x)
    mag, flip = backend.sector_weights(v, sc12._to_c())
    want_mag, want_flip = submap_ref.sector_weights(x, (sc12, 0, 0))
    assert np.array_equal(mag, want_mag) and np.array_equal(flip, want_flip)
    with pytest.raises(ValueError, match='amplitudes'):
        backend.subspace_map(v, sc12._to_c(), backend.Vec(2048, swz=0), full._to_c())


@pytest.mark.parametrize('make', [lambda: Parity('odd', L=11), lambda: _auto(10), lambda: Explicit([5, 3, 1020, 77], L=10)],
                         ids=['parity', 'auto', 'explicit'])
def test_round_trip_through_full(make):
    sub = make()
    s = integer_state(sub, 5)
    up = s.to_subspace(Full())
    assert up.L == sub.L and up.subspace.get_dimension() == 1 << sub.L
    assert np.array_equal(np.flatnonzero(up.to_numpy()), np.sort(sub.idx_to_state(np.flatnonzero(s.to_numpy()))))
    assert np.array_equal(up.to_subspace(sub).to_numpy(), s.to_numpy())


def _close(got, want):
    g, w = got.view(np.float64), want.view(np.float64)
    return bool(np.all(np.abs(g - w) <= REL * np.abs(w)))


@pytest.mark.parametrize('sector', ['+', '-'])
@pytest.mark.parametrize('parent', [lambda: Full(L=11), lambda: Parity('even', L=12), lambda: SpinConserve(12, 6)],
                         ids=['full', 'parity', 'spin_conserve'])
def test_xparity_to_parent_and_back(parent, sector):
    xp = XParity(parent(), sector=sector)
    s = integer_state(xp, 6)
    up = s.to_subspace(xp.parent)
    x = s.to_numpy()
    assert _close(up.to_numpy(), xp.convert_state(s).to_numpy())
    assert _close(up.to_subspace(xp).to_numpy(), x)
    other = XParity(xp.parent, sector='-' if sector == '+' else '+')
    assert not up.to_subspace(other).to_numpy().any()
    assert not s.to_subspace(other).to_numpy().any()
    assert np.array_equal(s.to_subspace(XParity(xp.parent, sector=sector)).to_numpy(), x)
    # the norm survives an embedding to rounding, and the weight outside the sector is nil
    assert abs(up.norm() ** 2 - np.vdot(x, x).real) <= 8 * REL * np.vdot(x, x).real


def test_sigmaz_correlations_survive_the_embedding(sc12):
    s = integer_state(sc12, 7)
    mz, zz = sigmaz_correlations(s)
    mz_full, zz_full = sigmaz_correlations(s.to_subspace(Full(L=12)))
    assert np.array_equal(mz, mz_full) and np.array_equal(zz, zz_full)


@pytest.mark.parametrize('sector,sign', [('+', 1.0), ('-', -1.0)])
def test_global_flip_of_an_embedded_sector_state(sector, sign):
    """The workflow the pass exists for: an XParity eigenvector taken to Full, where products of site operators act."""
    s = integer_state(XParity(SpinConserve(12, 6), sector=sector), 8)
    up = s.to_subspace(Full(L=12))
    flipped = up.apply_site_operators(np.array([[0, 1], [1, 0]]))
    assert np.count_nonzero(up.to_numpy()) > 800
    assert np.array_equal(flipped.to_numpy(), sign * up.to_numpy())


def test_python_layer_refuses():
    s = integer_state(Full(L=10), 1)
    with pytest.raises(ValueError, match='spins'):
        s.to_subspace(Full(L=9))
    with pytest.raises(ValueError, match='another state'):
        to_subspace(s, Full(L=10), result=s)
    with pytest.raises(ValueError, match='target subspace'):
        to_subspace(s, SpinConserve(10, 5), result=State(subspace=SpinConserve(10, 4)))
    with pytest.raises(Exception):
        State(subspace=SpinConserve(10, 5)).to_subspace(Full(L=10))          # not initialised


# ---- sector weights -------------------------------------------------------------------------------------------------
def run_weights(side, x, flip=True):
    config._initialize()
    xd = _device(x)
    mag = np.full(side[0].L + 1, 777.0)
    fl = np.full(2, 777.0)
    _lib.check(_lib.lib().dnm_sector_weights(C.c_void_p(xd.data_ptr()), C.byref(_desc(side[0], side[2])), side[1],
                                             _lib.pf64(mag), _lib.pf64(fl) if flip else None, backend._stream()))
    return mag, (fl if flip else None)


def weight_sides():
    rng = np.random.default_rng(16)
    return {
        'full12': (Full(L=12), 0, 0),
        'full12_swizzled': (Full(L=12), 0, 5),
        'parity12': (Parity('even', L=12), 0, 6),
        'parity13_odd': (Parity('odd', L=13), 0, 0),
        'sc12_6': (SpinConserve(12, 6), 0, 0),
        'sc13_4': (SpinConserve(13, 4), 0, 0),
        'x_full11_plus': (Full(L=11), 1, 0),
        'x_full11_minus': (Full(L=11), -1, 5),
        'x_sc12_6_minus': (SpinConserve(12, 6), -1, 0),
        'explicit': (Explicit(rng.choice(1 << 12, size=3000, replace=False), L=12), 0, 0),
    }


@pytest.mark.parametrize('name', list(weight_sides()))
def test_sector_weights_against_numpy(name):
    side = weight_sides()[name]
    n = submap_ref.rows_of(side)
    want_flip = side[1] != 0 or submap_ref.carries_flip(side[0])
    planted = np.zeros(n, dtype=np.complex128)
    rows = [r for r in (0, 1, 1023, 1024, 2047, 2048, n - 1025, n - 1024, n - 2, n - 1) if 0 <= r < n]
    planted[rows] = submap_ref.gaussian_integers(len(rows), 9) + (1 + 1j)
    for x in (submap_ref.gaussian_integers(n, 8), planted):
        mag, flip = run_weights(side, x, flip=want_flip)
        want_mag, want = submap_ref.sector_weights(x, side)
        assert np.array_equal(mag, want_mag), name
        assert mag.sum() == np.sum(x.real ** 2 + x.imag ** 2)
        if want_flip:
            assert np.array_equal(flip, want), name
            assert flip.sum() == mag.sum()
        else:
            assert want is None
            with pytest.raises(_lib.BackendError, match='flip'):
                run_weights(side, x, flip=True)


def test_sector_weights_are_the_norms_the_maps_keep():
    L = 10
    s = integer_state(Full(L=L), 10)
    mag, flip = s.sector_weights()
    assert mag.shape == (L + 1,) and flip.shape == (2,)
    for k in range(L + 1):
        y = s.to_subspace(SpinConserve(L, k)).to_numpy()
        assert mag[k] == np.sum(y.real ** 2 + y.imag ** 2), k
    for m, sector in enumerate('+-'):
        y = s.to_subspace(XParity(Full(L=L), sector=sector)).to_numpy()
        assert abs(flip[m] - np.sum(y.real ** 2 + y.imag ** 2)) <= REL * flip[m]
    # where the flip is not defined the Python layer says so
    assert integer_state(SpinConserve(L, 3), 11).sector_weights()[1] is None
    assert integer_state(Explicit([1, 2, 1000], L=L), 12).sector_weights()[1] is None
    xs = integer_state(XParity(SpinConserve(L, 5), sector='-'), 13)
    mag, flip = xs.sector_weights()
    n2 = float(np.sum(np.abs(xs.to_numpy()) ** 2))
    assert flip[0] == 0.0 and flip[1] == n2 and mag[5] == n2 and mag.sum() == n2


def test_two_calls_return_the_same_bits():
    rng = np.random.default_rng(17)
    side = (Full(L=14), 0, 6)
    x = rng.standard_normal(1 << 14) + 1j * rng.standard_normal(1 << 14)
    a, b = run_weights(side, x), run_weights(side, x)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # every sum has at most n = 2^14 positive terms of three or four roundings each: (n + 4) u relative on the device
    # and as much in numpy, whatever the order
    want_mag, want_flip = submap_ref.sector_weights(x, side)
    tol = 2 * ((1 << 14) + 4) * 2.0 ** -53
    assert np.all(np.abs(a[0] - want_mag) <= tol * want_mag) and np.all(np.abs(a[1] - want_flip) <= tol * want_flip)
