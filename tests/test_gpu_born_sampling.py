"""
Born sampling and the participation entropies of a state on the device (csrc/born_kernels.hip, csrc/born.h,
csrc/observables.cpp: dnm_born_block_sums / _search / _sample, dnm_vec_power_sums; backend.born_*, backend.power_sums,
computations.sample, computations.participation_entropies).

The reference is tests/born_ref.py: numpy's cumulative sum in index order and searchsorted, the clamps and the
zero-weight rule.  States with small integer amplitudes make every weight an integer <= 18 and every prefix an integer
below 2^53: kernel and reference must then agree exactly, whatever the shape of the sums.  Random states are held to
the bound of a sum of `rows` terms, 2 rows 2^-53 W, which holds for any summation order.
"""
import ctypes as C

import numpy as np
import pytest

import born_ref
from dynamite_amd import _lib, backend
from dynamite_amd.computations import participation_entropies
from dynamite_amd.config import config
from dynamite_amd.states import State
from dynamite_amd.subspaces import Full, Parity, SpinConserve, XParity
from test_gpu_zz_moments import embed, int_amplitudes, shuffled_explicit, small_layout, state_from  # noqa: F401

pytestmark = pytest.mark.gpu
R = born_ref.BLOCK_ROWS


def weights(amps):
    return amps.real ** 2 + amps.imag ** 2


def no_zero_weight(rows, w, row0=0):
    """Every test's last word: no returned row has weight zero (-1 marks a target of another block)."""
    rows = np.asarray(rows)
    hit = rows[rows >= 0] - row0
    assert np.all((hit >= 0) & (hit < len(w)))
    assert np.all(np.asarray(w)[hit] > 0)


def all_targets(W):
    """Every half-integer and every integer in [0, W]: the integers are the ties."""
    return np.arange(0, 2 * int(W) + 1) * 0.5


def natural(st):
    """(device tensor in index order, descriptor saying so) of a one-rank state."""
    d = _lib.Subspace.from_buffer_copy(st.subspace._c())
    d.vec_swizzle = 0
    d.site_perm = None
    return st.vec.local_natural().contiguous(), d


def check_search(st, amps, extra=()):
    """dnm_born_search of the state as it lies against the reference, on every tie and every half-integer."""
    w = weights(amps)
    W = w.sum()
    t = np.concatenate([all_targets(W), np.asarray(extra, dtype=np.float64)])
    rows = backend.born_search(st.vec.array, st.subspace._c(), 0, w.size, t)
    want = born_ref.search(w, t)
    assert np.array_equal(rows, want), np.flatnonzero(rows != want)[:8]
    no_zero_weight(rows, w)
    return rows


# ---- 5. exact search ----------------------------------------------------------------------------------------------
EXACT = [
    pytest.param(lambda: Full(L=11), 1 << 11, id="full11"),
    pytest.param(lambda: Full(L=14), 1 << 14, id="full14"),
    pytest.param(lambda: Parity('even', L=13), 1 << 12, id="parity13_even"),
    pytest.param(lambda: SpinConserve(12, 6), 924, id="sc12_6_ragged"),
    pytest.param(lambda: SpinConserve(14, 7), 3432, id="sc14_7"),
    pytest.param(shuffled_explicit, 1000, id="explicit40_shuffled"),
]


@pytest.mark.parametrize("make,rows", EXACT)
def test_search_integer_amplitudes(make, rows):
    sub = make()
    assert sub.get_dimension() == rows
    amps = int_amplitudes(rows, 3)
    st = state_from(sub, amps)
    assert not st.vec.internal
    check_search(st, amps)


@pytest.mark.parametrize("shift", [5, 6])
def test_search_returns_indices_not_positions(shift):
    """A swizzled vector is read as it lies; what comes back are indices."""
    config.vec_swizzle = shift          # (conftest's fixture puts the old value back)
    sub = Full(L=12)
    amps = int_amplitudes(1 << 12, 4)
    st = state_from(sub, amps)
    assert st.vec.swz == shift and int(sub._c().vec_swizzle) == shift
    idx = np.arange(1 << 12)
    assert np.any(st.vec.positions(idx) != idx)
    check_search(st, amps)


# ---- 6. zeros -----------------------------------------------------------------------------------------------------
def test_zero_runs():
    sub = Full(L=14)
    n = 1 << 14
    amps = int_amplitudes(n, 6)
    amps[:3 * R] = 0                    # the first three blocks
    amps[6 * R + 100:9 * R + 7] = 0     # a run that covers blocks 7 and 8 whole
    amps[-R:] = 0                       # the last block
    w = weights(amps)
    W = w.sum()
    first, last = np.flatnonzero(w)[[0, -1]]
    assert first >= 3 * R and last < n - R and not w[7 * R:9 * R].any()
    st = state_from(sub, amps)
    rows = check_search(st, amps, extra=[W + 0.5, W + 1, 2 * W, 1e300])
    assert rows[0] == first                         # target 0
    t = all_targets(W)
    assert np.all(rows[:t.size][t >= W] == last) and np.all(rows[-4:] == last)
    assert not np.any((rows >= 7 * R) & (rows < 9 * R))


@pytest.mark.parametrize("row", [0, 5, R - 1, R, 3 * R + 17, (1 << 13) - 1])
def test_single_row_support(row):
    sub = Full(L=13)
    amps = np.zeros(1 << 13, dtype=np.complex128)
    amps[row] = 2 - 3j
    st = state_from(sub, amps)
    rows = check_search(st, amps, extra=[14.0, 1e9])
    assert np.all(rows == row)


def test_no_weight_at_all():
    sub = Full(L=11)
    amps = np.zeros(1 << 11, dtype=np.complex128)
    st = state_from(sub, amps)
    rows = backend.born_search(st.vec.array, sub._c(), 0, 1 << 11, np.array([0.0, 0.5, 3.0]))
    assert np.array_equal(rows, [-1, -1, -1])
    no_zero_weight(rows, weights(amps))
    with pytest.raises(ValueError):
        st.sample(4, seed=1)


# ---- 7. blocks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", [(5000,), (1000, 9001), (37, 1061, 4096, 12289)])
def test_pieces(cuts):
    """The state cut into pieces at block-unaligned rows, each searched with its own first row and the weight in front
    of it: exactly one piece claims each target and the union is the single call's answer."""
    sub = Full(L=14)
    n = 1 << 14
    amps = int_amplitudes(n, 8)
    w = weights(amps)
    W = w.sum()
    st = state_from(sub, amps)
    x, d = natural(st)
    t = np.concatenate([all_targets(W), [W + 3.0]])
    whole = backend.born_search(x, d, 0, n, t)
    assert np.array_equal(whole, born_ref.search(w, t))
    edges = (0,) + tuple(cuts) + (n,)
    claimed = np.zeros(t.size, dtype=np.int64)
    union = np.full(t.size, -1, dtype=np.int64)
    for lo, hi in zip(edges[:-1], edges[1:]):
        before = float(w[:lo].sum())
        rows = backend.born_search(x[lo:hi], d, lo, hi - lo, t, before=before, final=hi == n)
        assert np.array_equal(rows, born_ref.search(w[lo:hi], t, before=before, final=hi == n, row0=lo))
        no_zero_weight(rows, w[lo:hi], row0=lo)
        claimed += rows >= 0
        union = np.where(rows >= 0, rows, union)
    assert np.array_equal(claimed, np.ones(t.size, dtype=np.int64))
    assert np.array_equal(union, whole)
    no_zero_weight(union, w)


# ---- 8. block sums ------------------------------------------------------------------------------------------------
def block_reference(w, before=0.0):
    pad = np.zeros(-(-w.size // R) * R)
    pad[:w.size] = w
    sums = pad.reshape(-1, R).sum(axis=1)
    return sums, before + np.cumsum(sums)


@pytest.mark.parametrize("make,rows", EXACT)
def test_block_sums_integer_amplitudes(make, rows):
    sub = make()
    amps = int_amplitudes(rows, 12)
    amps[R // 2:R // 2 + 40] = 0
    w = weights(amps)
    st = state_from(sub, amps)
    for before in (0.0, 77.0):
        sums, scan = backend.born_block_sums(st.vec.array, sub._c(), 0, rows, before)
        want_sums, want_scan = block_reference(w, before)
        assert np.array_equal(sums, want_sums) and np.array_equal(scan, want_scan)
    assert backend.born_plan(sub._c(), rows) == (R, sums.size, 8 * sums.size)
    no_zero_weight(backend.born_search(st.vec.array, sub._c(), 0, rows, scan, before=77.0), w)


def test_block_sums_swizzled_and_ragged_pieces():
    config.vec_swizzle = 5
    sub = Full(L=12)
    amps = int_amplitudes(1 << 12, 14)
    w = weights(amps)
    st = state_from(sub, amps)
    assert st.vec.swz == 5
    sums, scan = backend.born_block_sums(st.vec.array, sub._c(), 0, 1 << 12)
    assert np.array_equal(sums, block_reference(w)[0])
    x, d = natural(st)
    for lo, n in ((0, 1), (3, R - 1), (100, R), (1000, R + 1), (517, 3000)):
        got = backend.born_block_sums(x[lo:lo + n], d, lo, n, 5.0)
        want = block_reference(w[lo:lo + n], 5.0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    no_zero_weight(backend.born_search(x, d, 0, 1 << 12, scan), w)


def test_scan_is_non_decreasing_on_adversarial_blocks():
    """Block sums alternating between 1 and 2^-60, with blocks of no weight in between: the scan never decreases."""
    sub = Full(L=15)
    n = 1 << 15
    amps = np.zeros(n, dtype=np.complex128)
    amps[0::2 * R] = 1.0
    amps[R + 5::2 * R] = 2.0 ** -30
    amps[10 * R:14 * R] = 0
    st = state_from(sub, amps)
    sums, scan = backend.born_block_sums(st.vec.array, sub._c(), 0, n)
    want = np.zeros(n // R)
    want[0::2], want[1::2] = 1.0, 2.0 ** -60
    want[10:14] = 0.0
    assert np.array_equal(sums, want)
    assert np.all(np.diff(scan) >= 0)
    assert np.array_equal(scan, backend.born_scan(sums)) and np.array_equal(scan[10:14], np.full(4, scan[9]))
    t = np.concatenate([scan, scan[:-1] + 2.0 ** -61, [0.0, 0.5]])
    rows = backend.born_search(st.vec.array, sub._c(), 0, n, t)
    no_zero_weight(rows, weights(amps))
    assert np.all(rows >= 0)


# ---- 9. random states ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=14), id="full14"),
                                  pytest.param(lambda: SpinConserve(14, 7), id="sc14_7")])
def test_random_states(make):
    sub = make()
    rows_n = sub.get_dimension()
    st = State(subspace=sub, state='random', seed=9)
    amps = st.to_numpy().astype(np.clongdouble)
    w = amps.real ** 2 + amps.imag ** 2
    Cl = np.cumsum(w)
    W = float(Cl[-1])
    delta = 2.0 * rows_n * 2.0 ** -53 * W
    t = np.random.default_rng(1).random(4096) * W
    rows = backend.born_search(st.vec.array, sub._c(), 0, rows_n, t)
    assert np.all(rows >= 0)
    below = np.where(rows > 0, Cl[np.maximum(rows - 1, 0)], 0)
    slack_lo, slack_hi = np.max(below - t), np.max(t - Cl[rows])
    print("random state, %d rows: target outside its row's interval by at most %.3e / %.3e (bound %.3e)"
          % (rows_n, slack_lo, slack_hi, delta))
    assert np.all(below - delta <= t) and np.all(t <= Cl[rows] + delta)
    no_zero_weight(rows, w)
    assert np.array_equal(backend.born_search(st.vec.array, sub._c(), 0, rows_n, t), rows)
    scan = backend.born_block_sums(st.vec.array, sub._c(), 0, rows_n)[1]
    assert abs(scan[-1] - W) <= delta and np.all(np.diff(scan) >= 0)


# ---- 10. dnm_born_sample ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make,rows", [pytest.param(lambda: Full(L=13), 1 << 13, id="full13"),
                                       pytest.param(lambda: SpinConserve(13, 6), 1716, id="sc13_6")])
def test_sample_abi(make, rows):
    sub = make()
    amps, W = born_ref.plant_power_of_two(int_amplitudes(rows, 15))
    w = weights(amps)
    st = state_from(sub, amps)
    seed, N = 0x1234567890ABCDEF, 1 << 16
    got, flips = backend.born_sample_block(st.vec.array, sub._c(), 0, rows, seed, 0, N)
    want, want_flips = born_ref.sample(w, seed, 0, N)
    assert np.array_equal(got, want) and np.array_equal(flips, want_flips)
    no_zero_weight(got, w)
    again = backend.born_sample_block(st.vec.array, sub._c(), 0, rows, seed, 0, N)
    assert np.array_equal(again[0], got) and np.array_equal(again[1], flips)
    parts = [backend.born_sample_block(st.vec.array, sub._c(), 0, rows, seed, lo, n)
             for lo, n in ((0, 1), (1, 4999), (5000, N - 5000))]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), got)
    assert np.array_equal(np.concatenate([p[1] for p in parts]), flips)
    # shots beyond 2^32, and a null flip array
    far, far_flips = backend.born_sample_block(st.vec.array, sub._c(), 0, rows, seed, (1 << 32) - 8, 16)
    want, want_flips = born_ref.sample(w, seed, (1 << 32) - 8, 16)
    assert np.array_equal(far, want) and np.array_equal(far_flips, want_flips)
    r = np.empty(16, dtype=np.int64)
    _lib.check(_lib.lib().dnm_born_sample(C.c_void_p(st.vec.array.data_ptr()), C.byref(sub._c()), 0, rows, seed,
                                          (1 << 32) - 8, 16, _lib.p64(r), None, backend._stream()))
    assert np.array_equal(r, far)
    # another seed draws other rows
    assert not np.array_equal(backend.born_sample_block(st.vec.array, sub._c(), 0, rows, seed + 1, 0, N)[0], got)


# ---- 11. the Python layer -----------------------------------------------------------------------------------------
def popcount(a):
    return np.array([bin(int(v)).count("1") for v in a])


def test_state_sample_full():
    sub = Full(L=12)
    amps = int_amplitudes(1 << 12, 17)
    st = state_from(sub, amps)
    out = st.sample(5000, seed=3)
    assert out.dtype == np.int64 and out.shape == (5000,)
    no_zero_weight(out, weights(amps))              # (Full: the configuration is the index)
    assert np.array_equal(st.sample(5000, seed=3), out) and np.array_equal(st.sample(100, seed=3), out[:100])
    assert not np.array_equal(st.sample(5000), st.sample(5000))         # seeds from os.urandom
    assert st.sample(0, seed=3).size == 0


def test_state_sample_spin_conserve_internal_layout(small_layout):
    sub = SpinConserve(12, 6)
    amps = int_amplitudes(924, 18)
    st = state_from(sub, amps)
    assert st.vec.internal
    out = st.sample(5000, seed=4)
    assert np.all(popcount(out) == 6)
    idx = sub.state_to_idx(out)
    no_zero_weight(idx, weights(amps))
    assert np.array_equal(idx, born_ref.sample(weights(amps), 4, 0, 5000)[0])


def test_state_sample_xparity():
    L = 12
    sub = XParity(SpinConserve(L, 6), sector='-')
    amps = int_amplitudes(sub.get_dimension(), 19)
    st = state_from(sub, amps)
    out = st.sample(5000, seed=5)
    assert np.all(popcount(out) == 6)
    top = (out >> (L - 1)) & 1                       # the representatives have spin L - 1 up (bit clear)
    assert 2000 < np.count_nonzero(top) < 3000
    rep = np.where(top == 1, out ^ ((1 << L) - 1), out)
    idx = sub.state_to_idx(rep)
    no_zero_weight(idx, weights(amps))
    rows, flips = born_ref.sample(weights(amps), 5, 0, 5000)
    assert np.array_equal(idx, rows) and np.array_equal(top, flips)


def test_histogram_of_a_dyadic_state():
    """With a fixed seed the histogram is that of the restatement, exactly (tests/test_born_host.py checks that this
    seed's histogram also lies within five sigma of the probabilities)."""
    amps, w, W = born_ref.dyadic_state()
    st = state_from(Full(L=6), amps)
    N = born_ref.HISTOGRAM_SHOTS
    out = st.sample(N, seed=born_ref.HISTOGRAM_SEED)
    want = born_ref.sample(w, born_ref.HISTOGRAM_SEED, 0, N)[0]
    assert np.array_equal(np.bincount(out, minlength=64), np.bincount(want, minlength=64))
    assert np.array_equal(out, want)
    no_zero_weight(out, w)


# ---- 12. power sums -----------------------------------------------------------------------------------------------
def check_power_sums_exact(st, amps):
    w = weights(amps).astype(np.int64)
    P, W, H, wmax, nnz = backend.power_sums(st.vec, [2, 3, 4])
    assert np.array_equal(P, [np.sum(w ** 2), np.sum(w ** 3), np.sum(w ** 4)])
    assert (W, wmax, nnz) == (w.sum(), w.max(), np.count_nonzero(w))
    pos = w[w > 0].astype(np.longdouble)
    terms = pos * np.log(pos)
    assert abs(H - float(terms.sum())) <= (2 * w.size + 16) * 2.0 ** -53 * float(np.abs(terms).sum())


@pytest.mark.parametrize("make,rows", [pytest.param(lambda: Full(L=13), 1 << 13, id="full13"),
                                       pytest.param(lambda: SpinConserve(13, 6), 1716, id="sc13_6")])
def test_power_sums_integer_amplitudes(make, rows):
    sub = make()
    amps = int_amplitudes(rows, 20)
    st = state_from(sub, amps)
    assert not st.vec.internal
    check_power_sums_exact(st, amps)


def test_power_sums_internal_layout(small_layout):
    """The vector goes in as it lies: the padding of the internal layout holds zeros and must not count."""
    amps = int_amplitudes(1716, 21)
    st = state_from(SpinConserve(13, 6), amps)
    assert st.vec.internal and st.vec.local_size > 1716
    check_power_sums_exact(st, amps)


def test_power_sums_swizzled():
    config.vec_swizzle = 5
    amps = int_amplitudes(1 << 12, 22)
    st = state_from(Full(L=12), amps)
    assert st.vec.swz == 5
    check_power_sums_exact(st, amps)


@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=14), id="full14"),
                                  pytest.param(lambda: SpinConserve(14, 7), id="sc14_7")])
def test_power_sums_random_states(make):
    sub = make()
    rows = sub.get_dimension()
    st = State(subspace=sub, state='random', seed=23)
    amps = st.to_numpy().astype(np.clongdouble)
    w = amps.real ** 2 + amps.imag ** 2
    qs = [0.5, 1.5, 2, 2.5]
    P, W, H, wmax, nnz = backend.power_sums(st.vec, qs)
    rel = (2 * rows + 16) * 2.0 ** -53
    for q, p in zip(qs, P):
        terms = w ** np.longdouble(q)
        err = abs(p - float(terms.sum()))
        print("q = %.1f: error %.3e (bound %.3e)" % (q, err, rel * float(terms.sum())))
        assert err <= rel * float(terms.sum())
    terms = w * np.log(w)
    print("H: error %.3e (bound %.3e)" % (abs(H - float(terms.sum())), rel * float(np.abs(terms).sum())))
    assert abs(H - float(terms.sum())) <= rel * float(np.abs(terms).sum())
    assert abs(W - float(w.sum())) <= rel * float(w.sum())
    assert abs(wmax - float(w.max())) <= 2.0 ** -51 * wmax          # (a weight takes three roundings)
    assert nnz == rows
    again = backend.power_sums(st.vec, qs)
    assert np.array_equal(again[0], P) and again[1:] == (W, H, wmax, nnz)
    # more than eight exponents take several passes and give the same sums
    many = [0.5, 1.5, 2, 2.5, 3, 4, 5, 6, 7, 0.25, 1.25]
    Pm = backend.power_sums(st.vec, many)[0]
    assert Pm.size == len(many) and np.array_equal(Pm[:4], P)


ALL_Q = [0, 0.5, 1, 1.5, 2, 3, 4, 7, np.inf]


def test_entropies_of_product_and_uniform_states():
    L = 12
    st = State(subspace=Full(L=L), state='UDUUDUDDUUDU')
    S = st.participation_entropies(ALL_Q)
    assert S.dtype == np.float64 and S.shape == (len(ALL_Q),) and np.all(np.abs(S) <= 1e-15)
    for sub in (Full(L=L), SpinConserve(L, 6)):
        dim = sub.get_dimension()
        st = state_from(sub, np.full(dim, 0.5 - 0.5j))               # not normalised
        assert np.max(np.abs(st.participation_entropies(ALL_Q) - np.log(dim))) <= 1e-13
    assert np.array_equal(st.participation_entropies(), participation_entropies(st, qs=(2,)))
    with pytest.raises(ValueError):
        st.participation_entropies([-1])


@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=12), id="full12"),
                                  pytest.param(lambda: SpinConserve(12, 6), id="sc12_6")])
def test_entropies_of_xparity_states(make):
    sub = XParity(make(), sector='+')
    rng = np.random.default_rng(24)
    x = rng.normal(size=sub.get_dimension()) + 1j * rng.normal(size=sub.get_dimension())
    x[::5] = 0
    st = state_from(sub, x)
    parent = state_from(Full(L=12), embed(sub, x))
    S, Sp = st.participation_entropies(ALL_Q), parent.participation_entropies(ALL_Q)
    print("xparity against the expanded state: largest difference %.3e" % np.max(np.abs(S - Sp)))
    assert np.max(np.abs(S - Sp)) <= 1e-13
