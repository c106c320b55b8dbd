"""
The host side of Born sampling and the participation entropies (csrc/born.h through dnm_born_plan, dnm_born_scan and
dnm_born_uniforms; computations.participation_from_sums) -- no GPU needed.
"""
import ctypes as C

import numpy as np
import pytest

import born_ref
from dynamite_amd import _lib, backend
from dynamite_amd.computations import participation_from_sums
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve


# ---- 1. plan ------------------------------------------------------------------------------------------------------
def _subspaces():
    rng = np.random.default_rng(3)
    states = np.unique(rng.integers(0, 1 << 40, 3000, dtype=np.int64))[:2500]
    return [Full(L=12), Parity('even', L=13), Parity('odd', L=13), SpinConserve(14, 7), Explicit(states, L=40)]


def test_plan():
    subs = _subspaces()
    br = backend.born_plan(subs[0]._c(), 1)[0]
    assert br == born_ref.BLOCK_ROWS and br > 0 and br & (br - 1) == 0
    for nrows in (1, br - 1, br, br + 1, 2 * br, 2 * br + 1, 2500):
        plans = {backend.born_plan(s._c(), nrows) for s in subs}
        assert plans == {(br, -(-nrows // br), 8 * -(-nrows // br))}, nrows
    assert backend.born_plan(subs[0]._c(), 0) == (br, 0, 0)
    # a function of the number of rows alone, far beyond what a test allocates
    assert backend.born_plan(Full(L=32)._c(), 1 << 32) == (br, (1 << 32) // br, 8 * ((1 << 32) // br))


def test_plan_outputs_are_optional_and_arguments_checked():
    d = Full(L=12)._c()
    nb = C.c_int64()
    _lib.check(_lib.lib().dnm_born_plan(C.byref(d), 3000, None, C.byref(nb), None))
    assert nb.value == 3
    assert _lib.lib().dnm_born_plan(C.byref(d), 4097, None, C.byref(nb), None) != 0       # more rows than the subspace
    assert _lib.lib().dnm_born_plan(None, 10, None, C.byref(nb), None) != 0
    # the SpinConserve internal layout is refused: rows are counted in reference order
    sc = _lib.Subspace.from_buffer_copy(SpinConserve(14, 7)._c())
    sc.vec_swizzle = 6 | 4 << 8
    assert _lib.lib().dnm_born_plan(C.byref(sc), 100, None, C.byref(nb), None) != 0
    assert b"reference order" in _lib.lib().dnm_last_error()


# ---- 2. scan ------------------------------------------------------------------------------------------------------
def test_scan_is_monotone_on_adversarial_input():
    sums = np.empty(1 << 16)
    sums[0::2], sums[1::2] = 1.0, 2.0 ** -60
    sums[1000:5000] = 0.0                                 # whole blocks without weight
    for before in (0.0, 3.0, 2.0 ** 40):
        scan = backend.born_scan(sums, before)
        assert np.all(np.diff(scan) >= 0) and scan[0] >= before
        assert np.array_equal(scan[1000:5000], np.full(4000, scan[999]))
        # the serial sum, to the bit (numpy accumulates a 1-D float64 array in order)
        assert np.array_equal(scan, np.cumsum(np.concatenate([[before], sums]))[1:])


def test_scan_is_exact_on_integers():
    rng = np.random.default_rng(5)
    sums = rng.integers(0, 18 * 1024 + 1, 1 << 12)
    for before in (0, 12345):
        scan = backend.born_scan(sums.astype(np.float64), float(before))
        assert np.array_equal(scan, (before + np.cumsum(sums)).astype(np.float64))
    assert backend.born_scan(np.empty(0)).size == 0


# ---- 3. the uniform stream ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 0xDEADBEEFCAFEF00D])
def test_uniform_stream(seed):
    for shot0, n in ((0, 1000), ((1 << 32) - 3, 8), ((1 << 40) + 17, 5)):
        u, flip = backend.born_uniforms(seed, shot0, n)
        want_u, want_flip = born_ref.uniforms(seed, shot0, n)
        assert np.array_equal(u, want_u) and np.array_equal(flip, want_flip)
        assert np.all((u >= 0) & (u < 1))
    u, flip = backend.born_uniforms(seed, 0, 1000)
    assert 300 < np.count_nonzero(flip) < 700 and 0.4 < u.mean() < 0.6
    # chunks are the same stream
    a, fa = backend.born_uniforms(seed, 0, 400)
    b, fb = backend.born_uniforms(seed, 400, 600)
    assert np.array_equal(np.concatenate([a, b]), u) and np.array_equal(np.concatenate([fa, fb]), flip)


def test_counter_words_differ_from_set_random():
    """With philox_normal's constant words shot i would reuse the bits behind |psi_i| of set_random(seed)."""
    import philox_ref
    assert (born_ref.BORN_C2, born_ref.BORN_C3) != (philox_ref.C2, philox_ref.C3)
    c = philox_ref.words(np.arange(16, dtype=np.uint64), 7)
    u_fill = (((c[0] << np.uint64(32)) | c[1]) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    assert not np.any(backend.born_uniforms(7, 0, 16)[0] == u_fill)


# ---- 4. entropies from the sums -----------------------------------------------------------------------------------
QS = [0, 0.5, 1, 1.5, 2, 3, 4, np.inf]


def _sums(w, qs):
    w = np.asarray(w, dtype=np.float64)
    pos = w[w > 0]
    need = [q for q in qs if np.isfinite(q) and q not in (0, 1)]
    return ([np.sum(pos ** q) for q in need], np.sum(w), np.sum(pos * np.log(pos)), np.max(w), float(pos.size))


def _direct(p, qs):
    """S_q of the probabilities p (summing to one), evaluated as written."""
    p = np.asarray(p, dtype=np.float64)
    p = p[p > 0]
    out = []
    for q in qs:
        if q == 0:
            out.append(np.log(p.size))
        elif q == 1:
            out.append(-np.sum(p * np.log(p)))
        elif np.isinf(q):
            out.append(-np.log(p.max()))
        else:
            out.append(np.log(np.sum(p ** q)) / (1 - q))
    return np.array(out)


def test_entropy_formulas():
    rng = np.random.default_rng(9)
    w = rng.random(500) ** 3 * 7.5           # not normalised
    w[rng.integers(0, 500, 60)] = 0.0
    got = participation_from_sums(QS, *_sums(w, QS))
    assert got.dtype == np.float64 and got.shape == (len(QS),)
    assert np.max(np.abs(got - _direct(w / w.sum(), QS))) < 1e-13
    # hand-made: two rows of weights 1 and 3
    got = participation_from_sums([0, 1, 2, np.inf], [10.0], 4.0, 3 * np.log(3.0), 3.0, 2.0)
    want = [np.log(2), np.log(4) - 0.75 * np.log(3), -np.log(10 / 16), -np.log(0.75)]
    assert np.max(np.abs(got - want)) < 1e-15
    # the exponents are taken in the order given
    assert np.array_equal(participation_from_sums([2, 3], [10.0, 28.0], 4.0, 0.0, 3.0, 2.0)[::-1],
                          participation_from_sums([3, 2], [28.0, 10.0], 4.0, 0.0, 3.0, 2.0))
    with pytest.raises(ValueError):
        participation_from_sums([2, 3], [10.0], 4.0, 0.0, 3.0, 2.0)


def test_entropy_formulas_xparity():
    """The sums over the representatives of an XParity state against the expanded 2 dim probabilities."""
    rng = np.random.default_rng(10)
    w = rng.random(300) * 2.0
    w[::7] = 0.0
    got = participation_from_sums(QS, *_sums(w, QS), flip_sector=True)
    expanded = np.concatenate([w, w]) / 2
    assert np.max(np.abs(got - _direct(expanded / expanded.sum(), QS))) < 1e-13
    plain = participation_from_sums(QS, *_sums(w, QS))
    assert np.max(np.abs(got - plain - np.log(2))) < 1e-13


# ---- the seed of the histogram test of tests/test_gpu_born_sampling.py ----------------------------------------------
def test_histogram_seed_lies_within_five_sigma():
    """The GPU test compares histograms exactly (a deterministic statement); that the chosen seed's histogram is also a
    fair draw is checked here, on the restatement."""
    _, w, W = born_ref.dyadic_state()
    N = born_ref.HISTOGRAM_SHOTS
    rows, _ = born_ref.sample(w, born_ref.HISTOGRAM_SEED, 0, N)
    counts = np.bincount(rows, minlength=w.size)
    p = w / W
    assert counts.sum() == N and np.all(counts[w == 0] == 0)
    assert np.all(np.abs(counts - N * p) <= 5 * np.sqrt(N * p * (1 - p)))
