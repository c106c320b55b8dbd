"""
Born sampling restated in numpy: the reference of the tests of csrc/born_kernels.hip.

Rows are counted in index order.  With C = before + cumsum(w), a target t belongs to the smallest row i with C_i > t
(``np.searchsorted(C, t, side='right')``); the clamps and the zero-weight rule of the kernels follow:
  - a target below ``before`` belongs to an earlier block: -1;
  - a target at or beyond the total goes to the last row of non-zero weight when the block is the final one, else -1;
  - a row of weight zero is never returned: the next row that carries weight takes its place.
The shots' uniform stream is tests/philox_ref.philox4x32_10 with the counter words of csrc/born.h.
"""
import math

import numpy as np

import philox_ref

BORN_C2, BORN_C3 = 0x13198A2E, 0x03707344      # the constant counter words of csrc/born.h
BLOCK_ROWS = 1024                              # rows of a block of the kernels (dnm_born_plan reports it)


def search(w, targets, before=0.0, final=True, row0=0):
    """Global rows (row0 + local) of ``targets`` among the weights ``w`` of a block, -1 for those of other blocks."""
    w = np.asarray(w)
    t = np.asarray(targets, dtype=np.float64)
    C = before + np.cumsum(w)
    i = np.searchsorted(C, t, side='right')
    carries = np.flatnonzero(w > 0)
    out = np.full(t.size, -1, dtype=np.int64)
    if carries.size == 0:
        return out
    inside = (t >= before) & (i < w.size)
    # zero-weight rule: the first row at or behind i that carries weight (a no-op where the prefix is exact)
    nxt = np.searchsorted(carries, i[inside], side='left')
    ok = nxt < carries.size
    rows = np.full(nxt.size, -1, dtype=np.int64)
    rows[ok] = carries[nxt[ok]]
    out[inside] = rows
    if final:
        out[(t >= before) & (i >= w.size)] = carries[-1]
        out[inside & (out < 0)] = carries[-1]
    keep = out >= 0
    out[keep] += row0
    return out


def uniforms(seed, shot0, nshots):
    """(u, flip) of the shots shot0 .. shot0 + nshots - 1: u = (((c0 << 32) | c1) >> 11) 2^-53, flip = c2 & 1."""
    seed = int(seed) & (2 ** 64 - 1)
    ctr = np.arange(nshots, dtype=np.uint64) + np.uint64(shot0)
    mask, sh = np.uint64(0xffffffff), np.uint64(32)
    c0, c1, c2, _ = philox_ref.philox4x32_10((ctr & mask, ctr >> sh, BORN_C2, BORN_C3), (seed & 0xffffffff, seed >> 32))
    u = (((c0 << sh) | c1) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return u, (c2 & np.uint64(1)).astype(np.uint8)


def sample(w, seed, shot0, nshots):
    """(rows, flips) as dnm_born_sample draws them from the weights ``w`` of a whole state: t = u W in one rounding,
    W = the serial sum of the block sums (exact where the tests compare bit for bit)."""
    u, flips = uniforms(seed, shot0, nshots)
    W = float(np.cumsum(np.asarray(w, dtype=np.float64))[-1])
    return search(w, u * W), flips


def four_squares(n):
    """(a, b, c, d) with a^2 + b^2 + c^2 + d^2 = n (Lagrange), largest first."""
    for a in range(math.isqrt(n), -1, -1):
        m = n - a * a
        for b in range(math.isqrt(m), -1, -1):
            m2 = m - b * b
            for c in range(math.isqrt(m2), -1, -1):
                d = math.isqrt(m2 - c * c)
                if d * d == m2 - c * c:
                    return a, b, c, d
    raise AssertionError(n)


def plant_power_of_two(amps):
    """Integer amplitudes whose last two entries are replaced so that the total weight is a power of two: u W is
    then exact for every 53-bit u.  Returns (amplitudes, W)."""
    amps = np.array(amps, dtype=np.complex128)
    rest = int(np.sum(amps[:-2].real ** 2 + amps[:-2].imag ** 2))
    W = 1 << max(rest, 1).bit_length()
    a, b, c, d = four_squares(W - rest)
    amps[-2], amps[-1] = a + 1j * b, c + 1j * d
    w = amps.real ** 2 + amps.imag ** 2
    assert int(w.sum()) == W
    return amps, W


def dyadic_state(L=6, seed=11):
    """Amplitudes of an L-spin state whose probabilities are multiples of 2^-m: small integer amplitudes with the
    total weight planted to a power of two.  Returns (amplitudes, weights, W)."""
    rng = np.random.default_rng(seed)
    n = 1 << L
    amps = (rng.integers(-3, 4, n) + 1j * rng.integers(-3, 4, n)).astype(np.complex128)
    amps, W = plant_power_of_two(amps)
    return amps, amps.real ** 2 + amps.imag ** 2, W


HISTOGRAM_SEED, HISTOGRAM_SHOTS = 2024, 1 << 16
