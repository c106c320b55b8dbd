"""
Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the Box-Muller
step of csrc/philox.h restated in numpy: the reference of the device generator's tests.  The integer part is exact;
the normal deviates are computed in numpy.longdouble.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85                                # key increments (Weyl sequence)
C2, C3 = 0x243F6A88, 0x85A308D3                                # the two constant counter words of csrc/philox.h
MASK = np.uint64(0xffffffff)
SH = np.uint64(32)


def philox4x32_10(counter, key):
    """The four output words (uint64 arrays holding 32-bit values) for ``counter`` (four words, scalars or arrays) under
    ``key`` (two words, Python ints)."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & MASK for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                           # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> SH) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> SH) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c


def words(ctr, seed):
    """Output words for the 64-bit counters ``ctr`` (uint64 array) under the 64-bit ``seed``, as philox_normal sets
    them up: counter (low, high, C2, C3), key (seed low, seed high)."""
    ctr = np.atleast_1d(np.asarray(ctr, dtype=np.uint64))
    seed = int(seed) & (2 ** 64 - 1)
    return philox4x32_10((ctr & MASK, ctr >> SH, C2, C3), (seed & 0xffffffff, seed >> 32))


def uniforms(ctr, seed):
    """u1 in (0, 1] (53 bits + 1) and u2 in [0, 1) (53 bits), both exact in longdouble."""
    c0, c1, c2, c3 = words(ctr, seed)
    s11 = np.uint64(11)
    a = ((c0 << SH) | c1) >> s11
    b = ((c2 << SH) | c3) >> s11
    two53 = np.longdouble(2) ** 53
    return (a.astype(np.longdouble) + 1) / two53, b.astype(np.longdouble) / two53


def normal(ctr, seed):
    """(re, im, rad) in longdouble: re + i im = rad (cos, sin)(2 pi u2), rad = sqrt(-2 ln u1)."""
    u1, u2 = uniforms(ctr, seed)
    rad = np.sqrt(-2 * np.log(u1))
    pi = 4 * np.arctan(np.longdouble(1))
    ang = 2 * pi * u2
    return rad * np.cos(ang), rad * np.sin(ang), rad


def counters(n, offset):
    """The counters of elements 0 .. n-1 of a fill at ``offset``: (offset + i) mod 2^64."""
    return (np.arange(n, dtype=np.uint64) + np.uint64(int(offset) & (2 ** 64 - 1)))
