"""
What of the vector layer can be checked without a device: the numpy restatement of the generator
(tests/philox_ref.py, the reference of tests/test_gpu_vec.py) against the published known answers of Philox-4x32-10,
and the argument checks of the vector ABI that return before anything is launched.
"""
import ctypes as C

import numpy as np
import pytest

from dynamite_amd import _lib
import philox_ref


# Random123 (kat_vectors): philox4x32 with 10 rounds
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,out", KNOWN)
def test_philox_known_answers(ctr, key, out):
    got = philox_ref.philox4x32_10(ctr, key)
    assert tuple(int(w[0]) for w in got) == out


def test_philox_reference_layout_of_counter_and_key():
    """words(): counter (low, high, 0x243F6A88, 0x85A308D3), key (seed low, seed high); vectorised = one at a time"""
    ctr = np.array([0, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3, 2 ** 64 - 1], dtype=np.uint64)
    seed = 2 ** 63 + 1
    all_at_once = philox_ref.words(ctr, seed)
    for j, c in enumerate(ctr.tolist()):
        one = philox_ref.philox4x32_10((c & 0xffffffff, c >> 32, 0x243F6A88, 0x85A308D3), (seed & 0xffffffff, seed >> 32))
        assert [int(w[0]) for w in one] == [int(w[j]) for w in all_at_once]
    u1, u2 = philox_ref.uniforms(ctr, seed)
    assert u1.dtype == np.longdouble and np.all(u1 > 0) and np.all(u1 <= 1) and np.all(u2 >= 0) and np.all(u2 < 1)
    assert np.array_equal(philox_ref.counters(3, 2 ** 64 - 1), np.array([2 ** 64 - 1, 0, 1], dtype=np.uint64))
    re, im, rad = philox_ref.normal(ctr, seed)
    assert np.max(np.abs(re * re + im * im - rad * rad)) < 1e-17 * np.max(rad * rad)


def _buf(n=16):
    a = np.zeros(n, dtype=np.complex128)
    return a, C.c_void_p(a.ctypes.data)


# a vector of n elements has a layout of swizzle shift S only when n <= 2^S or n is a multiple of 2^S
BAD_SIZES = [(5, 32 + 16), (5, 33), (6, 64 + 16), (6, 3 * 64 + 1), (16, 2 ** 16 + 16), (24, 2 ** 24 + 2 ** 23)]


@pytest.mark.parametrize("S,n", BAD_SIZES)
def test_swizzle_entry_points_refuse_sizes_without_a_layout(S, n):
    """return code and message only: nothing is launched (the pointers are host memory that no kernel may see)"""
    L = _lib.lib()
    (a, pa), (b, pb) = _buf(), _buf()
    assert L.dnm_vec_set_random_swz(pa, n, 1, 0, S, None) != 0
    assert b"multiple of 2^%d" % S in L.dnm_last_error()
    assert L.dnm_vec_swizzle_copy(pa, pb, n, S, None) != 0
    assert b"multiple of 2^%d" % S in L.dnm_last_error()
    assert L.dnm_vec_unpack_real(pa, pb, n, S, 0, None) != 0            # n_packed under swizzle_packed
    assert b"multiple of 2^%d" % S in L.dnm_last_error()
    if n % 2 == 0:
        assert L.dnm_vec_unpack_real(pa, pb, n // 2, 0, S, None) != 0   # 2 n_packed under swizzle_out
        assert (b"%d elements" % n) in L.dnm_last_error() and b"multiple of 2^%d" % S in L.dnm_last_error()
    assert not a.any() and not b.any()


def test_swizzle_entry_points_still_refuse_bad_shifts():
    L = _lib.lib()
    (a, pa), (b, pb) = _buf(), _buf()
    for S in (1, 4, 25, -1):
        assert L.dnm_vec_set_random_swz(pa, 64, 1, 0, S, None) != 0 and b"out of range" in L.dnm_last_error()
        assert L.dnm_vec_swizzle_copy(pa, pb, 64, S, None) != 0 and b"out of range" in L.dnm_last_error()
        assert L.dnm_vec_unpack_real(pa, pb, 64, S, 0, None) != 0 and b"out of range" in L.dnm_last_error()
        assert L.dnm_vec_unpack_real(pa, pb, 64, 0, S, None) != 0 and b"out of range" in L.dnm_last_error()


@pytest.mark.parametrize("nv", [0, 257, -1])
def test_mdot_refuses_bad_nv_before_any_launch(nv):
    L = _lib.lib()
    (a, pa), (b, pb) = _buf(), _buf()
    h = np.zeros(2 * 257)
    assert L.dnm_vec_mdot(pa, 16, nv, pb, 16, _lib.pf64(h), None) != 0
    assert b"nv out of range" in L.dnm_last_error()


def test_library_exports_the_sweeps_the_check_program_links():
    """tests/vec_sweeps_check.cpp links dnm::vec_lanczos_update_host, dnm::vec_lanczos_dot_host and
    dnm::vk_reduce_partials from the in-tree library"""
    import shutil
    import subprocess
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm")
    out = subprocess.run([nm, "-DC", "--defined-only", _lib.lib()._name], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    for sym in ("dnm::vec_lanczos_update_host(", "dnm::vec_lanczos_dot_host(", "dnm::vk_reduce_partials(",
                "dnm::vk_reduce_scratch("):
        assert sym in out.stdout, sym
