"""Every handle tests/test_gpu_wide_sectors.py multiplies on, built on the host (DNM_MAT_HOST_ONLY): the kernel route it
takes, the reference order of its vectors and its sizes -- so that a GPU case cannot pass on another route than the one
it claims -- and the refusal of a dense reduced density matrix on a subspace too wide for its kernel to end."""
import ctypes as C

import numpy as np
import pytest

import wide_ref as w
from dynamite_amd import _lib, backend
from dynamite_amd.subspaces import Explicit, Full, SpinConserve


def host_handle(c, flags=0, rank=0, nranks=1):
    left, right = c.subspaces()
    lc, rc = left._c(), right._c()
    assert lc.vec_swizzle == 0 and rc.vec_swizzle == 0          # too few states for the internal layout
    h = backend.create_mat(*c.arrs, lc, rc, False, flags | _lib.MAT_HOST_ONLY, rank, nranks)
    return backend.ShellMat(h, lc, rc, nranks, rank)


@pytest.mark.parametrize("name", sorted(w.HANDLES))
def test_route_layout_and_sizes(monkeypatch, name):
    left, right, op, flags, knobs, route = w.HANDLES[name]
    assert flags in (0, _lib.MAT_FORCE_GATHER) and w.FORCE_GATHER == _lib.MAT_FORCE_GATHER
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    c = w.case(left, op, right)
    mat = host_handle(c, flags)
    d = mat.describe()
    sc_pair = left in w.SC and right in w.SC
    if route == w.BLOCK:
        # the block kernel's tables live on the device: a host-only handle of the same pair reads as the row kernel
        # (csrc/mat.cpp, dnm_mat_create); what the knob asks for has to be on offer, the GPU test asserts the rest
        assert sc_pair and not flags and w.ROWS in d, d
        assert c.nmasks <= 64 and 13 < c.L <= 34
    else:
        assert route in d, d
        assert (route == w.ROWS) == (sc_pair and not flags), d
    assert w.BLOCK not in d and 'internal layout' not in d and 'tiled=1' not in d, d
    assert (mat.swz_left, mat.swz_right) == (0, 0)
    assert (mat.M, mat.N, mat.m_local, mat.n_local) == (c.M, c.N, c.M, c.N)
    mat.destroy()


@pytest.mark.parametrize("s", ['sc63_2', 'sc50_2'])
def test_partitioned_shares(s):
    c = w.case(s, 'far')
    for r in range(3):
        mat = host_handle(c, rank=r, nranks=3)
        assert w.ROWS in mat.describe(), mat.describe()
        assert (mat.row0, mat.m_local) == backend.split_ownership(c.M, 3, r)
        assert (mat.swz_left, mat.swz_right) == (0, 0)
        mat.destroy()


def rdm_call(sub, keep):
    """dnm_reduced_density_matrix on host buffers: a call that is refused never looks at them."""
    x = np.zeros(4, dtype=np.complex128)
    keep = np.ascontiguousarray(keep, dtype=np.int64)
    rho = np.zeros(4 ** keep.size, dtype=np.complex128)
    _lib.check(_lib.lib().dnm_reduced_density_matrix(C.c_void_p(x.ctypes.data), C.byref(sub._c()), keep.size,
                                                     _lib.p64(keep), C.c_void_p(rho.ctypes.data), None))


@pytest.mark.parametrize("sub", [SpinConserve(63, 2), Explicit(np.array([1, 5, 1 << 40], dtype=np.int64), L=41),
                                 Full(L=41)], ids=['sc63_2', 'explicit41', 'full41'])
def test_dense_rdm_refuses_more_than_40_spins(sub):
    """2^(L - k) traced configurations per kept one, whatever the dimension: refused with the count in the message,
    before the subspace is uploaded (this test has no device)."""
    with pytest.raises(_lib.BackendError, match=r"2\^L = 2\^%d amplitudes" % sub.L):
        rdm_call(sub, [0, 3, 7])
