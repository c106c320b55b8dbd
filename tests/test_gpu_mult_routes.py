"""The one-rank multiply y = A x - b z + c z2 [, sums] on every kernel route of a handle (csrc/mat.h: Route; the one
switch is mult_fused in csrc/mat_mult.cpp), for the route / entry point pairs no other file runs: the SpinConserve block
kernel and the internal layout's row kernel under dnm_mat_mult_sub2, the row kernels with their fused twins switched off
(DNM_ROW_FUSE=0), and dnm_mat_fuses_init -- what the Krylov drivers decide an extra sweep by -- on one handle per route.
The reference is the handle's own plain multiply followed by the sweeps in numpy; the bar is the suite's for that
comparison, nnz_per_row * eps * 100 relative (tests/test_gpu_interior.py)."""
import ctypes as C

import numpy as np
import pytest

from dynamite_amd import _lib, backend
from dynamite_amd.config import config
from dynamite_amd.subspaces import Explicit, Full, SpinConserve
from gpu_util import shell, vec_from
from test_gpu_interior import EPS, dm_chain, heisenberg
from test_gpu_matvec import cfg

pytestmark = pytest.mark.gpu

B, CZ = 0.37, complex(-0.4, 0.9)


@pytest.fixture
def small_layout():
    """(6, 4) field split for every SpinConserve subspace with L >= 11, as tests/test_gpu_sc3.py makes such handles."""
    old = (config.sc_layout, config.sc_layout_min_dim)
    config.sc_layout, config.sc_layout_min_dim = (6, 4), 0
    yield
    config.sc_layout, config.sc_layout_min_dim = old


@pytest.fixture
def no_layout():
    old = config.sc_layout
    config.sc_layout = None
    yield
    config.sc_layout = old


def explicit_half_filling(L):
    sub = SpinConserve(L, L // 2)
    return Explicit(sub.idx_to_state(np.arange(sub.get_dimension())), L=L)


class Run:
    """A handle with seeded vectors x, z, z2 on the device and its plain product H x."""

    def __init__(self, H, sub, diag=None):
        self.mat = mat = shell(H, sub)
        if diag or (diag is None and mat.uses_cached_diagonal()):
            mat.precompute_diagonal()
        n = mat.N
        rs = np.random.RandomState(11)
        self.x, self.z, self.z2 = (rs.standard_normal(n) + 1j * rs.standard_normal(n) for _ in range(3))
        self.xv, self.yv = mat.createVecs()
        self.xv.set_local_from_numpy(self.x)
        sub_c = mat._keep[0] if mat.swz_left >= 256 else None
        self.zv, self.z2v = vec_from(self.z, mat.swz_left, sub_c), vec_from(self.z2, mat.swz_left, sub_c)
        self.yv.set(777.0)          # every multiply below must overwrite, not accumulate
        mat.mult(self.xv, self.yv)
        self.Hx = self.yv.local_numpy()
        self.bar = len(np.unique(H.msc['masks'])) * EPS * 100

    def fuses_init(self):
        return _lib.lib().dnm_mat_fuses_init(self.mat.handle)

    def sub2(self, with_z2):
        """(what dnm_mat_mult_sub2 left in y, the same by the plain multiply and numpy)"""
        self.yv.set(777.0)
        _lib.check(_lib.lib().dnm_mat_mult_sub2(self.mat.handle, self.xv.ptr, self.yv.ptr, self.zv.ptr, B,
                                                self.z2v.ptr if with_z2 else None, CZ.real if with_z2 else 0.0,
                                                CZ.imag if with_z2 else 0.0, backend._stream()))
        return self.yv.local_numpy(), self.Hx - B * self.z + (CZ * self.z2 if with_z2 else 0.0)

    def lanczos(self, with_z):
        self.yv.set(777.0)
        dot = (C.c_double * 3)()
        _lib.check(_lib.lib().dnm_mat_mult_lanczos(self.mat.handle, self.xv.ptr, self.yv.ptr,
                                                   self.zv.ptr if with_z else None, B if with_z else 0.0, dot,
                                                   backend._stream()))
        return self.yv.local_numpy(), np.array(dot), self.Hx - (B * self.z if with_z else 0.0)

    def check_sub2(self, with_z2):
        got, want = self.sub2(with_z2)
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print("sub2 z2=%s: %.2e of %.2e" % (with_z2, err, self.bar))
        assert err <= self.bar, (with_z2, self.mat.describe())

    def check_sums(self, dot, want):
        """the three sums against numpy on `want`, to the bar (as test_row_kernels_fuse_start_vectors_and_sums)"""
        scale = np.linalg.norm(self.x) * np.linalg.norm(want)
        assert abs(complex(dot[0], dot[1]) - np.vdot(self.x, want)) <= self.bar * scale
        assert abs(dot[2] - np.vdot(want, want).real) <= self.bar * np.vdot(want, want).real


@pytest.mark.parametrize("diag", [False, True])
def test_block_kernel_sub2(no_layout, monkeypatch, diag):
    """SpinConserve block kernel: the start vectors open its accumulators, with the diagonal cached and on the fly."""
    monkeypatch.setenv("DNM_SC_BLOCK", "10")
    r = Run(dm_chain(13), SpinConserve(13, 6), diag=diag)
    assert "block form" in r.mat.describe(), r.mat.describe()
    assert r.fuses_init() == 1
    for with_z2 in (True, False):
        r.check_sub2(with_z2)
    r.mat.destroy()


def test_internal_layout_row_kernel_sub2(small_layout, monkeypatch):
    """The internal layout's row kernel takes both start vectors (padding and all: the vectors are longer than dim)."""
    monkeypatch.setenv("DNM_SC3_TILED", "0")
    r = Run(dm_chain(16), SpinConserve(16, 8))
    d = r.mat.describe()
    assert "internal layout" in d and "row kernel" in d, d
    assert r.fuses_init() == 1
    r.check_sub2(True)
    r.mat.destroy()


@pytest.mark.parametrize("name", ["sc_rows", "explicit"])
def test_unfused_fallback(no_layout, monkeypatch, name):
    """DNM_ROW_FUSE=0: the row kernels run plain and every extra term is a sweep of its own -- dnm_mat_fuses_init says
    so, and dnm_mat_mult_sub2 / dnm_mat_mult_lanczos give what the fused handle of the same operator gives."""
    monkeypatch.setenv("DNM_SC_BLOCK", "0")
    H = dm_chain(12)
    sub = SpinConserve(12, 6) if name == "sc_rows" else explicit_half_filling(12)
    fused = Run(H, sub)
    monkeypatch.setenv("DNM_ROW_FUSE", "0")
    plain = Run(H, sub)
    assert fused.fuses_init() == 1 and plain.fuses_init() == 0
    assert "block form" not in plain.mat.describe() and "tiled=1" not in plain.mat.describe(), plain.mat.describe()
    assert np.array_equal(plain.Hx, fused.Hx)          # the same plain kernel on both handles
    for with_z2 in (True, False):
        plain.check_sub2(with_z2)
        got, want = plain.sub2(with_z2)
        ref, _ = fused.sub2(with_z2)
        assert np.max(np.abs(got - ref)) <= plain.bar * np.max(np.abs(want))
    for with_z in (True, False):
        y, dot, want = plain.lanczos(with_z)
        yf, dotf, _ = fused.lanczos(with_z)
        assert np.max(np.abs(y - want)) <= plain.bar * np.max(np.abs(want))
        assert np.max(np.abs(y - yf)) <= plain.bar * np.max(np.abs(want))
        plain.check_sums(dot, want)
        fused.check_sums(dotf, want)
    fused.mat.destroy()
    plain.mat.destroy()


# (route, operator, subspace, knobs, fixture of the SpinConserve layout, what describe() says, dnm_mat_fuses_init)
ROUTES = {
    "tiled": (lambda: heisenberg(12), lambda: Full(12), {}, "no_layout", "tiled=1", 1),
    "sc3_tiled": (lambda: heisenberg(12), lambda: SpinConserve(12, 6), {}, "small_layout", "two-pass", 1),
    "sc3_rows": (lambda: heisenberg(12), lambda: SpinConserve(12, 6), {"DNM_SC3_TILED": "0"}, "small_layout",
                 "SpinConserve row kernel", 1),
    "sc_block": (lambda: heisenberg(13), lambda: SpinConserve(13, 6), {"DNM_SC_BLOCK": "10"}, "no_layout", "block form", 1),
    "sc_rows": (lambda: heisenberg(12), lambda: SpinConserve(12, 6), {"DNM_SC_BLOCK": "0"}, "no_layout",
                "one row per thread", 1),
    "gather": (lambda: heisenberg(12), lambda: explicit_half_filling(12), {}, "no_layout", "row-gather", 1),
    "sc_rows_unfused": (lambda: heisenberg(12), lambda: SpinConserve(12, 6), {"DNM_SC_BLOCK": "0", "DNM_ROW_FUSE": "0"},
                        "no_layout", "one row per thread", 0),
    "gather_unfused": (lambda: heisenberg(12), lambda: explicit_half_filling(12), {"DNM_ROW_FUSE": "0"}, "no_layout",
                       "row-gather", 0),
}


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_fuses_init_on_every_route(request, monkeypatch, name):
    """dnm_mat_fuses_init is 1 on a handle of every route and 0 on the fallback handles, and on the same handles
    dnm_mat_mult_sub2(b, z2) is the multiply followed by the two sweeps, whichever way the route gets there."""
    mkH, mksub, knobs, layout, says, fuses = ROUTES[name]
    request.getfixturevalue(layout)
    if name == "tiled":
        cfg(monkeypatch)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    r = Run(mkH(), mksub())
    assert says in r.mat.describe(), r.mat.describe()
    assert r.fuses_init() == fuses, r.mat.describe()
    r.check_sub2(True)
    r.mat.destroy()
