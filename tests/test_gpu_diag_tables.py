"""
The diagonal of a pass from tables (dynamite_amd/csrc/plan.h: DevPass::dblock) on the GPU: the kernel instances that read
one number per workgroup and one table entry per row instead of the diagonal's term lists, against the CPU oracle and,
where the arithmetic is exact, bit for bit against the instances that keep the lists (DNM_DIAG_BLOCK_TABLE=0).  Shapes as
in test_gpu_flipflop.py: one tile with nothing outside it, then a window pass and a contiguous pass with the boundary
bond of the diagonal's tile on a thread bit and on a k bit.
"""
import ctypes as C

import numpy as np
import pytest

from dynamite_amd import _lib, backend, models
from dynamite_amd.subspaces import Full
from oracle import oracle as orc
from gpu_util import marshal, orc_msc, orc_sub, shell, vec_from, mult_numpy, rand_state, partner_slice
from test_gpu_matvec import tol_for, cfg
from test_gpu_flipflop import SHAPES, _case
from test_diag_tables import DYADIC, dy_cross

pytestmark = pytest.mark.gpu

_REF = {}


def _on(mat):
    return "diag_tables=1" in mat.describe()


def _int_state(n, seed):
    rs = np.random.RandomState(seed)
    return (rs.randint(-8, 9, n) + 1j * rs.randint(-8, 9, n)).astype(np.complex128)


@pytest.mark.parametrize("L,B,logR,mode,amin", SHAPES)
@pytest.mark.parametrize("name", ["mbl", "aniso", "xxz"])
def test_tables_vs_oracle(monkeypatch, name, L, B, logR, mode, amin):
    cfg(monkeypatch, B, logR, mode, amin)
    H, arrs, sub, x, ref = _case(name, L)
    for tables in ("1", "0"):
        monkeypatch.setenv("DNM_DIAG_BLOCK_TABLE", tables)
        for flip in ("1", "0"):
            monkeypatch.setenv("DNM_FLIPFLOP", flip)
            for flags in (0, _lib.MAT_USE_GLDS):
                mat = shell(H, sub, flags=flags)
                assert "tiled=1" in mat.describe() and "diag=1" in mat.describe()
                assert _on(mat) == (tables == "1"), mat.describe()
                y = mult_numpy(mat, x)
                err = np.max(np.abs(y - ref))
                print(name, L, B, logR, "tables", tables, "flipflop", flip, "flags", flags,
                      "err %.3e tol %.3e" % (err, tol_for(arrs, x)))
                assert err <= tol_for(arrs, x), mat.describe()
                mat.destroy()


@pytest.mark.parametrize("L,B,logR,mode,amin", SHAPES)
@pytest.mark.parametrize("name", sorted(DYADIC))
def test_tables_on_and_off_bit_identical(monkeypatch, name, L, B, logR, mode, amin):
    """Dyadic coefficients and integer-valued amplitudes: every product and every partial sum of a row is exact in double,
    so the order of the diagonal's sum cannot show -- the two forms of the diagonal give the same bits."""
    cfg(monkeypatch, B, logR, mode, amin)
    H = DYADIC[name](L)
    sub = Full(L=L)
    x = _int_state(1 << L, L)
    for flip in ("1", "0"):
        monkeypatch.setenv("DNM_FLIPFLOP", flip)
        ys = {}
        for tables in ("1", "0"):
            monkeypatch.setenv("DNM_DIAG_BLOCK_TABLE", tables)
            mat = shell(H, sub)
            assert _on(mat) == (tables == "1"), mat.describe()
            ys[tables] = mult_numpy(mat, x)
            mat.destroy()
        assert np.any(ys["1"] != 0) and np.array_equal(ys["1"], ys["0"]), (name, flip)


@pytest.mark.parametrize("name", ["mbl", "aniso"])
def test_tables_ranges_of_one_pass(monkeypatch, name):
    """dnm_mat_mult_local_part on the pass that carries the diagonal: four ranges of its workgroups (block_offset != 0 in
    three of them: the index into DevPass::dblock) write, bit for bit, what the whole launch writes."""
    L = 14
    cfg(monkeypatch, 10, 2, 1, 3)
    H, arrs, sub, x, ref = _case(name, L)
    for flip in ("1", "0"):
        monkeypatch.setenv("DNM_FLIPFLOP", flip)
        for flags in (0, _lib.MAT_USE_GLDS):
            mat = shell(H, sub, flags=flags)
            assert _on(mat), mat.describe()
            vals = [C.c_int() for _ in range(6)]
            _lib.check(_lib.lib().dnm_mat_plan_counts(mat.handle, *[C.byref(v) for v in vals]))
            assert vals[0].value == 1 and vals[2].value == 1, mat.describe()
            xv = vec_from(x, mat.swz_right)
            yw, yp = backend.Vec(mat.M, swz=mat.swz_left), backend.Vec(mat.M, swz=mat.swz_left)
            yw.set_local_from_numpy(np.full(1 << L, np.nan + 1j * np.nan))
            yp.set_local_from_numpy(np.full(1 << L, np.nan + 1j * np.nan))
            _lib.check(_lib.lib().dnm_mat_mult_local(mat.handle, xv.ptr, yw.ptr, None))
            for part in range(4):
                _lib.check(_lib.lib().dnm_mat_mult_local_part(mat.handle, xv.ptr, yp.ptr, part, 4, None))
            y_whole, y_parts = yw.local_numpy(), yp.local_numpy()
            assert np.array_equal(y_parts, y_whole), mat.describe()
            assert np.max(np.abs(y_whole - ref)) <= tol_for(arrs, x), mat.describe()
            mat.destroy()


def test_tables_fused_entry_points(monkeypatch):
    """y = H x - b z (+ c z2) with the start vectors riding on the first pass and <x, y>, |y|^2 on the last, held as
    test_flipflop_fused_entry_points holds them"""
    L, B, logR, mode, amin = SHAPES[3]
    cfg(monkeypatch, B, logR, mode, amin)
    H, arrs, sub, x, ref = _case("mbl", L)
    z, z2 = rand_state(1 << L, seed=91), rand_state(1 << L, seed=92)
    b, c = 0.37, 0.2 - 0.6j
    mat = shell(H, sub)
    assert _on(mat), mat.describe()
    xv, zv, z2v = vec_from(x, mat.swz_right), vec_from(z, mat.swz_left), vec_from(z2, mat.swz_left)
    yv = backend.Vec(mat.M, swz=mat.swz_left)
    tol = tol_for(arrs, x) + 4 * 2.2e-16 * (abs(b) * np.abs(z).max() + abs(c) * np.abs(z2).max())
    dot = (C.c_double * 3)()
    _lib.check(_lib.lib().dnm_mat_mult_lanczos(mat.handle, xv.ptr, yv.ptr, zv.ptr, b, dot, None))
    want = ref - b * z
    assert np.max(np.abs(yv.local_numpy() - want)) <= tol
    nn = np.vdot(want, want).real
    assert abs(complex(dot[0], dot[1]) - np.vdot(x, want)) <= 1e-13 * max(1.0, abs(np.vdot(x, want))) * np.sqrt(x.size)
    assert abs(dot[2] - nn) <= 1e-13 * nn
    _lib.check(_lib.lib().dnm_mat_mult_sub2(mat.handle, xv.ptr, yv.ptr, zv.ptr, b, z2v.ptr, c.real, c.imag, None))
    assert np.max(np.abs(yv.local_numpy() - (ref - b * z + c * z2))) <= tol
    _lib.check(_lib.lib().dnm_mat_mult_sub2(mat.handle, xv.ptr, yv.ptr, zv.ptr, b, None, 0.0, 0.0, None))
    assert np.max(np.abs(yv.local_numpy() - want)) <= tol
    mat.destroy()


def test_tables_on_a_nonzero_rank(monkeypatch):
    """Rank 3 of a 4-rank partition at L = 16, run on this one GPU (exchange = slicing): the rank bits enter the tables
    through DevPass::sign_base"""
    cfg(monkeypatch, 10, 2, 2, 3)
    L, P, r = 16, 4, 3
    H, arrs, sub, x, ref = _case("mbl", L)
    nloc = (1 << L) // P
    Lb = _lib.lib()
    xls = [vec_from(x[q * nloc:(q + 1) * nloc], sub.vec_swizzle) for q in range(P)]
    h = backend.create_mat(*arrs, sub._c(), sub._c(), flags=0, rank=r, nranks=P)
    mat = backend.ShellMat(h, sub._c(), sub._c(), P, r)
    assert _on(mat), mat.describe()
    yl = backend.Vec(nloc, swz=mat.swz_left)
    _lib.check(Lb.dnm_mat_mult_local(mat.handle, xls[r].ptr, yl.ptr, None))
    for i, (p, off, cnt) in enumerate(mat.recvs):
        xr = partner_slice(xls[p], off, cnt)
        _lib.check(Lb.dnm_mat_mult_remote(mat.handle, i, xr.ptr, yl.ptr, None))
    assert np.max(np.abs(yl.local_numpy() - ref[r * nloc:(r + 1) * nloc])) <= tol_for(arrs, x)
    mat.destroy()


@pytest.mark.parametrize("name,L,B", [("cross", 14, 10), ("long_range", 14, 10), ("syk", 12, 8)])
def test_passes_that_keep_their_lists(monkeypatch, name, L, B):
    """More than three outside parts (ZZ couplings across the tile boundary, test_diag_tables.dy_cross), grouped diagonal terms (long_range), table records (SYK):
    the plan says that no pass reads its diagonal from tables, and the product is right."""
    cfg(monkeypatch, B, 2, 2, 3)
    H = {"cross": dy_cross, "long_range": models.long_range, "syk": models.syk}[name](L)
    sub = Full(L=L)
    arrs = marshal(H)
    x = rand_state(1 << L, seed=L)
    ref = orc.matvec(orc_msc(H), orc_sub(sub), orc_sub(sub), x, nthreads=4)
    for flags in (0, _lib.MAT_USE_GLDS):
        mat = shell(H, sub, flags=flags)
        d = mat.describe()
        assert "tiled=1" in d and "diag=1" in d and "diag_tables" not in d, d
        y = mult_numpy(mat, x)
        assert np.max(np.abs(y - ref)) <= tol_for(arrs, x), d
        mat.destroy()
