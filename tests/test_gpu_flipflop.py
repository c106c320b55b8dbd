"""
Flip-flop records (dynamite_amd/csrc/plan.h: DevFlip) on the GPU: the tiled multiply of the chains whose bonds run as
such records against the CPU oracle, at the smallest shapes at which each record class exists, with the records on and
off (DNM_FLIPFLOP) and on both tile staging paths; and the fused entry points (dnm_mat_mult_lanczos, dnm_mat_mult_sub2)
on the same plans.
"""
import ctypes as C

import numpy as np
import pytest

from dynamite_amd import _lib, backend, models
from dynamite_amd.subspaces import Full
from oracle import oracle as orc
from gpu_util import marshal, orc_msc, orc_sub, shell, vec_from, mult_numpy, rand_state
from test_flipflop import CHAINS, NO_ZZ, count_flips
from test_gpu_matvec import tol_for, cfg

pytestmark = pytest.mark.gpu

# L = 12 with one tile of 2^10: tile records only (thread bits and k bits); L = 20: a window pass and a contiguous pass,
# gathered records with both bits outside the tile and across its boundary (on a thread bit and on a k bit)
SHAPES = [(12, 10, 2, 2, 3), (20, 10, 4, 2, 4), (20, 11, 3, 2, 3), (20, 12, 3, 2, 4)]
_REF = {}


def _case(name, L):
    """operator, its arrays, the input and the oracle's product: once per (chain, size)"""
    if (name, L) not in _REF:
        H = CHAINS[name](L)
        sub = Full(L=L)
        x = rand_state(1 << L, seed=L)
        ref = orc.matvec(orc_msc(H), orc_sub(sub), orc_sub(sub), x, nthreads=4)
        ref.setflags(write=False)
        _REF[(name, L)] = (H, marshal(H), sub, x, ref)
    return _REF[(name, L)]


def _classes(mat):
    """flip-flop records the handle runs on"""
    vals = [C.c_int() for _ in range(6)]
    _lib.check(_lib.lib().dnm_mat_plan_counts(mat.handle, *[C.byref(v) for v in vals]))
    return count_flips(mat.handle, vals[0].value)


@pytest.mark.parametrize("L,B,logR,mode,amin", SHAPES)
@pytest.mark.parametrize("name", sorted(CHAINS))
def test_flipflop_vs_oracle(monkeypatch, name, L, B, logR, mode, amin):
    cfg(monkeypatch, B, logR, mode, amin)
    H, arrs, sub, x, ref = _case(name, L)
    for knob in ("1", "0"):
        monkeypatch.setenv("DNM_FLIPFLOP", knob)
        for flags in (0, _lib.MAT_USE_GLDS):
            mat = shell(H, sub, flags=flags)
            assert "tiled=1" in mat.describe()
            assert _classes(mat) == (L - 1 if knob == "1" else 0), mat.describe()
            y = mult_numpy(mat, x)
            err = np.max(np.abs(y - ref))
            print(name, L, B, logR, "flipflop", knob, "flags", flags, "err %.3e tol %.3e" % (err, tol_for(arrs, x)))
            assert err <= tol_for(arrs, x), mat.describe()
            mat.destroy()


@pytest.mark.parametrize("L,B,logR,mode,amin", SHAPES)
@pytest.mark.parametrize("name", ["mbl", "aniso"])
def test_flipflop_fused_entry_points(monkeypatch, name, L, B, logR, mode, amin):
    """y = H x - b z (+ c z2) with the start vectors riding on the first pass and <x, y>, |y|^2 on the last"""
    cfg(monkeypatch, B, logR, mode, amin)
    H, arrs, sub, x, ref = _case(name, L)
    z, z2 = rand_state(1 << L, seed=91), rand_state(1 << L, seed=92)
    b, c = 0.37, 0.2 - 0.6j
    mat = shell(H, sub)
    assert _classes(mat) == L - 1
    xv, zv, z2v = vec_from(x, mat.swz_right), vec_from(z, mat.swz_left), vec_from(z2, mat.swz_left)
    yv = backend.Vec(mat.M, swz=mat.swz_left)
    # the product at tol_for; the start vectors add their own roundings: b z is one multiply, c z2 two fused
    # multiply-adds per part, and each is added to a partial sum once -- at most four roundings of that size in all
    tol = tol_for(arrs, x) + 4 * 2.2e-16 * (abs(b) * np.abs(z).max() + abs(c) * np.abs(z2).max())
    dot = (C.c_double * 3)()
    _lib.check(_lib.lib().dnm_mat_mult_lanczos(mat.handle, xv.ptr, yv.ptr, zv.ptr, b, dot, None))
    want = ref - b * z
    y = yv.local_numpy()
    assert np.max(np.abs(y - want)) <= tol
    nn = np.vdot(want, want).real
    assert abs(complex(dot[0], dot[1]) - np.vdot(x, want)) <= 1e-13 * max(1.0, abs(np.vdot(x, want))) * np.sqrt(x.size)
    assert abs(dot[2] - nn) <= 1e-13 * nn
    _lib.check(_lib.lib().dnm_mat_mult_sub2(mat.handle, xv.ptr, yv.ptr, zv.ptr, b, z2v.ptr, c.real, c.imag, None))
    assert np.max(np.abs(yv.local_numpy() - (ref - b * z + c * z2))) <= tol
    _lib.check(_lib.lib().dnm_mat_mult_sub2(mat.handle, xv.ptr, yv.ptr, zv.ptr, b, None, 0.0, 0.0, None))
    assert np.max(np.abs(yv.local_numpy() - want)) <= tol
    mat.destroy()


@pytest.mark.parametrize("name,L,B,logR,mode,amin", [("xy_field", 12, 10, 2, 2, 3), ("xy_field", 20, 12, 3, 2, 4),
                                                     ("long_range_xy", 14, 8, 2, 2, 3), ("long_range_xy", 14, 10, 2, 2, 3),
                                                     ("long_range_xy", 16, 12, 2, 2, 4)])
def test_flipflop_bonds_without_zz(monkeypatch, name, L, B, logR, mode, amin):
    """Bonds a (XX + YY) with no ZZ term on their pair (an XY chain in a field, XY couplings between all pairs): their
    gathered form runs as flip-flop records, their tile form stays generic, and the passes launch."""
    cfg(monkeypatch, B, logR, mode, amin)
    key = (name, L)
    if key not in _REF:
        H = NO_ZZ[name](L)
        sub = Full(L=L)
        x = rand_state(1 << L, seed=L)
        ref = orc.matvec(orc_msc(H), orc_sub(sub), orc_sub(sub), x, nthreads=4)
        ref.setflags(write=False)
        _REF[key] = (H, marshal(H), sub, x, ref)
    H, arrs, sub, x, ref = _REF[key]
    for knob in ("1", "0"):
        monkeypatch.setenv("DNM_FLIPFLOP", knob)
        for flags in (0, _lib.MAT_USE_GLDS):
            mat = shell(H, sub, flags=flags)
            assert "tiled=1" in mat.describe()
            n = _classes(mat)
            assert (0 < n < len(arrs[0]) - 1) if knob == "1" else n == 0, mat.describe()
            y = mult_numpy(mat, x)
            err = np.max(np.abs(y - ref))
            print(name, L, B, logR, "flipflop", knob, "flags", flags, "records", n, "err %.3e tol %.3e" % (err, tol_for(arrs, x)))
            assert err <= tol_for(arrs, x), mat.describe()
            mat.destroy()


@pytest.mark.parametrize("name", ["mbl", "aniso"])
def test_flipflop_ranges_of_one_pass(monkeypatch, name):
    """dnm_mat_mult_local_part on a pass with flip-flop records: four ranges of the workgroups of the one local pass
    (L = 14, one tile of 2^10, everything else gathered: 13 records in all four classes, 7 / 2 / 3 / 1 in the order of
    the FL_* ranges -- the smallest chain that has all four) write, bit for bit, what the whole launch writes -- same kernel, same arithmetic per row, only the grid and the first workgroup
    differ -- and leave no row out."""
    L = 14
    cfg(monkeypatch, 10, 2, 1, 3)
    H, arrs, sub, x, ref = _case(name, L)
    for knob in ("1", "0"):
        monkeypatch.setenv("DNM_FLIPFLOP", knob)
        for flags in (0, _lib.MAT_USE_GLDS):
            mat = shell(H, sub, flags=flags)
            vals = [C.c_int() for _ in range(6)]
            _lib.check(_lib.lib().dnm_mat_plan_counts(mat.handle, *[C.byref(v) for v in vals]))
            assert vals[0].value == 1 and vals[2].value == 1, mat.describe()
            assert _classes(mat) == (13 if knob == "1" else 0), mat.describe()
            xv = vec_from(x, mat.swz_right)
            yw, yp = backend.Vec(mat.M, swz=mat.swz_left), backend.Vec(mat.M, swz=mat.swz_left)
            yw.set_local_from_numpy(np.full(1 << L, np.nan + 1j * np.nan))
            yp.set_local_from_numpy(np.full(1 << L, np.nan + 1j * np.nan))
            _lib.check(_lib.lib().dnm_mat_mult_local(mat.handle, xv.ptr, yw.ptr, None))
            for part in range(4):
                _lib.check(_lib.lib().dnm_mat_mult_local_part(mat.handle, xv.ptr, yp.ptr, part, 4, None))
            y_whole, y_parts = yw.local_numpy(), yp.local_numpy()
            assert np.array_equal(y_parts, y_whole), mat.describe()
            err = np.max(np.abs(y_whole - ref))
            print(name, "flipflop", knob, "flags", flags, "err %.3e tol %.3e" % (err, tol_for(arrs, x)))
            assert err <= tol_for(arrs, x), mat.describe()
            mat.destroy()
