"""
The tables of the SpinConserve passes through the C ABI (dnm_mat_export_sc3) on host-only handles -- no GPU needed: the
hop counts the kernels are handed are the chooser's, and the hop records give back the masks the handle was built from.
(Every table against its definition: tests/test_sc3_tables_host.py.)
"""
import ctypes as C

import numpy as np

from dynamite_amd import _lib, backend, models, msc_tools
from dynamite_amd.subspaces import Full, SpinConserve, XParity


def _handle(msc, L, k, xparity):
    masks, offs = msc_tools.get_mask_offsets(msc)
    d = _lib.Subspace.from_buffer_copy(SpinConserve(L, k)._c())
    d.vec_swizzle = 14 | (10 << 8)
    perm, counts = backend.choose_site_perm(masks, L, 14, 10, fix_top=xparity)
    dp = backend.with_site_perm(d, perm)
    h = backend.create_mat(masks, offs, msc['signs'], msc['coeffs'], dp, dp, xparity, _lib.MAT_HOST_ONLY, 0, 1)
    return h, masks, perm, counts


def _reduced(H):
    H.establish_L()
    H.reduce_msc()
    return H.msc


def test_exported_hops_are_the_operator():
    kag = _reduced(models.kagome("30"))
    cases = [("kagome30", kag, 30, False),
             ("kagome30 xparity", XParity(SpinConserve(30, 15), '-').reduce_msc(kag), 30, True),
             ("long range 28", _reduced(models.bench_long_range(28)), 28, False)]
    for name, msc, L, xparity in cases:
        h, masks, perm, counts = _handle(msc, L, L // 2, xparity)
        op = backend.sc3_op_fields(h)
        live = sorted(int(m) for m in masks.tolist() if m and bin(m).count('1') % 2 == 0)
        to_ref = np.argsort(perm)                       # layout bit -> the spin handed in
        assert op["tiled"] and op["sym"] and not op["real"], name
        if op["graph"]:
            # [Lo, W, T, Lo-W, Lo-T, W-T]: in LDS where both spins share Lo or W, gathered by the lo pass where one is in Lo
            assert [op["nldsA"], op["ngatA"], op["nldsB"], op["ngatB"]] == \
                [counts[0], counts[3] + counts[4], counts[1], counts[2] + counts[5]], name
            hops = np.frombuffer(backend.export_sc3(h, "hops"), dtype=np.int32).reshape(-1, 16)
            assert len(hops) == len(live)
            got = []
            for mT, mW, mLo in hops[:, :3].astype(np.uint32).tolist():
                m = (mT << 24) | (mW << 14) | mLo
                got.append(sum(1 << int(to_ref[b]) for b in range(L) if (m >> b) & 1))
            assert sorted(got) == live, name
        else:
            # a chain: the bonds it has, the two that its passes gather across the fields' borders
            assert name == "long range 28" and np.array_equal(perm, np.arange(L))
            assert sorted(3 << b for b in range(L - 1) if (op["present"] >> b) & 1) == live
            assert bin(op["bondsA"]).count('1') == counts[3] and bin(op["bondsB"]).count('1') == counts[2] + counts[5]
            assert len(backend.export_sc3(h, "hops")) == 0 and op["diag_mode"] == 1
        _lib.check(_lib.lib().dnm_mat_destroy(h))
    # any other handle has no such tables
    Hc = _reduced(models.kagome("12"))
    masks, offs = msc_tools.get_mask_offsets(Hc)
    f = Full()
    f.L = 12
    h = backend.create_mat(masks, offs, Hc['signs'], Hc['coeffs'], f._c(), f._c(), False, _lib.MAT_HOST_ONLY, 0, 1)
    n = C.c_size_t()
    assert _lib.lib().dnm_mat_export_sc3(h, b"op", None, 0, C.byref(n)) != 0
    _lib.check(_lib.lib().dnm_mat_destroy(h))
