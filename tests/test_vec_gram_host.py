"""
The Gram matrix of many vectors, host side (dnm_vec_gram_plan, dnm_vec_gram; backend.vec_gram_plan -- no GPU needed).

The plan is pinned exactly: the number of workgroups fixes the order of the sums and with it the bits of a result, the
panel fixes the time.  The sweep keeps the bond-swap sweep's workgroups -- one per 2^9 rows, at most 1024 and at least
one -- and its layout of the panel and the partial tiles, but has a panel rule of its own, measured against the
inherited one (docs/lab/state_gram.md): 2^7 rows at one and two tile rows, 2^6 at three and four.  vgram_rule is that
sibling of gram_rule (test_gram_plan_host.py), written out here once more.  Every refusal happens before any device
call: the pointers handed over here are never followed.
"""
import ctypes as C

import numpy as np
import pytest

from dynamite_amd import _lib, backend

from test_gram_plan_host import LDS_BUDGET, MAX_WG, gram_rule

NVEC = (1, 16, 17, 32, 33, 48, 49, 64)
ROWS = (0, 1, 127, 128, 129, 511, 512, 513, 1 << 19, (1 << 19) + 515, 1 << 30, 1 << 40)
PANEL_LOG2 = {1: 7, 2: 7, 3: 6, 4: 6}      # by tile rows


def vgram_rule(nvec, n):
    """(tile rows, log2 of the panel's rows, workgroups, bytes of LDS, bytes of partial tiles)"""
    nb = -(-nvec // 16)
    B = PANEL_LOG2[nb]
    lds = (16 * nb + 1) * 16 << B
    nacc = nb * (nb + 1) // 2 + nb * nb
    assert nacc * 256 * 8 <= lds <= LDS_BUDGET       # the wavefronts' sum takes the panel's place
    npanels = (n + (1 << B) - 1) >> B
    nwg = max(1, min((n + 511) >> 9, npanels, MAX_WG))
    return nb, B, nwg, lds, nwg * nacc * 256 * 8


def test_rule_is_gram_rule_but_for_the_panel():
    """Tile rows and, where the workgroups are as many, the partial tiles are those of the inherited rule."""
    for nvec in NVEC:
        for n in ROWS:
            mine, theirs = vgram_rule(nvec, n), gram_rule(nvec, n, 0, lambda npanels: (n + 511) >> 9)
            assert mine[0] == theirs[0] and mine[2] == theirs[2] and mine[4] == theirs[4] and mine[1] <= theirs[1]


@pytest.mark.parametrize("nvec", NVEC)
def test_plan(nvec):
    for n in ROWS:
        assert backend.vec_gram_plan(nvec, n) == vgram_rule(nvec, n), n


def test_plan_by_hand():
    """The rule itself at a few points, so that a slip common to gram_rule and the library would show."""
    assert backend.vec_gram_plan(64, 1 << 26) == (4, 6, 1024, 65 * 16 * 64, 1024 * 26 * 2048)
    assert backend.vec_gram_plan(48, 513) == (3, 6, 2, 49 * 16 * 64, 2 * 15 * 2048)
    assert backend.vec_gram_plan(16, 513) == (1, 7, 2, 17 * 16 * 128, 2 * 2 * 2048)
    assert backend.vec_gram_plan(17, 0) == (2, 7, 1, 33 * 16 * 128, 7 * 2048)


def test_plan_outputs_are_optional():
    assert _lib.lib().dnm_vec_gram_plan(5, 1000, None, None, None, None, None) == 0


def _refused(ptrs, n, nvec=None, give_xs=True, give_out=True):
    """dnm_vec_gram with pointers that are never followed: the call is refused first."""
    out = np.full(2 * 65 * 65, 7.0)
    xs = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
    rc = _lib.lib().dnm_vec_gram(xs if give_xs else None, len(ptrs) if nvec is None else nvec, n,
                                 _lib.pf64(out) if give_out else None, None)
    assert rc != 0
    assert np.all(out == 7.0)
    return _lib.lib().dnm_last_error().decode()


def test_refusals():
    good = [0x1000 + 0x100 * c for c in range(64)]
    assert "0 vectors (1 to 64 in one call)" in _refused([], 8, nvec=0)
    assert "65 vectors (1 to 64 in one call)" in _refused(good, 8, nvec=65)
    assert "vectors of -1 elements" in _refused(good[:3], -1)
    assert "null argument" in _refused(good[:3], 8, give_xs=False)
    assert "null argument" in _refused(good[:3], 8, give_out=False)
    assert "vector 1 is a null pointer" in _refused([0x1000, None, 0x3000], 8)
    msg = _refused([0x1000, 0x2000, 0x3008], 8)
    assert "vector 2" in msg and "not 16-byte aligned" in msg
    assert "not 16-byte aligned" in _refused([0x1008], 0)
    with pytest.raises(_lib.BackendError, match="65 vectors"):
        backend.vec_gram_plan(65, 8)
    with pytest.raises(_lib.BackendError, match="0 vectors"):
        backend.vec_gram_plan(0, 8)
    with pytest.raises(_lib.BackendError, match="-5 elements"):
        backend.vec_gram_plan(3, -5)


@pytest.mark.parametrize("nvec", (1, 5, 64))
def test_empty_vectors_give_zeros(nvec):
    """n == 0: a zero matrix without a launch, null elements allowed."""
    out = np.full(2 * nvec * nvec + 2, 7.0)
    xs = (C.c_void_p * nvec)(*([None] * nvec))
    assert _lib.lib().dnm_vec_gram(xs, nvec, 0, _lib.pf64(out), None) == 0
    assert np.all(out[:2 * nvec * nvec] == 0.0) and np.all(out[2 * nvec * nvec:] == 7.0)
