"""
All <sigmaz_i> and <sigmaz_i sigmaz_j> of a state in one matrix-core pass (csrc/zz_kernels.hip, csrc/gram_tile.h,
csrc/observables.cpp: dnm_zz_moments; backend.zz_moments, computations.sigmaz_correlations).

The reference is numpy on the host: the configurations of the subspace, a sign matrix S~ = (1, s_0, ..., s_{L-1}) from
their bits and S~^T (w S~) with w = |psi|^2.  States with small integer amplitudes make every weight an integer <= 18
and every sum an integer below 2^53: kernel and reference must then agree to the last bit in any summation order.
Random states are held to the bound of a sum of `rows` terms, 2 rows 2^-53 <psi|psi> (once for the kernel, once for the
reference).
"""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest

from dynamite_amd import _lib, backend
from dynamite_amd.computations import sigmaz_correlations
from dynamite_amd.config import config
from dynamite_amd.operators import sigmaz
from dynamite_amd.states import State
from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve, XParity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


# ---- reference ----------------------------------------------------------------------------------------------------
def sign_matrix(states, L):
    """Rows s~(c) = (1, s_0(c), ..., s_{L-1}(c)), s_i = +1 for a clear bit and -1 for a set one."""
    S = np.ones((len(states), L + 1))
    S[:, 1:] = 1.0 - 2.0 * ((np.asarray(states, dtype=np.int64)[:, None] >> np.arange(L)) & 1)
    return S


def reference(sub, w, lo=0, hi=None):
    """M of the rows [lo, hi) of the subspace with the weights w (one per row of the range)."""
    hi = sub.get_dimension() if hi is None else hi
    S = sign_matrix(sub.idx_to_state(np.arange(lo, hi)), sub.L)
    return S.T @ (np.asarray(w, dtype=np.float64)[:, None] * S)


def int_amplitudes(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-3, 4, n) + 1j * rng.integers(-3, 4, n)).astype(np.complex128)


def state_from(sub, amps):
    st = State(subspace=sub)
    lo, hi = st.vec.getOwnershipRange()
    st.vec.set_local_from_numpy(amps[lo:hi])
    st.set_initialized()
    return st


def moments(st):
    return backend.zz_moments(st.vec, st.subspace._to_c())


def tolerance(rows, norm2):
    return 2.0 * rows * 2.0 ** -53 * norm2


def expectation(op, st):
    op.L = st.subspace.L
    op.add_subspace(st.subspace)
    return op.expectation(st)


@pytest.fixture
def small_layout():
    """(6, 4) field split for every SpinConserve subspace with L >= 11, whatever its dimension (test_gpu_sc3.py)."""
    old = (config.sc_layout, config.sc_layout_min_dim)
    config.sc_layout, config.sc_layout_min_dim = (6, 4), 0
    yield
    config.sc_layout, config.sc_layout_min_dim = old


def shuffled_explicit():
    rng = np.random.default_rng(5)
    states = np.unique(rng.integers(0, 1 << 40, 1100, dtype=np.int64))[:1000]
    rng.shuffle(states)
    assert states.size == 1000 and np.any(states[1:] < states[:-1])
    return Explicit(states, L=40)


# ---- 1. convention ------------------------------------------------------------------------------------------------
def test_convention_is_that_of_expectation():
    """mz[i] is what sigmaz(i).expectation gives, zz[i, j] what (sigmaz(i) * sigmaz(j)).expectation gives."""
    L = 6
    st = State(subspace=Full(L=L), state='random', seed=7)
    mz, zz = sigmaz_correlations(st)
    tol = tolerance(1 << L, st.dot(st).real)
    worst = 0.0
    for i in range(L):
        worst = max(worst, abs(mz[i] - expectation(sigmaz(i), st)))
        for j in range(L):
            worst = max(worst, abs(zz[i, j] - expectation(sigmaz(i) * sigmaz(j), st)))
    print("convention: largest deviation %.3e (bound %.3e)" % (worst, tol))
    assert worst <= tol
    # a spin that is up ('U', bit clear) has <sigmaz> = +1
    up = State(subspace=Full(L=L), state='UDUUDU')
    mzu, zzu = up.sigmaz_correlations()
    assert np.array_equal(mzu, [1, -1, 1, 1, -1, 1]) and np.array_equal(zzu, np.outer(mzu, mzu))
    _, conn = up.sigmaz_correlations(connected=True)
    assert np.array_equal(conn, np.zeros((L, L)))


# ---- 2. exact arithmetic ------------------------------------------------------------------------------------------
EXACT = [
    pytest.param(lambda: Full(L=4), 16, id="full4"),
    pytest.param(lambda: Full(L=15), 1 << 15, id="full15"),
    pytest.param(lambda: Full(L=16), 1 << 16, id="full16"),
    pytest.param(lambda: Full(L=20), 1 << 20, id="full20_swizzle16", marks=pytest.mark.default_layout),
    pytest.param(lambda: Parity('even', L=17), 1 << 16, id="parity17_even"),
    pytest.param(lambda: Parity('odd', L=17), 1 << 16, id="parity17_odd"),
    pytest.param(lambda: SpinConserve(16, 8), 12870, id="sc16_8"),
    pytest.param(lambda: SpinConserve(34, 2), 561, id="sc34_2"),
    pytest.param(lambda: SpinConserve(50, 2), 1225, id="sc50_2"),
    pytest.param(lambda: SpinConserve(63, 1), 63, id="sc63_1"),
    pytest.param(shuffled_explicit, 1000, id="explicit40_shuffled"),
]


def check_exact(sub, rows, seed=3):
    assert sub.get_dimension() == rows
    amps = int_amplitudes(rows, seed)
    st = state_from(sub, amps)
    M = moments(st)
    want = reference(sub, amps.real ** 2 + amps.imag ** 2)
    assert M.shape == (sub.L + 1, sub.L + 1) and M.dtype == np.float64
    assert np.array_equal(M, want), np.argwhere(M != want)[:8]
    return st, M


@pytest.mark.parametrize("make,rows", EXACT)
def test_integer_amplitudes_bit_for_bit(make, rows):
    sub = make()
    st, M = check_exact(sub, rows)
    if isinstance(sub, Full) and sub.L == 20:
        assert st.vec.swz == 16          # the production layout: index bits 16-19 folded onto bits 4-7
    if isinstance(sub, SpinConserve):
        assert not st.vec.internal
    mz, zz = sigmaz_correlations(st)
    assert np.array_equal(mz, M[0, 1:]) and np.array_equal(zz, M[1:, 1:])


def test_integer_amplitudes_internal_layout(small_layout):
    """A SpinConserve state in the internal layout goes through reference order."""
    sub = SpinConserve(22, 11)
    st, _ = check_exact(sub, 705432)
    assert st.vec.internal


# ---- 3. XParity ---------------------------------------------------------------------------------------------------
def embed(sub, x):
    """The state in the 2^L product basis; an XParity state as (|c> + sector |~c>) / sqrt 2 on its representatives
    (tests/test_gpu_rdm_sectors.py)."""
    L = sub.L
    full = np.zeros(1 << L, dtype=np.complex128)
    states = np.asarray(sub.idx_to_state(np.arange(sub.get_dimension())))
    if isinstance(sub, XParity):
        full[states] = x / np.sqrt(2)
        full[states ^ ((1 << L) - 1)] = sub.sector * x / np.sqrt(2)
    else:
        full[states] = x
    return full


XPARENTS = [pytest.param(lambda: Full(L=12), id="full12"), pytest.param(lambda: Parity('even', L=12), id="parity12"),
            pytest.param(lambda: SpinConserve(12, 6), id="sc12_6")]


@pytest.mark.parametrize("make", XPARENTS)
def test_xparity(make):
    L = 12
    for sector in ('+', '-'):
        sub = XParity(make(), sector=sector)
        rows = sub.get_dimension()
        amps = int_amplitudes(rows, 21)
        st = state_from(sub, amps)
        mz, zz = sigmaz_correlations(st)
        # the embedded state with its 1 / sqrt 2 taken out: amplitudes sqrt 2 * psi are the integers again, the weights
        # twice those of the state
        full = embed(sub, amps) * np.sqrt(2)
        full = np.rint(full.real) + 1j * np.rint(full.imag)
        assert np.array_equal(np.abs(full) ** 2 > 0, np.abs(embed(sub, amps)) > 0)
        want = reference(Full(L=L), full.real ** 2 + full.imag ** 2)
        assert np.array_equal(2.0 * zz, want[1:, 1:])
        assert np.array_equal(mz, np.zeros(L)) and not np.signbit(mz).any()
        assert np.array_equal(want[0, 1:], np.zeros(L))          # (the embedded state's magnetisations do vanish)
    # a random state against the operator route on the XParity subspace itself
    st = State(subspace=sub, state='random', seed=4)
    mz, zz = sigmaz_correlations(st)
    n = st.dot(st).real
    tol = tolerance(rows, n)
    worst = 0.0
    for i in range(L):
        assert abs(zz[i, i] - n) <= tol
        for j in range(i + 1, L):
            worst = max(worst, abs(zz[i, j] - expectation(sigmaz(i) * sigmaz(j), st)))
    print("xparity: largest deviation %.3e (bound %.3e)" % (worst, tol))
    assert worst <= tol


# ---- 4. planted rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=16), id="full16"),
                                  pytest.param(lambda: SpinConserve(16, 8), id="sc16_8")])
def test_planted_rows(make):
    """One amplitude 1 + 2i in an otherwise empty state: M = 5 s~ s~^T of that row's configuration, wherever the row
    falls -- the tail of the sweep, the hand-round inside a wavefront step, the boundaries of the workgroups' shares."""
    sub = make()
    rows = sub.get_dimension()
    st = State(subspace=sub)
    st.set_initialized()
    for row in sorted({0, 1, 63, 64, 255, 256, 1023, 1024, rows // 2, rows - 2, rows - 1}):
        if not 0 <= row < rows:
            continue
        st.vec.set(0)
        st.vec.array[st.vec.positions(int(row))] = 1 + 2j
        s = sign_matrix([sub.idx_to_state(row)], sub.L)[0]
        M = moments(st)
        assert np.array_equal(M, 5.0 * np.outer(s, s)), row


# ---- 5. random states ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [pytest.param(lambda: Full(L=20), id="full20", marks=pytest.mark.default_layout),
                                  pytest.param(lambda: SpinConserve(16, 8), id="sc16_8")])
def test_random_states(make):
    sub = make()
    rows = sub.get_dimension()
    st = State(subspace=sub, state='random', seed=9)
    M = moments(st)
    amps = st.to_numpy()
    want = reference(sub, amps.real ** 2 + amps.imag ** 2)
    n = want[0, 0]
    tol = tolerance(rows, n)
    err = np.max(np.abs(M - want))
    print("random state, %d rows: largest error %.3e (bound %.3e)" % (rows, err, tol))
    assert err <= tol
    assert np.array_equal(M, M.T)
    assert np.array_equal(np.diag(M), np.full(sub.L + 1, M[0, 0]))
    assert np.array_equal(moments(st), M)


# ---- 6. blocks through the C ABI ----------------------------------------------------------------------------------
def test_blocks_spin_conserve():
    sub = SpinConserve(16, 8)
    st, whole = check_exact(sub, 12870, seed=13)
    x, d = st.vec.array, sub._c()
    total, lo = np.zeros_like(whole), 0
    for n in (1000, 7001, 4869):
        total += backend.zz_moments_block(x[lo:lo + n], d, lo, n)
        lo += n
    assert lo == 12870 and np.array_equal(total, whole)


@pytest.mark.default_layout
def test_blocks_full_swizzled():
    """The two halves of a Full L = 20 state as two ranks would hold them: each half a block of its own in the
    swizzled layout (the swizzle acts on the block's own positions), with its own first row."""
    import torch
    sub = Full(L=20)
    st, whole = check_exact(sub, 1 << 20, seed=17)
    S = st.vec.swz
    assert S == 16
    nat, half = st.vec.local_natural(), 1 << 19
    total = np.zeros_like(whole)
    for h in range(2):
        blk = torch.empty(half, dtype=nat.dtype, device=nat.device)
        _lib.check(_lib.lib().dnm_vec_swizzle_copy(C.c_void_p(blk.data_ptr()),
                                                   C.c_void_p(nat[h * half:(h + 1) * half].data_ptr()), half, S,
                                                   backend._stream()))
        total += backend.zz_moments_block(blk, sub._c(), h * half, half)
    assert np.array_equal(total, whole)


# ---- 7. two ranks -------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK=str(rank), RANK=str(rank),
                      WORLD_SIZE=str(world))
    import faulthandler
    faulthandler.dump_traceback_later(int(os.environ.get("DNM_TEST_HANG_S", "600")), exit=True)
    import datetime
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=900))
    # small vectors: a swizzle shift that really permutes them (conftest's choice for the one-process GPU tests)
    config.vec_swizzle = int(os.environ.get("DNM_TEST_SWZ", "6"))
    config.L = 12
    config._initialize()
    for sub in (Full(L=12), SpinConserve(12, 6)):
        rows = sub.get_dimension()
        amps = int_amplitudes(rows, 31)
        st = state_from(sub, amps)
        assert st.vec.rows == rows // world
        want = reference(sub, amps.real ** 2 + amps.imag ** 2)
        assert np.array_equal(moments(st), want), "rank %d, %r" % (rank, sub)
        mz, zz = sigmaz_correlations(st)
        assert np.array_equal(mz, want[0, 1:]) and np.array_equal(zz, want[1:, 1:])
    dist.barrier()
    faulthandler.cancel_dump_traceback_later()
    open(os.path.join(out_dir, "ok_%d" % rank), "w").write("ok")
    dist.destroy_process_group()


def test_two_ranks_one_gpu(tmp_path):
    """Each rank sweeps its block, the sums are added over the ranks (gloo staging: RCCL refuses two ranks on one
    device) and every rank gets the whole result."""
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert all(os.path.exists(os.path.join(str(tmp_path), "ok_%d" % r)) for r in range(2))
