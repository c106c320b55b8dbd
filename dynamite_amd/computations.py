"""
``evolve`` and ``eigsolve``: the Krylov callers of the hot path, with the
signatures, defaults and error behaviour of ``dynamite.computations``
(reference ``src/dynamite/computations.py:10-126, 128-292, 511-534``).  The
solvers themselves are native (``dnm_expm_multiply`` / ``dnm_eigsolve``).
"""
import ctypes as C
import warnings

import numpy as np

from . import _lib
from .backend import _stream, _dist
from .config import config, knob


class ConvergenceError(Exception):
    pass


class MaxIterationsError(ConvergenceError):
    pass


def _hooks(mat, keep):
    """Distributed hooks for the native solvers: the partitioned multiply and
    the small all-reduces run through torch.distributed (RCCL)."""
    d = _dist()
    if d is None:
        return None
    import torch
    from .backend import Vec, RawVec
    h = mat.native_hooks()          # the library's own communicator: every solver step stays native
    if h is not None:
        keep.append(h)
        return h

    def mult(ctx, xp, yp):
        try:
            n = mat.n_local
            # wrap raw device pointers as Vec views without copying
            if mat.real_packed:
                x, y = RawVec(_tensor_from_ptr(xp, n), mat.swz_right), RawVec(_tensor_from_ptr(yp, n), mat.swz_left)
            else:
                x = Vec(mat.N, array=_tensor_from_ptr(xp, n), swz=mat.swz_right, sub_c=mat._keep[1])
                y = Vec(mat.M, array=_tensor_from_ptr(yp, n), swz=mat.swz_left, sub_c=mat._keep[0])
            mat.mult(x, y)
            return 0
        except Exception as e:   # pragma: no cover
            print('mult hook failed:', e)
            return 1

    def red(op):
        def f(ctx, buf, n):
            try:
                arr = np.ctypeslib.as_array(buf, shape=(n,))
                t = torch.tensor(arr, dtype=torch.float64, device=config.device)
                d.all_reduce(t, op=op)
                arr[:] = t.cpu().numpy()
                return 0
            except Exception as e:   # pragma: no cover
                print('allreduce hook failed:', e)
                return 1
        return f

    h = _lib.Hooks()
    h.ctx = None
    h.mult = _lib.MULT_FN(mult)
    h.allreduce_sum = _lib.REDUCE_FN(red(d.ReduceOp.SUM))
    h.allreduce_max = _lib.REDUCE_FN(red(d.ReduceOp.MAX))
    keep.append(h)
    return h


def _min_over_ranks(*vals):
    """The smallest of each value over the ranks (decisions taken from free device memory must agree)."""
    d = _dist()
    if d is None:
        return vals if len(vals) > 1 else vals[0]
    import torch
    t = torch.tensor([float(v) for v in vals], dtype=torch.float64, device=config.device)
    d.all_reduce(t, op=d.ReduceOp.MIN)
    out = tuple(int(v) for v in t.tolist())
    return out if len(out) > 1 else out[0]


def _tensor_from_ptr(ptr, n):
    """torch complex128 tensor aliasing n amplitudes at a raw device pointer."""
    import torch

    class _W:
        pass
    w = _W()
    w.__cuda_array_interface__ = {'shape': (2 * n,), 'typestr': '<f8', 'data': (int(ptr), False),
                                  'version': 2}
    return torch.as_tensor(w, device=config.device).view(torch.complex128)


def _adopt(mat, state, result):
    """The vectors of ``state`` and ``result`` in the layout ``mat`` works in: where it differs from theirs (a
    relabelled SpinConserve layout, backend._relabelled) the state is converted once and keeps the new layout, the
    result gets a fresh vector in it.  Returns (input Vec, result Vec)."""
    state._vec = mat.vec_in(state.vec)
    if result is not state:
        result._vec = mat.vec_out(result.vec)
    return state.vec, result.vec


def _solver_mat(H, subspace, real):
    """The operator on the partition made for the exchange (Operator.get_solver_mat) if every rank has one, else None."""
    if not config.sc_solver_partition or not H.solver_partition_applies(subspace):
        return None         # (the same answer on every rank: no collective)
    sm = H.get_solver_mat(subspace, real)
    return sm if _min_over_ranks(0 if sm is None else 1) == 1 else None


class _OnSolverPartition:
    """x and y of a solve on the partition made for the exchange: the input state's share moves there block by block
    (backend.reorder_blocks: one vector's worth of traffic, where every multiply of the solve saves about that much --
    SpinConserve(36,18) on 8 ranks: 42 -> 14 GiB on the busiest rank), the result moves back into the State."""

    def __init__(self, sm, xin, yout):
        import torch
        from . import backend
        self.sm, self.yout = sm, yout
        self.x = backend.reorder_blocks(xin.array, xin.sub_c, sm._keep[1])
        self.y = torch.empty_like(self.x)
        self.xptr, self.yptr = C.c_void_p(self.x.data_ptr()), C.c_void_p(self.y.data_ptr())

    @staticmethod
    def applies(sm, xin, yout):
        return (sm is not None and xin.internal and yout.internal and not xin.half and not yout.half
                and xin.perm is None and yout.perm is None
                and (xin.swz & 0xffff) == (yout.swz & 0xffff) == (sm.swz_right & 0xffff))

    def finish(self):
        from . import backend
        self.x = None
        self.yout.array.copy_(backend.reorder_blocks(self.y, self.sm._keep[1], self.yout.sub_c))
        self.y = None


def evolve(H, state, t, result=None, tol=None, ncv=None, algo=None, max_its=None):
    r"""result = exp(-i H t) state   (computations.py:10-126)."""
    state.assert_initialized()
    config._initialize()
    H.establish_L()
    if not H.has_subspace(state.subspace, state.subspace):
        raise ValueError('Hamiltonian and state are defined on different subspaces.')
    if result is None:
        from .states import State
        result = State(L=H.L, subspace=state.subspace)
    elif state.subspace != result.subspace:
        raise ValueError('input and result states are on different subspaces.')
    if algo not in (None, 'expokit', 'krylov', 'chebyshev', 'exact'):
        raise ValueError("algo must be 'expokit', 'krylov', 'chebyshev' or 'exact'")
    if algo == 'exact':
        return _evolve_exact(H, state, t, result)
    if t == 0.0:
        state.copy(result)
        return result
    if algo == 'chebyshev':
        return _evolve_chebyshev(H, state, t, result, tol)

    scale = -1j * complex(t)
    mat = H.get_mat(subspaces=(state.subspace, state.subspace))
    keep = []
    hooks = _hooks(mat, keep)
    stats = _lib.SolverStats()
    import torch
    # (an operator on a bond graph works in a relabelled layout of its own: the states adopt it, as in Operator.dot)
    xin, yout = _adopt(mat, state, result)
    mat.check_layout(xin, yout)
    # several ranks, SpinConserve in the internal layout: the iteration runs on the partition made for the exchange
    sm = _solver_mat(H, state.subspace, False)
    side = None
    if _OnSolverPartition.applies(sm, xin, yout):
        side = _OnSolverPartition(sm, xin, yout)
        mat = sm
        hooks = _hooks(mat, keep)
        xptr, yptr = side.xptr, side.yptr
    else:
        xptr, yptr = xin.ptr, yout.ptr
    evolve.last_mat = mat
    mat.prepare_exchange(state.vec.array)
    free, _ = torch.cuda.mem_get_info()
    if free < 34 * 16 * mat.n_local:      # the default basis would not fit: hand torch's cached blocks back first
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
    # a Krylov basis of fewer than ~10 vectors needs many restarts; for real times the Chebyshev recurrence does
    # the same job with four work vectors
    cached = C.c_size_t()
    _lib.check(_lib.lib().dnm_workspace_bytes(C.byref(cached)))
    fit = int((free * 0.9 + cached.value) // (16 * mat.n_local)) - 2
    fit, free = _min_over_ranks(fit, free)        # Krylov or Chebyshev, and the work limit: the same on every rank
    if ncv is None and fit < 10:
        if complex(t).imag == 0.0 and fit >= 2:
            warnings.warn('evolve: only %d Krylov vectors of %.1f GiB fit in device memory; using '
                          "algo='chebyshev' (4 work vectors)" % (max(fit, 0), 16 * mat.n_local / 2 ** 30),
                          stacklevel=2)
            side = None
            return _evolve_chebyshev(H, state, t, result, tol)
        if fit < 3:
            raise RuntimeError('not enough device memory for a Krylov basis: %d vectors of %.1f GiB fit'
                               % (max(fit, 0), 16 * mat.n_local / 2 ** 30))
    _lib.check(_lib.lib().dnm_expm_multiply(
        mat.handle, xptr, yptr, mat.n_local, scale.real, scale.imag,
        0.0 if tol is None else float(tol), 0 if ncv is None else int(ncv),
        # an explicit algo='krylov' / 'expokit' keeps the Krylov scheme to the end (the driver hands the rest of a
        # real-time interval to the Chebyshev expansion only under all-default parameters)
        (100 if algo is not None else 0) if max_its is None else int(max_its), int(free * 0.9),
        C.byref(hooks) if hooks is not None else None, C.byref(stats), _stream()))
    evolve.last_stats = {'reason': stats.reason, 'its': stats.its, 'matvecs': stats.matvecs,
                         'err_est': stats.err_est}
    # converged-reason mapping of computations.py:114-122
    if stats.reason == _lib.DIVERGED_ITS:
        raise MaxIterationsError('solver reached maximum number of iterations without '
                                 'converging. perhaps try increasing the max iterations with '
                                 'the max_its argument.')
    elif stats.reason == _lib.DIVERGED_BREAKDOWN:
        raise ConvergenceError('solver failed to converge with MFN_DIVERGED_BREAKDOWN.')
    elif stats.reason <= 0:
        raise ConvergenceError('solver failed to converge.')
    if side is not None:
        side.finish()
    result.set_initialized()
    return result


evolve.last_stats = None
evolve.last_mat = None            # the handle the last call multiplied with


def _evolve_chebyshev(H, state, t, result, tol):
    """``algo='chebyshev'`` (not in the reference): the Chebyshev expansion of exp(-iHt) for real t -- one
    multiply and two thirds of a vector sweep per term, four work vectors, no Krylov basis.  Needs about
    ||H||_inf t + 6 (||H||_inf t)^(1/3) + 10 multiplies."""
    if complex(t).imag != 0.0:
        raise ValueError("algo='chebyshev' needs a real time t (use the default Krylov algorithm otherwise)")
    mat = H.get_mat(subspaces=(state.subspace, state.subspace))
    keep = []
    hooks = _hooks(mat, keep)
    stats = _lib.SolverStats()
    xin, yout = _adopt(mat, state, result)
    mat.check_layout(xin, yout)
    sm = _solver_mat(H, state.subspace, False)
    side = None
    xptr, yptr = xin.ptr, yout.ptr
    if _OnSolverPartition.applies(sm, xin, yout):
        side = _OnSolverPartition(sm, xin, yout)
        mat = sm
        hooks = _hooks(mat, keep)
        xptr, yptr = side.xptr, side.yptr
    evolve.last_mat = mat
    mat.prepare_exchange(state.vec.array)
    _lib.check(_lib.lib().dnm_expm_chebyshev(
        mat.handle, xptr, yptr, mat.n_local, float(complex(t).real),
        0.0 if tol is None else float(tol), C.byref(hooks) if hooks is not None else None, C.byref(stats),
        _stream()))
    evolve.last_stats = {'reason': stats.reason, 'its': stats.its, 'matvecs': stats.matvecs,
                         'err_est': stats.err_est}
    if stats.reason <= 0:
        raise ConvergenceError('solver failed to converge.')
    if side is not None:
        side.finish()
    result.set_initialized()
    return result


def product_operator_fields(H):
    """Whether the operator ``H`` is one that ``evolve(algo='exact')`` serves, from its terms on the host:
    ``(kind, a, c0)`` with ``kind`` = ``'diagonal'`` (every mask is 0: a function of the sigma-z alone),
    ``'single-site'`` (a sum over sites of h_j = a_x sigmax_j + a_y sigmay_j + a_z sigmaz_j plus a constant: every mask
    is 0 or one bit, every sign is 0 or one bit, the mask's bit where the mask is set) or None (anything else).  For
    ``'single-site'`` ``a`` is the complex array (L, 3) of the fields (a_x, a_y, a_z) and ``c0`` the constant; a
    diagonal operator is ``'diagonal'`` even where it is a sum of sigma-z fields, and then ``a`` is None."""
    H.establish_L()
    H.reduce_msc()
    msc = H.msc
    masks = np.asarray(msc['masks'], dtype=np.int64)
    signs = np.asarray(msc['signs'], dtype=np.int64)
    if not masks.any():
        return 'diagonal', None, 0j
    one_bit = lambda v: (v & (v - 1)) == 0                    # (0 counts)
    if not (one_bit(masks).all() and one_bit(signs).all() and np.all((masks == 0) | (signs == 0) | (signs == masks))):
        return None, None, 0j
    a = np.zeros((H.L, 3), dtype=np.complex128)
    c0 = 0j
    for mask, sign, coeff in zip(masks.tolist(), signs.tolist(), np.asarray(msc['coeffs']).tolist()):
        if mask == 0 and sign == 0:
            c0 += coeff
        elif mask == 0:
            a[sign.bit_length() - 1, 2] += coeff              # sigmaz_j = (0, 1 << j, 1)
        elif sign == 0:
            a[mask.bit_length() - 1, 0] += coeff              # sigmax_j = (1 << j, 0, 1)
        else:
            a[mask.bit_length() - 1, 1] += coeff / 1j         # sigmay_j = (1 << j, 1 << j, i)
    return 'single-site', a, c0


def site_exponentials(a, t):
    """U_j = exp(-i t h_j) for h_j = a_j . sigma, the fields ``a`` an array (L, 3) and ``t`` real or complex: complex
    array (L, 2, 2) of cos(t |a|) - i sin(t |a|) (a . sigma) / |a|, with |a| = sqrt(a . a) -- the norm of real fields;
    |a| = 0 gives the identity exactly (for complex fields with a . a = 0, 1 - i t a . sigma)."""
    a = np.asarray(a, dtype=np.complex128).reshape(-1, 3)
    t = complex(t)
    out = np.empty((a.shape[0], 2, 2), dtype=np.complex128)
    for j, (ax, ay, az) in enumerate(a):
        if ax == 0 and ay == 0 and az == 0:
            out[j] = np.eye(2)
            continue
        if ax.imag == 0 and ay.imag == 0 and az.imag == 0:
            th = float(np.sqrt(ax.real ** 2 + ay.real ** 2 + az.real ** 2))
        else:
            th = np.sqrt(ax * ax + ay * ay + az * az)
        if th == 0:
            c, s_over = 1.0, t                                # sin(t th) / th -> t
        elif t.imag == 0 and np.imag(th) == 0:
            c, s_over = np.cos(t.real * th), np.sin(t.real * th) / th
        else:
            c, s_over = np.cos(t * th), np.sin(t * th) / th
        out[j] = [[c - 1j * s_over * az, -1j * s_over * (ax - 1j * ay)],
                  [-1j * s_over * (ax + 1j * ay), c + 1j * s_over * az]]
    return out


_EXACT_STATS = {'reason': _lib.CONVERGED_TOL, 'its': 0, 'matvecs': 0, 'err_est': 0.0}


def _evolve_exact(H, state, t, result):
    """``algo='exact'`` (not in the reference): exp(-iHt) of a diagonal operator -- an element-wise phase, on any subspace
    (``backend.expm_diagonal``) -- or of a sum of single-site operators -- a product of single-site rotations on the Full
    space (``backend.site_ops_apply``) -- in one to four streaming passes, with no multiply and no tolerance; ``t`` may
    be complex.  Anything else raises ``ValueError``."""
    from . import backend
    from .subspaces import Full
    kind, a, c0 = product_operator_fields(H)
    if kind is None:
        raise ValueError("algo='exact' serves two classes of operators: diagonal ones (functions of the sigma-z alone) and "
                         "sums of single-site operators plus a constant; this operator is neither (kicks alternate the "
                         "two: evolve each factor on its own)")
    sp = state.subspace
    if kind == 'diagonal':
        mat = H.get_mat(subspaces=(sp, sp))
        if mat.nranks > 1:
            raise NotImplementedError("algo='exact' on a partitioned state")
        xin, yout = _adopt(mat, state, result)
        backend.expm_diagonal(mat, xin, yout, -1j * complex(t))
    else:
        if type(sp) is not Full:
            raise ValueError("algo='exact' with an operator that flips spins needs a state on the Full space, not %r "
                             "(single-site rotations leave every other subspace)" % (sp,))
        mats = site_exponentials(a, t)
        if c0 != 0:
            # the constant: a phase on the first site that is rotated at all
            live = np.flatnonzero(np.any(a != 0, axis=1))
            mats[int(live[0]) if live.size else 0] *= np.exp(-1j * complex(t) * c0)
        backend.site_ops_apply(state.vec, sp._to_c(), mats, result.vec)
    evolve.last_stats = dict(_EXACT_STATS)
    evolve.last_mat = None
    result.set_initialized()
    return result


def eigsolve(H, getvecs=False, nev=1, which='lowest', target=None, tol=None, subspace=None,
             max_its=None, ncv=None, seed=0, interior=None):
    """A few extremal eigenpairs (computations.py:128-292), or -- ``target=E, interior='filter'``, not in the
    reference, whose only interior method is shift-invert on a stored matrix -- the ``nev`` eigenpairs nearest
    ``E``, matrix-free, by a Chebyshev filter of the folded spectrum (dnm_eigsolve_interior): ordered by
    ``|E_i - target|``, converged when ``|H v - E_i v| <= tol * ||H||_inf``.  Without ``interior``, ``target`` is
    refused as the reference refuses it for shell matrices."""
    H.establish_L()
    if subspace is None:
        subspace = H.subspace
    elif not H.has_subspace(subspace):
        raise ValueError('Requested subspace has not been added to operator.')
    if interior is not None and interior != 'filter':
        raise ValueError(f'invalid value "{interior}" for interior (the matrix-free interior method is "filter")')
    if interior is not None and target is None:
        raise ValueError("Must specify target when setting interior='filter'")
    if target is not None and interior is None:
        # computations.py:211-220: refused for shell matrices and on GPUs
        raise RuntimeError('Shift-invert ("target") not supported for shell matrices.')
    config._initialize()
    if target is not None:
        which = 'target'              # computations.py:208-213: a target decides what "which" means
    elif which == 'target':
        raise ValueError("Must specify target when setting which='target'")
    if which in ['smallest', 'largest']:
        warnings.warn('values "smallest" and "largest" for eigsolve parameter "which" '
                      'are deprecated, and have been replaced by "lowest" and "highest" respectively.',
                      DeprecationWarning, stacklevel=2)
        which = {'smallest': 'lowest', 'largest': 'highest'}[which]
    if which not in _lib.WHICH:
        raise ValueError(f'invalid value "{which}" for which')

    mat = H.get_mat(subspaces=(subspace, subspace))
    # A real-symmetric operator (Heisenberg, XXZ, Ising, random-field chains: every matrix element real in the
    # product basis) needs no complex arithmetic for its eigenpairs: on one rank, from 2^23 amplitudes on, the solver
    # runs on real vectors stored two amplitudes to a complex128 element (DNM_MAT_REAL_PACKED) -- half the bytes per
    # multiply and per Krylov vector, twice the basis in the same memory -- and the eigenvectors are handed back as
    # the complex states the reference returns.  config.eigs_real_arithmetic (DNM_EIGS_REAL=0 / 1 in tests) forces the choice.
    cmat = mat
    er = knob('DNM_EIGS_REAL')
    want_real = config.eigs_real_arithmetic
    if er:
        want_real = er[:1] == '1'
    if want_real is None:
        # (the smallest block decides: blocks of the partitioned SpinConserve layout differ by up to 10 %, and ranks
        # on either side of the threshold would build handles whose exchanges do not match -- ADVICE r4)
        want_real = _min_over_ranks(mat.n_local) >= (1 << 23)
    if want_real:                   # (Full / Parity on 2^p ranks; SpinConserve in the internal layout on any count)
        pm = H.get_real_packed_mat(subspace)
        # every rank or none: a rank whose build was refused keeps its peers on complex128 as well
        if _min_over_ranks(0 if pm is None else 1) == 1:
            mat = pm
    packed = mat is not cmat
    # The solver's own vectors need not lie in the reference's order: on several ranks a SpinConserve operator in the internal
    # layout is solved on a partition made for the exchange (dnm_subspace.vec_swizzle bits 16-19 = 1, csrc/sc3.h: the T
    # blocks ordered so that contiguous ranges cut ONE bond of a chain instead of log2(ranks) + 1 -- SpinConserve(36,18) on
    # 8 ranks: 14.3 GiB to the busiest rank per multiply instead of 42.4).  The start vector holds the numbers the
    # reference order would (keyed by reference index), so the Krylov space is the same one.
    # Eigenvectors move back block by block at the end (backend.reorder_blocks).
    base = mat
    sm = _solver_mat(H, subspace, packed)
    if sm is not None:
        mat = sm
    eigsolve.last_mat = mat
    keep = []
    hooks = _hooks(mat, keep)
    import torch
    vec_bytes = 16 * mat.n_local
    mat.prepare_exchange(torch.empty(0, dtype=torch.complex128, device=config.device))
    # all converged pairs are returned (computations.py:259-281) -- but not at the price of a second basis:
    # large vectors are limited to the nev requested
    nev_max = max(nev, int(ncv) if ncv else max(2 * nev, nev + 15))
    if getvecs and vec_bytes * nev_max > (1 << 30):
        nev_max = nev
    # one extremal pair of a large operator: the native driver runs Lanczos without a stored basis (four work
    # vectors; DNM_EIGS_BASISFREE=0/1 forces the choice) -- nothing to fit into memory then
    import os
    ncv_native = 0 if ncv is None else int(ncv)
    bf = knob('DNM_EIGS_BASISFREE')
    basis_free = (ncv is None and nev == 1 and mat.N > 64 and interior is None and
                  (bf[:1] == '1' if bf else _min_over_ranks(mat.n_local) >= (1 << 22)))
    work_vecs = 4 if interior else 3      # beside the basis: the residual vector and the filter's work vectors
    if ncv is None and not basis_free:
        # SLEPc's default max(2 nev, nev + 15) (+1 for the residual vector), reduced to what fits in HBM
        cached = C.c_size_t()
        _lib.check(_lib.lib().dnm_workspace_bytes(C.byref(cached)))
        want = max(2 * nev, nev + 15)

        def fitting():
            # (beside the want + 1 basis vectors the driver may take two work vectors for its Chebyshev filter: a
            # multiply's own vectors, freed by the caller but still in torch's cache, once made a solve at
            # SpinConserve(33,16) run out of memory with "17 fit")
            free, _ = torch.cuda.mem_get_info()
            return int((free + cached.value) // vec_bytes) - work_vecs - (nev_max if getvecs else 0)
        torch.cuda.empty_cache()            # memory torch holds for reuse counts as free
        fit = _min_over_ranks(fitting())
        if fit < want and interior:
            if fit < nev + 2:
                raise RuntimeError('not enough device memory for eigsolve(nev=%d, target=%g): %d vectors of %.1f GiB '
                                   'fit, the filtered solver needs %d' % (nev, target, max(fit + work_vecs, 0),
                                                                          vec_bytes / 2 ** 30, nev + 2 + work_vecs))
            ncv_native = -(fit + work_vecs)
        elif fit < want:
            if fit < nev + 5:
                # no room for a restarted basis worth the name (at least nev + 2 vectors beside the Chebyshev filter's
                # work vectors): the native driver takes the pairs one after the other through the basis-free
                # recurrence on the operator deflated by the pairs found -- four work vectors and the pairs themselves
                # (the caller's buffer when the vectors are wanted)
                need = 4 + (0 if getvecs else nev - 1)
                if fit + 3 < need or mat.N <= max(64, 4 * nev):
                    raise RuntimeError('not enough device memory for eigsolve(nev=%d): %d vectors of %.1f GiB fit, '
                                       'the basis-free solver needs %d' % (nev, max(fit + 3, 0), vec_bytes / 2 ** 30,
                                                                           need))
                fit = max(fit, 0)
            # the default basis, capped at what fits (fit + 1 vectors in all): the native driver keeps its automatic
            # choices -- a Chebyshev filter for several pairs of a large operator -- inside that budget
            ncv_native = -(fit + 1)
    evals = np.zeros(nev_max, dtype=np.float64)
    evec_buf = None
    if getvecs:
        from .backend import device_zeros
        evec_buf = device_zeros(nev_max * mat.n_local, empty=True)
    stats = _lib.SolverStats()
    tail = (ncv_native, 0 if max_its is None else int(max_its), int(seed),
            C.byref(hooks) if hooks is not None else None, nev_max, _lib.pf64(evals),
            C.c_void_p(evec_buf.data_ptr()) if evec_buf is not None else None, C.byref(stats), _stream())
    if interior:
        _lib.check(_lib.lib().dnm_eigsolve_interior(
            mat.handle, mat.n_local, int(nev), float(target), 0.0 if tol is None else float(tol), *tail))
    else:
        _lib.check(_lib.lib().dnm_eigsolve(
            mat.handle, mat.n_local, int(nev), _lib.WHICH[which], 0.0 if tol is None else float(tol), *tail))
    # (max_rel_residual: relative to |E_i| for the extremal solver, to ||H||_inf for the interior one)
    eigsolve.last_stats = {'reason': stats.reason, 'its': stats.its, 'matvecs': stats.matvecs,
                           'nconv': stats.nconv, 'max_rel_residual': stats.err_est, 'real_arithmetic': packed}
    nconv = stats.nconv
    if stats.reason == _lib.DIVERGED_ITS:
        raise MaxIterationsError('eigensolver reached maximum number of iterations without '
                                 'converging. Try increasing the maximum iterations of the '
                                 'eigensolver via the "max_its" argument to eigsolve() '
                                 f'(current value: {max_its})')
    elif stats.reason == _lib.DIVERGED_BREAKDOWN:
        raise ConvergenceError('eigsolver failed to converge with reason EPS_DIVERGED_BREAKDOWN')
    elif stats.reason <= 0 or nconv < nev:
        raise ConvergenceError('eigsolver failed to converge')

    vals = evals[:nconv].copy()
    if not getvecs:
        return vals
    from .states import State
    from .backend import Vec
    evecs = []
    pieces = [evec_buf[i * mat.n_local:(i + 1) * mat.n_local] for i in range(nconv)]
    if mat is not base:
        # from the solver's partition to the one States live on, one vector at a time (the buffer goes as the last leaves)
        from .backend import reorder_blocks
        moved = []
        for i in range(nconv):
            moved.append(reorder_blocks(pieces[i], mat._keep[1], base._keep[1], per_position=1 if packed else 2))
            pieces[i] = None
        pieces, evec_buf, mat = moved, None, base
    for i in range(nconv):
        v = State(L=H.L, subspace=subspace)
        piece = pieces[i]
        if packed:
            # the real eigenvector as the complex state of the full dimension (imaginary parts zero)
            if mat.swz_right >= 256:      # SpinConserve: one double per position of the PACKED handle's own layout
                # (its descriptor and site relabelling, not the complex handle's: the two builds choose theirs
                # separately, and positions of one are not positions of the other -- ADVICE r5)
                v._vec = Vec(cmat.N, swz=mat.swz_right, sub_c=mat._keep[1])
                _lib.check(_lib.lib().dnm_vec_layout_unpack_real(C.byref(mat._keep[1]), C.byref(v._vec._part),
                                                                 v._vec.ptr, C.c_void_p(piece.data_ptr()), _stream()))
                v.set_initialized()
                evecs.append(v)
                continue
            v._vec = Vec(cmat.N, swz=cmat.swz_right, sub_c=cmat._keep[1])
            if v._vec.internal:
                raise RuntimeError('internal: a packed Full / Parity handle beside a SpinConserve layout')
            else:                         # Full / Parity: two amplitudes per element
                _lib.check(_lib.lib().dnm_vec_unpack_real(v._vec.ptr, C.c_void_p(piece.data_ptr()), mat.n_local,
                                                          mat.swz_right, cmat.swz_right, _stream()))
        else:
            # (views of one buffer: no second copy of the vectors)
            v._vec = Vec(mat.N, array=piece, swz=mat.swz_right, sub_c=mat._keep[1])
        v.set_initialized()
        evecs.append(v)
    return vals, evecs


eigsolve.last_stats = None
eigsolve.last_mat = None          # the handle the last call multiplied with (bench.py: its exchange summary)


def reduced_density_matrix(state, keep):
    """Reduced density matrix of ``state`` on the (sorted) spins ``keep``, everything else
    traced out (computations.py:294-349).  Computed on the GPU; returned as a numpy array on
    process 0, ``[[-1]]`` on the other processes, as the reference does."""
    return _reduced_density_matrix(state, keep, on_device=False)


def _check_keep(state, keep):
    for n in range(1, keep.size):
        if keep[n] <= keep[n - 1]:
            raise ValueError('keep array must be strictly increasing')
    if any(idx < 0 for idx in keep):
        raise ValueError('spin index less than zero. keep: %s' % str(keep))
    if any(idx >= state.L for idx in keep):
        raise ValueError('spin index greater than spin chain length minus one. keep: %s' % str(keep))


def _reduced_density_matrix(state, keep, on_device):
    """The argument checks of computations.py:294-349, then the kernel; ``on_device``: a device tensor on process 0
    and None elsewhere instead of the host array / ``[[-1]]``."""
    from . import backend
    state.assert_initialized()
    config._initialize()
    if not state.subspace.product_state_basis:
        raise ValueError('reduced density matrices currently only supported '
                         'for product state basis subspace types.')
    keep = np.array(keep, dtype=np.int64)
    if keep.size == 0:
        return np.array([[1]], dtype=np.complex128)
    _check_keep(state, keep)
    return backend.reduced_density_matrix(state.vec, state.subspace._to_c(), keep, on_device=on_device)


# reduced density matrices from this size on are diagonalised where they are computed: the spectrum of a
# 2^k x 2^k matrix by the device's dense Hermitian solver (0.9 s at k = 13, where the copy to the host alone takes
# 0.2 s and host LAPACK minutes); smaller ones go through numpy exactly as the reference does
_DEVICE_EIG_FROM = 256


def _rdm_spectrum(state, keep):
    """Eigenvalues of the reduced density matrix (numpy array, ascending) on process 0, None elsewhere."""
    if (1 << len(keep)) < _DEVICE_EIG_FROM:
        reduced = reduced_density_matrix(state, keep)
        if reduced[0, 0] == -1:
            return None
        return np.linalg.eigvalsh(reduced)
    import torch
    rho = _reduced_density_matrix(state, keep, on_device=True)
    if rho is None:
        return None
    from .subspaces import Parity, SpinConserve
    if type(state.subspace) in (SpinConserve, Parity):
        # a state of fixed magnetisation: rho couples only kept configurations with equal numbers of up spins -- the
        # spectrum is that of its blocks (C(k, n) rows each: at 13 of 26 spins 14 blocks of <= 1716 rows instead of
        # one matrix of 8192); a state of fixed parity: equal parities of that number, two blocks of half the size
        K = rho.shape[0]
        a = torch.arange(K, device=rho.device)
        label = torch.zeros(K, dtype=torch.int64, device=rho.device)
        for b in range(len(keep)):
            label += (a >> b) & 1
        if type(state.subspace) is Parity:
            label &= 1
        out = []
        for n in range(int(label.max()) + 1):
            idx = torch.nonzero(label == n).flatten()
            out.append(torch.linalg.eigvalsh(rho.index_select(0, idx).index_select(1, idx)))
        return np.sort(torch.cat(out).cpu().numpy())
    return torch.linalg.eigvalsh(rho).cpu().numpy()


def _sector_subspace(state):
    """(SpinConserve subspace, XParity sector or 0) when the state's reduced density matrices are direct sums over the
    number of up spins kept -- a SpinConserve state, or an XParity state on top of one -- else None."""
    from .subspaces import SpinConserve, XParity
    sp = state.subspace
    if type(sp) is SpinConserve:
        return sp, 0
    if type(sp) is XParity and type(sp.parent) is SpinConserve:
        return sp.parent, int(sp.sector)
    return None


def reduced_density_matrix_sectors(state, keep, sectors=None, on_device=False):
    """The reduced density matrix of a fixed-magnetisation state block by block: ``{n: rho_n}``, n the number of set
    bits (down spins, as SpinConserve counts them) among the kept spins.  ``rho_n`` couples the kept configurations
    with n set bits in ascending integer order -- it is ``rho[idx][:, idx]`` of the dense matrix, ``idx`` the indices
    of popcount n, and all entries of the dense matrix outside the blocks are zero.  Only the blocks are computed (by
    kernels that never touch a product state outside the subspace), so cuts of more than 15 spins are possible as
    long as the blocks fit the device.

    ``state`` lives on ``SpinConserve`` or on ``XParity(SpinConserve)``; any other subspace raises ValueError.
    ``sectors``: the n wanted (default: every feasible one, max(0, k - (L - len(keep))) <= n <= min(k, len(keep))).
    Blocks are numpy arrays, or device tensors with ``on_device``; on the other processes of a partitioned run every
    block is ``[[-1]]`` (None with ``on_device``), as for ``reduced_density_matrix``."""
    from . import backend
    state.assert_initialized()
    config._initialize()
    route = _sector_subspace(state)
    if route is None:
        raise ValueError('sector-resolved reduced density matrices need a SpinConserve state or an XParity state on '
                         'top of SpinConserve, not %r' % (state.subspace,))
    sub, xsec = route
    keep = np.array(keep, dtype=np.int64).reshape(-1)
    _check_keep(state, keep)
    if keep.size == 0:
        if sectors is not None and [int(n) for n in sectors] != [0]:
            raise ValueError('no kept spins: the only block is n = 0')
        return {0: np.array([[1]], dtype=np.complex128)}
    sub_c = state.subspace._to_c() if xsec == 0 else sub._to_c()
    plan = backend.rdm_sector_plan(sub_c['data'], keep, xsec)[0]
    if sectors is None:
        sectors = [n for n, _, _ in plan]
    sectors = [int(n) for n in sectors]
    blocks = backend.rdm_sector_blocks(state.vec, sub_c, keep, xsec, sectors, plan=plan)
    if blocks is None:
        return {n: (None if on_device else np.array([[-1]], dtype=np.complex128)) for n in sectors}
    return blocks if on_device else {n: b.cpu().numpy() for n, b in blocks.items()}


def _sector_spectrum(state, keep):
    """Eigenvalues of the reduced density matrix through its blocks, one block at a time: compute, diagonalise on the
    device, free -- the peak is the largest block plus the solver's workspace.  An XParity state's blocks n and
    len(keep) - n have the same spectrum (the global flip maps one onto the other): the lower half is computed and
    counted twice.  numpy array, ascending, on process 0; None elsewhere."""
    import torch
    from . import backend
    state.assert_initialized()
    config._initialize()
    sub, xsec = _sector_subspace(state)
    keep = np.array(keep, dtype=np.int64).reshape(-1)
    _check_keep(state, keep)
    if keep.size == 0:
        return np.array([1.0])
    sub_c = state.subspace._to_c() if xsec == 0 else sub._to_c()
    plan = backend.rdm_sector_plan(sub_c['data'], keep, xsec)[0]
    whole = backend._whole_state_on_rank0(state.vec, sub_c)      # (reference order: gathered / copied once)
    if whole[0] is None:
        return None
    out = []
    for n, _, _ in plan:
        if xsec and 2 * n > keep.size:
            continue
        blocks = backend.rdm_sector_blocks(state.vec, sub_c, keep, xsec, [n], plan=plan, whole=whole)
        w = torch.linalg.eigvalsh(blocks.pop(n)).cpu().numpy()
        out.append(w)
        if xsec and 2 * n != keep.size:
            out.append(w)
    return np.sort(np.concatenate(out))


def _takes_sector_route(state, keep):
    """Where the entropies go through the blocks: the cases the dense form cannot do -- XParity(SpinConserve) states
    (no dense form exists for them) and SpinConserve states with more than 15 spins kept.  Smaller SpinConserve cuts
    stay on the dense route (_rdm_spectrum) until the two are timed against each other at 13 of 26 spins
    (tools/rdm_sectors_timing.py); entanglement_spectrum takes the blocks at every size."""
    route = _sector_subspace(state)
    if route is None:
        return False
    return route[1] != 0 or len(keep) > 15


def _spectrum(state, keep):
    if _takes_sector_route(state, keep):
        return _sector_spectrum(state, keep)
    return _rdm_spectrum(state, keep)


def entanglement_spectrum(state, keep):
    """All eigenvalues of the reduced density matrix of ``state`` on the spins ``keep``, ascending (numpy array; None
    on the processes other than 0).  SpinConserve and XParity(SpinConserve) states go block by block through
    ``reduced_density_matrix_sectors``' kernels, whatever the size of the cut; every other state through the dense
    matrix."""
    if _sector_subspace(state) is not None:
        return _sector_spectrum(state, keep)
    return _rdm_spectrum(state, keep)


def sigmaz_correlations(state, connected=False):
    """Every local magnetisation and every two-site sigma-z correlator of ``state`` from one pass over it (one
    matrix-core kernel, ``backend.zz_moments``) instead of L (L + 1) / 2 calls of ``Operator.expectation``, each a
    multiply and a temporary vector.  Returns ``(mz, zz)``, float64: ``mz[i]`` = <psi|sigmaz_i|psi> and ``zz[i, j]`` =
    <psi|sigmaz_i sigmaz_j|psi>, with the sign ``sigmaz(i).expectation`` gives and nothing normalised, as
    ``expectation`` normalises nothing; ``zz`` is symmetric and its diagonal is <psi|psi>.  ``connected``: ``zz`` is
    ``zz / n - outer(mz, mz) / n**2`` with n = <psi|psi>, the connected correlator of the normalised state.

    States on XParity subspaces: sigmaz_i sigmaz_j commutes with the global flip, so ``zz`` is the same sum over the
    representatives, and every <sigmaz_i> vanishes by symmetry -- ``mz`` is exact zeros.  Every process gets the result."""
    from . import backend
    from .subspaces import XParity
    state.assert_initialized()
    config._initialize()
    sp = state.subspace
    flip_sector = type(sp) is XParity
    if not (sp.product_state_basis or flip_sector):
        raise ValueError('sigma-z correlations need a product state basis or an XParity subspace, not %r' % (sp,))
    # (an XParity descriptor is its parent's: the vector holds the parent's first dim / 2 rows)
    M = backend.zz_moments(state.vec, sp._to_c())
    mz = np.zeros(M.shape[0] - 1) if flip_sector else M[0, 1:].copy()
    zz = M[1:, 1:].copy()
    if connected:
        n = M[0, 0]
        zz = zz / n - np.outer(mz, mz) / n ** 2
    return mz, zz


def _basis_weights_subspace(state, what):
    """The subspace of ``state`` and whether it is an XParity one, for the passes over |psi_c|^2."""
    from .subspaces import XParity
    state.assert_initialized()
    config._initialize()
    sp = state.subspace
    flip_sector = type(sp) is XParity
    if not (sp.product_state_basis or flip_sector):
        raise ValueError('%s needs a product state basis or an XParity subspace, not %r' % (what, sp))
    return sp, flip_sector


def apply_site_operators(state, mats, sites=None, result=None):
    """(x)_j M_j |state>: a product of single-site operators on a Full-space state, in place when ``result`` is
    ``state``, into a new State when it is None.  ``mats`` is one 2 x 2 matrix for every spin of ``sites`` (all spins
    when ``sites`` is None) or an array (n, 2, 2) with ``mats[i]`` for spin ``sites[i]``; the other spins get the
    identity.  M acts on spin j with bit 0 = up, as everywhere here: (M psi)(.. c'_j ..) = sum_c M[c'_j][c_j] psi(.. c_j
    ..); nothing requires M to be unitary.  One to four streaming passes on the device (``backend.site_ops_apply``).
    A product of single-site operators leaves every symmetry sector: a Parity, SpinConserve or Explicit state is expanded
    first, ``identity()`` with ``add_subspace(Full(), subspace)`` applied to it, an XParity state with
    ``subspace.convert_state`` -- or either, on the device, with ``state.to_subspace(Full())``; these raise
    ``ValueError``.  On more than one rank: ``NotImplementedError``."""
    from . import backend
    from .states import State
    from .subspaces import Full, XParity
    state.assert_initialized()
    config._initialize()
    sp = state.subspace
    if type(sp) is XParity:
        raise ValueError('site operators leave an XParity sector: expand with `convert_state` first (to the parent, and '
                         'from there to Full)')
    if type(sp) is not Full:
        raise ValueError('site operators act on the Full space, not on %r: expand the state first -- op = identity(); '
                         'op.add_subspace(Full(), state.subspace); op.dot(state)' % (sp,))
    L = sp.L
    mats = np.asarray(mats, dtype=np.complex128)
    where = np.arange(L) if sites is None else np.asarray(sites).reshape(-1)
    if where.size and (not np.issubdtype(where.dtype, np.integer) or where.min() < 0 or where.max() >= L
                       or np.unique(where).size != where.size):
        raise ValueError('sites must be distinct integers in [0, %d)' % L)
    if mats.shape == (2, 2):
        mats = np.broadcast_to(mats, (where.size, 2, 2))
    if mats.shape != (where.size, 2, 2):
        raise ValueError('site operators for %d sites are one (2, 2) matrix or an array (%d, 2, 2), not of shape %r'
                         % (where.size, where.size, mats.shape))
    full = np.broadcast_to(np.eye(2, dtype=np.complex128), (L, 2, 2)).copy()
    full[where] = mats
    if result is None:
        result = State(L=L, subspace=sp)
    elif result.subspace != sp:
        raise ValueError('subspace of state and result must match')
    backend.site_ops_apply(state.vec, sp._to_c(), full, result.vec)
    result.set_initialized()
    return result


_SQRT_HALF = 1.0 / np.sqrt(2.0)
# the rotation that takes the +1 eigenvector of a Pauli matrix to |0> (up) and the -1 eigenvector to |1>
_BASIS_ROTATIONS = {'x': _SQRT_HALF * np.array([[1, 1], [1, -1]], dtype=np.complex128),
                    'y': _SQRT_HALF * np.array([[1, -1j], [1, 1j]], dtype=np.complex128),
                    'z': np.eye(2, dtype=np.complex128)}


def basis_rotations(bases, L):
    """The rotations (L, 2, 2) that precede a sigma-z measurement for ``bases``: a string of ``x`` / ``y`` / ``z`` of
    length 1 (every spin) or L (character i for spin i), or an array (L, 2, 2) of unitaries of the caller's."""
    if isinstance(bases, str):
        if len(bases) not in (1, L) or set(bases.lower()) - set('xyz'):
            raise ValueError("bases is a string of 'x', 'y', 'z' of length 1 or %d, not %r" % (L, bases))
        chars = bases.lower() * L if len(bases) == 1 and L != 1 else bases.lower()
        return np.array([_BASIS_ROTATIONS[ch] for ch in chars])
    mats = np.asarray(bases, dtype=np.complex128)
    if mats.shape != (L, 2, 2):
        raise ValueError('bases is a string or an array of shape (%d, 2, 2), not %r' % (L, mats.shape))
    if not np.allclose(np.einsum('jab,jcb->jac', mats, mats.conj()), np.eye(2), rtol=0, atol=1e-8):
        raise ValueError('bases: every matrix must be unitary')
    return mats


def _rotated_copy(state, mats):
    """A Full-space copy of ``state`` with the single-site rotations ``mats`` applied (for sampling in another basis)."""
    import torch
    from .operators import identity
    from .states import State
    from .subspaces import Full, XParity
    sp = state.subspace
    if type(sp) is XParity:
        raise ValueError('sampling in another basis leaves an XParity sector: expand with `convert_state` first')
    if not sp.product_state_basis:
        raise ValueError('sampling in another basis needs a product state basis, not %r' % (sp,))
    if config.world_size > 1:
        raise NotImplementedError('sampling a partitioned state in another basis')
    need = 16 << sp.L
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
    if free < need:
        raise MemoryError('sampling in another basis rotates a Full-space copy of the state: %d bytes, %d free on the '
                          'device' % (need, free))
    if type(sp) is Full:
        work = state.copy()
    else:
        expand = identity()
        expand.L = sp.L
        expand.add_subspace(Full(L=sp.L), sp)
        work = expand.dot(state)
    return apply_site_operators(work, mats, result=work)


def sample(state, shots, seed=None, bases=None):
    """``shots`` measurements of ``state``: int64 array of outcomes as integers (bit i = spin i).  ``bases`` = None
    measures every spin in the computational (sigma-z) basis, as described below.  Otherwise ``bases`` is a string of
    ``x`` / ``y`` / ``z`` of length 1 or L, or an array (L, 2, 2) of unitaries applied before a sigma-z measurement:
    bit i of an outcome set means eigenvalue -1 of the Pauli matrix measured on spin i (bit 0 is up, as everywhere
    here).  A Full-space copy of the state is rotated on the device (``apply_site_operators``) and sampled; Parity,
    SpinConserve and Explicit states are expanded first (16 * 2^L bytes must be free), XParity raises ``ValueError``.
    All-``z`` bases take the path of ``bases=None``.

    Computational basis: product states as integers (bit
    i = spin i, as ``subspace.idx_to_state`` gives them), drawn with probability |psi_c|^2 / <psi|psi> on the device
    (``backend.born_sample``: one pass over the state and a search per shot; the state is not copied to the host and
    need not be normalised).  A configuration of weight zero is never returned.  ``seed`` (an integer; None draws one
    from ``os.urandom``) fixes the shots: shot s is the same whatever ``shots`` is.

    Full, Parity, SpinConserve, Explicit / Auto and XParity states on one process.  A basis vector of an XParity
    subspace is (|c> +- |~c>) / sqrt 2, so each shot returns the representative c or its global flip ~c by a fair coin
    of the same generator.  A state of zero norm raises ``ValueError``."""
    from . import backend
    sp, flip_sector = _basis_weights_subspace(state, 'sampling')
    shots = int(shots)
    if shots < 0:
        raise ValueError('shots must not be negative')
    if seed is None:
        import os
        seed = int.from_bytes(os.urandom(8), 'little')
    if bases is not None:
        mats = basis_rotations(bases, sp.L)
        if not np.array_equal(mats, np.broadcast_to(np.eye(2), mats.shape)):
            return sample(_rotated_copy(state, mats), shots, seed=seed)
    # (an XParity descriptor is its parent's: the vector holds the parent's first dim / 2 rows)
    rows, flips = backend.born_sample(state.vec, sp._to_c(), shots, seed)
    if np.any(rows < 0):
        raise ValueError('cannot sample a state of zero norm')
    out = np.asarray(sp.idx_to_state(rows), dtype=np.int64).reshape(-1)
    if flip_sector:
        out = np.where(flips != 0, out ^ ((1 << sp.L) - 1), out)
    return out


def _power_exponents(qs):
    """The exponents of ``qs`` that need a power sum: the finite ones other than 0 and 1."""
    return [q for q in qs if np.isfinite(q) and q != 0 and q != 1]


def participation_from_sums(qs, P, W, H, wmax, nnz, flip_sector=False):
    """The participation entropies S_q, q in ``qs``, from the sums over the weights w of a state's amplitudes: ``P``
    = sum w^q for the exponents ``_power_exponents(qs)`` in their order, ``W`` = sum w, ``H`` = sum w ln w, the largest
    weight and the number of non-zero ones.  S_q = (ln P_q - q ln W) / (1 - q); q = 1: ln W - H / W; q = inf:
    -ln(wmax / W); q = 0: ln nnz.  ``flip_sector``: the sums run over the representatives of an XParity state, each of
    whose weights splits in two in the product basis -- P_q picks up 2^(1-q), H loses W ln 2, wmax halves and nnz
    doubles (every entropy gains ln 2)."""
    P = np.asarray(P, dtype=np.float64)
    need = _power_exponents(qs)
    if P.size != len(need):
        raise ValueError('%d power sums for %d exponents' % (P.size, len(need)))
    if flip_sector:
        P = P * np.exp2(1.0 - np.array(need, dtype=np.float64)) if need else P
        H, wmax, nnz = H - W * np.log(2.0), wmax / 2.0, 2.0 * nnz
    out, k = np.empty(len(qs), dtype=np.float64), 0
    for i, q in enumerate(qs):
        if q == 0:
            out[i] = np.log(nnz)
        elif q == 1:
            out[i] = np.log(W) - H / W
        elif np.isinf(q):
            out[i] = -np.log(wmax / W)
        else:
            out[i] = (np.log(P[k]) - q * np.log(W)) / (1.0 - q)
            k += 1
    return out


def participation_entropies(state, qs=(2,)):
    """The participation (basis Renyi) entropies S_q = ln(sum_c p_c^q) / (1 - q) of ``state`` in the product basis, p_c
    = |psi_c|^2 / <psi|psi>: float64 array, one value per q of ``qs`` (q >= 0; q = 1 is the Shannon entropy, ``np.inf``
    the min-entropy -ln max p, 0 the logarithm of the number of non-zero amplitudes).  One pass over the state on the
    device for up to 8 exponents other than 0, 1 and inf (``backend.power_sums``); the state need not be normalised.
    States on XParity subspaces count in the product basis, where each representative's weight splits in two.  One
    process only."""
    from . import backend
    sp, flip_sector = _basis_weights_subspace(state, 'participation entropies')
    qs = [float(q) for q in np.atleast_1d(np.asarray(qs, dtype=np.float64))]
    if any(np.isnan(q) or q < 0 for q in qs):
        raise ValueError('participation entropies are defined for q >= 0')
    P, W, H, wmax, nnz = backend.power_sums(state.vec, _power_exponents(qs))
    if not W > 0:
        raise ValueError('participation entropies of a state of zero norm')
    return participation_from_sums(qs, P, W, H, wmax, nnz, flip_sector)


def _pm_subspace(state, what):
    from .subspaces import Explicit, Full, Parity, SpinConserve, XParity
    sp = state.subspace
    if type(sp) is XParity:
        raise ValueError('%s of an XParity state: sigma+_i sigma-_j does not commute with the global spin flip, so the '
                         'sum over the representatives is not the expectation value (expand the state first)' % what)
    if isinstance(sp, Explicit) or not isinstance(sp, (Full, Parity, SpinConserve)):
        raise ValueError('%s need a Full, Parity or SpinConserve subspace, not %r' % (what, sp))
    return sp


def sigma_pm_correlations(state):
    """Every <psi|sigma_plus(i) sigma_minus(j)|psi> of ``state`` from one pass over it (one matrix-core kernel,
    ``backend.pm_moments``) instead of L (L - 1) calls of ``Operator.expectation``, each a multiply and a temporary
    vector.  Returns ``pm``, complex128 of shape (L, L): ``pm[i, j]`` = <psi|sigma_plus(i) sigma_minus(j)|psi> with
    sigma_plus = sigmax + i sigmay without a factor 1/2 and nothing normalised, as ``expectation`` normalises nothing.
    ``Operator.expectation`` builds Hermitian operators only; in its terms ``pm.real[i, j]`` is
    ``(sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j)).expectation(state)`` -- <sigmax_i sigmax_j + sigmay_i sigmay_j>
    for i != j -- and ``pm.imag[i, j]`` is ``(sigmay(i) * sigmax(j) - sigmax(i) * sigmay(j)).expectation(state)``.
    ``pm`` is Hermitian to the last bit and its diagonal is that of sigma_plus(i) sigma_minus(i) = 2 (1 + sigmaz_i),
    from the same sums ``sigmaz_correlations`` returns.

    Full, Parity and SpinConserve states on one process.  XParity states are refused: sigma+_i sigma-_j does not
    commute with the global flip, the sum over the representatives is not the answer."""
    from . import backend
    state.assert_initialized()
    config._initialize()
    sp = _pm_subspace(state, 'sigma+ sigma- correlations')
    return 4.0 * backend.pm_moments(state.vec, sp._to_c())


def spin_correlations(state):
    """``ss[i, j]`` = <psi|sigma_i . sigma_j|psi> = <sigmax_i sigmax_j + sigmay_i sigmay_j + sigmaz_i sigmaz_j>, float64
    of shape (L, L), nothing normalised: ``zz[i, j] + pm[i, j].real`` off the diagonal (``sigmaz_correlations`` and
    ``sigma_pm_correlations``: two passes over the state) and 3 <psi|psi> on it."""
    _pm_subspace(state, 'spin correlations')
    _, zz = sigmaz_correlations(state)
    ss = zz + sigma_pm_correlations(state).real
    np.fill_diagonal(ss, 3.0 * np.diag(zz))
    return ss


_SWAP_CALL_MAX = 63       # bonds of one call of backend.swap_moments
_SWAP_CHUNK = 31          # longer lists: chunks of this size, one call per pair of chunks on their union


def _swap_subspace(state, what='bond correlations'):
    """(descriptor's subspace, XParity sector or 0) for the bond-swap and the rotation pass: Full, Parity and
    SpinConserve, and XParity over those (the descriptor is then the parent's)."""
    from .subspaces import Explicit, Full, Parity, SpinConserve, XParity
    sp = state.subspace
    base, sector = (sp.parent, int(sp.sector)) if type(sp) is XParity else (sp, 0)
    if isinstance(base, Explicit) or not isinstance(base, (Full, Parity, SpinConserve)):
        raise ValueError('%s need a Full, Parity or SpinConserve subspace, or XParity over one of them, not %r'
                         % (what, sp))
    return sp, sector


def _swap_gram(state, bonds):
    """G of backend.swap_moments for any number of bonds: G[0, 0], G[0, 1 + m] and G[1 + m, 1 + m']."""
    from . import backend
    sp, sector = _swap_subspace(state)
    sub_c = sp._to_c()
    n = len(bonds)
    if n <= _SWAP_CALL_MAX:
        return backend.swap_moments(state.vec, sub_c, bonds, sector)
    G = np.zeros((n + 1, n + 1), dtype=np.complex128)
    chunks = [np.arange(lo, min(lo + _SWAP_CHUNK, n)) for lo in range(0, n, _SWAP_CHUNK)]
    for i in range(len(chunks)):
        for j in range(i + 1, len(chunks)):
            # (with more than one chunk every chunk has a partner: the diagonal blocks come with the pairs)
            sel = np.concatenate([chunks[i], chunks[j]])
            g = backend.swap_moments(state.vec, sub_c, bonds[sel], sector)
            at = np.concatenate([[0], 1 + sel])
            G[np.ix_(at, at)] = g
    return G


def bond_correlations(state, bonds, connected=False):
    """Every bond energy and every bond-bond (dimer-dimer) correlator of ``state`` from one pass over it (one
    matrix-core kernel, ``backend.swap_moments``) instead of one ``Operator.expectation`` per pair of bonds.  ``bonds``
    is a list of pairs of sites (a_m, b_m), a_m != b_m; a bond may repeat and bonds may share sites.  Returns
    ``(b, bb)``: ``b[m]`` = <psi|sigma_a . sigma_b|psi>, float64, and ``bb[m, m']`` = <psi|(sigma_a . sigma_b)(sigma_c .
    sigma_d)|psi>, complex128 and Hermitian (real for a real state), with sigma . sigma = sigmax sigmax + sigmay sigmay
    + sigmaz sigmaz and nothing normalised, as ``expectation`` normalises nothing.  ``connected``: ``bb`` is ``bb / n -
    outer(b, b) / n**2`` with n = <psi|psi>, the connected correlator of the normalised state.

    sigma_a . sigma_b = 2 P_ab - 1 with P_ab the exchange of the two spins, so both come from the Gram matrix G of the
    swapped amplitudes: ``b[m] = 2 G[0, 1 + m] - G[0, 0]`` and ``bb[m, m'] = 4 G[1 + m, 1 + m'] - 2 G[1 + m, 0] - 2 G[0, 1
    + m'] + G[0, 0]``.  An exchange commutes with the global spin flip: states on XParity subspaces are served as they
    lie.  Full, Parity and SpinConserve states and XParity over those, on one process.  One call of the kernel takes 63
    bonds; longer lists are cut into chunks of 31 and every pair of chunks takes one call."""
    state.assert_initialized()
    config._initialize()
    sp, _ = _swap_subspace(state)
    bonds = np.asarray(bonds, dtype=np.int64)
    if bonds.size == 0:
        raise ValueError('bond correlations of an empty list of bonds')
    if bonds.ndim != 2 or bonds.shape[1] != 2:
        raise ValueError('bonds must be pairs of sites, not an array of shape %r' % (bonds.shape,))
    if bonds.min() < 0 or bonds.max() >= sp.L:
        raise ValueError('a bond has a site outside [0, %d)' % sp.L)
    if np.any(bonds[:, 0] == bonds[:, 1]):
        raise ValueError('a bond joins a site to itself')
    G = _swap_gram(state, bonds)
    n = G[0, 0].real
    b = 2.0 * G[0, 1:].real - n
    # (the two cross terms are added to each other first: bb is then Hermitian to the last bit, as G is)
    bb = 4.0 * G[1:, 1:] - 2.0 * (G[1:, :1] + G[:1, 1:]) + G[0, 0]
    if connected:
        bb = bb / n - np.outer(b, b) / n ** 2
    return b, bb


_CYC_CALL_MAX = 31        # triangles of one call of backend.cyc_moments: two columns each, 63 in all
_CYC_CHUNK = 15           # longer lists: chunks of this size, one call per pair of chunks on their union


def _cyc_gram(state, triangles):
    """G of backend.cyc_moments for any number of triangles, with the columns 1 + 2 t for the rotation of (a, b, c) and
    2 + 2 t for that of (a, c, b), its inverse."""
    from . import backend
    sp, sector = _swap_subspace(state, 'chirality correlations')
    sub_c = sp._to_c()
    n = len(triangles)

    def both_senses(sel):
        t = triangles[sel]
        return np.stack([t, t[:, [0, 2, 1]]], axis=1).reshape(-1, 3)

    if n <= _CYC_CALL_MAX:
        return backend.cyc_moments(state.vec, sub_c, both_senses(np.arange(n)), sector)
    G = np.zeros((2 * n + 1, 2 * n + 1), dtype=np.complex128)
    chunks = [np.arange(lo, min(lo + _CYC_CHUNK, n)) for lo in range(0, n, _CYC_CHUNK)]
    for i in range(len(chunks)):
        for j in range(i + 1, len(chunks)):
            # (with more than one chunk every chunk has a partner: the diagonal blocks come with the pairs)
            sel = np.concatenate([chunks[i], chunks[j]])
            g = backend.cyc_moments(state.vec, sub_c, both_senses(sel), sector)
            at = np.concatenate([[0], np.stack([1 + 2 * sel, 2 + 2 * sel], axis=1).reshape(-1)])
            G[np.ix_(at, at)] = g
    return G


def chirality_correlations(state, triangles, connected=False):
    """Every scalar chirality and every chirality-chirality correlator of a list of triangles from one pass over
    ``state`` (one matrix-core kernel, ``backend.cyc_moments``) instead of one ``Operator.expectation`` of a product of
    two six-term three-body operators per pair of triangles.  ``triangles`` is a list of triples of pairwise distinct
    sites (a, b, c); a triangle may repeat, triangles may share sites, and the orientation is the caller's
    (``lattices.kagome_triangles`` gives every triangle of the kagome torus the same sense).  Returns ``(chi, cc)``:
    ``chi[t]`` = <psi|sigma_a . (sigma_b x sigma_c)|psi>, float64, and ``cc[t, t']`` = <psi|chi_t chi_t'|psi>,
    complex128 and Hermitian (real for a real state), nothing normalised, as ``expectation`` normalises nothing.
    ``connected``: ``cc`` is ``cc / n - outer(chi, chi) / n**2`` with n = <psi|psi>, the connected correlator of the
    normalised state.

    For spin 1/2, sigma_a . (sigma_b x sigma_c) = 2i (C - C^H) with C = P_ab P_bc the rotation of the three spins, and
    C^H is the rotation of (a, c, b).  With the columns f = 1 + 2 t for (a, b, c) and b = 2 + 2 t for (a, c, b) of the Gram
    matrix G of the rotated amplitudes: ``chi[t] = -2 (Im G[0, f] - Im G[0, b])`` and ``cc[t, t'] = 4 (G[f, f'] + G[b, b']
    - G[f, b'] - G[b, f'])``; ``cc[t, t] = 8 G[0, 0] - 8 Re <C_t>`` (chi^2 is 12 on the two doublets of the three spins and
    0 on the quartet).  A permutation of sites commutes with the global spin flip: states on XParity subspaces are
    served as they lie.  Full, Parity and SpinConserve states and XParity over those, on one process.  One call of the
    kernel takes 31 triangles; longer lists are cut into chunks of 15 and every pair of chunks takes one call."""
    state.assert_initialized()
    config._initialize()
    sp, _ = _swap_subspace(state, 'chirality correlations')
    triangles = np.asarray(triangles, dtype=np.int64)
    if triangles.size == 0:
        raise ValueError('chirality correlations of an empty list of triangles')
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError('triangles must be triples of sites, not an array of shape %r' % (triangles.shape,))
    if triangles.min() < 0 or triangles.max() >= sp.L:
        raise ValueError('a triangle has a site outside [0, %d)' % sp.L)
    if np.any((triangles[:, 0] == triangles[:, 1]) | (triangles[:, 1] == triangles[:, 2])
              | (triangles[:, 2] == triangles[:, 0])):
        raise ValueError('the sites of a triangle must be pairwise distinct')
    G = _cyc_gram(state, triangles)
    n = G[0, 0].real
    F, B = G[1::2], G[2::2]             # rows of the two senses
    chi = -2.0 * (G[0, 1::2].imag - G[0, 2::2].imag)
    # (the like terms are added to each other first, then the cross terms: cc is then Hermitian to the last bit, as G
    # is)
    cc = 4.0 * ((F[:, 1::2] + B[:, 2::2]) - (F[:, 2::2] + B[:, 1::2]))
    if connected:
        cc = cc / n - np.outer(chi, chi) / n ** 2
    return chi, cc


_PAULI_CALL_MAX = 63      # columns of one call of backend.pauli_moments
_PAULI_CHUNK = 31         # longer lists: chunks of at most this size, one call per pair of chunks on their union
_PAULI_KINDS = (1, 2, 3)  # the kinds of backend.pauli_moments for the axis index 0, 1, 2 = x, y, z


def _pauli_subspace(state, what='Pauli correlations'):
    from .subspaces import Explicit, Full, Parity, SpinConserve, XParity
    sp = state.subspace
    if type(sp) is XParity:
        raise ValueError('%s of an XParity state: sigmaz_i does not commute with the global spin flip, so the sum over '
                         'the representatives is not the expectation value (expand the state first)' % what)
    if isinstance(sp, Explicit) or not isinstance(sp, (Full, Parity, SpinConserve)):
        raise ValueError('%s need a Full, Parity or SpinConserve subspace, not %r' % (what, sp))
    return sp


def _pauli_chunks(cols):
    """The columns ``cols`` (site, kind) cut into chunks of at most _PAULI_CHUNK: the flipping columns in the order of
    their sites, so that the sigma-x and sigma-y columns of a site (and repeats) share a chunk, a call and its loads
    wherever the site has no more columns than a chunk holds; then the columns that only sign."""
    flips = cols[:, 1] != 3
    order = np.concatenate([np.flatnonzero(flips)[np.argsort(cols[flips, 0], kind='stable')], np.flatnonzero(~flips)])
    groups, at = [], 0
    while at < len(order):
        c = order[at]
        end = at + 1
        while flips[c] and end < len(order) and flips[order[end]] and cols[order[end], 0] == cols[c, 0]:
            end += 1
        groups += [order[lo:min(lo + _PAULI_CHUNK, end)] for lo in range(at, end, _PAULI_CHUNK)]
        at = end
    chunks = [[]]
    for g in groups:
        if len(chunks[-1]) + len(g) > _PAULI_CHUNK:
            chunks.append([])
        chunks[-1].extend(g)
    return [np.array(c, dtype=np.int64) for c in chunks]


def _pauli_gram(state, cols):
    """G of backend.pauli_moments for any number of columns (site, kind): G[0, 0], G[0, 1 + c] and G[1 + c, 1 + c'] in
    the order of ``cols``, without the phase of the sigma-y columns."""
    from . import backend
    sub_c = state.subspace._to_c()
    cols = np.asarray(cols, dtype=np.int64).reshape(-1, 2)
    n = len(cols)
    if n <= _PAULI_CALL_MAX:
        return backend.pauli_moments(state.vec, sub_c, cols)
    G = np.zeros((n + 1, n + 1), dtype=np.complex128)
    chunks = _pauli_chunks(cols)
    for i in range(len(chunks)):
        for j in range(i + 1, len(chunks)):
            # (with more than one chunk every chunk has a partner: the diagonal blocks come with the pairs)
            sel = np.concatenate([chunks[i], chunks[j]])
            g = backend.pauli_moments(state.vec, sub_c, cols[sel])
            at = np.concatenate([[0], 1 + sel])
            G[np.ix_(at, at)] = g
    return G


def _pauli_sites(state, sites):
    L = state.subspace.L
    sites = np.arange(L, dtype=np.int64) if sites is None else np.asarray(sites, dtype=np.int64)
    if sites.size == 0:
        raise ValueError('Pauli correlations of an empty list of sites')
    if sites.ndim != 1:
        raise ValueError('sites must be a list of sites, not an array of shape %r' % (sites.shape,))
    if sites.min() < 0 or sites.max() >= L:
        raise ValueError('a site outside [0, %d)' % L)
    return sites


def _pauli_from_u1(state, sites):
    """(one, two) of a SpinConserve state from the sigma-z and the sigma+ sigma- pass: the flipping operators come in
    the pairs that conserve the magnetisation only."""
    mz, zz = sigmaz_correlations(state)
    pm = sigma_pm_correlations(state)
    n = len(sites)
    at = np.ix_(sites, sites)
    one = np.zeros((3, n))
    one[2] = mz[sites]
    two = np.zeros((3, n, 3, n), dtype=np.complex128)
    half = 0.5 * pm[at]
    two[0, :, 0, :] = half.real
    two[1, :, 1, :] = half.real
    two[1, :, 0, :] = half.imag
    two[0, :, 1, :] = -half.imag
    two[2, :, 2, :] = zz[at]
    # the same site twice: sigma^a sigma^a = 1 and sigmax sigmay = i sigmaz (sigmay sigmaz = i sigmax and sigmaz sigmax
    # = i sigmay have no expectation value in the sector)
    norm2 = zz[0, 0]
    same = sites[:, None] == sites[None, :]
    for a in range(2):
        two[a, :, a, :][same] = norm2
    i_mz = 1j * np.broadcast_to(mz[sites][:, None], (n, n))
    two[0, :, 1, :][same] = i_mz[same]
    two[1, :, 0, :][same] = -i_mz[same]
    return one, two


def pauli_correlations(state, sites=None):
    """Every single-site Pauli expectation value and every two-site Pauli correlator of ``state`` on the spins ``sites``
    (default: all of them; a site may repeat) from one pass over it (one matrix-core kernel, ``backend.pauli_moments``)
    instead of one ``Operator.expectation`` per correlator, each a multiply and a temporary vector -- for the states
    without a U(1) symmetry, where <sigmax sigmax> != <sigmay sigmay> and <sigmax sigmaz> and <sigmax> need not vanish.
    Returns ``(one, two)`` with the axis index a = 0, 1, 2 for x, y, z: ``one[a, i]`` = <psi|sigma^a_{s_i}|psi>, float64
    of shape (3, n), and ``two[a, i, b, j]`` = <psi|sigma^a_{s_i} sigma^b_{s_j}|psi>, complex128 of shape (3, n, 3, n),
    nothing normalised, as ``expectation`` normalises nothing.  Entries at the same site follow from the definition:
    ``two[0, i, 1, i]`` = i <sigmaz_i> and ``two[a, i, a, i]`` = <psi|psi>.  Reshaped to 3n x 3n, ``two`` is Hermitian to
    the last bit.

    sigmax_j psi, i sigmay_j psi and sigmaz_j psi are each one partner amplitude times a sign; ``two`` is the Gram
    matrix of those columns with the phase -i of sigma-y applied afterwards (the row times the conjugate phase, the
    column times the phase: both exact).  One call of the kernel takes 63 columns; longer lists (all sites from L = 22
    on) are cut into chunks of at most 31 and every pair of chunks takes one call.  Full and Parity states on one
    process; on Parity the entries with an odd number of flips are exact zeros.  SpinConserve states are assembled from
    ``sigmaz_correlations`` and ``sigma_pm_correlations`` (XX = YY = Re pm / 2, YX = -XY = Im pm / 2, nothing else with
    a flip survives).  XParity states are refused: sigmaz_i does not commute with the global flip."""
    from .subspaces import SpinConserve
    state.assert_initialized()
    config._initialize()
    sp = _pauli_subspace(state)
    sites = _pauli_sites(state, sites)
    if isinstance(sp, SpinConserve):
        return _pauli_from_u1(state, sites)
    n = len(sites)
    # column 3 i + a of the list: kind a + 1 at site s_i
    cols = np.stack([np.repeat(sites, 3), np.tile(_PAULI_KINDS, n)], axis=1)
    G = _pauli_gram(state, cols)
    phase = np.tile(np.array([1.0, -1j, 1.0]), n)
    one = (G[0, 1:] * phase).real.reshape(n, 3).T.copy()
    two = (np.conj(phase)[:, None] * G[1:, 1:]) * phase[None, :]
    return one, two.reshape(n, 3, n, 3).transpose(1, 0, 3, 2).copy()


_PAULI_MATRICES = np.array([[[1, 0], [0, 1]], [[0, 1], [1, 0]], [[0, -1j], [1j, 0]], [[1, 0], [0, -1]]],
                           dtype=np.complex128)       # 1, x, y, z on (clear bit, set bit)


def _pair_density_matrices(one, two, norm2, at):
    """rho_ij for the pairs ``at`` of positions in the site list of (one, two): the index of the basis is bit_i + 2 bit_j,
    as reduced_density_matrix(state, [i, j]) has it."""
    out = np.empty((len(at), 4, 4), dtype=np.complex128)
    for n, (i, j) in enumerate(at):
        # c[a, b] = <sigma^a_i sigma^b_j> with a, b = 0 for the identity
        c = np.empty((4, 4), dtype=np.complex128)
        c[0, 0] = norm2
        c[1:, 0] = one[:, i]
        c[0, 1:] = one[:, j]
        c[1:, 1:] = two[:, i, :, j]
        out[n] = np.einsum('ab,bkl,amn->kmln', c, _PAULI_MATRICES, _PAULI_MATRICES).reshape(4, 4) / (4.0 * norm2)
    return out


def two_site_density_matrices(state, pairs=None):
    """The reduced density matrices of pairs of spins from the Pauli correlators of one pass over ``state``
    (``pauli_correlations``) instead of one ``reduced_density_matrix`` per pair: array of shape (len(pairs), 4, 4),
    complex128, ``rho_ij = 1/4 sum_{a, b in 1, x, y, z} <sigma^a_i sigma^b_j> sigma^a (x) sigma^b / <psi|psi>`` in the
    basis order of ``reduced_density_matrix(state, [i, j])``.  ``pairs`` are (i, j) with i < j; default: all of them."""
    state.assert_initialized()
    _pauli_subspace(state, 'two-site density matrices')
    L = state.subspace.L
    if pairs is None:
        pairs = [(i, j) for i in range(L) for j in range(i + 1, L)]
    pairs = np.asarray(pairs, dtype=np.int64)
    if pairs.size == 0:
        raise ValueError('two-site density matrices of an empty list of pairs')
    if pairs.ndim != 2 or pairs.shape[1] != 2:
        raise ValueError('pairs must be pairs of sites, not an array of shape %r' % (pairs.shape,))
    if pairs.min() < 0 or pairs.max() >= L:
        raise ValueError('a pair has a site outside [0, %d)' % L)
    if np.any(pairs[:, 0] >= pairs[:, 1]):
        raise ValueError('a pair (i, j) must have i < j')
    sites, at = np.unique(pairs, return_inverse=True)
    one, two = pauli_correlations(state, sites)
    return _pair_density_matrices(one, two, two[0, 0, 0, 0].real, at.reshape(-1, 2))


def mutual_information(state, sites=None):
    """The mutual information ``I_ij = S_i + S_j - S_ij`` (natural logarithm) of every pair of the spins ``sites``
    (default: all of them) from the Pauli correlators of one pass over ``state``: (n, n) float64, symmetric with a zero
    diagonal.  The spectra of the one- and two-site density matrices come from ``numpy.linalg.eigvalsh``, clipped at 0."""
    state.assert_initialized()
    _pauli_subspace(state, 'mutual information')
    sites = _pauli_sites(state, sites)
    one, two = pauli_correlations(state, sites)
    n = len(sites)
    norm2 = two[0, 0, 0, 0].real

    def entropy(rho):
        return _entropy_of_spectrum(np.clip(np.linalg.eigvalsh(rho), 0.0, None))

    single = [entropy(0.5 * (_PAULI_MATRICES[0] + np.einsum('a,akl->kl', one[:, i] / norm2, _PAULI_MATRICES[1:])))
              for i in range(n)]
    out = np.zeros((n, n))
    at = [(i, j) for i in range(n) for j in range(i + 1, n)]
    if at:
        for (i, j), rho in zip(at, _pair_density_matrices(one, two, norm2, at)):
            out[i, j] = out[j, i] = single[i] + single[j] - entropy(rho)
    return out


_GRAM_CALL_MAX = 64       # vectors of one call of backend.vec_gram
_GRAM_CHUNK = 32          # longer lists: chunks of at most this size, one call per pair of chunks


def _gram_states(states, what):
    """The list ``states``, checked: not empty, every state initialised, all on one subspace."""
    states = list(states)
    if not states:
        raise ValueError('%s of an empty list of states' % what)
    for s in states:
        s.assert_initialized()
    if any(not s.subspace.identical(states[0].subspace) for s in states[1:]):
        raise ValueError('%s: the states must all be on the same subspace' % what)
    return states


def _gram_chunks(n):
    return [np.arange(lo, min(lo + _GRAM_CHUNK, n)) for lo in range(0, n, _GRAM_CHUNK)]


def overlap_matrix(states, others=None):
    """The overlaps of many states from one pass over them (one matrix-core kernel, ``backend.vec_gram``) instead of
    one ``State.dot`` -- a launch and a host synchronisation -- per pair: complex128 numpy array ``S[a, b]`` =
    <states[a]|states[b]>, or with ``others`` of shape (len(states), len(others)), ``S[a, b]`` = <states[a]|others[b]>.
    The inner product is conjugate-linear in its first argument and nothing is normalised.  All states must be
    initialised and on one subspace.  Up to 64 columns in all -- ``len(states) + len(others)`` -- take one call; longer
    lists are cut into chunks of at most 32 and every pair of chunks takes one call.  Without ``others`` the result is
    Hermitian to the last bit and its diagonal is real, chunked or not.  States on one process."""
    from . import backend
    config._initialize()
    states = _gram_states(states, 'overlap matrix')
    if others is None:
        n = len(states)
        if n <= _GRAM_CALL_MAX:
            return backend.vec_gram([s.vec for s in states])
        S = np.zeros((n, n), dtype=np.complex128)
        chunks = _gram_chunks(n)
        for i in range(len(chunks)):
            for j in range(i + 1, len(chunks)):
                # (with more than one chunk every chunk has a partner: the diagonal blocks come with the pairs)
                sel = np.concatenate([chunks[i], chunks[j]])
                S[np.ix_(sel, sel)] = backend.vec_gram([states[k].vec for k in sel])
        return S
    others = _gram_states(others, 'overlap matrix')
    if not others[0].subspace.identical(states[0].subspace):
        raise ValueError('overlap matrix: the states must all be on the same subspace')
    ns, no = len(states), len(others)
    if ns + no <= _GRAM_CALL_MAX:
        return backend.vec_gram([s.vec for s in states + others])[:ns, ns:].copy()
    S = np.zeros((ns, no), dtype=np.complex128)
    for ci in _gram_chunks(ns):
        for cj in _gram_chunks(no):
            g = backend.vec_gram([states[k].vec for k in ci] + [others[k].vec for k in cj])
            S[np.ix_(ci, cj)] = g[:len(ci), len(ci):]
    return S


_PERM_CALL_MAX = 64       # permutations of one call of backend.perm_apply / backend.perm_dots


def _site_perms(state, perms, what, single=False):
    """(subspace whose ``_to_c()`` the pass takes, XParity sector or 0, int32 array (G, L)) for a state and a site
    permutation (``single``) or a list of them, checked: the right length, every row a bijection of [0, L)."""
    state.assert_initialized()
    sp, sector = _swap_subspace(state, what)
    L = sp.L
    perms = np.asarray(perms)
    if single:
        if perms.ndim != 1:
            raise ValueError('%s: a site permutation is a one-dimensional array, not one of shape %r'
                             % (what, perms.shape))
        perms = perms.reshape(1, -1)
    if perms.size == 0:
        raise ValueError('%s of an empty list of permutations' % what)
    if perms.ndim != 2 or perms.shape[1] != L:
        raise ValueError('%s: a site permutation of %d sites has length %d, not an array of shape %r'
                         % (what, L, L, perms.shape))
    if not np.issubdtype(perms.dtype, np.integer):
        raise ValueError('%s: site permutations are arrays of integers' % what)
    if not np.array_equal(np.sort(perms, axis=1), np.broadcast_to(np.arange(L), perms.shape)):
        bad = int(np.flatnonzero(np.any(np.sort(perms, axis=1) != np.arange(L), axis=1))[0])
        raise ValueError('%s: permutation %d is not a bijection of [0, %d) (a site outside the range, or a repeated '
                         'site)' % (what, bad, L))
    return sp, sector, np.ascontiguousarray(perms, dtype=np.int32)


def _perm_result(state, result, what):
    from .states import State
    if result is state:
        raise ValueError('%s: the result must be another state than the input (the pass gathers)' % what)
    if result is None:
        result = State(L=state.L, subspace=state.subspace)
    elif result.subspace != state.subspace:
        raise ValueError('subspace of state and result must match')
    return result


def permute_sites(state, perm, result=None):
    """P_pi|state> for the site permutation ``perm`` = pi, an int array of length L and a bijection of [0, L): P_pi moves
    the spin at site i to site pi(i), P_pi|c> = |c'> with c'_{pi(i)} = c_i, so (P_pi psi)(c') = psi(c) where the source
    configuration c has bit i equal to bit pi(i) of c'; hence P_pi sigma^a_i P_pi^H = sigma^a_{pi(i)}.  One gather pass on
    the device (``backend.perm_apply``), which rounds nothing: the result holds the bits of the state.  A permutation
    keeps the number of up spins and the parity and commutes with the global flip: Full, Parity and SpinConserve states
    and XParity over those, on one process; Explicit and Auto are refused.  ``result``: a state on the same subspace to
    write into -- not ``state`` itself, which raises ``ValueError``."""
    from . import backend
    config._initialize()
    sp, sector, perms = _site_perms(state, perm, 'site permutation', single=True)
    result = _perm_result(state, result, 'site permutation')
    backend.perm_apply(state.vec, sp._to_c(), perms, [1.0], result.vec, sector)
    result.set_initialized()
    return result


def symmetrize(state, perms, characters=None, result=None):
    """(1 / G) sum_g conj(chi_g) P_g|state> for the G site permutations ``perms`` (the convention of ``permute_sites``)
    and the characters ``characters`` = chi, all ones when None: with the elements of a group and the characters of a
    one-dimensional representation, the projection of the state onto it -- e.g. ``lattices.chain_translations(L)`` with
    chi_g = exp(-2 pi i k g / L) for the momentum 2 pi k / L, in which P_1 has the eigenvalue chi_1.  One pass over the
    state per 64 permutations (``backend.perm_apply``), the later ones accumulating.  Nothing is normalised.  Subspaces
    and ``result`` as for ``permute_sites``."""
    from . import backend
    config._initialize()
    sp, sector, perms = _site_perms(state, perms, 'symmetrize')
    G = perms.shape[0]
    chi = np.ones(G, dtype=np.complex128) if characters is None else np.asarray(characters, dtype=np.complex128).reshape(-1)
    if chi.size != G:
        raise ValueError('symmetrize: %d characters for %d permutations' % (chi.size, G))
    result = _perm_result(state, result, 'symmetrize')
    coef = chi.conj() / G
    sub_c = sp._to_c()
    for lo in range(0, G, _PERM_CALL_MAX):
        hi = min(lo + _PERM_CALL_MAX, G)
        backend.perm_apply(state.vec, sub_c, perms[lo:hi], coef[lo:hi], result.vec, sector, accumulate=lo > 0)
    result.set_initialized()
    return result


def symmetry_expectations(state, perms, other=None):
    """<other|P_g|state> for every site permutation of ``perms`` (the convention of ``permute_sites``), ``other`` being
    ``state`` when None: complex128 numpy array of shape (G,), nothing normalised, as ``expectation`` normalises
    nothing.  One pass over the two states per 64 permutations (``backend.perm_dots``); two calls return the same
    bits.  With the elements of the space group of a lattice these are the numbers that label an eigenstate by momentum
    and point-group quantum number.  Subspaces as for ``permute_sites``; ``other`` must be on the subspace of
    ``state``."""
    from . import backend
    config._initialize()
    sp, sector, perms = _site_perms(state, perms, 'symmetry expectations')
    if other is None:
        other = state
    else:
        other.assert_initialized()
        if not other.subspace.identical(state.subspace):
            raise ValueError('symmetry expectations: the two states must be on the same subspace')
    sub_c = sp._to_c()
    out = [backend.perm_dots(other.vec, state.vec, sub_c, perms[lo:lo + _PERM_CALL_MAX], sector)
           for lo in range(0, perms.shape[0], _PERM_CALL_MAX)]
    return np.concatenate(out)


def symmetry_representation(states, perms):
    """``D[g, m, n]`` = <states[m]|P_g|states[n]> for a list of N states -- a multiplet -- and G site permutations (the
    convention of ``permute_sites``): complex128 numpy array of shape (G, N, N), nothing normalised; for an orthonormal
    basis of an invariant space, the matrices of the representation it carries, whose traces are its characters.  One
    ``symmetry_expectations`` per pair of states.  All states must be initialised and on one subspace."""
    states = _gram_states(states, 'symmetry representation')
    _, _, perms = _site_perms(states[0], perms, 'symmetry representation')
    N = len(states)
    D = np.empty((perms.shape[0], N, N), dtype=np.complex128)
    for m in range(N):
        for n in range(N):
            D[:, m, n] = symmetry_expectations(states[n], perms, other=states[m])
    return D


def _map_side(subspace, what):
    """(subspace whose ``_to_c()`` the subspace maps take, XParity sector or 0): Full, Parity, SpinConserve, Explicit
    and Auto, and XParity over those (the descriptor is then the parent's)."""
    from .subspaces import Explicit, Full, Parity, SpinConserve, XParity
    base, sector = (subspace.parent, int(subspace.sector)) if type(subspace) is XParity else (subspace, 0)
    if not isinstance(base, (Full, Parity, SpinConserve, Explicit)):
        raise ValueError('%s need a Full, Parity, SpinConserve, Explicit or Auto subspace, or XParity over one of them, '
                         'not %r' % (what, subspace))
    return subspace, sector


def to_subspace(state, subspace, result=None):
    """``state`` moved to ``subspace``, a subspace of the same spins, as a new ``State`` on it (or into ``result``, a
    state on ``subspace``): the orthogonal projection, onto the span of ``subspace``, of the state seen as a vector of
    the whole 2^L space -- an embedding when the configurations of the state's subspace lie in ``subspace`` (a
    SpinConserve or XParity eigenvector taken to Full, where ``apply_site_operators``, ``sample(bases=...)`` and the
    Pauli correlators accept it), a restriction the other way round.  One gather pass over the target on the device
    (``backend.subspace_map``); nothing travels through the host.  It is not normalised: the squared norm of the result
    is the weight of the state inside the target subspace, 1 for an embedding of a normalised state.  Full, Parity,
    SpinConserve, Explicit and Auto on either side, and XParity over those (``XParity.convert_state`` does the two cases
    sector <-> parent on the host and agrees to rounding: it divides by sqrt(2) where this pass multiplies by
    0.70710678118654752440).  Between two plain subspaces and between two XParity sectors the result holds the bits of
    the state.  One process; on more it raises ``NotImplementedError``."""
    from . import backend
    from .states import State
    config._initialize()
    state.assert_initialized()
    what = 'subspace maps'
    if subspace.L is None:
        subspace = subspace.copy()
        subspace.L = state.L
    if subspace.L != state.L:
        raise ValueError('%s: a state of %d spins and a subspace of %d' % (what, state.L, subspace.L))
    src, ssec = _map_side(state.subspace, what)
    dst, dsec = _map_side(subspace, what)
    if result is state:
        raise ValueError('%s: the result must be another state than the input (the pass gathers)' % what)
    if result is None:
        result = State(L=state.L, subspace=subspace)
    elif result.subspace != subspace:
        raise ValueError('subspace of result must be the target subspace')
    backend.subspace_map(state.vec, src._to_c(), result.vec, result.subspace._to_c(), ssec, dsec)
    result.set_initialized()
    return result


def sector_weights(state):
    """``(magnetization, flip)`` of a state from one streaming pass over it on the device
    (``backend.sector_weights``).  ``magnetization``: array of L + 1 numbers, entry k the sum of |psi(c)|^2 over the
    configurations c with k set bits -- the full counting statistics of the magnetisation, and the squared norm
    ``to_subspace(SpinConserve(L, k))`` keeps.  ``flip``: array (F+, F-), the squared norms the two sectors of the global
    spin flip keep (``to_subspace(XParity(..., '+'))`` and ``'-'``), or ``None`` where the flip is not defined: on
    Explicit and Auto subspaces, Parity with odd L and SpinConserve away from half filling.  Neither is normalised; two
    calls return the same bits.  Subspaces as for ``to_subspace``; one process."""
    from . import backend
    from .subspaces import Explicit
    config._initialize()
    state.assert_initialized()
    sp, sector = _map_side(state.subspace, 'sector weights')
    base = sp.parent if sector else sp
    has_flip = bool(sector) or (not isinstance(base, Explicit) and _carries_flip(base))
    return backend.sector_weights(state.vec, sp._to_c(), sector, flip=has_flip)


def _carries_flip(subspace):
    """Does a Full, Parity or SpinConserve subspace carry the global spin flip (its rows i and dim - 1 - i are then
    complements of each other)?"""
    from .subspaces import Full, XParity
    return isinstance(subspace, Full) or XParity._flip_closed(subspace) is None


def _entropy_of_spectrum(w):
    log = np.zeros(w.shape)
    np.log(w, where=w > 0, out=log)
    return -np.sum(w * log)


def entanglement_entropy(state, keep):
    """Bipartite entanglement entropy across the cut keep | rest (computations.py:351-383)."""
    w = _spectrum(state, keep)
    if w is None:                # everything is computed on process 0
        return -1
    return _entropy_of_spectrum(w)


def dm_entanglement_entropy(dm):
    """Von Neumann entropy of a density matrix (computations.py:385-408)."""
    return _entropy_of_spectrum(np.linalg.eigvalsh(dm))


def renyi_entropy(state, keep, alpha, method='eigsolve'):
    """Renyi entropy of the reduced density matrix (computations.py:410-454)."""
    if method == 'eigsolve' or alpha in (0, 1, 'inf'):
        w = _spectrum(state, keep)
        if w is None:
            return -1
        return _renyi_of_spectrum(w, alpha)
    reduced = reduced_density_matrix(state, keep)
    if reduced[0, 0] == -1:
        return -1
    return dm_renyi_entropy(reduced, alpha, method)


def _renyi_of_spectrum(eigs, alpha):
    if alpha == 0:
        return np.log(np.sum(eigs > 1E-10))
    if alpha == 1:
        return _entropy_of_spectrum(eigs)
    if alpha == 'inf':
        return -np.log(np.max(eigs))
    return 1 / (1 - alpha) * np.log(np.sum(eigs ** alpha))


def dm_renyi_entropy(dm, alpha, method='eigsolve'):
    """H_alpha = log Tr rho^alpha / (1 - alpha), with the alpha = 0, 1, 'inf' limits
    (computations.py:456-507)."""
    if alpha == 0:
        eigs = np.linalg.eigvalsh(dm)
        return np.log(np.sum(eigs > 1E-10))
    if alpha == 1:
        return dm_entanglement_entropy(dm)
    if alpha == 'inf':
        return -np.log(np.max(np.linalg.eigvalsh(dm)))
    if method == 'matrix_power':
        if alpha == int(alpha):
            trace = np.trace(np.linalg.matrix_power(dm, int(alpha))).real
        else:
            raise TypeError('alpha must be an integer for matrix_power method.')
    elif method == 'eigsolve':
        trace = np.sum(np.linalg.eigvalsh(dm) ** alpha)
    else:
        raise ValueError('Valid methods are "eigsolve" and "matrix_power"')
    return 1 / (1 - alpha) * np.log(trace)


def get_tstep(ncv, nrm, tol=1E-7):
    """First-step size of an Expokit solve (computations.py:511-519)."""
    f = ((ncv + 1) / 2.72) ** (ncv + 1) * np.sqrt(2 * np.pi * (ncv + 1))
    t = ((1 / nrm) * (f * tol) / (4.0 * nrm)) ** (1 / ncv)
    s = 10.0 ** (np.floor(np.log10(t)) - 1)
    return np.ceil(t / s) * s


def estimate_compute_time(t, ncv, nrm, tol=1E-7):
    """Cost estimate in matrix multiplies (computations.py:521-528)."""
    return ncv * np.ceil(t / get_tstep(ncv, nrm, tol))
