"""The dense reference of the rectangular-operator tests (tests/test_gpu_rectangular.py) and its own checks.

An operator whose left and right subspaces differ is D = A[left states][:, right states], A the dense 2^L x 2^L matrix of
the MSC term list: for a term (mask m, sign s, coefficient c) and a column state b, A[b ^ m, b] += (-1)^popcount(b & s) c.
That is all of it, in numpy, without the library's index maps or the C oracle: the states of a subspace are written down
here as well (Full: all; Parity: the states of that parity, ascending; SpinConserve: the states of that popcount,
ascending, which is colex order; Explicit: the list as given).

The cases are made so that arithmetic is exact in double: every coefficient is a multiple of 1/8 (1/64 for the projector),
every amplitude a Gaussian integer with parts in [-8, 8] \\ {0}.  Every product and every partial sum is then a multiple of
1/64 far below 2^53 / 64, whatever the order of summation -- a multiply is compared bit for bit, and no tolerance has to
be chosen.

This file runs without a GPU: it checks the builder against the oracle's matvec, infinity norm and CheckConserves on all
49 ordered pairs of the seven subspaces, and the conditions that keep the GPU file from passing vacuously.
"""
import numpy as np
import pytest

from gpu_util import marshal
from oracle import oracle as orc

L = 10
NAMES = ("full", "even", "odd", "sc5", "sc4", "expA", "expB")
TYPE = {"full": "F", "even": "P", "odd": "P", "sc5": "S", "sc4": "S", "expA": "E", "expB": "E"}
PAIRS = [(ln, rn) for ln in NAMES for rn in NAMES]


def popcount(a):
    a = np.asarray(a, dtype=np.int64)
    n = np.zeros(a.shape, dtype=np.int64)
    for b in range(63):
        n += (a >> b) & 1
    return n


def explicit_lists(nbits=L, na=300, nb=210):
    """A: ``na`` sorted states.  B: ``nb`` states of another seed in shuffled order, states 0 and 2^nbits - 1 among them."""
    dim = 1 << nbits
    a = np.sort(np.random.RandomState(41).choice(dim, size=na, replace=False)).astype(np.int64)
    rs = np.random.RandomState(97)
    b = np.concatenate([[0, dim - 1], 1 + rs.choice(dim - 2, size=nb - 2, replace=False)]).astype(np.int64)
    b = b[rs.permutation(nb)]
    return a, b


def states_of(name, nbits=L):
    """The states of a subspace in index order (int64)."""
    s = np.arange(1 << nbits, dtype=np.int64)
    if name == "full":
        return s
    if name in ("even", "odd"):
        return s[(popcount(s) & 1) == (name == "odd")]
    if name.startswith("sc"):
        return s[popcount(s) == int(name[2:])]
    return explicit_lists(nbits)[name == "expB"]


def make_subspace(name, nbits=L):
    """The library's subspace object of that name."""
    from dynamite_amd.subspaces import Explicit, Full, Parity, SpinConserve
    if name == "full":
        return Full(L=nbits)
    if name in ("even", "odd"):
        return Parity(name, L=nbits)
    if name.startswith("sc"):
        return SpinConserve(nbits, int(name[2:]))
    return Explicit(states_of(name, nbits), L=nbits)


def orc_subspace(name, nbits=L):
    if name == "full":
        return orc.full(nbits)
    if name in ("even", "odd"):
        return orc.parity(nbits, int(name == "odd"))
    if name.startswith("sc"):
        return orc.spin_conserve(nbits, int(name[2:]))
    return orc.explicit(nbits, states_of(name, nbits))


# ---------------------------------------------------------------------- operators
def pauli_operator():
    """A seeded sum of Pauli strings of X, Y, Z on up to five sites, coefficients k / 8: a pure-Z string (mask 0), X_0 X_3
    and X_0 Y_3 on one mask (a real and an imaginary term), single flips (they change parity and magnetisation) and 26
    random strings."""
    from dynamite_amd.operators import sigmax, sigmay, sigmaz, op_sum, op_product
    rs = np.random.RandomState(2024)
    P = (sigmax, sigmay, sigmaz)
    terms = [0.625 * sigmaz(1) * sigmaz(4) * sigmaz(7), 0.5 * sigmax(0) * sigmax(3), 0.375 * sigmax(0) * sigmay(3),
             -0.25 * sigmax(2), 0.125 * sigmay(9)]
    for _ in range(26):
        sites = rs.choice(L, size=int(rs.randint(1, 6)), replace=False)
        k = int(rs.choice([-8, -7, -6, -5, -4, -3, -2, -1, 1, 2, 3, 4, 5, 6, 7, 8]))
        terms.append(k / 8.0 * op_product([P[int(rs.randint(3))](int(i)) for i in sites]))
    H = op_sum(terms)
    H.L = L
    return H


def heisenberg_operator():
    from dynamite_amd import models
    return models.heisenberg(L)


def projector_arrays(nbits, config):
    """prod_i (1 +- sigma_z_i) / 2 onto the one configuration ``config``: 2^nbits terms of +-2^-nbits on mask 0 -- the
    diagonal is 1 at ``config`` and cancels to an exact zero everywhere else."""
    signs = np.arange(1 << nbits, dtype=np.int64)
    coeffs = (1 - 2 * (popcount(signs & config) & 1)) / float(1 << nbits)
    return (np.zeros(1, dtype=np.int64), np.array([0, 1 << nbits], dtype=np.int64), signs, coeffs.astype(np.complex128))


_CACHE = {}


def operator_arrays(opname):
    if opname not in _CACHE:
        _CACHE[opname] = marshal({"pauli": pauli_operator, "heisenberg": heisenberg_operator}[opname]())
    return _CACHE[opname]


def dense(arrs, nbits=L):
    """The 2^nbits x 2^nbits matrix of an MSC term list, straight from the definition."""
    masks, offs, signs, coeffs = arrs
    dim = 1 << nbits
    A = np.zeros((dim, dim), dtype=np.complex128)
    b = np.arange(dim, dtype=np.int64)
    for m, mask in enumerate(masks):
        for t in range(offs[m], offs[m + 1]):
            A[b ^ int(mask), b] += (1 - 2 * (popcount(b & int(signs[t])) & 1)) * coeffs[t]
    return A


def dense_of(opname):
    key = ("dense", opname)
    if key not in _CACHE:
        _CACHE[key] = dense(operator_arrays(opname))
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def block(A, left, right):
    """D = A[left states][:, right states].  ``left`` / ``right``: names of the L = 10 subspaces, or arrays of states."""
    lst, rst = (states_of(s) if isinstance(s, str) else s for s in (left, right))
    return A[np.ix_(lst, rst)]


def conserves_dense(A, left, right):
    """CheckConserves, dense: the rows of A outside the left subspace, restricted to the columns in the right one, are all
    zero.  ``left`` / ``right``: names of the L = 10 subspaces, or arrays of states."""
    lst, rst = (states_of(s) if isinstance(s, str) else s for s in (left, right))
    out = np.ones(A.shape[0], dtype=bool)
    out[lst] = False
    return not A[np.ix_(np.flatnonzero(out), rst)].any()


def infnorm_dense(D):
    return float(np.abs(D).sum(axis=1).max()) if D.size else 0.0


def gauss_ints(n, seed):
    """n Gaussian integers, real and imaginary parts in [-8, 8] and none of them zero"""
    rs = np.random.RandomState(seed)
    vals = np.array([-8, -7, -6, -5, -4, -3, -2, -1, 1, 2, 3, 4, 5, 6, 7, 8], dtype=np.float64)
    return rs.choice(vals, size=n) + 1j * rs.choice(vals, size=n)


def mixes_real_and_imaginary(arrs):
    """Does any mask carry both a real and an imaginary term?  (Where none does, row sums of |D_ij| are sums of |reals|.)"""
    masks, offs, signs, coeffs = arrs
    return any(np.any(coeffs[offs[m]:offs[m + 1]].real != 0) and np.any(coeffs[offs[m]:offs[m + 1]].imag != 0)
               for m in range(masks.size))


# Heisenberg conserves the magnetisation (and with it the parity): a pair has no matrix element at all exactly when no
# popcount occurs on both sides.  The open chain of 10 sites has 9 ZZ bonds, so its diagonal, a sum of nine +-1/4, is
# never zero: two subspaces that share a state are coupled.
HEISENBERG_ZERO_PAIRS = [("even", "odd"), ("even", "sc5"), ("odd", "even"), ("odd", "sc4"), ("sc5", "even"), ("sc5", "sc4"),
                         ("sc4", "odd"), ("sc4", "sc5")]

# CheckConserves at L = 6 with the projector onto CONFIG (three spins down: odd parity): the verdict is True exactly when
# the left subspace holds CONFIG or the right one does not
PBITS, CONFIG = 6, 0b010110
PNAMES = ("full", "even", "odd", "sc3", "sc2", "expA", "expB")
PTYPE = {"full": "F", "even": "P", "odd": "P", "sc3": "S", "sc2": "S", "expA": "E", "expB": "E"}


def projector_states_of(name):
    """The L = 6 subspaces of the projector case; expA holds CONFIG, expB does not."""
    if name == "expA":
        return np.array([1, 5, 9, CONFIG, 30, 33, 41, 52, 63], dtype=np.int64)
    if name == "expB":
        return np.array([62, 0, 7, 21, 23, 40, 11], dtype=np.int64)
    return states_of(name, PBITS)


def projector_subspace(name, kind):
    """kind 'lib': the library's object; 'orc': the oracle's"""
    if name in ("expA", "expB"):
        st = projector_states_of(name)
        if kind == "orc":
            return orc.explicit(PBITS, st)
        from dynamite_amd.subspaces import Explicit
        return Explicit(st, L=PBITS)
    return orc_subspace(name, PBITS) if kind == "orc" else make_subspace(name, PBITS)


def projector_verdict(left, right):
    return bool(CONFIG in projector_states_of(left) or CONFIG not in projector_states_of(right))


def absent_column(left, right):
    """Index of the first right state that is not in the left subspace, or None"""
    out = np.flatnonzero(~np.isin(states_of(right), states_of(left)))
    return int(out[0]) if out.size else None


def assert_verdicts_cover(seen):
    """seen: {(left type, right type): set of CheckConserves verdicts}.  Every pair of types must have shown True, and False
    wherever False can be: a Full left subspace has no rows outside it."""
    for lt in "FPSE":
        for rt in "FPSE":
            assert seen[(lt, rt)] == ({True} if lt == "F" else {True, False}), (lt, rt, seen[(lt, rt)])


# ---------------------------------------------------------------------- the checks of the reference itself
def test_subspace_states_are_the_oracles():
    for name in NAMES:
        sub = orc_subspace(name)
        st = states_of(name)
        assert sub.dim == st.size
        assert np.array_equal(sub.i2s(np.arange(st.size)), st), name
    a, b = explicit_lists()
    assert a.size == 300 and np.all(np.diff(a) > 0)
    assert b.size == 210 and np.unique(b).size == 210 and not np.all(np.diff(b) > 0)
    assert 0 in b and (1 << L) - 1 in b
    both = np.intersect1d(a, b).size
    assert 0 < both < 210 and np.setdiff1d(b, a).size > 0 and np.setdiff1d(a, b).size > 0


def test_operators_are_what_the_cases_need():
    masks, offs, signs, coeffs = operator_arrays("pauli")
    assert masks[0] == 0 and 25 <= offs[-1] <= 31
    assert np.array_equal(coeffs * 8, np.round(coeffs * 8)) and np.all(coeffs != 0)
    assert mixes_real_and_imaginary(operator_arrays("pauli"))
    assert not mixes_real_and_imaginary(operator_arrays("heisenberg"))
    assert np.array_equal(operator_arrays("heisenberg")[3] * 4, np.round(operator_arrays("heisenberg")[3] * 4))
    for opname in ("pauli", "heisenberg"):
        A = dense_of(opname)
        assert np.array_equal(A, A.conj().T)
    x = gauss_ints(4096, 3)
    assert np.all(x.real != 0) and np.all(x.imag != 0) and np.abs(x.real).max() == 8 and np.abs(x.imag).max() == 8


@pytest.mark.parametrize("opname", ["pauli", "heisenberg"])
def test_dense_blocks_against_the_oracle(opname):
    """All 49 pairs: D @ x is the oracle's multiply bit for bit, max_i sum_j |D_ij| its norm (exactly where no mask mixes
    real and imaginary terms), the dense verdict its CheckConserves."""
    arrs = operator_arrays(opname)
    A = dense_of(opname)
    msc = orc.Msc(*arrs)
    exact_norm = not mixes_real_and_imaginary(arrs)
    zero = []
    for ln, rn in PAIRS:
        D = block(A, ln, rn)
        ol, orr = orc_subspace(ln), orc_subspace(rn)
        x = gauss_ints(D.shape[1], 11)
        want = D @ x
        assert np.array_equal(want, orc.matvec(msc, ol, orr, x)), (ln, rn)
        if not D.any():
            zero.append((ln, rn))
            assert not want.any()
        else:
            assert want.any(), (ln, rn)
        nrm, onrm = infnorm_dense(D), orc.infnorm(msc, ol, orr)
        assert nrm == onrm if exact_norm else abs(nrm - onrm) <= 1e-12 * max(1.0, nrm), (ln, rn, nrm, onrm)
        assert conserves_dense(A, ln, rn) == orc.check_conserves(msc, ol, orr), (ln, rn)
    if opname == "pauli":
        assert zero == []               # every pair has a product to get wrong
    else:
        assert zero == HEISENBERG_ZERO_PAIRS
        rule = [(ln, rn) for ln, rn in PAIRS
                if not np.intersect1d(popcount(states_of(ln)), popcount(states_of(rn))).size]
        assert zero == rule


def test_planted_columns_exist():
    """A right state that the left subspace does not hold exists for every pair but those whose right subspace lies in the
    left one; the GPU file plants a column there."""
    none = [(ln, rn) for ln, rn in PAIRS if absent_column(ln, rn) is None]
    assert sorted(none) == sorted([("full", rn) for rn in NAMES] + [(n, n) for n in NAMES[1:]] + [("even", "sc4"), ("odd", "sc5")])


def test_conserves_verdicts_cover_every_type_pair():
    """Heisenberg and the Pauli sum on the 49 pairs plus the projector on its 49: every pair of subspace types is seen with
    the verdict True, and with False wherever False can be -- a Full left subspace has no rows outside it."""
    seen = {}
    for opname in ("pauli", "heisenberg"):
        A = dense_of(opname)
        for ln, rn in PAIRS:
            seen.setdefault((TYPE[ln], TYPE[rn]), set()).add(conserves_dense(A, ln, rn))
    arrs = projector_arrays(PBITS, CONFIG)
    A = dense(arrs, PBITS)
    assert np.array_equal(A, np.diag((np.arange(1 << PBITS) == CONFIG).astype(np.complex128)))
    msc = orc.Msc(*arrs)
    for ln in PNAMES:
        for rn in PNAMES:
            want = projector_verdict(ln, rn)
            assert conserves_dense(A, projector_states_of(ln), projector_states_of(rn)) == want, (ln, rn)
            assert orc.check_conserves(msc, projector_subspace(ln, "orc"), projector_subspace(rn, "orc")) == want, (ln, rn)
            seen.setdefault((PTYPE[ln], PTYPE[rn]), set()).add(want)
    assert_verdicts_cover(seen)


def test_same_subspace_question_on_host_only_handles():
    """What dnm_mat_mult_lanczos (and dnm_mat_precompute_diagonal) decide their refusal by, on handles that need no
    device: two descriptors name one subspace when they hold the same states at the same indices -- not when the
    dimensions agree, and also when two Explicit objects hold the same list.  A host-only handle of one subspace gets as
    far as the refusal to launch."""
    import ctypes as C
    from dynamite_amd import _lib, backend
    from dynamite_amd.subspaces import Explicit, SpinConserve
    arrs = operator_arrays("pauli")
    a, _ = explicit_lists()

    def refusal(left, right):
        # (x and y are two doubles each, never read: a pair of two subspaces is refused by the question asked here, one
        # subspace by mult_fused's first check, "host-only handle cannot multiply", before anything looks at a vector --
        # should those checks ever change places, give these the handle's dimensions)
        h = backend.create_mat(*arrs, left._c(), right._c(), flags=_lib.MAT_HOST_ONLY)
        x, y, d = (C.c_double * 2)(), (C.c_double * 2)(), (C.c_double * 3)()
        with pytest.raises(_lib.BackendError) as e:
            _lib.check(_lib.lib().dnm_mat_mult_lanczos(h, x, y, None, 0.0, d, None))
        _lib.check(_lib.lib().dnm_mat_destroy(h))
        return str(e.value)

    S = make_subspace
    for left, right in ((S("full"), S("sc5")), (S("sc4"), SpinConserve(L, 6)), (S("even"), S("odd")),
                        (Explicit(a[:210], L=L), S("expB")), (S("expA"), S("expB"))):
        assert "same subspace" in refusal(left, right), (left, right)
    for left, right in ((S("expA"), Explicit(a.copy(), L=L)), (S("sc4"), SpinConserve(L, 4)), (S("odd"), S("odd")),
                        (S("full"), S("full"))):
        assert "host-only" in refusal(left, right), (left, right)
