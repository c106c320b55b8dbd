"""Interior eigenpairs (eigsolve(target=, interior='filter')): what runs without a GPU -- the filter's parameters
(dnm_interior_filter_plan) against their closed forms, the factorised recurrence of csrc/krylov.cpp
(Ops::apply_fold, its coefficients and final scale in FoldPoly, csrc/krylov_host.h) restated in numpy on a matrix of
known spectrum, and the argument checks of the Python entry.  (The window estimate and the dense helpers:
tests/test_krylov_host.py.)"""
import ctypes as C

import numpy as np
import pytest

from dynamite_amd import _lib


def plan(emin, emax, target, a, damping):
    d, c, e = C.c_int(), C.c_double(), C.c_double()
    _lib.check(_lib.lib().dnm_interior_filter_plan(emin, emax, target, a, damping, C.byref(d), C.byref(c), C.byref(e)))
    return d.value, c.value, e.value


@pytest.mark.parametrize("emin,emax,target,a,damping", [
    (-7.0, 6.4, -0.347, 0.057, 100.0),        # mid-band
    (-8.2, 7.3, -4.975, 0.19, 100.0),         # off-centre: h is the distance to the FAR end
    (-3.0, 5.0, 4.9, 0.3, 14.0),              # target near the upper end
    (-3.0, 5.0, -2.99, 0.001, 1e3),           # target near the lower end, narrow window
    (0.0, 1.0, 0.5, 0.25, 2.0),
])
def test_filter_plan_closed_forms(emin, emax, target, a, damping):
    d, c, e = plan(emin, emax, target, a, damping)
    h = max(target - emin, emax - target)
    assert c == pytest.approx((h * h + a * a) / 2, rel=1e-15)
    assert e == pytest.approx((h * h - a * a) / 2, rel=1e-15)
    th = np.arccosh(c / e)
    # the smallest degree whose damping reaches the one asked for
    assert d >= 1 and np.cosh(d * th) >= damping * (1 - 1e-12)
    assert d == 1 or np.cosh((d - 1) * th) < damping * (1 + 1e-12)
    assert d == max(1, int(np.ceil(np.arccosh(damping) / th)))


def test_filter_plan_refuses_bad_arguments():
    for args in ((1.0, 0.0, 0.5, 0.1, 100.0),        # emax <= emin
                 (0.0, 1.0, 0.5, 0.0, 100.0),        # no window
                 (0.0, 1.0, 0.5, 0.6, 100.0),        # window covers the interval
                 (0.0, 1.0, 0.5, 0.1, 1.0)):         # no damping
        with pytest.raises(_lib.BackendError):
            plan(*args)


def fold_filter(H, sigma, d, c, e, x):
    """p(H) x by the solver's recurrence: u_j = e^j T_j((G - c) / e) / 2^(j-1), every (G - c) u as two multiplies
    v = H u - (sigma - sqrt c) u, H v - (sigma + sqrt c) v."""
    rc = np.sqrt(c)
    b1, b2 = sigma - rc, sigma + rc
    um, uc = None, x
    for j in range(1, d + 1):
        v = H @ uc - b1 * uc
        b = 0.0 if j == 1 else (0.5 * e * e if j == 2 else 0.25 * e * e)
        un = H @ v - b2 * v - (b * um if j > 1 else 0.0)
        um, uc = uc, un
    dth = d * np.arccosh(c / e)
    scale = (-1.0) ** d * np.exp(-(d * np.log(e) - (d - 1) * np.log(2.0)) - (dth - np.log(2.0) + np.log1p(np.exp(-2 * dth))))
    return scale * uc


@pytest.mark.parametrize("target,a,damping", [(0.13, 0.21, 100.0), (-1.4, 0.35, 30.0), (1.71, 0.1, 8.0)])
def test_factorised_recurrence_on_a_known_spectrum(target, a, damping):
    rs = np.random.RandomState(5)
    n = 60
    lam = np.sort(rs.uniform(-2.0, 2.0, n))
    lam[n // 2] = target                                 # an eigenvalue AT the target: p = 1 there
    Q, _ = np.linalg.qr(rs.standard_normal((n, n)))
    H = (Q * lam) @ Q.T
    H = 0.5 * (H + H.T)
    emin, emax = -2.05, 2.1
    d, c, e = plan(emin, emax, target, a, damping)
    # one factorised step is (G - c) u formed densely
    u = rs.standard_normal(n)
    G = (H - target * np.eye(n)) @ (H - target * np.eye(n))
    rc = np.sqrt(c)
    v = H @ u - (target - rc) * u
    step = H @ v - (target + rc) * v
    dense = (G - c * np.eye(n)) @ u
    assert np.max(np.abs(step - dense)) <= 1e-13 * np.max(np.abs(dense))
    # p on the eigenvectors
    bound = 1.0 / np.cosh(d * np.arccosh(c / e))
    assert bound <= 1.0 / damping * (1 + 1e-12)
    outside = 0
    for i in range(n):
        q = Q[:, i]
        pq = fold_filter(H, target, d, c, e, q)
        val = q @ pq
        assert np.linalg.norm(pq - val * q) <= 1e-10           # an eigenvector stays one
        if i == n // 2:
            assert abs(val - 1.0) <= 1e-10
        elif abs(lam[i] - target) >= a:
            outside += 1
            assert abs(val) <= bound * (1 + 1e-12) + 1e-12 * bound, (lam[i], val, bound)
        else:
            assert bound * (1 - 1e-9) <= val <= 1.0 + 1e-10      # inside the window: between the bound and p(sigma)
    assert outside > n // 2


def _chain(L=6):
    from dynamite_amd.operators import sigmax, sigmay, sigmaz, index_sum, op_sum
    return index_sum(op_sum(0.25 * s(0) * s(1) for s in (sigmax, sigmay, sigmaz)), size=L)


def test_target_without_interior_is_still_refused():
    with pytest.raises(RuntimeError, match="not supported for shell matrices"):
        _chain().eigsolve(nev=2, target=0.0)


def test_interior_argument_checks():
    with pytest.raises(ValueError, match="interior"):
        _chain().eigsolve(nev=2, target=0.0, interior='bogus')
    with pytest.raises(ValueError, match="target"):
        _chain().eigsolve(nev=2, interior='filter')
    assert _lib.WHICH["target"] == 3
