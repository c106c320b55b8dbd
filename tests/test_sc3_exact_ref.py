"""tests/sc3_exact_ref.py -- the int64 reference of the SpinConserve multiply in the internal layout that
tests/test_gpu_sc3_exact.py compares the kernels with -- pinned to the oracle (oracle.matvec: the restatement of the
reference's MatMult_CPU_General) on EVERY (operator, subspace) pair the GPU file uses, and to the pure-Python
tests/wide_ref.py at two tiny shapes.  With dyadic coefficients and integer amplitudes the oracle's doubles are exact
too, so every comparison is array_equal.  ``Ref.apply`` asserts the 2^53 condition on the numbers of each case while it
computes them: a case that left the exact range would fail here, before any GPU saw it."""
import numpy as np
import pytest

import sc3_exact_ref as ref
import wide_ref
from oracle import oracle as orc


def _oracle(r, x):
    sub = orc.spin_conserve(r.L, r.k)
    if r.sector is not None:
        sub = orc.xparity(sub)
    return orc.matvec(orc.Msc(*r.arrs), sub, sub, x, nthreads=min(8, orc.max_threads()))


def test_states_are_the_subspace_order():
    for L, k in ((12, 0), (12, 12), (12, 1), (13, 6), (22, 11), (34, 2)):
        st = ref.sc_states(L, k)
        assert np.array_equal(st, orc.spin_conserve(L, k).i2s(np.arange(st.size, dtype=np.int64)))
    assert np.array_equal(ref.sc_states(34, 2), np.array(wide_ref.sc_states(34, 2), dtype=np.int64))


@pytest.mark.parametrize("pair", ref.pairs_used(),
                         ids=lambda p: "%s-%d-%d%s%s" % (p[0], p[1], p[2], p[3] or "", "-real" if p[4] else ""))
def test_reference_is_the_oracle(pair):
    """H x, H x - b z and H x - b z + c z2 of the case's own vectors (complex, or real where the GPU case runs in real
    arithmetic) against the oracle; the fused sums against a longdouble sum of the oracle's exact products (integers below 2^53 in units of
    1/64: exact in any float type with 53 bits or more)."""
    r = ref.get(*pair[:4])
    real = pair[4]
    assert pair[0] in ref.REAL_OPS or not real
    p = ref.product(*pair)
    hx = _oracle(r, np.array(p.x))
    assert np.array_equal(p.y, hx)
    assert np.array_equal(p.y_z, hx - ref.B * p.z)
    assert np.array_equal(p.y_z2, (hx - ref.B * p.z) + p.c * p.z2)
    if real:
        assert not p.y.imag.any() and not p.y_z2.imag.any() and p.sums[1] == 0 and p.sums_z[1] == 0
    for y, sums in ((p.y, p.sums), (p.y_z, p.sums_z)):
        d = np.sum(np.conj(p.x).astype(np.clongdouble) * y.astype(np.clongdouble))
        n2 = np.sum(y.real.astype(np.longdouble) ** 2 + y.imag.astype(np.longdouble) ** 2)
        assert (float(d.real), float(d.imag), float(n2)) == tuple(sums.tolist())
    if r.N > 1 << 20:
        ref.release()


@pytest.mark.parametrize("name,op", [('sc34_2', 'dm'), ('sc34_32', 'chain')])
def test_reference_is_wide_ref(name, op):
    """... and against the plain-Python reference: product, fused sums and columns."""
    c = wide_ref.case(name, op)
    L, k = wide_ref.SC[name]
    r = ref.Ref(op, L, k, arrs=c.arrs)
    assert r.N == c.N
    x = wide_ref.int_vector(c.N, seed=5)
    y, sums = r.apply(x)
    want = wide_ref.apply(c, x)
    assert np.array_equal(y, want)
    assert np.array_equal(sums, wide_ref.fused_sums(x, want))
    for j in (0, 1, c.N // 2, c.N - 1):
        rows, vals = r.column(j)
        col = {}
        for row, elems in enumerate(c.rows):
            for cj, re, im in elems:
                if cj == j:
                    col[row] = col.get(row, 0) + complex(re / 8, im / 8)
        assert rows.tolist() == sorted(col) and vals.tolist() == [col[q] for q in sorted(col)]


@pytest.mark.parametrize("pair", ref.PLANTED, ids=str)
def test_columns_are_the_products_of_unit_vectors(pair):
    r = ref.get(*pair)
    for j in (0, r.N // 3, r.N - 1):
        e = np.zeros(r.N, dtype=np.complex128)
        e[j] = 1
        want = _oracle(r, e)
        rows, vals = r.column(j)
        got = np.zeros(r.N, dtype=np.complex128)
        got[rows] = vals
        assert np.array_equal(got, want)
        assert set(np.flatnonzero(want).tolist()) <= set(rows.tolist())


def test_operators_are_what_their_names_say():
    """Real operators have real arrays; the chains are chains, the graphs are not."""
    for name in ref.OPERATORS:
        L = {'kagome12': 12, 'kagome15': 15, 'dense_lo': 25}.get(name, 13)
        arrs = ref.Ref(name, L, 1).arrs if name != 'graph_xp' else ref.Ref(name, 14, 7).arrs
        assert (not arrs[3].imag.any()) == (name in ref.REAL_OPS), name
        two = [m for m in arrs[0].tolist() if m]
        assert all(bin(m).count('1') == 2 for m in two)
        adjacent = all(m & (m >> 1) for m in two)
        assert adjacent == (name not in ref.GRAPH_OPS), name
