#!/usr/bin/env python
"""Bit-for-bit record of the SpinConserve passes' host tables (csrc/sc3_tables.cpp): one sha256 line per (operator, handle
flags, rank, table) from dnm_mat_export_sc3 over host-only handles -- no GPU needed.  Two builds whose builders make the
same tables print the same file:

    DNM_LIB=<other build>/libdynamite_amd.so python tools/sc3_tables_ab.py > a.txt
    python tools/sc3_tables_ab.py > b.txt && cmp a.txt b.txt

Operators: Heisenberg chains at L = 12, 24, 32, 36 (the last on ranks 0, 3, 7 of 8), the kagome tori 12, 15, 18a, 27b, 30,
XParity of kagome 12 and 30 in both sectors, the harness's long-range model at L = 28 and the 32 random pair graphs of
tests/test_gpu_sc3_graph.py::test_fuzz_pair_graphs; each as a complex and as a real-packed handle, relabelled where
build_mat would relabel (one rank, an operator that is no chain)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from dynamite_amd import _lib, backend, models, msc_tools  # noqa: E402
from dynamite_amd.operators import sigmax, sigmay, sigmaz, index_sum, op_sum  # noqa: E402
from dynamite_amd.subspaces import SpinConserve, XParity  # noqa: E402


def heisenberg(L, seed=1234):
    rng = np.random.RandomState(seed)
    H = (index_sum(op_sum(0.25 * s(0) * s(1) for s in (sigmax, sigmay, sigmaz)), size=L) +
         op_sum(0.5 * rng.uniform(-2, 2) * sigmaz(i) for i in range(L)))
    H.L = L
    return H


def pair_graph(L, seed, nbonds, complex_hops, fields):
    """tests/test_gpu_sc3_graph.py: pair_graph"""
    rs = np.random.RandomState(seed)
    pairs = [(i, j) for i in range(L) for j in range(i + 1, L)]
    pick = rs.choice(len(pairs), size=min(len(pairs), nbonds or 2 * L), replace=False)
    terms = []
    for q in pick:
        i, j = pairs[q]
        J, Jz, D = rs.uniform(-1, 1, 3)
        terms.append(J * (sigmax(i) * sigmax(j) + sigmay(i) * sigmay(j)) + Jz * sigmaz(i) * sigmaz(j))
        if complex_hops:
            terms.append(D * (sigmax(i) * sigmay(j) - sigmay(i) * sigmax(j)))
    if fields:
        terms += [rs.uniform(-1, 1) * sigmaz(i) for i in range(L)]
    H = op_sum(terms)
    H.L = L
    return H


def cases():
    """(name, msc, L, k, xparity sector or None, ranks as (rank, nranks) pairs)"""
    for L in (12, 24, 32):
        yield "chain%d" % L, heisenberg(L), L, L // 2, None, [(0, 1)]
    yield "chain36", heisenberg(36), 36, 18, None, [(0, 8), (3, 8), (7, 8)]
    for name in ("12", "15", "18a", "27b", "30"):
        H = models.kagome(name)
        yield "kagome" + name, H, H.L, H.L // 2, None, [(0, 1)]
    for name in ("12", "30"):
        for sector in "+-":
            H = models.kagome(name)
            yield "kagome%s_xparity%s" % (name, sector), H, H.L, H.L // 2, sector, [(0, 1)]
    yield "long_range28", models.bench_long_range(28), 28, 14, None, [(0, 1)]
    for seed in range(32):
        rs = np.random.RandomState(1000 + seed)
        L = int(rs.randint(11, 16))
        k = int(rs.randint(1, L))
        nb = int(rs.randint(1, L * (L - 1) // 2 + 1))
        yield "fuzz%02d" % seed, pair_graph(L, seed, nb, bool(seed & 1), bool(seed & 2)), L, k, None, [(0, 1)]


def main():
    for name, H, L, k, sector, ranks in cases():
        H.establish_L()
        H.reduce_msc()
        msc = H.msc
        sub = SpinConserve(L, k)
        if sector is not None:
            msc = XParity(sub, sector).reduce_msc(msc)
        masks, offs = msc_tools.get_mask_offsets(msc)
        a, w = (14, 10) if L - 24 >= 1 else (6, 4)
        d = _lib.Subspace.from_buffer_copy(sub._c())
        d.vec_swizzle = a | (w << 8)
        for rank, nranks in ranks:
            dd = d
            if nranks == 1:
                perm, _ = backend.choose_site_perm(masks, L, a, w, fix_top=sector is not None)
                if not np.array_equal(perm, np.arange(L)):
                    dd = backend.with_site_perm(d, perm)
            for flags, tag in ((_lib.MAT_HOST_ONLY, "complex"), (_lib.MAT_HOST_ONLY | _lib.MAT_REAL_PACKED, "real")):
                head = "%-20s %-7s rank %d/%d" % (name, tag, rank, nranks)
                try:
                    h = backend.create_mat(masks, offs, msc['signs'], msc['coeffs'], dd, dd, sector is not None, flags,
                                           rank, nranks)
                except Exception:
                    print("%s no such handle" % head, flush=True)
                    continue
                for t in ("op",) + backend.SC3_TABLES:
                    raw = backend.export_sc3(h, t)
                    print("%s %-8s %9d bytes %s" % (head, t, len(raw), hashlib.sha256(raw).hexdigest()[:32]), flush=True)
                _lib.check(_lib.lib().dnm_mat_destroy(h))


if __name__ == "__main__":
    main()
