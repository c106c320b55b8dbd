"""
lattices.kagome_triangles: the elementary triangles of the kagome tori, in the site numbering of lattices.kagome and all
in one sense -- no GPU needed.  For every cluster: 2 N / 3 triangles, every edge of kagome(cluster) in exactly one of
them, a the smallest site, and one sense, checked through coordinates this file rebuilds with its own copy of the walk
(the cross product of the two neighbour steps a -> b and b -> c has one sign everywhere).  Cluster '12': the spectrum of
H = sum_t chi_t on SpinConserve(12, 6), built here in numpy from the rotations as 2i (C - C^H), which a triangle of the
other sense changes.
"""
import numpy as np
import pytest

from dynamite_amd import lattices

STEPS = ((0, 1), (1, 0), (1, -1), (0, -1), (-1, 0), (-1, 1))


def walk(cluster):
    """This file's own copy of the breadth-first numbering: (points by number, reduction into the torus)."""
    (a0, a1), (b0, b1) = lattices.KAGOME_CLUSTERS[cluster]
    A, B = (2 * a0, 2 * a1), (2 * b0, 2 * b1)
    det = A[0] * B[1] - A[1] * B[0]
    sgn = 1 if det > 0 else -1

    def wrap(p):
        nu, nv = sgn * (p[0] * B[1] - p[1] * B[0]), sgn * (A[0] * p[1] - A[1] * p[0])
        fu, fv = nu // abs(det), nv // abs(det)
        return (p[0] - fu * A[0] - fv * B[0], p[1] - fu * A[1] - fv * B[1])

    seen = {(0, 0): 0}
    order = [(0, 0)]
    at = 0
    while at < len(order):
        x, y = order[at]
        for dx, dy in STEPS:
            q = wrap((x + dx, y + dy))
            if q[0] % 2 == 0 or q[1] % 2 == 1:
                if q not in seen:
                    seen[q] = len(order)
                    order.append(q)
        at += 1
    return order, wrap


@pytest.mark.parametrize("cluster", sorted(lattices.KAGOME_CLUSTERS))
def test_triangles_of_every_cluster(cluster):
    N, edges = lattices.kagome(cluster)
    tris = lattices.kagome_triangles(cluster)
    assert len(tris) == 2 * N // 3 and 3 * len(tris) == 2 * N
    assert len(set(tris)) == len(tris)
    sides = []
    for a, b, c in tris:
        assert a < b and a < c and b != c
        sides += [tuple(sorted(s)) for s in ((a, b), (b, c), (c, a))]
    # every edge in exactly one triangle, and no side that is not an edge
    assert sorted(sides) == sorted(edges)

    order, wrap = walk(cluster)
    assert len(order) == N

    def step(i, j):
        hits = [s for s in STEPS if wrap((order[i][0] + s[0], order[i][1] + s[1])) == order[j]]
        assert len(hits) == 1, (cluster, i, j, hits)
        return hits[0]

    senses = set()
    for a, b, c in tris:
        (x1, y1), (x2, y2), (x3, y3) = step(a, b), step(b, c), step(c, a)
        # the three steps close geometrically: a triangle of the lattice, not a 3-cycle round the torus
        assert (x1 + x2 + x3, y1 + y2 + y3) == (0, 0)
        senses.add(x1 * y2 - y1 * x2)
    # +1: anticlockwise with (1, 0) along x and (0, 1) at 60 degrees
    assert senses == {1}


def rotation_matrix(configs, rank, a, b, c):
    """C = P_ab P_bc on the basis `configs`: (C psi)(r) = psi(r'), bit a of r' = bit b of r, b <- c, c <- a."""
    xa, xb, xc = (configs >> a) & 1, (configs >> b) & 1, (configs >> c) & 1
    moved = configs & ~((1 << a) | (1 << b) | (1 << c)) | (xb << a) | (xc << b) | (xa << c)
    C = np.zeros((configs.size, configs.size))
    C[np.arange(configs.size), [rank[int(m)] for m in moved]] = 1.0
    return C


def chirality_spectrum(tris, L=12, k=6):
    configs = np.array([s for s in range(1 << L) if bin(s).count("1") == k], dtype=np.int64)
    rank = {int(s): i for i, s in enumerate(configs)}
    H = np.zeros((configs.size, configs.size), dtype=np.complex128)
    for a, b, c in tris:
        C = rotation_matrix(configs, rank, a, b, c)
        H += 2j * (C - C.T)
    assert np.array_equal(H, H.conj().T)
    return np.linalg.eigvalsh(H)


def test_cluster_12_spectrum_of_the_total_chirality():
    tris = lattices.kagome_triangles('12')
    w = chirality_spectrum(tris)
    assert abs(w[0] - (-17.8772153)) < 1e-6, w[:3]
    assert abs(w[1] - (-16.8219381)) < 1e-6, w[:3]
    # one triangle of the other sense gives another spectrum
    a, b, c = tris[3]
    mixed = list(tris)
    mixed[3] = (a, c, b)
    assert abs(chirality_spectrum(mixed)[0] - w[0]) > 1e-3
