"""
The site permutations of the lattices' symmetries (lattices.chain_translations, chain_reflection, square_translations,
kagome_translations, kagome_point_group) -- host only.  Every permutation is a bijection and maps the edge set of its
lattice onto itself; the kagome translations map the elementary triangles onto themselves, keeping their sense;
translations and point group are each closed under composition; there are N / 3 kagome translations, the identity first
and each under its smallest (u, v); and the point group of every cluster has the size that follows from its spanning
vectors: 12 where the torus has the full C6v of the lattice about a hexagon centre, 6 with the rotations alone, 4 with the
rotation by 180 degrees and a pair of mirrors, 2 with that rotation alone (every torus has it: it maps each lattice
vector to its negative).
"""
import pytest

from dynamite_amd import lattices

CLUSTERS = ['12', '15', '18a', '18b', '21', '24', '27a', '27b', '30', '33', '36a', '36b', '36c', '36d']
POINT_GROUP = {'12': 12, '15': 4, '18a': 4, '18b': 2, '21': 6, '24': 4, '27a': 2, '27b': 12, '30': 2, '33': 2, '36a': 2,
               '36b': 2, '36c': 2, '36d': 12}


def is_bijection(perm, n):
    return len(perm) == n and sorted(perm) == list(range(n))


def image_of_edges(perm, edges):
    return {(min(perm[i], perm[j]), max(perm[i], perm[j])) for i, j in edges}


def compose(second, first):
    """The permutation of applying ``first`` and then ``second``: the spin at i goes to first[i], then to
    second[first[i]]."""
    return [second[first[i]] for i in range(len(first))]


def closed(perms):
    have = {tuple(p) for p in perms}
    return len(have) == len(perms) and all(tuple(compose(a, b)) in have for a in perms for b in perms)


@pytest.mark.parametrize("L", [2, 3, 8, 13])
def test_chain(L):
    n, edges = lattices.chain(L, periodic=True)
    trans = lattices.chain_translations(L)
    assert len(trans) == L and trans[0] == list(range(L))
    for g, perm in enumerate(trans):
        assert is_bijection(perm, L)
        assert perm == [(i + g) % L for i in range(L)]
        assert image_of_edges(perm, edges) == set(edges)
    assert closed(trans)
    refl = lattices.chain_reflection(L)
    assert is_bijection(refl, L) and refl[0] == L - 1
    assert image_of_edges(refl, edges) == set(edges)
    assert image_of_edges(refl, lattices.chain(L)[1]) == set(lattices.chain(L)[1])
    assert compose(refl, refl) == list(range(L))
    # with the translations: the dihedral group
    assert closed(trans + [compose(t, refl) for t in trans]) or L <= 2


@pytest.mark.parametrize("nx,ny", [(3, 3), (4, 3), (2, 5), (4, 4)])
def test_square(nx, ny):
    n, edges = lattices.square(nx, ny)
    trans = lattices.square_translations(nx, ny)
    assert len(trans) == n and trans[0] == list(range(n))
    for at, perm in enumerate(trans):
        assert is_bijection(perm, n)
        a, b = at % nx, at // nx
        assert perm[0] == a + nx * b
        assert image_of_edges(perm, edges) == set(edges)
    assert closed(trans)


@pytest.mark.parametrize("cluster", CLUSTERS)
def test_kagome_translations(cluster):
    n, edges = lattices.kagome(cluster)
    triangles = set(lattices.kagome_triangles(cluster))
    trans = lattices.kagome_translations(cluster)
    assert len(trans) == n // 3
    assert trans[0] == ((0, 0), list(range(n)))
    labels = [uv for uv, _ in trans]
    assert labels == sorted(labels) and all(u >= 0 and v >= 0 for u, v in labels)
    for (u, v), perm in trans:
        assert is_bijection(perm, n)
        assert image_of_edges(perm, edges) == set(edges)
        moved = set()
        for t in triangles:
            s = tuple(perm[i] for i in t)
            first = s.index(min(s))
            moved.add(s[first:] + s[:first])
        assert moved == triangles
        # no translation but the identity fixes a site
        assert (u, v) == (0, 0) or all(perm[i] != i for i in range(n))
    perms = [p for _, p in trans]
    assert closed(perms)
    # abelian
    assert all(compose(a, b) == compose(b, a) for a in perms for b in perms)
    # the smallest label: no earlier (u, v) gives the same translation
    order, index, wrap, _ = lattices._kagome_walk(cluster)
    for (u, v), perm in trans[1:]:
        for uu in range(u + 1):
            for vv in range(v if uu == u else n // 3):
                assert [index[wrap((x + 2 * uu, y + 2 * vv))] for x, y in order] != perm


@pytest.mark.parametrize("cluster", CLUSTERS)
def test_kagome_point_group(cluster):
    n, edges = lattices.kagome(cluster)
    group = lattices.kagome_point_group(cluster)
    assert len(group) == POINT_GROUP[cluster]
    assert group[0] == ((0, 0), list(range(n)))
    assert (0, 3) in [mk for mk, _ in group]
    for (m, k), perm in group:
        assert m in (0, 1) and 0 <= k < 6
        assert is_bijection(perm, n)
        assert image_of_edges(perm, edges) == set(edges)
    perms = [p for _, p in group]
    assert closed(perms)
    by_label = dict(group)
    # a mirror is an involution; k rotations are the k-th power of one
    for (m, k), perm in group:
        if m == 1:
            assert compose(perm, perm) == list(range(n))
    if (0, 1) in by_label:
        power = list(range(n))
        for k in range(6):
            assert by_label[(0, k)] == power
            power = compose(by_label[(0, 1)], power)
        assert power == list(range(n))
    # with the translations: the space group, closed, of the product of the two orders
    trans = [p for _, p in lattices.kagome_translations(cluster)]
    space = [compose(t, g) for t in trans for g in perms]
    assert len({tuple(p) for p in space}) == len(trans) * len(perms)
    if n <= 21:
        assert closed(space)


def test_kagome_point_group_of_spanning_vectors():
    assert len(lattices.kagome_point_group(((2, 0), (0, 2)))) == 12
    assert lattices.kagome_point_group(((2, 0), (0, 2))) == lattices.kagome_point_group('12')
