"""
Bond graphs of the lattices the reference's example scripts run on.

``kagome(cluster)``: the kagome lattice on the tori of the reference's flagship large-scale example
(``examples/scripts/kagome/lattice_library.py:9-29``: the clusters of Lauchli et al., PRB 83, 212401 (2011) and
PRB 100, 155142 (2019), each given by two spanning vectors in units of the two-site-long cell edge), with the
vertex numbering of ``basis_to_graph`` (``lattice_library.py:32-85``: breadth-first from the origin, neighbours
visited in a fixed order), so that operators built on these edges are the ones the reference script builds
(``run_kagome.py:20-28``).  The reduction of a point into the torus is done here with exact integer arithmetic on the
coordinates in the spanning basis (any representative works: the numbering depends on the graph and the visiting
order only); ``tests/golden/kagome_edges.json`` holds the reference's own edge lists for every cluster.
"""

KAGOME_CLUSTERS = {
    '12': ((2, 0), (0, 2)), '15': ((2, -1), (-1, 3)), '18a': ((2, -1), (0, 3)), '18b': ((2, -2), (-2, -1)),
    '21': ((2, 1), (-1, 3)), '24': ((1, 2), (-3, 2)), '27a': ((2, 1), (-3, 3)), '27b': ((3, 0), (0, 3)),
    '30': ((2, 1), (-2, 4)), '33': ((1, 2), (4, -3)), '36a': ((-2, 3), (4, 0)), '36b': ((3, 0), (-3, 4)),
    '36c': ((3, 0), (-1, 4)), '36d': ((4, -2), (-2, 4)), '39a': ((-1, 3), (5, -2)), '39b': ((1, 3), (-3, 4)),
    '42a': ((-1, 3), (5, -1)), '42b': ((-2, 4), (4, -1)), '48': ((4, 0), (0, 4)),
}

# the six neighbours of a point of the triangular lattice (skew coordinates), in the reference's visiting order
_NEIGHBOURS = ((0, 1), (1, 0), (1, -1), (0, -1), (-1, 0), (-1, 1))


def _is_site(p):
    """The kagome lattice is the triangular lattice without the points (odd, even)."""
    return p[0] % 2 == 0 or p[1] % 2 == 1


def _kagome_walk(cluster):
    """(points in the order of their numbering, point -> number, the reduction into the torus, set of edges) of a
    kagome torus."""
    (a0, a1), (b0, b1) = KAGOME_CLUSTERS[cluster] if isinstance(cluster, str) else cluster
    A, B = (2 * a0, 2 * a1), (2 * b0, 2 * b1)
    det = A[0] * B[1] - A[1] * B[0]
    if det == 0:
        raise ValueError('spanning vectors are linearly dependent')

    def wrap(p):
        # p = u A + v B; subtract floor(u) A + floor(v) B (u = det(p, B) / det, v = det(A, p) / det)
        nu, nv = p[0] * B[1] - p[1] * B[0], A[0] * p[1] - A[1] * p[0]
        if det < 0:
            nu, nv, d = -nu, -nv, -det
        else:
            d = det
        fu, fv = nu // d, nv // d
        return (p[0] - fu * A[0] - fv * B[0], p[1] - fu * A[1] - fv * B[1])

    index = {(0, 0): 0}
    order = [(0, 0)]
    edges = set()
    at = 0
    while at < len(order):
        x, y = order[at]
        for dx, dy in _NEIGHBOURS:
            q = wrap((x + dx, y + dy))
            if not _is_site(q):
                continue
            j = index.get(q)
            if j is None:
                j = index[q] = len(order)
                order.append(q)
            if at < j:
                edges.add((at, j))
        at += 1
    return order, index, wrap, edges


def kagome(cluster):
    """(number of sites, sorted list of edges (i, j), i < j) of a kagome torus; ``cluster`` is a name of
    ``KAGOME_CLUSTERS`` or a pair of spanning vectors."""
    order, _, _, edges = _kagome_walk(cluster)
    return len(order), sorted(edges)


def kagome_triangles(cluster):
    """The 2 N / 3 elementary triangles of the torus ``kagome(cluster)`` builds, with its site numbering: a sorted list
    of (a, b, c) with a the smallest site, every triangle in the same sense -- (p, p + n_{k+1}, p + n_k) for consecutive
    entries n_k, n_{k+1} of ``_NEIGHBOURS`` with all three points sites, which is anticlockwise in the usual embedding
    of the skew coordinates ((1, 0) along x, (0, 1) at 60 degrees).  These are the geometric triangles, each edge in
    exactly one of them, not the 3-cycles of the edge graph, of which small tori have more.  With this list
    ``State.chirality_correlations`` gives the scalar chiralities of one orientation of the plane."""
    order, index, wrap, _ = _kagome_walk(cluster)
    found = set()
    for at, (x, y) in enumerate(order):
        for k in range(len(_NEIGHBOURS)):
            (dx0, dy0), (dx1, dy1) = _NEIGHBOURS[k], _NEIGHBOURS[(k + 1) % len(_NEIGHBOURS)]
            q1, q0 = wrap((x + dx1, y + dy1)), wrap((x + dx0, y + dy0))
            if not (_is_site(q1) and _is_site(q0)):
                continue
            t = (at, index[q1], index[q0])
            first = t.index(min(t))
            found.add(t[first:] + t[:first])
    return sorted(found)


# ---- site permutations of the lattices' symmetries (host only) ---------------------------------------------------------
# A site permutation is a list pi of length N, a bijection of [0, N): the spin at site i moves to site pi(i)
# (``computations.permute_sites``).  A geometric map f of the lattice gives pi(i) = the number of the point f(point i).

def chain_translations(L):
    """The L translations of the periodic chain: the g-th is pi(i) = (i + g) mod L; the identity comes first."""
    return [[(i + g) % L for i in range(L)] for g in range(L)]


def chain_reflection(L):
    """The reflection of the chain, pi(i) = L - 1 - i."""
    return [L - 1 - i for i in range(L)]


def square_translations(nx, ny):
    """The nx ny translations of the periodic nx x ny square lattice (site (x, y) -> x + nx * y): the one by (a, b) at
    place a + nx * b, the identity first."""
    return [[(x + a) % nx + nx * ((y + b) % ny) for y in range(ny) for x in range(nx)]
            for b in range(ny) for a in range(nx)]


def _kagome_image(order, index, wrap, f):
    """The site permutation of the map f of points of a kagome torus, or None where an image is not a site of it or two
    sites share one."""
    perm = []
    for p in order:
        q = wrap(f(p))
        j = index.get(q) if _is_site(q) else None
        if j is None:
            return None
        perm.append(j)
    return perm if len(set(perm)) == len(perm) else None


def kagome_translations(cluster):
    """The N / 3 translations of the torus ``kagome(cluster)`` builds, with its site numbering: a list of ``((u, v),
    perm)`` for the translation by u (2, 0) + v (0, 2) in the skew coordinates of the walk -- each distinct translation
    once, under its lexicographically smallest (u, v) with u, v >= 0, in that order, so that the identity comes
    first."""
    order, index, wrap, _ = _kagome_walk(cluster)
    n = len(order) // 3             # the order of the translation group: n times any translation is the identity
    found, seen = [], set()
    for u in range(n):
        for v in range(n):
            perm = _kagome_image(order, index, wrap, lambda p: (p[0] + 2 * u, p[1] + 2 * v))
            if tuple(perm) not in seen:
                seen.add(tuple(perm))
                found.append(((u, v), perm))
    return found


def kagome_point_group(cluster):
    """The elements of C6v about the hexagon centre (1, 0) that are symmetries of the torus ``kagome(cluster)`` builds,
    with its site numbering: a list of ``((m, k), perm)`` over m = 0, 1 and k = 0..5 for k rotations by 60 degrees, (x,
    y) -> (-y, x + y), after -- when m = 1 -- the mirror (x, y) -> (y, x), both relative to the centre.  Only the
    elements that map the torus onto itself (the spanning vectors onto vectors of their lattice) and edges onto edges
    are returned, the identity (0, 0) first: 12 of them on the most symmetric clusters, 2 on most."""
    order, index, wrap, edges = _kagome_walk(cluster)
    (a0, a1), (b0, b1) = KAGOME_CLUSTERS[cluster] if isinstance(cluster, str) else cluster
    spanning = ((2 * a0, 2 * a1), (2 * b0, 2 * b1))
    cx, cy = 1, 0

    def linear(p, m, k):
        x, y = (p[1], p[0]) if m else p
        for _ in range(k):
            x, y = -y, x + y
        return x, y

    found = []
    for m in (0, 1):
        for k in range(6):
            if any(wrap(linear(s, m, k)) != (0, 0) for s in spanning):
                continue

            def f(p):
                x, y = linear((p[0] - cx, p[1] - cy), m, k)
                return x + cx, y + cy

            perm = _kagome_image(order, index, wrap, f)
            if perm is None:
                continue
            if {(min(perm[i], perm[j]), max(perm[i], perm[j])) for i, j in edges} != edges:
                continue
            found.append(((m, k), perm))
    return found


def chain(L, periodic=False):
    edges = [(i, i + 1) for i in range(L - 1)]
    if periodic and L > 2:
        edges.append((0, L - 1))
    return L, edges


def square(nx, ny, periodic=True):
    """nx x ny square lattice, site (x, y) -> x + nx * y."""
    edges = set()
    for y in range(ny):
        for x in range(nx):
            i = x + nx * y
            for (u, v) in ((x + 1, y), (x, y + 1)):
                if periodic:
                    u, v = u % nx, v % ny
                elif u >= nx or v >= ny:
                    continue
                j = u + nx * v
                if i != j:
                    edges.add((min(i, j), max(i, j)))
    return nx * ny, sorted(edges)
