"""tests/state_pass_ref.py -- the integer reference that tests/test_gpu_state_passes_exact.py compares the site
permutations, the subspace maps, the sector weights and the products of site operators with -- pinned two ways (no GPU
needed):

(a) at L <= 6 to dense operators built from Kronecker products: permutation matrices (products of exchanges (1 +
    sigma.sigma) / 2, their direction pinned by P sigma^z_i P^H = sigma^z_pi(i)), the isometry of every subspace and of
    both XParity sectors (1 / sqrt 2 on a representative and on its complement) and the projector E E^H it gives, the
    projectors onto a magnetisation and onto a sector of the global flip X x ... x X, and (x)_j M_j.  The bases are
    written out by brute force here (every c < 2^L with the popcount or the parity asked for, ascending).
(b) to the library's host tables -- dnm_perm_partner_indices, dnm_subspace_map_indices, dnm_idx_to_state and
    dnm_state_to_idx themselves -- on a sample of the rows of every shape the GPU file uses (both ends, the rows around
    each multiple of 1024, 3000 random ones) and on all rows of the shapes with L >= 62.  The reference ranks and
    enumerates on its own, so a ranking error that the kernels share with the host tables shows here.

And (c) the COVERAGE PROOF of the GPU file's case tables: the plan of every case (dnm_perm_plan, dnm_subspace_map_plan,
dnm_sector_weights_plan, dnm_site_ops_plan) says which kernel instance runs, with how many workgroups, whether the
threads stride the grid, which runs are ragged and how much LDS the launch takes.  The union over the tables must hold
every instance and regime; what cannot be reached is named in a test of its own."""
import collections
import ctypes as C
import os
from math import comb

import numpy as np
import pytest

import state_pass_ref as ref
from dynamite_amd import _lib, backend
import test_gpu_state_passes_exact as gpu_file
from test_gpu_vec import ints

U64 = np.uint64
FULL, PARITY, EXPLICIT, SC = 0, 1, 2, 3
PERM_CASES, MAP_CASES, WEIGHT_CASES = gpu_file.PERM_CASES, gpu_file.MAP_CASES, gpu_file.WEIGHT_CASES
ATOL = 1e-9          # (values are integers, or integers times 1 / sqrt 2 or 1 / 2: a wrong one is off by 0.2 at least)


# ---------------------------------------------------------------------------------------------------------------------
# (a) the reference against dense operators, L <= 6
# ---------------------------------------------------------------------------------------------------------------------

I2 = np.eye(2, dtype=np.complex128)
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)


def at_site(op, j, L):
    """op on site j: bit j of a configuration is site j, so the last Kronecker factor is site 0"""
    out = np.ones((1, 1), dtype=np.complex128)
    for s in range(L - 1, -1, -1):
        out = np.kron(out, op if s == j else I2)
    return out


def exchange(a, b, L):
    return (np.eye(1 << L) + sum(at_site(P, a, L) @ at_site(P, b, L) for P in (X, Y, Z))) / 2


def dense_perm(perm):
    """P_pi as a product of exchanges: selection sort of the labels; P Z_i P^H = Z_pi(i) is asserted"""
    L = len(perm)
    P = np.eye(1 << L, dtype=np.complex128)
    at = list(range(L))                  # at[s]: the spin that sits at site s now
    for target in range(L):
        # the spin that must end at site `target` is the i with perm[i] == target
        i = [j for j in range(L) if perm[j] == target][0]
        s = at.index(i)
        if s != target:
            P = exchange(s, target, L) @ P
            at[s], at[target] = at[target], at[s]
    for i in range(L):
        assert np.allclose(P @ at_site(Z, i, L) @ P.conj().T, at_site(Z, int(perm[i]), L))
    return P


def brute_basis(spec):
    """the configurations of a subspace in index order, by brute force"""
    kind, L = spec[0], spec[1]
    if kind == "ex":
        return [int(c) for c in spec[2]]
    every = range(1 << L)
    if kind == "full":
        return list(every)
    if kind == "parity":
        return [c for c in every if bin(c).count("1") % 2 == spec[2]]
    return [c for c in every if bin(c).count("1") == spec[2]]


def small_sub(spec):
    if spec[0] == "ex":
        return ref.Sub("explicit", spec[1], states=spec[2])
    return ref.Sub({"full": "full", "parity": "parity", "sc": "sc"}[spec[0]], spec[1],
                   k=spec[2] if spec[0] == "sc" else 0, space=spec[2] if spec[0] == "parity" else 0)


def isometry(spec, sector):
    """E (2^L x rows): a row of the subspace is its configuration; a representative of a sector is (|c> + s |cbar>) /
    sqrt 2"""
    L = spec[1]
    basis = brute_basis(spec)
    if sector:
        assert len(basis) % 2 == 0
        basis = basis[:len(basis) // 2]
    E = np.zeros((1 << L, len(basis)), dtype=np.complex128)
    for r, c in enumerate(basis):
        if sector:
            assert not (c >> (L - 1)) & 1
            E[c, r] = 1 / np.sqrt(2)
            E[c ^ ((1 << L) - 1), r] = sector / np.sqrt(2)
        else:
            E[c, r] = 1
    assert np.allclose(E.conj().T @ E, np.eye(len(basis)))
    return E


_E6 = [3, 60, 5, 58, 17, 46, 0, 63]
_E6 = [c for c in _E6 if not c >> 5] + [c for c in _E6 if c >> 5]                # representatives first
SMALL = [("full", 5), ("full", 6), ("parity", 6, 0), ("parity", 6, 1), ("parity", 5, 1), ("parity", 5, 0), ("sc", 6, 3),
         ("sc", 5, 2), ("sc", 6, 1), ("sc", 6, 5), ("sc", 4, 0), ("sc", 4, 4), ("sc", 4, 2),
         ("ex", 6, tuple(_E6)), ("ex", 6, (9, 33, 2, 61, 30, 7, 44)), ("ex", 5, (1, 30, 7, 24, 12, 19, 0, 31)[::-1])]


def carries(spec):
    if spec[0] == "ex":
        lst, L = list(spec[2]), spec[1]
        h = len(lst) // 2
        return len(lst) % 2 == 0 and all(not (c >> (L - 1)) & 1 for c in lst[:h]) and \
            sorted(c ^ ((1 << L) - 1) for c in lst[:h]) == sorted(lst[h:])
    return small_sub(spec).carries_flip() and small_sub(spec).dim % 2 == 0


SMALL_SIDES = [(s, x) for s in SMALL for x in (0, 1, -1) if x == 0 or carries(s)]
assert sum(1 for s, x in SMALL_SIDES if x and s[0] == "ex") == 2       # (the flip-closed list, both sectors)


def amps(n, seed):
    re, im = ints(n, seed)
    return (re, im), re + 1j * im


@pytest.mark.parametrize("spec,sector", [s for s in SMALL_SIDES if s[0][0] != "ex"], ids=str)
def test_permutations_are_the_dense_permutation_matrices(spec, sector):
    L = spec[1]
    side = (small_sub(spec), sector, 0)
    E = isometry(spec, sector)
    n = E.shape[1]
    perms = gpu_file.permutations(L, 7)
    coef = gpu_file.coefficients(7, L)
    (xr, xi), x = amps(n, 3 * L)
    (yr, yi), y = amps(n, 3 * L + 1)
    dense = [E.conj().T @ dense_perm(p) @ E for p in perms]
    got = ref.perm_apply((xr, xi), side, perms, coef, y=(yr, yi))
    want = y + sum((cr + 1j * ci) * (D @ x) for (cr, ci), D in zip(coef, dense))
    assert np.allclose(got[0] + 1j * got[1], want, atol=ATOL, rtol=0)
    got = ref.perm_dots((yr, yi), (xr, xi), side, perms)
    for g, D in enumerate(dense):
        assert abs(complex(*got[g]) - np.vdot(y, D @ x)) <= ATOL
        pos, s = ref.perm_gather(side, perms[g])
        assert np.allclose(s * x[pos], D @ x, atol=ATOL, rtol=0)


MAP_PAIRS = [(a, b) for a in SMALL_SIDES for b in SMALL_SIDES if a[0][1] == b[0][1]]


def test_the_small_map_pairs_hold_every_type_pair_and_mode():
    kinds = {(a[0][0], b[0][0], bool(a[1]), bool(b[1])) for a, b in MAP_PAIRS}
    assert len(kinds) == 4 * 4 * 4


@pytest.mark.parametrize("i", range(len(MAP_PAIRS)))
def test_maps_are_the_dense_projections(i):
    """y = E_dst^H E_src x: the coordinates, in the target, of the projection E_dst E_dst^H of the source state"""
    (sspec, ssec), (dspec, dsec) = MAP_PAIRS[i]
    src, dst = (small_sub(sspec), ssec, 0), (small_sub(dspec), dsec, 0)
    Es, Ed = isometry(sspec, ssec), isometry(dspec, dsec)
    _, x = amps(Es.shape[1], i % 11)
    got = ref.map_apply(x, src, dst)
    assert np.allclose(got, Ed.conj().T @ (Es @ x), atol=ATOL, rtol=0)
    assert np.allclose(Ed @ got, (Ed @ Ed.conj().T) @ (Es @ x), atol=ATOL, rtol=0)
    idx, sign, scale = ref.map_terms(src, dst)
    by_terms = scale * sum(np.where(idx[:, m] >= 0, sign[:, m] * x[np.maximum(idx[:, m], 0)], 0) for m in range(2))
    assert np.allclose(by_terms, got, atol=ATOL, rtol=0)


@pytest.mark.parametrize("spec,sector", SMALL_SIDES, ids=str)
def test_sector_weights_are_the_norms_of_the_dense_projections(spec, sector):
    L = spec[1]
    side = (small_sub(spec), sector, 0)
    E = isometry(spec, sector)
    (xr, xi), x = amps(E.shape[1], 5 * L + 2)
    psi = E @ x
    number = sum((np.eye(1 << L) - at_site(Z, j, L)) / 2 for j in range(L)).diagonal().real
    flip = np.eye(1, dtype=np.complex128)
    for _ in range(L):
        flip = np.kron(flip, X)
    mag2, flip2 = ref.sector_weights((xr, xi), side)
    for k in range(L + 1):
        assert abs(mag2[k] / 2 - np.linalg.norm(psi[number == k]) ** 2) <= ATOL
    closed = np.allclose(E @ E.conj().T @ flip, flip @ E @ E.conj().T)         # the subspace carries the flip
    if flip2 is None:
        assert spec[0] == "ex" or not closed
    else:
        assert closed
        for m, s in enumerate((1, -1)):
            assert abs(flip2[m] / 2 - np.linalg.norm((psi + s * flip @ psi) / 2) ** 2) <= ATOL


@pytest.mark.parametrize("L", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("swz", [0, 5])
def test_site_products_are_the_dense_kronecker_products(L, swz):
    import site_ops_ref
    if swz >= L:
        return
    for seed in range(3):
        mats = site_ops_ref.exact_matrices(L, 40 + seed, classes=[2] * L if seed == 0 else None)
        dense = np.ones((1, 1), dtype=np.complex128)
        for j in range(L - 1, -1, -1):
            dense = np.kron(dense, mats[j])
        (xr, xi), x = amps(1 << L, L + seed)
        pos = ref.vec_pos(np.arange(1 << L), swz)
        got = ref.site_product((xr, xi), mats, swz)
        want = np.empty(1 << L, dtype=np.complex128)
        want[pos] = dense @ x[pos]
        assert np.array_equal(got[0] + 1j * got[1], want)


# ---------------------------------------------------------------------------------------------------------------------
# (b) the reference against the library's host tables, on the shapes of the GPU file
# ---------------------------------------------------------------------------------------------------------------------

def sample(nrows, seed, everything=False):
    if everything or nrows <= 5000:
        return np.arange(nrows, dtype=np.int64)
    rng = np.random.default_rng(seed)
    edges = (np.arange(1024, nrows, 1024)[:, None] + np.array([-1, 0, 1])).reshape(-1)
    rows = np.concatenate([np.arange(64), np.arange(nrows - 64, nrows), edges, rng.integers(0, nrows, 3000)])
    return np.unique(rows[(rows >= 0) & (rows < nrows)]).astype(np.int64)


SPECS = sorted({c.spec for c in PERM_CASES} | {s[0] for c in MAP_CASES for s in (c.src, c.dst)}
               | {c.side[0] for c in WEIGHT_CASES}, key=str)


def test_the_wide_shapes_are_in_the_tables():
    assert {("sc", 34, 2), ("sc", 50, 2), ("sc", 63, 2), ("sc", 64, 1), ("sc", 64, 2)} <= {c.spec for c in PERM_CASES}
    assert {("sc", 63, 1), ("sc", 50, 2), ("ex", "e63"), ("ex", "e63flip"), ("ex", "e50sub"), ("ex", "e50super")} \
        <= {s[0] for c in MAP_CASES for s in (c.src, c.dst)}
    # bit 62 is set in listed states and in SpinConserve rows, so that c ^ (2^63 - 1) clears it
    assert any(c >> 62 for c in gpu_file.explicit_list("e63flip")[1]) and (1 << 62) in gpu_file.explicit_list("e63")[1]
    # the lists of more than L bits, and the unsorted ones
    assert any(c >> 13 for c in gpu_file.explicit_list("e13wide")[1])
    assert gpu_file.explicit_list("e13sorted")[1] == sorted(gpu_file.explicit_list("e13unsorted")[1])


@pytest.mark.parametrize("spec", [s for s in SPECS if gpu_file.spec_L(s) <= 63], ids=gpu_file.spec_name)
def test_reference_is_idx_to_state_and_state_to_idx(spec):
    """dnm_idx_to_state and dnm_state_to_idx themselves (they run Sub<T>::i2s and s2i of csrc/subspace.h, which the
    kernels call): every configuration the reference enumerates, and the index it gives to members, to their
    complements and to strangers.  (L = 64 is beyond these two entry points; it is pinned through the partner table.)"""
    sub = gpu_file.ref_sub(spec)
    L = sub.L
    d = gpu_file.descriptor(spec)
    rows = sample(sub.dim, len(str(spec)), everything=L >= 62)
    states = np.empty(rows.size, dtype=np.int64)
    _lib.check(_lib.lib().dnm_idx_to_state(C.byref(d), rows.size, _lib.p64(rows), _lib.p64(states)))
    cfg = sub.configs()[rows]
    assert np.array_equal(states.view(U64), cfg)
    rng = np.random.default_rng(L)
    strangers = rng.integers(0, 1 << min(L, 62), 2000).astype(U64)
    strangers |= rng.integers(0, 2, 2000).astype(U64) << U64(L - 1)
    inside = cfg[(cfg & ~ref.all_sites(L)) == 0]         # (a listed state of more than L bits is asked for below)
    ask = np.concatenate([inside, inside ^ ref.all_sites(L), strangers]).view(np.int64)
    got = np.empty(ask.size, dtype=np.int64)
    _lib.check(_lib.lib().dnm_state_to_idx(C.byref(d), ask.size, _lib.p64(np.ascontiguousarray(ask)), _lib.p64(got)))
    want = sub.index(ask.view(U64))
    assert np.array_equal(got, want)
    assert np.array_equal(got[:inside.size], rows[(cfg & ~ref.all_sites(L)) == 0])


def _perm_shapes():
    seen, out = set(), []
    for c in PERM_CASES:
        for swz in c.swz:
            key = (c.spec, c.xsec, swz, min(c.nperm, 11))
            if key not in seen:
                seen.add(key)
                out.append((c, swz))
    return out


PERM_SHAPES = _perm_shapes()


@pytest.mark.parametrize("i", range(len(PERM_SHAPES)), ids=["%s-s%d" % (c.name, s) for c, s in PERM_SHAPES])
def test_reference_is_the_host_partner_table(i):
    case, swz = PERM_SHAPES[i]
    side = gpu_file.ref_side((case.spec, case.xsec, swz))
    n = ref.rows_of(side)
    L = side[0].L
    perms = gpu_file.permutations(L, min(case.nperm, 11))
    rows = sample(n, i, everything=L >= 62)
    idx, sign = backend.perm_partner_indices(gpu_file.descriptor(case.spec, swz), perms, rows, case.xsec)
    for g in range(perms.shape[0]):
        pos, s = ref.perm_gather(side, perms[g], rows)
        assert np.array_equal(idx[:, g], pos) and np.array_equal(sign[:, g].astype(np.int64), s), (case.name, g)


@pytest.mark.parametrize("name", [c.name for c in MAP_CASES])
def test_reference_is_the_host_map_table(name):
    case = gpu_file.MAP_BY_NAME[name]
    src, dst = gpu_file.ref_side(case.src), gpu_file.ref_side(case.dst)
    rows = sample(ref.rows_of(dst), len(name), everything=dst[0].L >= 62)
    sd, dd = gpu_file.descriptor(case.src[0], case.src[2]), gpu_file.descriptor(case.dst[0], case.dst[2])
    idx, sign, scale = backend.subspace_map_indices(sd, dd, rows, case.src[1], case.dst[1])
    widx, wsign, wscale = ref.map_terms(src, dst, rows)
    assert scale == wscale
    assert np.array_equal(idx, widx) and np.array_equal(sign.astype(np.int64), wsign), name
    assert bool(np.any(widx >= 0)) != case.zero or rows.size < ref.rows_of(dst)


# ---------------------------------------------------------------------------------------------------------------------
# (c) coverage of the GPU file's case tables, from the plans
# ---------------------------------------------------------------------------------------------------------------------

NT, ROWS_PER_WG, MAX_WG, RUN = 256, 1024, 4096, 4        # csrc/perm.h and csrc/submap.h say the same for both passes
SW_MAX_WG = 2048


def workgroups(rows, cap):
    return max(1, min(cap, -(-rows // ROWS_PER_WG)))


PermPlan = collections.namedtuple("PermPlan", "type rows runs nwg trips capped ragged gp_log2 idle lds")


def perm_plan_of(case):
    """The plan entry takes no sector: there its answer is asserted to be the rule, which is applied to dim / 2 rows
    under a sector."""
    side = gpu_file.ref_side((case.spec, case.xsec, 0))
    rows = ref.rows_of(side)
    sc = case.spec[0] == "sc"
    nwg, lds, scratch = backend.perm_plan(gpu_file.descriptor(case.spec), case.nperm)
    table = (side[0].k + 1) * (side[0].L + 1) * 8 if sc else 0
    assert nwg == workgroups(side[0].dim, MAX_WG)
    assert lds == (table + 68 * case.nperm + 15) // 16 * 16
    nwg = workgroups(rows, MAX_WG)
    runs = -(-rows // RUN) if sc else rows
    gp = (case.nperm - 1).bit_length()
    return PermPlan(gpu_file.KIND_TYPE[case.spec[0]], rows, runs, nwg, -(-runs // (nwg * NT)), rows > MAX_WG * ROWS_PER_WG,
                    rows % RUN if sc else 0, gp, case.nperm < 1 << gp, lds)


PERM_PLANS = [(c, perm_plan_of(c)) for c in PERM_CASES]


@pytest.mark.parametrize("kernel", ["apply", "dots"])
def test_every_perm_instance_and_regime_is_reached(kernel):
    mine = [(c, p) for c, p in PERM_PLANS if c.only in (None, kernel)]
    for t in (FULL, PARITY, SC):
        of_type = [(c, p) for c, p in mine if p.type == t]
        assert len(of_type) >= 2
        assert {p.gp_log2 for c, p in of_type} == set(range(7))              # 1 to 64 permutations side by side
        assert sum(1 for c, p in of_type if p.idle) >= 2                     # lanes of a group without a permutation
        for x in (1, -1):
            assert sum(1 for c, p in of_type if c.xsec == x) >= 2
        assert sum(1 for c, p in of_type if p.nwg > 1) >= 2
        assert sum(1 for c, p in of_type if p.rows <= 2) >= 2                # dimension 1, or 2 under a sector
    for t in (FULL, PARITY):
        for s in (5, 6):
            assert sum(1 for c, p in mine if p.type == t and s in c.swz) >= 2
            assert sum(1 for c, p in mine if p.type == t and s in c.swz and c.xsec) >= 2
    assert sum(1 for c, p in mine if c.spec == ("full", 20) and 16 in c.swz) >= 2
    for r in (1, 2, 3):
        assert sum(1 for c, p in mine if p.ragged == r and p.rows > RUN) >= 2, r
    assert sum(1 for c, p in mine if p.type == SC and p.rows < RUN) >= 2      # fewer rows than one run
    for L in (34, 50, 63, 64):
        assert sum(1 for c, p in mine if c.spec[1] == L) >= 2
    # the grid stride: every thread of a Full / Parity launch makes four trips, and one launch is at the cap
    assert all(p.trips == 4 for c, p in mine if p.type != SC and p.rows >= 2048 and not p.capped)
    capped = [c.name for c, p in mine if p.capped]
    assert len(capped) == 1 and "Full(23)" in capped[0]
    assert dict(PERM_PLANS)[gpu_file.PERM_BY_NAME[capped[0]]].trips == 8
    if kernel == "dots":                 # the groups of lanes stride too: 64 permutations leave 4 slots per workgroup
        assert max(-(-p.runs // ((p.nwg * NT) >> p.gp_log2)) for c, p in mine if p.type == SC) >= 32


MapPlan = collections.namedtuple("MapPlan", "stype dtype mode rows nwg trips capped ragged lds nonzero")


def map_plan_of(case):
    src, dst = gpu_file.ref_side(case.src), gpu_file.ref_side(case.dst)
    sd, dd = gpu_file.descriptor(case.src[0], case.src[2]), gpu_file.descriptor(case.dst[0], case.dst[2])
    srows, drows, run, nwg, lds = backend.subspace_map_plan(sd, dd, case.src[1], case.dst[1])
    assert (srows, drows) == (ref.rows_of(src), ref.rows_of(dst))
    assert run == (RUN if dst[0].kind == "sc" else 1) and nwg == workgroups(drows, MAX_WG)
    tables = sum((s[0].k + 1) * (s[0].L + 1) * 8 for s in (src, dst) if s[0].kind == "sc")
    assert lds == (tables + 15) // 16 * 16
    runs = -(-drows // run)
    return MapPlan(gpu_file.KIND_TYPE[case.src[0][0]], gpu_file.KIND_TYPE[case.dst[0][0]], ref.map_mode(src, dst), drows,
                   nwg, -(-runs // (nwg * NT)), drows > MAX_WG * ROWS_PER_WG, drows % RUN if run > 1 else 0, lds,
                   not case.zero)


MAP_PLANS = [(c, map_plan_of(c)) for c in MAP_CASES]
TYPES = (FULL, PARITY, EXPLICIT, SC)


@pytest.mark.parametrize("stype", TYPES)
@pytest.mark.parametrize("dtype", TYPES)
def test_every_map_instance_is_reached_in_every_mode_with_a_non_zero_result(stype, dtype):
    """(that a case marked non-zero is so is asserted against the host table above and on the device)"""
    mine = [(c, p) for c, p in MAP_PLANS if (p.stype, p.dtype) == (stype, dtype) and p.nonzero]
    assert len(mine) >= 2
    for mode in (ref.COPY, ref.FROM_SECTOR, ref.TO_SECTOR):
        assert sum(1 for c, p in mine if p.mode == mode) >= 2, mode
    assert sum(1 for c, p in mine if c.src[1] and c.dst[1]) >= 2             # sector -> the same sector
    zeros = [c for c, p in MAP_PLANS if (p.stype, p.dtype) == (stype, dtype) and c.src[1] * c.dst[1] == -1]
    assert len(zeros) >= 2                                                   # sector -> the opposite one
    assert sum(1 for c, p in mine if p.nwg > 1) >= 2


def test_every_map_regime_is_reached():
    for s in (FULL, PARITY):
        for d in (FULL, PARITY):
            swz = {(c.src[2], c.dst[2]) for c, p in MAP_PLANS if (p.stype, p.dtype) == (s, d) and p.mode == ref.COPY}
            assert swz >= {(a, b) for a in (0, 5, 6) for b in (0, 5, 6)}
    for r in (1, 2, 3):
        assert sum(1 for c, p in MAP_PLANS if p.ragged == r and p.rows > RUN) >= 2, r
    assert sum(1 for c, p in MAP_PLANS if p.dtype == SC and p.rows < RUN) >= 1
    ex = {s[0][1] for c, p in MAP_PLANS for s in (c.src, c.dst) if s[0][0] == "ex"}
    assert {"e13sorted", "e13unsorted", "e13wide"} <= ex
    capped = [c.name for c, p in MAP_PLANS if p.capped]
    assert capped == ["Parity(23,1)>Full(23)-stride"] and dict(MAP_PLANS)[gpu_file.MAP_BY_NAME[capped[0]]].trips == 8
    for L in (50, 63):
        assert sum(1 for c, p in MAP_PLANS if gpu_file.spec_L(c.src[0]) == L and p.nonzero) >= 2
    assert sum(1 for c, p in MAP_PLANS if p.lds > 0 and gpu_file.spec_L(c.src[0]) == 63) >= 2    # wide binomials in LDS


WeightPlan = collections.namedtuple("WeightPlan", "type branch items nwg trips lds")


def weight_plan_of(case):
    side = gpu_file.ref_side(case.side)
    branch = ref.weights_branch(side)
    items = side[0].dim // 2 if branch == "pairs" else ref.rows_of(side)
    nwg, scratch = backend.sector_weights_plan(gpu_file.descriptor(case.side[0], case.side[2]), case.side[1])
    ncols = side[0].L + 3
    assert nwg == workgroups(items, SW_MAX_WG), (case.name, nwg, items)      # (so the plan takes the branch named)
    assert scratch == (nwg + 1) * ncols * 8
    return WeightPlan(gpu_file.KIND_TYPE[case.side[0][0]], branch, items, nwg, -(-items // (nwg * ROWS_PER_WG)),
                      ncols * NT * 8)


WEIGHT_PLANS = [(c, weight_plan_of(c)) for c in WEIGHT_CASES]
BRANCHES = {FULL: ("pairs", "sector"), PARITY: ("pairs", "sector", "plain"), SC: ("pairs", "sector", "plain"),
            EXPLICIT: ("sector", "plain")}


@pytest.mark.parametrize("type_", TYPES)
def test_every_weights_instance_is_reached_in_every_branch_it_has(type_):
    mine = [(c, p) for c, p in WEIGHT_PLANS if p.type == type_]
    assert {p.branch for c, p in mine} == set(BRANCHES[type_])
    for b in BRANCHES[type_]:
        assert sum(1 for c, p in mine if p.branch == b and p.lds <= 65536) >= 2, b
    assert sum(1 for c, p in mine if p.nwg > 1) >= 2
    if type_ in (SC, EXPLICIT):          # dynamic LDS above 64 KB: the launch needs its hipFuncSetAttribute
        assert sum(1 for c, p in mine if p.lds > 65536) >= 2
        assert max(p.lds for c, p in mine) == 66 * 2048 == 135168
        assert sum(1 for c, p in mine if p.lds > 65536 and p.branch == "plain") >= 2
    if type_ == EXPLICIT:
        assert sum(1 for c, p in mine if p.lds > 65536 and p.branch == "sector") >= 2
    if type_ in (FULL, PARITY):          # the stride: twice what a launch covers without it
        assert [p.trips for c, p in mine if p.items > SW_MAX_WG * ROWS_PER_WG] == [2]


def test_weights_on_full_and_parity_above_64_kb_and_two_branches_are_out_of_reach():
    """UNREACHABLE, not passed over.  (L + 3) * 2048 bytes exceed 64 KB from L = 30: a Full or Parity vector of 2^29
    amplitudes at the least, 8 GiB -- and a SpinConserve subspace that carries the flip there has C(30, 15) = 155 117 520
    rows, 2.3 GiB, whose reference takes minutes; the large launches run on SpinConserve (plain) and Explicit (plain and
    sector), the same kernel text with the same LDS layout.  A plain branch on Full does not exist (Full always
    carries the flip), nor a pairs branch on Explicit (the plan asks for the closed form)."""
    assert (29 + 3) * 2048 == 65536 and (1 << 29) * 16 == 8 << 30 and comb(30, 15) == 155117520
    assert not any(p.lds > 65536 for c, p in WEIGHT_PLANS if p.type in (FULL, PARITY))
    assert not any(p.lds > 65536 and p.branch != "plain" for c, p in WEIGHT_PLANS if p.type == SC)
    for L in range(1, 25):
        assert ref.weights_branch((ref.Sub("full", L), 0, 0)) == "pairs"
    assert ref.weights_branch(gpu_file.ref_side((("ex", "e14par"), 0, 0))) == "plain"


def test_the_cap_of_workgroups_on_spin_conserve_rows_and_on_tiles_is_out_of_reach_of_a_quick_test():
    """NOT IN THE TABLES.  A SpinConserve launch of perm_apply or a SpinConserve target of a map strides only beyond
    4096 * 1024 rows: SpinConserve(25, 12), 5 200 300 rows, whose host reference takes several seconds per test.  The
    loop is the one line the Full and Parity instances run four or eight trips of, and perm_dots strides on
    SpinConserve at any size.  site_ops_kernel strides over its tiles beyond 2^16 of them: L = 29 at the least, 8 GiB."""
    assert comb(25, 12) == 5200300 > MAX_WG * ROWS_PER_WG > comb(24, 12)
    assert not any(p.capped for c, p in PERM_PLANS if p.type == SC)
    assert not any(p.capped for c, p in MAP_PLANS if p.dtype == SC)
    assert (16 << 29) == 8 << 30 and 29 - 12 > 16


SitePlan = collections.namedtuple("SitePlan", "name tile_bits L npasses nwg lds diag_outside general")


def site_plans(tb):
    old = os.environ.get("DNM_SITE_OPS_TILE_BITS")
    os.environ["DNM_SITE_OPS_TILE_BITS"] = str(tb)
    try:
        out = []
        for case in gpu_file.site_cases(tb):
            mats = gpu_file.site_matrices(case)
            tile, npasses, site_pass, nwg, lds = backend.site_ops_plan(gpu_file.site_desc(case.L, 0), mats)
            assert tile == tb and lds == 16 << min(tb, case.L) and nwg == 1 << max(0, case.L - tb)
            hi = site_pass[4:]
            general = int(np.sum(site_pass >= 0))
            # pass 0 gives its tile to its general sites first, then to diagonal ones: the rest are a factor per tile
            first = int(np.sum(hi == 0))
            outside = max(0, int(np.sum(hi == -2)) - max(0, (tb - 4) - first)) if case.L > tb else 0
            out.append(SitePlan(case.name, tile, case.L, npasses, nwg, lds, outside, general))
        return out
    finally:
        if old is None:
            del os.environ["DNM_SITE_OPS_TILE_BITS"]
        else:
            os.environ["DNM_SITE_OPS_TILE_BITS"] = old


@pytest.mark.parametrize("tb", [12, 13])
def test_both_site_product_instances_are_reached(tb):
    """twelve tile bits launch site_ops_kernel<256>, thirteen site_ops_kernel<512> (csrc/site_ops_kernels.hip:
    launch_site_ops_pass); the knob is read at every call, so the GPU file sets it in its own process"""
    assert os.environ.get("DNM_EXPERIMENTAL") == "1"
    plans = site_plans(tb)
    assert len(plans) == len(gpu_file.site_cases(12))
    by = {p.name: p for p in plans}
    assert sum(1 for p in plans if p.nwg > 1) >= 2 and sum(1 for p in plans if p.L < 4) >= 2
    assert by["three-passes"].npasses == 3 and by["three-passes"].L == 4 + 2 * (tb - 4) + 1
    assert by["diagonal-outside"].diag_outside == 3 and by["diagonal-outside"].general == 3
    assert by["diagonal-top"].diag_outside == 1 and by["diagonal-outside-2"].diag_outside == 2
    assert by["all-diagonal"].general == 0 and by["all-diagonal"].npasses == 1 and by["all-diagonal"].diag_outside == 2
    assert by["all-diagonal-L3"].general == 0
    assert sum(1 for p in plans if p.lds == 16 << tb) >= 2 and sum(1 for p in plans if p.lds < 16 << tb) >= 2
    assert {by["alone-site%d" % j].general for j in range(14)} == {1}
    assert by["general-tb+1"].npasses == 2 and by["general-tb"].npasses == 1


def test_coverage_table():
    """the tables of docs/lab/state_passes_exact_tests.md, as computed here (python -m pytest -s prints them)"""
    name = {FULL: "Full", PARITY: "Parity", EXPLICIT: "Explicit", SC: "SpinConserve"}
    for kernel in ("apply", "dots"):
        for t in (FULL, PARITY, SC):
            mine = [(c, p) for c, p in PERM_PLANS if p.type == t and c.only in (None, kernel)]
            print("perm_%s<%s>: %d cases; workgroups %d..%d; trips %s; ragged %s; LDS %d..%d bytes; L %d..%d"
                  % (kernel, name[t], len(mine), min(p.nwg for c, p in mine), max(p.nwg for c, p in mine),
                     sorted({p.trips for c, p in mine}), sorted({p.ragged for c, p in mine}),
                     min(p.lds for c, p in mine), max(p.lds for c, p in mine),
                     min(c.spec[1] for c, p in mine), max(c.spec[1] for c, p in mine)))
    for s in TYPES:
        for d in TYPES:
            mine = [(c, p) for c, p in MAP_PLANS if (p.stype, p.dtype) == (s, d)]
            print("submap<%s, %s>: %d cases, %d non-zero; workgroups %d..%d; trips %s; ragged %s; LDS %d..%d bytes; L %d..%d"
                  % (name[s], name[d], len(mine), sum(p.nonzero for c, p in mine), min(p.nwg for c, p in mine),
                     max(p.nwg for c, p in mine), sorted({p.trips for c, p in mine}), sorted({p.ragged for c, p in mine}),
                     min(p.lds for c, p in mine), max(p.lds for c, p in mine),
                     min(gpu_file.spec_L(c.src[0]) for c, p in mine), max(gpu_file.spec_L(c.src[0]) for c, p in mine)))
    for t in TYPES:
        mine = [(c, p) for c, p in WEIGHT_PLANS if p.type == t]
        print("sector_weights<%s>: %d cases; %s; workgroups %d..%d; trips %s; LDS %d..%d bytes; L %d..%d"
              % (name[t], len(mine), ", ".join("%s %d" % (b, sum(p.branch == b for c, p in mine)) for b in BRANCHES[t]),
                 min(p.nwg for c, p in mine), max(p.nwg for c, p in mine), sorted({p.trips for c, p in mine}),
                 min(p.lds for c, p in mine), max(p.lds for c, p in mine),
                 min(gpu_file.spec_L(c.side[0]) for c, p in mine), max(gpu_file.spec_L(c.side[0]) for c, p in mine)))
    for tb in (12, 13):
        plans = site_plans(tb)
        print("site_ops_kernel<%d>: %d cases; workgroups %d..%d; passes %s; LDS %d..%d bytes; L %d..%d"
              % (256 if tb == 12 else 512, len(plans), min(p.nwg for p in plans), max(p.nwg for p in plans),
                 sorted({p.npasses for p in plans}), min(p.lds for p in plans), max(p.lds for p in plans),
                 min(p.L for p in plans), max(p.L for p in plans)))
    assert len(PERM_PLANS) + len(MAP_PLANS) + len(WEIGHT_PLANS) >= 500
