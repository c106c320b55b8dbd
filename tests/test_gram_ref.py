"""tests/gram_ref.py -- the int64 reference that tests/test_gpu_gram_exact.py compares the four Gram-panel observable
sweeps with -- pinned three ways (no GPU needed): at L <= 6 to dense operators built from Kronecker products of exchange,
rotation and Pauli matrices, <psi|O_m^H O_m'|psi>; to the host partner tables (dnm_pm_partner_indices,
dnm_swap_partner_indices, dnm_cyc_partner_indices, dnm_pauli_partner_indices) on a sample of the rows of every shape
the GPU file uses, and on all rows of its L = 63 and L = 64 shapes; and its two ways of ranking a SpinConserve
configuration to each other.

And the COVERAGE PROOF of the GPU file's case table: the plan of every case (dnm_*_moments_plan; for the calls with an
XParity sector, which the plan entries do not take, the rule of tests/test_gram_plan_host.py with nrows = dim / 2) says
which kernel instance gram_dispatch picks (TYPE x tile rows), the panel (lowered or not), the panels per workgroup,
whether the last panel is ragged and whether trailing workgroups have nothing to do.  The union over the table must
hold every instance and every such situation; what cannot be reached is named in its own test."""
import collections
from math import comb

import numpy as np
import pytest

import gram_ref as ref
from dynamite_amd import backend
import test_gpu_gram_exact as gpu_file
from test_gpu_vec import ints

CASES = gpu_file.CASES
FULL, PARITY, SC = 0, 1, 3


# ---------------------------------------------------------------------------------------------------------------------
# the reference against dense operators, L <= 6
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


def dense_ops(sweep, L, items):
    if sweep == "pm":                   # sigma_minus = sigma-x - i sigma-y sets bit j with matrix element 2
        return [at_site(X - 1j * Y, j, L) / 2 for j in range(L)]         # <sigma+_i sigma-_j> = 4 P[i][j]
    one = [np.eye(1 << L, dtype=np.complex128)]
    if sweep == "swap":
        return one + [exchange(a, b, L) for a, b in items]
    if sweep == "cyc":                  # C = P_ab P_bc
        return one + [exchange(a, b, L) @ exchange(b, c, L) for a, b, c in items]
    return one + [at_site({1: X, 2: 1j * Y, 3: Z}[kind], site, L) for site, kind in items]


DENSE = [("full", 5, 0, 0), ("full", 6, 0, 0), ("parity", 6, 0, 0), ("parity", 6, 0, 1), ("parity", 5, 0, 1),
         ("sc", 6, 3, 0), ("sc", 5, 2, 0), ("sc", 6, 1, 0), ("sc", 6, 5, 0), ("sc", 4, 0, 0), ("sc", 4, 4, 0)]


@pytest.mark.parametrize("sweep", ref.SWEEPS)
@pytest.mark.parametrize("xsec", [0, 1, -1])
@pytest.mark.parametrize("kind,L,k,space", DENSE, ids=str)
def test_reference_is_the_dense_operators(kind, L, k, space, xsec, sweep):
    sub = ref.Sub(kind, L, k, space)
    if sweep == "pauli" and kind == "sc":
        return                          # (a flip leaves the sector: the sweep refuses SpinConserve)
    if xsec and (sweep in ("pm", "pauli") or (kind == "parity" and L % 2) or (kind == "sc" and L != 2 * k)):
        return                          # (no such call)
    items = None if sweep == "pm" else gpu_file.ITEMS[sweep](L, 14)
    n = ref.state_size(sub, xsec)
    xr, xi = ints(n, 7 * L + k + space)
    got_r, got_i = ref.reference(sweep, sub, xsec, items, xr, xi)
    cfg = sub.configs()[:n].astype(np.int64)
    psi = np.zeros(1 << L, dtype=np.complex128)
    psi[cfg] = xr + 1j * xi
    if xsec:
        psi[cfg ^ ((1 << L) - 1)] = xsec * (xr + 1j * xi)
    cols = np.stack([O @ psi for O in dense_ops(sweep, L, items)], axis=1)
    want = cols.conj().T @ cols / (2 if xsec else 1)      # (the representatives are half of the rows)
    assert np.array_equal(got_r.astype(np.float64), want.real) and np.array_equal(got_i.astype(np.float64), want.imag)
    assert got_r.shape[0] < 3 or n < 4 or np.any(got_i != 0)


# ---------------------------------------------------------------------------------------------------------------------
# the two ways of ranking; the reference against the host partner tables on the GPU file's shapes
# ---------------------------------------------------------------------------------------------------------------------

def sample(nrows, seed, everything=False):
    if everything or nrows <= 5000:
        return np.arange(nrows, dtype=np.int64)
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([np.arange(64), np.arange(nrows - 64, nrows), [511, 512, 513],
                                     rng.integers(0, nrows, 3000)])).astype(np.int64)


SC_SHAPES = sorted({(c.L, c.k + (c.sweep == "pm")) for c in CASES if c.kind == "sc"}
                   | {(c.L, c.k) for c in CASES if c.kind == "sc"})


@pytest.mark.parametrize("L,k", SC_SHAPES, ids=str)
def test_colex_rank_is_the_position_in_the_enumeration(L, k):
    c = ref.combs(L, k)
    assert c.size == comb(L, k)
    if c.size == 0:
        return
    rows = sample(c.size, L + k, everything=L >= 63)
    assert np.array_equal(ref.colex_rank(c[rows], L), rows)
    assert np.array_equal(ref.Sub("sc", L, k).index(c[rows]), rows)
    assert np.all(ref.popcount(c[rows]) == k) and (c.size < 2 or np.all(c[1:] > c[:-1]))


def _shapes():
    seen, out = set(), []
    for c in CASES:
        key = (c.sweep, c.kind, c.L, c.k, c.space, c.xsec, c.items)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


SHAPES = _shapes()


def test_the_wide_shapes_are_in_the_table():
    wide = {(c.sweep, c.L, c.k) for c in SHAPES if c.L >= 63}
    assert {("pm", 64, 1), ("swap", 64, 2), ("cyc", 64, 2), ("pm", 63, 59), ("swap", 63, 60), ("cyc", 63, 60),
            ("swap", 63, 3), ("cyc", 63, 3)} <= wide
    assert comb(63, 60) == comb(63, 3) == 39711


@pytest.mark.parametrize("name", [c.name for c in SHAPES if c.sweep != "pm" or c.kind == "sc"])
def test_reference_is_the_host_partner_table(name):
    """Row by row: the index into the vector and the factor of every column.  All rows of the L = 63 and L = 64 shapes,
    a sample with both ends elsewhere.  (The sigma+ sigma- entry serves SpinConserve alone: Full and Parity have no
    host table -- their partners are index ^ mask -- and are pinned to the dense operators above.)"""
    c = gpu_file.BY_NAME[name]
    sub = gpu_file.ref_sub(c)
    cfgs = ref.row_configs(c.sweep, sub, c.xsec)
    if cfgs.size == 0:
        return
    rows = sample(cfgs.size, len(name), everything=c.L >= 63)
    idx, sgn = ref.partner_table(c.sweep, sub, c.xsec, c.items, cfgs[rows])
    d = gpu_file.descriptor(c)
    if c.sweep == "pm":
        got = backend.pm_partner_indices(d, rows)
        assert np.array_equal(got, np.where(sgn == 1, idx, -1))
        return
    if c.sweep == "swap":
        gi, gs = backend.swap_partner_indices(d, c.items, rows, c.xsec)
    elif c.sweep == "cyc":
        gi, gs = backend.cyc_partner_indices(d, c.items, rows, c.xsec)
    else:
        gi, gs = backend.pauli_partner_indices(d, c.items, rows)
    assert np.array_equal(idx[:, 0], rows) and np.all(sgn[:, 0] == 1)         # the state's own column
    assert np.array_equal(gi, idx[:, 1:]) and np.array_equal(gs.astype(np.int64), sgn[:, 1:])


# ---------------------------------------------------------------------------------------------------------------------
# coverage of the GPU file's case table, from the plans
# ---------------------------------------------------------------------------------------------------------------------

PLANS = [(c, gpu_file.plan_of(c)) for c in CASES]       # (asserts plan entry == rule wherever there is an entry)
NB = (1, 2, 3, 4)


def seen(pred, what):
    return {what(c, p) for c, p in PLANS if pred(c, p)}


def test_every_instance_of_swap_rotation_and_pauli_is_reached():
    for sweep, types in (("swap", (FULL, PARITY, SC)), ("cyc", (FULL, PARITY, SC)), ("pauli", (FULL, PARITY))):
        got = seen(lambda c, p: c.sweep == sweep, lambda c, p: (p.type, p.nb))
        assert got == {(t, nb) for t in types for nb in NB}, sweep


def test_every_reachable_instance_of_pm_is_reached():
    got = seen(lambda c, p: c.sweep == "pm" and p.nrows > 0, lambda c, p: (p.type, p.nb))
    assert got == {(SC, nb) for nb in NB} | {(t, nb) for t in (FULL, PARITY) for nb in (1, 2)}


def test_pm_on_full_and_parity_with_three_or_four_tile_rows_is_out_of_reach():
    """UNREACHABLE, not passed over: sigma+ sigma- has one column per site, so three tile rows need L >= 33 -- a vector
    of 2^32 amplitudes (Parity) or 2^33 (Full), 64 GiB at the least.  pm_moments_kernel<Full, 3>, <Full, 4>,
    <Parity, 3> and <Parity, 4> run the same pm_tile_multiply<3>, <4> as the SpinConserve instances and the same fill
    as the instances of one and two tile rows, which are all reached."""
    for L in range(1, 33):
        assert -(-L // 16) <= 2
    assert -(-33 // 16) == 3 and (1 << (33 - 1)) * 16 == 64 << 30
    assert not any(c.sweep == "pm" and c.kind != "sc" and p.nb > 2 for c, p in PLANS)


def test_both_xparity_sectors_over_every_parent_at_every_tile_row_count():
    for sweep in ("swap", "cyc"):
        got = seen(lambda c, p: c.sweep == sweep and c.xsec != 0, lambda c, p: (p.type, c.xsec, p.nb))
        assert got == {(t, s, nb) for t in (FULL, PARITY, SC) for s in (1, -1) for nb in NB}, sweep


def test_every_panel_size_is_reached_and_the_lowered_ones_by_lowering():
    assert seen(lambda c, p: True, lambda c, p: p.B) == {6, 7, 8, 9}
    lowered = seen(lambda c, p: p.B < p.B_unlowered, lambda c, p: (c.sweep, p.B))
    assert {("swap", 8), ("swap", 6), ("cyc", 8), ("cyc", 6), ("pm", 6)} <= lowered
    # the figures of the lowered cases: (63, 60) takes 8 for 9 at 16 columns and 6 for 7 at 64; the table of 31 KB
    # still fits beside the panels of 17 and 48 columns
    by = {c.name: p for c, p in PLANS}
    for sweep in ("swap", "cyc"):
        assert [by["%s-SC(63,60)-w%d" % (sweep, w)].B for w in (16, 17, 48, 64)] == [8, 7, 7, 6]
        assert [by["%s-SC(63,3)-w%d" % (sweep, w)].B for w in (16, 64)] == [9, 7]
    assert by["pm-SC(63,59)"].B == 6 and by["pm-SC(63,2)"].B == 7
    # at B = 6 the wave-sum buffer (26 tiles of 256 doubles at four tile rows) takes the panel's place
    assert 26 * 256 * 8 <= (65 * 16) << 6


FILLS = [("pm", FULL), ("pm", PARITY), ("pm", SC), ("swap", FULL), ("swap", PARITY), ("swap", SC), ("cyc", FULL),
         ("cyc", PARITY), ("cyc", SC), ("pauli", FULL), ("pauli", PARITY)]


@pytest.mark.parametrize("sweep,type_", FILLS, ids=str)
def test_one_and_several_panels_per_workgroup_on_every_fill(sweep, type_):
    got = seen(lambda c, p: c.sweep == sweep and p.type == type_ and p.nrows > 0, lambda c, p: p.per_wg > 1)
    assert got == {False, True}
    if sweep in ("swap", "cyc"):        # and under an XParity sector
        got = seen(lambda c, p: c.sweep == sweep and p.type == type_ and c.xsec, lambda c, p: p.per_wg > 1)
        assert got == {False, True}


@pytest.mark.parametrize("sweep", ["pm", "swap", "cyc"])
def test_ragged_panels_and_idle_workgroups_on_every_spin_conserve_fill(sweep):
    mine = [(c, p) for c, p in PLANS if c.sweep == sweep and p.type == SC]
    assert any(p.ragged and p.npanels > 1 for c, p in mine)
    assert any(p.ragged and p.per_wg > 1 for c, p in mine)            # the per-panel guard on a second trip
    assert any(p.busy < p.nwg for c, p in mine)                        # workgroups that store zeros
    assert any(p.busy < p.nwg and p.ragged for c, p in mine)
    if sweep != "pm":
        assert any(p.ragged and c.xsec for c, p in mine)


def test_the_figures_of_the_large_cases():
    by = {c.name: p for c, p in PLANS}
    p = by["pm-SC(20,9)"]
    assert (p.nrows, p.npanels, p.per_wg, p.busy, p.nwg - p.busy) == (184756, 1444, 2, 722, 302)
    for sweep in ("swap", "cyc"):
        p = by["%s-SC(22,11)-w16" % sweep]
        assert (p.nrows, p.per_wg, p.busy, p.nwg - p.busy) == (705432, 2, 689, 335)
        p = by["%s-SC(22,11)-w17" % sweep]
        assert (p.per_wg, p.busy, p.nwg - p.busy) == (6, 919, 105)
        assert by["%s-SC(22,11)-x--w17" % sweep].per_wg > 1
    assert by["pm-Full(18)"].per_wg == 2 and by["pauli-Full(20)-w16"].per_wg == 2


def test_swizzles_and_wide_configurations_are_in_the_table():
    for sweep in ref.SWEEPS:
        for kind in ("full", "parity"):
            assert any(c.sweep == sweep and c.kind == kind and {0, 5, 6} <= set(c.swz) for c in CASES), (sweep, kind)
        assert any(c.sweep == sweep and c.kind == "full" and c.L == 20 and 16 in c.swz for c in CASES), sweep
    for sweep in ("pm", "swap", "cyc"):
        assert any(c.sweep == sweep and c.L == 64 for c in CASES)
    for sweep in ("swap", "cyc"):
        assert any(c.L == 64 and any(63 in it for it in c.items) for c in CASES if c.sweep == sweep)
        assert any(c.L == 63 and c.k == 60 and any(62 in it for it in c.items) for c in CASES if c.sweep == sweep)


def test_coverage_table():
    """the table of docs/lab/gram_exact_tests.md, as computed here (python -m pytest -s prints it)"""
    rows = collections.defaultdict(list)
    for c, p in PLANS:
        key = (c.sweep, c.kind + (" x%+d" % c.xsec if c.xsec else ""), p.nb)
        rows[key].append("%s B=%d%s per_wg=%d%s%s" % (c.name, p.B, "(lowered)" if p.B < p.B_unlowered else "", p.per_wg,
                                                      " ragged" if p.ragged else "",
                                                      " idle=%d" % (p.nwg - p.busy) if p.busy < p.nwg else ""))
    for key in sorted(rows):
        print("%-6s %-12s NB=%d: %d cases; %s" % (key + (len(rows[key]), "; ".join(rows[key][:3]))))
    assert len(rows) >= 4 * 3 + 4 * 3 + 2 * 4 + 8 + 2 * 6 * 4
