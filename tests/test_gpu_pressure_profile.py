"""compute.PressureProfile on the GPU against tests/pressure_profile_ref.py (pinned by tests/test_pressure_profile.py).

All coordinates and box lengths are multiples of 2^-12 (times the cutoff, itself a short binary fraction), so separations,
minimum images, rsq and the bin coordinates are exact: a contracted and an uncontracted sum agree and no pair is in
doubt at a cutoff or at a bin edge.

Against the reference, per bin and component, in units of 2^-shift:
    |GPU - ref| <= K u sum |terms of the bin| + (terms of the bin),    u = 2^-53.
K = B + 8: B = max(4 K_REF, 8) is the bar tests/test_gpu_evaluator_cases.py holds that evaluator's force to (K_REF of
tests/test_evaluator_cases.py for the parameter set and mode used here, the sweep's force constant), and 8 roundings for
force_divr d_a, d_b, lambda_k (a difference, a quotient) and the product. Evaluators without a K_REF:
* special_pair.LJ is the reference's closed form in IEEE operations: B = 8, the project's floor for a short evaluator.
* the tables: r from a refined reciprocal square root (<= 1 ulp), s = (r - r_min) inv_dr with s <= r inv_dr, so the
  interpolation parameter is off by 2 u r inv_dr and F by that times |dF_k|; for the exponential tables used here
  |dF_k| / F = dr, which makes 2 r <= 5 roundings; with the floor 8 and rounded up: B = 16.
The measured worst ratio of every case is printed (run with -s). On an MI355X the rows equal the reference's word for
word in every case but Hertz (worst 4.1e-4 of the bound) and pair.Table (5.3e-4): a unit of 2^-shift (2^-36 at N = 343)
is far coarser than the rounding of the evaluators."""

import functools

import numpy as np
import pytest

import exclusion_ref as xref
import pressure_profile_ref as R
import table_ref as TR
from test_evaluator_cases import K_REF, generator

import azplugins_amd as azp
from azplugins_amd import _lib, compute
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

GRID = 2.0 ** -12
META = generator().load()[1]
ORACLE_NAME = {"DPDConservativeGeneralWeight": "DPDConservative"}
PBC = (True, True, True)
ORTHO = (0.0, 0.0, 0.0)


def force_bar(key):
    return max(4.0 * K_REF[key][1], 8.0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def quantise(x):
    return np.round(np.asarray(x, dtype=np.float64) / GRID) * GRID


@functools.lru_cache(maxsize=None)
def lattice(n_side, seed, jitter=0.12):
    """n_side^3 points of a jittered cubic lattice in the unit cube centred on 0, on the 2^-12 grid."""
    g = (np.arange(n_side) + 0.5) / n_side - 0.5
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    n = xyz.shape[0]
    u = np.stack([syn.u01(seed, np.arange(n, dtype=np.uint64), c) for c in range(3)], axis=1) - 0.5
    out = quantise(xyz + jitter * u / n_side)
    out.setflags(write=False)
    return out


def random_points(n, L, seed):
    u = np.stack([syn.u01(seed, np.arange(n, dtype=np.uint64), c) for c in range(3)], axis=1) - 0.5
    return quantise(u * np.asarray(L) * (1.0 - 2.0 ** -10))


def wrap_tilted(xyz, L, tilt):
    """wrap_into_box of azp_device.hpp for points of the cube [-L/2, L/2)^3: into the tilted cell (exact on the grid)."""
    xy, xz, yz = tilt
    x, y, z = (np.array(c) for c in np.asarray(xyz, dtype=np.float64).T)
    h = 0.5 * L[1]
    up, down = y >= h + z * yz, y < -h + z * yz
    y = y - L[1] * up + L[1] * down
    x = x - L[1] * xy * up + L[1] * xy * down
    h, s = 0.5 * L[0], y * xy + z * (xz - xy * yz)
    x = x - L[0] * (x >= h + s) + L[0] * (x < -h + s)
    return np.stack([x, y, z], axis=1)


def make_sim(xyz, L, tilt=ORTHO, periodic=PBC, types=None, type_names=("A",), **topology):
    snap = azp.Snapshot.from_arrays(xyz, azp.Box(L[0], L[1], L[2], *tilt, periodic=periodic), typeid=types, types=type_names, **topology)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    return sim


def attach(sim, forces):
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=forces, methods=[azp.ConstantVolume()])
    sim.run(0)


def add_profile(sim, axis, num_bins, path=0, **kw):
    p = compute.PressureProfile(axis, num_bins, **kw)
    p.path = path
    sim.operations.add(p)
    return p


def state_arrays(sim):
    st = sim.state
    pos4 = st.pos[: st.N].cpu().numpy()
    types = (np.ascontiguousarray(pos4[:, 3]).view(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return pos4[:, :3].copy(), types, st.tag[: st.N].cpu().numpy().view(np.uint32).astype(np.int64)


def reference(sim, prof, pair_forces=(), listed_forces=()):
    pos, types, tags = state_arrays(sim)
    box = sim.state.box
    shift, _ = compute.pressure_profile_shift(sim.state.N, prof.max_term)
    return R.profile(pos, types, tags, (box.Lx, box.Ly, box.Lz), prof._axis, prof.num_bins, shift, prof.max_term, pair_forces,
                     listed_forces, lower=prof._lower, upper=prof._upper, tilt=(box.xy, box.xz, box.yz), periodic=box.periodic)


def check(what, row, acc, K):
    """The summary words exactly, every bin word within the bound; prints the worst |GPU - ref| / bound."""
    want = acc.row()
    assert row[-4:].tolist() == want[-4:], (what, row[-4:], want[-4:])
    assert acc.pairs > 0
    diff = np.abs(np.array([int(a) - int(b) for a, b in zip(row[:-4], want[:-4])], dtype=np.float64)).reshape(acc.nb, 6)
    tol = R.tolerance(acc, K)
    used = acc.n_terms > 0
    assert not diff[~used].any(), (what, "a word no term went to")
    worst = (diff[used] / tol[used]).max() if used.any() else 0.0
    print("%-60s pairs %6d terms %8d  worst |GPU - ref| / bound %.3g (K = %g)" % (what, acc.pairs, acc.terms, worst, K))
    assert worst <= 1.0, (what, worst)


# ---------------------------------------------------------------------------
# forces: the GPU object and the reference evaluator from one description
# ---------------------------------------------------------------------------
def pair_force(oracle, name, sets, r_cut, mode="none", r_on=None, exclusions=()):
    """``sets[i][j]``: parameter dicts per type pair; ``r_cut`` (T, T). Returns (force, reference dict)."""
    T = len(sets)
    names = [chr(ord("A") + i) for i in range(T)]
    nl = azp.nlist.Cell(buffer=0.25, exclusions=exclusions)
    cls = getattr(azp.pair, name)
    f = cls(nl) if name == "DPDConservativeGeneralWeight" else cls(nl, mode=mode)
    r_cut = np.asarray(r_cut, dtype=np.float64)
    r_on = np.zeros((T, T)) if r_on is None else np.asarray(r_on, dtype=np.float64)
    for i in range(T):
        for j in range(i, T):
            f.params[(names[i], names[j])] = sets[i][j]
            f.r_cut[(names[i], names[j])] = float(r_cut[i, j])
            if mode == "xplor":
                f.r_on[(names[i], names[j])] = float(r_on[i, j])
    ev = R.oracle_pair(oracle, ORACLE_NAME.get(name, name), sets, r_cut, r_on, mode)
    return f, {"eval": ev, "r_max": float(r_cut.max())}


def fixture_pair(oracle, name, mode, k=0, exclusions=()):
    m = META["pair"][ORACLE_NAME.get(name, name)][k]
    f, ref = pair_force(oracle, name, [[m["params"]]], [[m["r_cut"]]], mode, [[m["r_on"]]], exclusions)
    return f, ref, m["r_cut"], force_bar("%s.%d.%s" % (ORACLE_NAME.get(name, name), k, mode)) + 8.0


def exp_table(r_min, r_end, width, closed):
    r = r_min + np.arange(width) * (r_end - r_min) / (width - 1 if closed else width)
    return np.exp(-r), np.exp(-r)


K_TABLE, K_SPECIAL = 16.0 + 8.0, 8.0 + 8.0

CASES = [(name, mode) for name in ("PerturbedLennardJones", "Hertz", "ExpandedYukawa", "Colloid") for mode in ("none", "shift", "xplor")]
CASES += [("DPDConservativeGeneralWeight", "none"), ("Table", "none")]


# ---------------------------------------------------------------------------
# 1. against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", CASES, ids=["%s-%s" % c for c in CASES])
def test_pair_evaluators_on_a_lattice(oracle, name, mode):
    """343 particles in a box of exactly three cells per axis (L = 3 r_cut), 16 bins along z, the automatic path (cells)."""
    if name == "Table":
        r_cut = 2.5
        U, F = exp_table(0.5, r_cut, 256, False)
        f = azp.pair.Table(azp.nlist.Cell(buffer=0.25))
        f.params[("A", "A")] = dict(r_min=0.5, U=U, F=F)
        f.r_cut[("A", "A")] = r_cut
        ref, K = {"eval": R.table_pair([[TR.pair_table(0.5, r_cut, U, F)]], [[r_cut]]), "r_max": r_cut}, K_TABLE
    else:
        f, ref, r_cut, K = fixture_pair(oracle, name, mode)
    L = (3.0 * r_cut,) * 3
    sim = make_sim(lattice(7, 5) * L[0], L)
    attach(sim, [f])
    prof = add_profile(sim, "z", 16)
    check("%s %s" % (name, mode), prof.row, reference(sim, prof, [ref]), K)


@pytest.mark.parametrize("path", [1, 2], ids=["all-pairs", "cells"])
def test_two_types_with_different_cutoffs(oracle, path):
    """Four cells along x, three along y, a non-periodic z (nothing wraps, nothing is outside): types A, B with r_cut 3,
    2.5 (A-B) and 2; profile along the non-periodic axis and along x."""
    m = META["pair"]["PerturbedLennardJones"]
    sets = [[m[0]["params"], m[1]["params"]], [m[1]["params"], m[0]["params"]]]
    r_cut = np.array([[3.0, 2.5], [2.5, 2.0]])
    K = max(force_bar("PerturbedLennardJones.0.shift"), force_bar("PerturbedLennardJones.1.shift")) + 8.0
    L = (12.0, 9.0, 9.0)
    xyz = lattice(7, 6) * np.array(L)
    types = (np.arange(343) % 3 == 0).astype(np.uint32)
    f, ref = pair_force(oracle, "PerturbedLennardJones", sets, r_cut, "shift")
    sim = make_sim(xyz, L, periodic=(True, True, False), types=types, type_names=("A", "B"))
    attach(sim, [f])
    for axis, nb in (("z", 16), ("x", 5)):
        prof = add_profile(sim, axis, nb, path)
        check("two types, axis %s, path %d" % (axis, path), prof.row, reference(sim, prof, [ref]), K)


def test_tilted_box(oracle):
    f, ref, r_cut, K = fixture_pair(oracle, "PerturbedLennardJones", "xplor")
    L = (8.0, 8.0, 8.0)
    tilt = (0.25, -0.125, 0.25)
    sim = make_sim(wrap_tilted(lattice(7, 7) * 8.0, L, tilt), L, tilt=tilt)
    attach(sim, [f])
    prof = add_profile(sim, "z", 16)
    check("tilted", prof.row, reference(sim, prof, [ref]), K)
    forced = add_profile(sim, "z", 16, path=2)
    with pytest.raises(azp.AzpError, match="orthorhombic"):
        forced.row
    sheared = add_profile(sim, "x", 16)
    with pytest.raises(azp.AzpError, match="sheared"):
        sheared.row
    bounded = add_profile(sim, "x", 4, lower=-2.0, upper=2.0)
    check("tilted, explicit range along x", bounded.row, reference(sim, bounded, [ref]), K)


@functools.lru_cache(maxsize=None)
def _sixty_five():
    return random_points(65, (8.0, 8.0, 8.0), 21)


@pytest.mark.parametrize("num_bins", [1, 2, 16, _lib.PRESSURE_PROFILE_LDS_BINS + 1, 8192, "r_cut / 64"])
def test_bin_counts(oracle, num_bins):
    """65 particles (one more than a wave) in L = 8 with r_cut = 2.5: one bin, two, 16, the first count past the LDS row,
    the most, and bins of r_cut / 64 (a pair crosses up to 66 of them). Hertz is soft: random points may come close."""
    f, ref, r_cut, K = fixture_pair(oracle, "Hertz", "none")
    f.r_cut[("A", "A")] = 2.5
    ref = {"eval": R.oracle_pair(oracle, "Hertz", [[META["pair"]["Hertz"][0]["params"]]], [[2.5]]), "r_max": 2.5}
    nb, kw = (num_bins, {}) if num_bins != "r_cut / 64" else (128, dict(lower=-2.5, upper=2.5))
    sim = make_sim(_sixty_five(), (8.0, 8.0, 8.0))
    attach(sim, [f])
    for path in (1, 2):
        prof = add_profile(sim, "y", nb, path, **kw)
        check("%s bins, path %d" % (num_bins, path), prof.row, reference(sim, prof, [ref]), K)


TWO = {"one bin": (0.25, 0.75), "three bins": (-0.5, 1.5), "periodic face": (3.5, -3.75), "no extent": (1.25, 1.25),
       "on an edge": (0.5, 2.0)}


@pytest.mark.parametrize("case", sorted(TWO))
def test_two_particles(oracle, case):
    m = META["pair"]["PerturbedLennardJones"][0]
    f, ref = pair_force(oracle, "PerturbedLennardJones", [[m["params"]]], [[2.5]])  # (three cells of 2.5 along z)
    K = force_bar("PerturbedLennardJones.0.none") + 8.0
    z = TWO[case]
    xyz = np.array([[0.0, 0.0, z[0]], [1.0, 0.25, z[1]]])
    sim = make_sim(xyz, (9.0, 9.0, 8.0))
    attach(sim, [f])
    for path in (1, 2):
        prof = add_profile(sim, "z", 8, path)
        acc = reference(sim, prof, [ref])
        assert acc.pairs == 1
        check("N = 2, %s, path %d" % (case, path), prof.row, acc, K)


def _chain_sim(oracle, exclusions, bond=None):
    """32 zig-zag chains of 4 (tests/test_gpu_rdf_exclusions.py's geometry) on the grid, PerturbedLJ between all beads."""
    xyz = []
    for c in range(32):
        x0, y0, z0 = -4.25 + 4.5 * (c % 2), -3.5 + 2.25 * ((c // 2) % 4), -3.5 + 2.25 * (c // 8)
        xyz += [(x0 + 0.875 * k, y0 + (0.25 if k % 2 else -0.25), z0 + 0.125 * k) for k in range(4)]
    bonds = xref.chain_bonds(32, 4)
    f, ref, r_cut, K = fixture_pair(oracle, "PerturbedLennardJones", "shift", exclusions=exclusions)
    forces = [f] + ([bond] if bond is not None else [])
    sim = make_sim(quantise(xyz), (9.0, 9.0, 9.0), bonds=np.asarray(bonds, dtype=np.uint32))
    attach(sim, forces)
    return sim, ref, K, bonds


def test_chains_with_excluded_pairs(oracle):
    """exclusions ("bond", "1-3"): the reference without those pairs, bit for bit in the summary words and within the
    bound in the bins (the subtraction is exact: it takes out what the walk put in); num_pairs is what is left."""
    sim, ref, K, bonds = _chain_sim(oracle, ("bond", "1-3"))
    excluded = {frozenset(p) for p in xref.pair_set(("bond", "1-3"), bonds=bonds)}
    assert len(excluded) == 96 + 64
    rows = {}
    for path in (1, 2):
        prof = add_profile(sim, "x", 16, path)
        rows[path] = prof.row
        acc = reference(sim, prof, [dict(ref, excluded=excluded)])
        check("chains less bonds and 1-3, path %d" % path, rows[path], acc, K)
        assert prof.num_pairs == acc.pairs
    assert np.array_equal(rows[1], rows[2])
    full = reference(sim, prof, [ref])
    assert full.pairs - acc.pairs == len(excluded)  # (every excluded pair is inside r_cut here)


def test_chain_of_three_with_its_bonds_excluded(oracle):
    """N = 3: the pair force sees the 1-3 pair alone, the bonds come from the bond force; the sum of two forces."""
    f, ref, r_cut, K = fixture_pair(oracle, "PerturbedLennardJones", "none", exclusions=("bond",))
    dw_params = META["bond"]["DoubleWell"][0]["params"]
    dw = azp.bond.DoubleWell()
    dw.params["A-A"] = dw_params
    xyz = np.array([[-1.0, 0.0, -0.75], [0.0, 0.25, 0.25], [1.0, 0.0, 1.25]])
    sim = make_sim(xyz, (9.0, 9.0, 8.0), bonds=np.array([[0, 1], [1, 2]], dtype=np.uint32))
    attach(sim, [f, dw])
    listed = {"eval": R.oracle_bond(oracle, "DoubleWell", [dw_params]), "groups": [(0, 1, 0), (1, 2, 0)]}
    Kb = force_bar("DoubleWell.0.bond") + 8.0
    prof = add_profile(sim, "z", 8)
    acc = reference(sim, prof, [dict(ref, excluded={frozenset((0, 1)), frozenset((1, 2))})], [listed])
    assert acc.pairs == 3
    check("N = 3, pair + bond", prof.row, acc, max(K, Kb))
    only = add_profile(sim, "z", 8, forces=[dw])
    check("N = 3, the bonds alone", only.row, reference(sim, only, [], [listed]), Kb)


BONDED = ["DoubleWell", "Quartic", "Table", "SpecialPairLJ"]


@pytest.mark.parametrize("name", BONDED)
def test_bonded_evaluators(oracle, name):
    """The chains' bonds (or, for the special pairs, their 1-4 pairs) under every two-body bonded force."""
    bonds = np.asarray(xref.chain_bonds(32, 4), dtype=np.uint32)
    topo = dict(bonds=bonds)
    groups = [(int(a), int(b), 0) for a, b in bonds]
    if name == "SpecialPairLJ":
        pairs = np.array([[4 * c, 4 * c + 3] for c in range(32)], dtype=np.uint32)
        topo = dict(bonds=bonds, pairs=pairs)
        groups = [(int(a), int(b), 0) for a, b in pairs]
        f = azp.special_pair.LJ()
        f.params["A-A"] = dict(epsilon=0.5, sigma=1.5)
        f.r_cut["A-A"] = 3.0
        ev, K = R.special_pair_lj([dict(epsilon=0.5, sigma=1.5, r_cut=3.0)]), K_SPECIAL
    elif name == "Table":
        U, F = exp_table(0.5, 2.0, 129, True)
        f = azp.bond.Table()
        f.params["A-A"] = dict(r_min=0.5, r_max=2.0, U=U, F=F)
        ev, K = R.table_bond([TR.bond_table(0.5, 2.0, U, F)]), K_TABLE
    else:
        p = META["bond"][name][0]["params"]
        f = getattr(azp.bond, name)()
        f.params["A-A"] = p
        ev, K = R.oracle_bond(oracle, name, [p]), force_bar("%s.0.bond" % name) + 8.0
    xyz = []
    for c in range(32):
        x0, y0, z0 = -4.25 + 4.5 * (c % 2), -3.5 + 2.25 * ((c // 2) % 4), -3.5 + 2.25 * (c // 8)
        xyz += [(x0 + 0.875 * k, y0 + (0.25 if k % 2 else -0.25), z0 + 0.125 * k) for k in range(4)]
    sim = make_sim(quantise(xyz), (9.0, 9.0, 9.0), **topo)
    attach(sim, [f])
    prof = add_profile(sim, "x", 16)
    acc = reference(sim, prof, [], [{"eval": ev, "groups": groups}])
    assert acc.pairs == len(groups)
    check("bonded %s" % name, prof.row, acc, K)


# ---------------------------------------------------------------------------
# 2. bit for bit
# ---------------------------------------------------------------------------
def test_calls_paths_and_reorderings_change_no_bit(oracle):
    import torch

    f, ref, r_cut, K = fixture_pair(oracle, "PerturbedLennardJones", "shift")
    sim = make_sim(lattice(7, 8) * 9.0, (9.0, 9.0, 9.0))
    attach(sim, [f])
    profs = {(nb, path): add_profile(sim, "z", nb, path) for nb in (16, _lib.PRESSURE_PROFILE_LDS_BINS + 1) for path in (1, 2)}
    first = {key: p.row for key, p in profs.items()}
    for nb in (16, _lib.PRESSURE_PROFILE_LDS_BINS + 1):
        assert np.array_equal(first[(nb, 1)], first[(nb, 2)])
        assert first[(nb, 1)][-4] > 3000 and first[(nb, 1)][-2] == 0
    for key, p in profs.items():
        assert np.array_equal(first[key], p.row)
    # the kinetic part too: the whole row, kinetic field included
    whole = profs[(16, 2)]._read("row").copy()
    st = sim.state
    n = st.N
    perm = torch.from_numpy(np.random.default_rng(12).permutation(n)).to(st.device)
    for name in ("pos", "vel", "tag", "image"):
        a = getattr(st, name)
        a[:n] = a[:n].index_select(0, perm)
    st.position_generation += 1
    st.order_generation += 1
    for key, p in profs.items():
        assert np.array_equal(first[key], p.row), key
    tag0 = st.tag[:n].cpu().numpy().copy()
    azp.ParticleSorter(particles_per_block=16).sort(sim)
    assert not np.array_equal(st.tag[:n].cpu().numpy(), tag0)
    for key, p in profs.items():
        assert np.array_equal(first[key], p.row), key
    assert np.array_equal(whole, profs[(16, 2)]._read("row"))


def test_translation_rotates_the_profile(oracle):
    """L = 8, 16 bins of 0.5: every particle moved by one bin width along z and wrapped: the row rotates by one bin."""
    f, ref, r_cut, K = fixture_pair(oracle, "PerturbedLennardJones", "shift")
    f.r_cut[("A", "A")] = 2.5
    xyz = lattice(6, 9) * 8.0
    moved = xyz.copy()
    moved[:, 2] = np.where(moved[:, 2] + 0.5 >= 4.0, moved[:, 2] + 0.5 - 8.0, moved[:, 2] + 0.5)
    rows = []
    for pts in (xyz, moved):
        sim = make_sim(pts, (8.0, 8.0, 8.0))
        attach(sim, [f])
        rows.append([add_profile(sim, "z", 16, path).row for path in (1, 2)])
        assert np.array_equal(*rows[-1])
    a, b = rows[0][0], rows[1][0]
    assert a[-4] > 1000 and np.array_equal(a[-4:], b[-4:])
    assert np.array_equal(np.roll(a[:-4].reshape(16, 6), 1, axis=0), b[:-4].reshape(16, 6))


# ---------------------------------------------------------------------------
# 3. consistency with the force's own virial
# ---------------------------------------------------------------------------
def test_row_sums_to_the_virial_of_the_force(oracle):
    """sum_k row_k 2^-shift against the sum over the particles of the force's per-particle virial (compute_virial on in
    this test only). Tolerance, per component: the bound of the profile summed over the bins, plus the force kernel's own:
    its per-pair bar B on the same terms, the <= 128 additions of a particle's row and the 9 levels of numpy's pairwise
    sum over the particles -- (K + B + 128 + 9) u sum |terms| + (terms) 2^-shift."""
    f, ref, r_cut, K = fixture_pair(oracle, "PerturbedLennardJones", "shift")
    sim = make_sim(lattice(7, 10) * 9.0, (9.0, 9.0, 9.0))
    f.compute_virial = True
    attach(sim, [f])
    prof = add_profile(sim, "z", 16)
    row = prof.row
    acc = reference(sim, prof, [ref])
    assert int(f.nlist.n_neigh.max()) <= 128
    virial = f._virial.cpu().numpy().reshape(6, -1)[:, : sim.state.N].sum(axis=1)
    total = row[:-4].reshape(16, 6).astype(np.float64).sum(axis=0) * 2.0 ** -int(row[-1])
    for c in range(6):
        tol = (K + (K - 8.0) + 128 + 9) * R.U_ROUND * acc.abs_terms[:, c].sum() + acc.n_terms[:, c].sum() * 2.0 ** -acc.shift
        print("component %d: profile %.17g force %.17g tolerance %.3g" % (c, total[c], virial[c], tol))
        assert abs(total[c] - virial[c]) <= tol, c
    # the profile itself needs no virial pass and turns none on
    g, _, _, _ = fixture_pair(oracle, "PerturbedLennardJones", "shift")
    other = make_sim(lattice(7, 10) * 9.0, (9.0, 9.0, 9.0))
    other.operations.add(compute.PressureProfile("z", 16))
    attach(other, [g])
    assert not g.compute_virial and np.array_equal(other.operations.computes[0].row, row)


# ---------------------------------------------------------------------------
# 4. refusals and the host quantities
# ---------------------------------------------------------------------------
def test_refusals(oracle):
    f, ref, r_cut, K = fixture_pair(oracle, "PerturbedLennardJones", "none")
    sim = make_sim(lattice(7, 11) * 9.0, (9.0, 9.0, 9.0))
    prof = add_profile(sim, "z", 16, forces=[f])
    with pytest.raises(azp.AzpError, match=r"sim\.run\(0\)"):
        prof.row
    attach(sim, [f])
    assert prof.row[-4] > 0
    # r_cut beyond half the width
    f.r_cut[("A", "A")] = 4.75
    with pytest.raises(azp.AzpError, match="half the perpendicular width"):
        prof.row
    f.r_cut[("A", "A")] = 3.0
    # a box too narrow for the cells, forced
    narrow = make_sim(lattice(5, 12) * 7.0, (7.0, 7.0, 7.0))
    g, _, _, _ = fixture_pair(oracle, "PerturbedLennardJones", "none")
    attach(narrow, [g])
    with pytest.raises(azp.AzpError):
        add_profile(narrow, "z", 8, path=2).row
    assert add_profile(narrow, "z", 8, path=0).row[-4] > 0
    # max_term small enough that a pair overflows: the read raises and names it, the counters can still be read
    tight = add_profile(sim, "z", 16, max_term=2.0 ** -6)
    with pytest.raises(azp.AzpError, match="max_term"):
        tight.normal_pressure
    assert tight.overflow > 0 and tight.num_pairs == prof.num_pairs
    # a decomposed run
    sim.domain = object()
    try:
        with pytest.raises(azp.AzpError, match="decomposed"):
            prof.row
    finally:
        sim.domain = None
    # forces the compute does not take are refused when they come from the integrator too
    h = azp.angle.Harmonic()
    chain = make_sim(np.array([[-1.0, 0, 0], [0, 0, 0], [1.0, 0, 0]]), (9.0, 9.0, 9.0), angles=np.array([[0, 1, 2]], dtype=np.uint32))
    h.params["A-A-A"] = dict(k=1.0, t0=2.0)
    attach(chain, [h])
    with pytest.raises(azp.AzpError, match="many-body"):
        add_profile(chain, "z", 8).row


def test_quantities_of_a_liquid(oracle):
    """The properties hang together: the tensor is the sum of its parts, P_N is its zz, the volumes tile the box, the
    kinetic part is the owned field's, and the trace agrees with ThermodynamicQuantities within the profile's bound."""
    sim, _ = _liquid(True)
    prof = add_profile(sim, "z", 8)
    p, pk, pc = prof.pressure_tensor, prof.kinetic_pressure_tensor, prof.configurational_pressure_tensor
    assert p.shape == (8, 6) and np.array_equal(p, pk + pc)
    assert np.array_equal(prof.normal_pressure, p[:, 5]) and np.array_equal(prof.tangential_pressure, 0.5 * (p[:, 0] + p[:, 3]))
    vol = prof.bin_volumes
    assert vol.sum() == pytest.approx(sim.state.box.volume, rel=1e-14)
    box = sim.state.box
    field = compute.CartesianThermodynamicField((0, 0, 8), (0, 0, -0.5 * box.Lz), (0, 0, 0.5 * box.Lz), streaming="subtract")
    sim.operations.add(field)
    want = compute.thermo_field_quantities(field.sums, field.bin_volumes, "subtract")["pressure_tensor"]
    assert np.abs(want[:, :6]).min() > 0.0 and np.array_equal(_bits(pk), _bits(want - _virial_part(field)))
    gamma = prof.surface_tension()
    assert gamma == pytest.approx(((prof.normal_pressure - prof.tangential_pressure) * box.Lz / 8).sum() / 2, rel=1e-12)
    assert prof.surface_tension(interfaces=1) == pytest.approx(2 * gamma, rel=1e-12)
    keep = add_profile(sim, "z", 8, streaming="keep")
    assert (keep.kinetic_pressure_tensor[:, 5] >= pk[:, 5]).all() and np.array_equal(keep.configurational_pressure_tensor, pc)
    assert not any(f.compute_virial for f in sim.operations.integrator.forces)


def _virial_part(field):
    """W / V of a field's rows (zero while no force was evaluated with virials)."""
    return field.sums[:, 11:17] / field.bin_volumes[:, None]


# ---------------------------------------------------------------------------
# 5. the recorder
# ---------------------------------------------------------------------------
def _liquid(bonded):
    cfg = syn.config_north_star(ncell=(8, 4, 4))
    n = cfg["xyz"].shape[0]
    tag = np.arange(n, dtype=np.uint64)
    v = np.stack([syn.normal(91, tag, c) for c in range(3)], axis=1)
    bonds = np.stack([np.arange(0, n, 4), np.arange(1, n, 4)], axis=1).astype(np.uint32) if bonded else None
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], velocity=v - v.mean(axis=0), bonds=bonds)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    plj = azp.pair.PerturbedLennardJones(nlist=azp.nlist.Cell(buffer=0.3), default_r_cut=cfg["r_cut"], mode="shift")
    plj.params[("A", "A")] = cfg["params"]
    forces = [plj]
    if bonded:
        dw = azp.bond.DoubleWell()
        dw.params["A-A"] = dict(r_0=1.0, r_1=1.5, U_1=1.0, U_tilt=0.5)
        forces.append(dw)
    sim.operations.integrator = azp.Integrator(dt=0.004, forces=forces, methods=[azp.ConstantVolume()])
    sim.run(0)
    return sim, plj


def _final(sim):
    st = sim.state
    order = np.argsort(st.tag[: st.N].cpu().numpy().view(np.uint32))
    return st.pos[: st.N].cpu().numpy()[order], st.vel[: st.N].cpu().numpy()[order]


def test_recorder_in_a_run():
    plain, _ = _liquid(True)
    plain.run(10)
    sim, f = _liquid(True)
    prof = add_profile(sim, "x", 12)
    rec = compute.PressureProfileRecorder(prof, 2)
    sim.operations.writers.append(rec)
    sim.run(10)
    assert not f.compute_virial
    for a, b in zip(_final(plain), _final(sim)):
        assert np.array_equal(_bits(a), _bits(b))  # (the recorder changes no bit of the trajectory)
    assert rec.timesteps.tolist() == [2, 4, 6, 8, 10]
    rows, table = rec.rows, rec.table()
    assert rows.shape == (5, 76) and table["pressure_tensor"].shape == (5, 12, 6) and table["surface_tension"].shape == (5,)
    twin, _ = _liquid(True)
    twin_prof = add_profile(twin, "x", 12)
    for k in range(5):
        twin.run(2)
        assert np.array_equal(rows[k], twin_prof.row), k
        assert np.array_equal(_bits(table["pressure_tensor"][k]), _bits(twin_prof.pressure_tensor)), k
        assert table["surface_tension"][k] == twin_prof.surface_tension()
    mean = rec.mean()
    whole = rec._rows[:5].cpu().numpy()
    ints, kin = prof._split(whole)
    want = compute.pressure_profile_quantities(ints.sum(axis=0), kin.sum(axis=0), np.repeat(prof.bin_volumes[None], 5, axis=0).sum(axis=0), 0,
                                               np.mean([sim.state.box.Lx / 12] * 5),
                                               "subtract", shift=int(ints[0, -1]))
    for name in ("pressure_tensor", "normal_pressure", "surface_tension"):
        assert np.array_equal(_bits(np.asarray(mean[name], dtype=np.float64)), _bits(np.asarray(want[name], dtype=np.float64))), name
    assert int(mean["num_pairs"]) == int(rows[:, -4].sum())
    rec.reset()
    assert rec.timesteps.size == 0 and rec.table() == {}
