"""angle.Table and dihedral.Table on the GPU against the float64 NumPy reference (tests/bonded_table_ref.py) and
against the analytic angle.Harmonic. The bound is the project's FP64 parity bound (tests/test_gpu_parity.py): 1e-10 of
the largest component of the array, every output finite; the per-particle form is asserted next to it."""

import math

import numpy as np
import pytest

import angle_cases
import azplugins_amd as azp
import bonded_table_ref as R
import dihedral_cases
from test_gpu_parity import TOL, assert_close, assert_per_particle

pytestmark = pytest.mark.gpu

KINDS = ("angle", "dihedral")
CASES = {"angle": angle_cases, "dihedral": dihedral_cases}
EVALUATE = {"angle": R.evaluate_angles, "dihedral": R.evaluate_dihedrals}
ROWS = ("xx", "xy", "xz", "yy", "yz", "zz")


def _tables(kind, widths=(2, 257)):
    """Two types with different widths in one system (the row offsets into the shared tensor): a two-sample table
    -- one interval over the whole domain -- and a smooth, NOT periodic curve on 256 intervals."""
    lo = 0.0 if kind == "angle" else -math.pi
    return [R.sample(kind, widths[0], lambda x: 1.5 - 0.8 * (x - lo), lambda x: 0.8 + 0.3 * (x - lo)),
            R.sample(kind, widths[1], lambda x: 3.0 * math.cos(2.0 * x) + 0.5 * x, lambda x: 6.0 * math.sin(2.0 * x) - 0.5)]


def _sim(kind, tables, xyz, groups, typeid, box, virial=True, forces_first=()):
    types = ["T%d" % t for t in range(len(tables))]
    kw = {kind + "s": groups, kind + "_typeid": typeid, kind + "_types": types}
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(xyz, box, **kw))
    sim.operations.tuners.clear()
    f = getattr(azp, kind).Table()
    for t, p in zip(types, tables):
        f.params[t] = p
    f.compute_virial = virial
    sim.operations.integrator = azp.Integrator(dt=0.0, forces=list(forces_first) + [f], methods=[azp.ConstantVolume()])
    return sim, f


def _check_against(f, out, what):
    print("%s: largest force %.3e, worst deviation %.3e" % (what, np.abs(out["force"]).max(), np.abs(f.forces - out["force"]).max()))
    assert_close(f.forces, out["force"], TOL, what + " forces")
    assert_per_particle(f.forces, out["force"])
    assert_close(f.energies, out["energies"], TOL, what + " energies")
    if f.compute_virial:
        for r, label in enumerate(ROWS):
            assert_close(f.virials[:, r], out["virial"][:, r], TOL, "%s virial %s" % (what, label))


_REFERENCES = {}


def _reference(kind, box):
    """The reference of the parity system of ``kind`` with the two tables, computed once per (kind, box)."""
    if (kind, box) not in _REFERENCES:
        xyz, groups, typeid, L, tilt = CASES[kind].parity_system(box)
        _REFERENCES[kind, box] = EVALUATE[kind](_tables(kind), xyz, groups, typeid, L, tilt)
    return _REFERENCES[kind, box]


# ---------------------------------------------------------------------------------------------------------------------
# one angle, one dihedral
# ---------------------------------------------------------------------------------------------------------------------
def test_angle_edges_collinear_reads_the_last_knot():
    """The edge system of the analytic tests: theta = pi exactly (twice: types 0 and 1), 5e-4 (sin theta under the 1e-3
    floor) and 1e-2. At theta == pi the index is n: the clamp gives the last knot, U = U[-1], and the forces are
    finite (zero: the direction factor vanishes)."""
    xyz, angles, typeid, L = angle_cases.edge_system()
    tables = _tables("angle")
    out = R.evaluate_angles(tables, xyz, angles, typeid, L)
    sim, f = _sim("angle", tables, xyz, angles, typeid, L)
    sim.run(0)
    _check_against(f, out, "angle edges")
    assert np.all(np.isfinite(f.forces)) and not f.forces[:6].any()
    for first, t in ((0, 0), (3, 1)):
        last = tables[t]["U"][-1]
        assert np.abs(f.energies[first:first + 3] - last / 3.0).max() <= TOL * abs(last)
    assert np.abs(f.forces[6:]).max() > 0.1


def test_dihedral_edges_and_both_ends_of_the_cut():
    """phi = 0, phi = pi exactly, pi - 1e-9 and -(pi - 1e-9) on either side of the cut, and phi = 1, with a table that
    is NOT periodic (U[0] != U[-1]): against the reference. Then planar trans with sin phi = -0, an exact construction
    in the plane z = 0 (b1 = (-2, -2, 0), b2 = (-1, -2, 0), b3 = (-2, -2, 0): every term of b1 . n2 is -0): phi = -pi
    reads the FIRST knot, where the construction of the edge system, with sin phi = +0, reads the LAST."""
    xyz, dihedrals, L = dihedral_cases.edge_system()
    table = _tables("dihedral")[1]
    assert abs(table["U"][0] - table["U"][-1]) > 3.0
    out = R.evaluate_dihedrals([table], xyz, dihedrals, np.zeros(5, dtype=np.int64), L)
    assert out["x"][1] == math.pi and out["x"][0] == 0.0
    sim, f = _sim("dihedral", [table], xyz, dihedrals, np.zeros(5, dtype=np.int64), L)
    sim.run(0)
    _check_against(f, out, "dihedral edges")
    mid = R.dihedral_table(table, 0.0)[0]
    assert np.abs(f.energies[0:4] - mid / 4.0).max() <= TOL * abs(mid)                       # phi = 0
    assert np.abs(f.energies[4:8] - table["U"][-1] / 4.0).max() <= TOL * abs(table["U"][-1])   # phi = +pi: the last knot
    assert abs(4.0 * f.energies[8] - table["U"][-1]) < 1e-7 and abs(4.0 * f.energies[12] - table["U"][0]) < 1e-7

    minus = np.array([[0.0, 0.0, 0.0], [-2.0, -2.0, 0.0], [-3.0, -4.0, 0.0], [-5.0, -6.0, 0.0]])
    plus = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 1.0]])
    for what, pos, end in (("sin phi = -0", minus, 0), ("sin phi = +0", plus, -1)):
        sim, f = _sim("dihedral", [table], pos, [(0, 1, 2, 3)], [0], L)
        sim.run(0)
        print("%s: U = %.17g (U[0] = %.17g, U[-1] = %.17g)" % (what, f.energy, table["U"][0], table["U"][-1]))
        assert np.all(np.isfinite(f.forces))
        assert np.abs(f.energies - table["U"][end] / 4.0).max() <= TOL * abs(table["U"][end]), what
        # the forces are those of the torque of that end: the reference's own phi is +pi for both constructions (its
        # dot product starts from +0), so it is given a table whose last knot holds the values of the end in question
        shown = dict(U=table["U"].copy(), tau=table["tau"].copy())
        shown["U"][-1], shown["tau"][-1] = table["U"][end], table["tau"][end]
        want = R.evaluate_dihedrals([shown], pos, [(0, 1, 2, 3)], [0], L)
        assert want["x"][0] == math.pi
        assert_close(f.forces, want["force"], TOL, what + " forces")
        assert np.abs(want["force"]).max() > 0.1


# ---------------------------------------------------------------------------------------------------------------------
# the parity systems: two widths, more groups per particle than BATCH, N above 256 and no multiple of 64, both boxes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("box", ["cubic", "triclinic"])
@pytest.mark.parametrize("kind", KINDS)
def test_parity_system_two_widths_and_virial(kind, box):
    xyz, groups, typeid, L, tilt = CASES[kind].parity_system(box)
    assert xyz.shape[0] > 256 and xyz.shape[0] % 64 != 0
    out = _reference(kind, box)
    sim, f = _sim(kind, _tables(kind), xyz, groups, typeid, azp.Box(L[0], L[1], L[2], *tilt))
    sim.run(0)
    tab = sim.state.group_table(kind)
    assert tab["width"] > 4          # the star / the branched cluster: more entries than the batch, the tail loop runs
    _check_against(f, out, "%s.Table %s" % (kind, box))
    # a bonded potential of angles alone is invariant under scaling: the trace of its virial vanishes
    W = f.virials.sum(axis=0)
    print("virial rows %s, trace %.3e" % (W, W[0] + W[3] + W[5]))
    assert abs(W[0] + W[3] + W[5]) <= 1e-10 * np.abs(W).max() and np.abs(W).max() > 1.0


@pytest.mark.parametrize("kind", KINDS)
def test_type_without_a_table_contributes_nothing(kind):
    """The C ABI: a type whose azp_table_params has n == 0 and d_rows == NULL adds no energy and no force (the Python
    class refuses an unset type before it gets there)."""
    xyz, groups, typeid, L, tilt = CASES[kind].parity_system("cubic")
    tables = _tables(kind)
    sim, f = _sim(kind, tables, xyz, groups, typeid, L)
    sim.run(0)
    f._tables[1].zero_()
    f.compute(0)
    width = len(tables[1]["U"])
    out = EVALUATE[kind]([tables[0], dict(U=np.zeros(width), tau=np.zeros(width))], xyz, groups, typeid, L, tilt)
    _check_against(f, out, kind + ".Table with one empty type")
    g = azp.angle.Table() if kind == "angle" else azp.dihedral.Table()
    g.params["T0"] = tables[0]
    sim.operations.integrator = azp.Integrator(dt=0.0, forces=[g], methods=[azp.ConstantVolume()])
    with pytest.raises(azp.AzpError, match="params\\['T1'\\] is not set"):
        sim.run(0)


def test_exact_against_the_analytic_harmonic_angle():
    """U = k/2 (theta - t0)^2 tabulated on 1024 intervals: tau = -k (theta - t0) is linear in theta, so its
    interpolation is exact and the forces equal angle.Harmonic's within the parity bound. The tabulated energy is the
    chord of a convex function: above the analytic one by at most k h^2 / 8 per angle, h = pi / (width - 1). (The
    tabulated energy is therefore not the integral of the tabulated force in the last digits: no claim of energy
    conservation beyond that bound.)"""
    width = 1025
    h = math.pi / (width - 1)
    params = angle_cases.PARAMS
    tables = [R.sample("angle", width, lambda t, p=p: 0.5 * p["k"] * (t - p["t0"]) ** 2, lambda t, p=p: -p["k"] * (t - p["t0"]))
              for p in params]
    xyz, angles, typeid, L, tilt = angle_cases.parity_system("triclinic")
    box = azp.Box(L[0], L[1], L[2], *tilt)
    ha = azp.angle.Harmonic()
    ha.params["T0"], ha.params["T1"] = params
    ha.compute_virial = True
    sim, f = _sim("angle", tables, xyz, angles, typeid, box, forces_first=[ha])
    sim.run(0)
    print("Table against Harmonic: forces %.3e of %.3e" % (np.abs(f.forces - ha.forces).max(), np.abs(ha.forces).max()))
    assert_close(f.forces, ha.forces, TOL, "forces against angle.Harmonic")
    assert_per_particle(f.forces, ha.forces)
    for r, label in enumerate(ROWS):
        assert_close(f.virials[:, r], ha.virials[:, r], TOL, "virial %s against angle.Harmonic" % label)
    bound = sum(p["k"] * h * h / 8.0 * int((typeid == t).sum()) for t, p in enumerate(params))
    excess = f.energy - ha.energy
    print("energy excess %.6e, bound %.6e" % (excess, bound))
    assert -TOL * ha.energy <= excess <= bound + TOL * ha.energy
    # per particle: a third of the bound of every angle it is in
    per_angle = np.array([params[t]["k"] for t in typeid]) * h * h / 8.0
    share = np.zeros(xyz.shape[0])
    np.add.at(share, angles.reshape(-1), np.repeat(per_angle / 3.0, 3))
    diff = f.energies - ha.energies
    assert np.all(diff >= -TOL * np.abs(ha.energies).max()) and np.all(diff <= share + TOL * np.abs(ha.energies).max())
    # and the reference module says the same of the same tables
    assert_close(f.forces, R.evaluate_angles(tables, xyz, angles, typeid, L, tilt)["force"], TOL, "forces against the reference")


@pytest.mark.parametrize("kind", KINDS)
def test_sorter_reindexes_the_groups(kind):
    xyz, groups, typeid, L, tilt = CASES[kind].parity_system("cubic")
    out = _reference(kind, "cubic")
    sim, f = _sim(kind, _tables(kind), xyz, groups, typeid, L)
    sim.run(0)
    order = azp.ParticleSorter(particles_per_block=16).sort(sim).cpu().numpy()
    assert (order != np.arange(order.size)).sum() > 300      # the sort did move the particles
    f.compute(0)
    tag = sim.state.tag.cpu().numpy().view(np.uint32).astype(np.int64)
    got = dict(force=np.zeros((order.size, 3)), energies=np.zeros(order.size), virial=np.zeros((order.size, 6)))
    got["force"][tag], got["energies"][tag], got["virial"][tag] = f.forces, f.energies, f.virials
    assert_close(got["force"], out["force"], TOL, kind + " after the sort: forces by tag")
    assert_close(got["energies"], out["energies"], TOL, kind + " after the sort: energies by tag")
    assert_close(got["virial"], out["virial"], TOL, kind + " after the sort: virials by tag")


@pytest.mark.parametrize("kind", KINDS)
def test_two_launches_give_the_same_bits(kind):
    xyz, groups, typeid, L, tilt = CASES[kind].parity_system("triclinic")
    sim, f = _sim(kind, _tables(kind), xyz, groups, typeid, azp.Box(L[0], L[1], L[2], *tilt))
    sim.run(0)
    first = (f.force_tensor.clone(), f._virial.clone())
    f.force_tensor.fill_(float("nan"))
    f.compute(0)
    assert (f.force_tensor == first[0]).all() and (f._virial == first[1]).all()
    for bs in (64, 128):
        f.block_size = bs
        f.compute(0)
        assert (f.force_tensor == first[0]).all() and (f._virial == first[1]).all(), bs
