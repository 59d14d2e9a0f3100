"""azplugins_amd.special_pair.LJ on the GPU: two-particle known answers, then 300 particles with random special pairs of
two types against a NumPy FP64 evaluation of U = 4 eps [(sigma / r)^12 - (sigma / r)^6] (r < r_cut, no shift) at the
project's FP64 parity bound (tests/test_gpu_parity.py): 1e-10 of the largest component of the array."""

import functools

import numpy as np
import pytest

import azplugins_amd as azp
from azplugins_amd import _lib
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

TOL = 1e-10
PARAMS = (dict(epsilon=1.0, sigma=1.0), dict(epsilon=0.5, sigma=1.2))
R_CUT = (2.5, 1.9)
TYPES = ("s", "t")
N, BOX = 300, 9.0


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    scale = np.abs(want).max()
    err = np.abs(got - want).max()
    print("%s: max deviation %.3e, largest component %.3e" % (what, err, scale))
    assert got.shape == want.shape and np.all(np.isfinite(got)) and err <= TOL * scale, "%s: %g > %g" % (what, err, TOL * scale)


def _sim(xyz, box, pairs, typeid, params=PARAMS, r_cut=R_CUT, types=TYPES, virial=True, extra=()):
    snap = azp.Snapshot.from_arrays(xyz, box, pairs=pairs, pair_typeid=typeid, pair_types=types)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(snap)
    sim.operations.tuners.clear()
    f = azp.special_pair.LJ()
    for t, p, rc in zip(types, params, r_cut):
        if p is not None:
            f.params[t] = p
        if rc is not None:
            f.r_cut[t] = rc
    f.compute_virial = virial
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=[f] + list(extra))
    return sim, f


def _two(d, eps=1.5, sigma=1.1, r_cut=3.0):
    xyz = np.array([[-0.5 * d, 0.0, 0.0], [0.5 * d, 0.0, 0.0]])
    sim, f = _sim(xyz, (20.0, 20.0, 20.0), [(0, 1)], [0], params=(dict(epsilon=eps, sigma=sigma),), r_cut=(r_cut,), types=("s",))
    sim.run(0)
    return f


def test_two_particle_known_answers():
    eps, sigma = 1.5, 1.1
    # U(sigma) = 0, F(sigma) = 24 eps / sigma pushing the two apart
    f = _two(sigma)
    assert abs(f.energy) <= TOL * eps
    _close(f.forces, np.array([[-24.0 * eps / sigma, 0.0, 0.0], [24.0 * eps / sigma, 0.0, 0.0]]), "F(sigma)")
    # the minimum: F = 0, U = -eps, half of it on each member
    f = _two(2.0 ** (1.0 / 6.0) * sigma)
    assert np.abs(f.forces).max() <= TOL * 24.0 * eps / sigma
    _close(f.energies, np.array([-0.5 * eps, -0.5 * eps]), "U(r_min)")
    # just inside the cutoff the unshifted value, at and beyond it exact zeros
    r_cut = 3.0
    f = _two(r_cut * (1.0 - 1e-9))
    u = 4.0 * eps * ((sigma / r_cut) ** 12 - (sigma / r_cut) ** 6)
    assert abs(f.energy - u) <= 1e-7 * abs(u) and f.energy < -1e-3
    for d in (r_cut, r_cut + 0.5, 9.0):
        f = _two(d)
        assert not f.forces.any() and not f.energies.any() and not f.virials.any()
    # across a periodic face: 19 apart in a box of 20 is 1 apart
    f = _two(19.0)
    want = 24.0 * eps * (2.0 * sigma ** 12 - sigma ** 6)
    _close(f.forces, np.array([[want, 0.0, 0.0], [-want, 0.0, 0.0]]), "across the face")


@functools.lru_cache(maxsize=None)
def _system():
    """300 particles on a jittered 7^3 lattice (spacing 9 / 7, no two closer than 0.9) and 420 special pairs of two types
    between lattice neighbors up to two steps apart, some across the periodic faces; particle 0 sits in 9 of them (the
    kernel loads four entries of a lane together and takes the rest in its tail loop), particle 299 in none."""
    tag = np.arange(N, dtype=np.uint64)
    site = np.argsort(syn.u01(11, np.arange(343, dtype=np.uint64), 0))[:N]
    cell = np.stack([site % 7, (site // 7) % 7, site // 49], axis=1)
    a = BOX / 7.0
    xyz = (cell + 0.5) * a - 0.5 * BOX + 0.3 * (np.stack([syn.u01(12, tag, c) for c in range(3)], axis=1) - 0.5)
    d = cell[:, None, :] - cell[None, :, :]
    d -= 7 * np.rint(d / 7.0).astype(np.int64)
    near = (np.abs(d).sum(axis=2) <= 2) & (np.arange(N)[:, None] < np.arange(N)[None, :])
    near[:, N - 1] = False
    cand = np.argwhere(near)
    pick = np.argsort(syn.u01(13, np.arange(len(cand), dtype=np.uint64), 0))
    hub = cand[cand[:, 0] == 0][:9]
    assert len(hub) == 9
    rest = cand[pick]
    rest = rest[rest[:, 0] != 0][:411]
    pairs = np.concatenate([hub, rest])
    flip = np.arange(len(pairs)) % 3 == 1     # both positions in a pair occur
    pairs[flip] = pairs[flip][:, ::-1]
    typeid = (np.arange(len(pairs)) % 2).astype(np.uint32)
    return xyz, pairs, typeid


@functools.lru_cache(maxsize=None)
def _reference():
    """force (N, 3), energies (N,), virial (N, 6) and the total energy, in NumPy FP64, pair by pair."""
    xyz, pairs, typeid = _system()
    force, energy, virial = np.zeros((N, 3)), np.zeros(N), np.zeros((N, 6))
    total = 0.0
    for (i, j), t in zip(pairs, typeid):
        d = xyz[i] - xyz[j]
        d -= BOX * np.rint(d / BOX)
        rsq = float(d @ d)
        if not rsq < R_CUT[t] ** 2:
            continue
        eps, sigma = PARAMS[t]["epsilon"], PARAMS[t]["sigma"]
        s6 = (sigma * sigma / rsq) ** 3
        u = 4.0 * eps * (s6 * s6 - s6)
        f_over_r = 24.0 * eps * (2.0 * s6 * s6 - s6) / rsq
        force[i] += f_over_r * d
        force[j] -= f_over_r * d
        w = 0.5 * f_over_r * np.array([d[0] * d[0], d[0] * d[1], d[0] * d[2], d[1] * d[1], d[1] * d[2], d[2] * d[2]])
        for m in (i, j):
            energy[m] += 0.5 * u
            virial[m] += w
        total += u
    for arr in (force, energy, virial):
        arr.setflags(write=False)
    return force, energy, virial, total


def test_system_is_what_the_tests_need():
    xyz, pairs, typeid = _system()
    count = np.bincount(pairs.reshape(-1), minlength=N)
    assert len(pairs) == 420 and count[0] == 9 and count[N - 1] == 0 and count.max() >= 9
    assert len({tuple(sorted(p)) for p in pairs.tolist()}) == 420
    d = xyz[pairs[:, 0]] - xyz[pairs[:, 1]]
    crossing = np.abs(d).max(axis=1) > 0.5 * BOX
    d -= BOX * np.rint(d / BOX)
    r = np.sqrt((d * d).sum(axis=1))
    beyond = r >= np.array(R_CUT)[typeid]
    print("r in [%.3f, %.3f], %d pairs beyond their cutoff, %d across a face" % (r.min(), r.max(), beyond.sum(), crossing.sum()))
    assert r.min() > 0.85 and beyond.sum() > 20 and (~beyond).sum() > 200 and crossing.sum() > 20


def test_parity_energy_shares_and_virial():
    xyz, pairs, typeid = _system()
    want_f, want_u, want_w, total = _reference()
    sim, f = _sim(xyz, (BOX, BOX, BOX), pairs, typeid)
    sim.run(0)
    tab = sim.state.pair_table()
    assert int(tab["n_pairs"][0]) == 9 and tab["width"] >= 9 and sim.state.n_pairs == 420
    _close(f.forces, want_f, "forces")
    _close(f.energies, want_u, "energies")
    for c, label in enumerate(("xx", "xy", "xz", "yy", "yz", "zz")):
        _close(f.virials[:, c], want_w[:, c], "virial " + label)
    # the shares sum to the total, and the forces to zero
    assert abs(f.energy - total) <= TOL * np.abs(want_u).sum()
    assert np.abs(f.forces.sum(axis=0)).max() <= TOL * np.abs(want_f).max() * 10
    # the virial against -1/2 sum r_ab (x) F_b over the pairs, i.e. per particle 1/2 sum_pairs d (x) F_on_me
    w = f.virials.sum(axis=0)
    want = want_w.sum(axis=0)
    _close(w, want, "total virial")
    assert not f.forces[N - 1].any() and f.energies[N - 1] == 0.0 and not f.virials[N - 1].any()


def test_block_sizes_agree_bit_for_bit():
    xyz, pairs, typeid = _system()
    sim, f = _sim(xyz, (BOX, BOX, BOX), pairs, typeid)
    sim.run(0)
    out = []
    for bs in (0, 64, 128, 256):
        f.block_size = bs
        f._force.fill_(float("nan"))
        f.compute()
        out.append((f.forces.copy(), f.energies.copy(), f.virials.copy()))
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)
    f.block_size = 96
    with pytest.raises(_lib.AzpError):
        f.compute()


def test_unset_parameters_raise():
    xyz, pairs, typeid = _system()
    sim, f = _sim(xyz, (BOX, BOX, BOX), pairs, typeid, params=(PARAMS[0], None))
    with pytest.raises(_lib.AzpError, match=r"params\['t'\] is not set"):
        sim.run(0)
    sim, f = _sim(xyz, (BOX, BOX, BOX), pairs, typeid, r_cut=(None, R_CUT[1]))
    with pytest.raises(_lib.AzpError, match=r"r_cut\['s'\] is not set"):
        sim.run(0)
    with pytest.raises(ValueError):
        f.params["s"] = dict(epsilon=1.0, sigma=-1.0)
    with pytest.raises(ValueError):
        f.r_cut["s"] = float("nan")


def test_thermodynamic_quantities_include_the_special_pairs():
    xyz, pairs, typeid = _system()
    total = _reference()[3]
    sim, f = _sim(xyz, (BOX, BOX, BOX), pairs, typeid)
    thermo = azp.compute.ThermodynamicQuantities(azp.All())
    sim.operations.computes.append(thermo)
    sim.run(0)
    assert abs(thermo.potential_energy - total) <= TOL * np.abs(_reference()[1]).sum()
    want_p = _reference()[2].sum(axis=0)[[0, 3, 5]].sum() / (3.0 * BOX ** 3)   # no velocities: the virial part alone
    assert abs(thermo.pressure - want_p) <= TOL * np.abs(_reference()[2]).sum() / BOX ** 3
