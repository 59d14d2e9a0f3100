"""The outer kernel the bond, angle and dihedral forces share (csrc/bonded_kernel.hpp), pinned on one small topology
for each kind: the batched prologue exactly filled, one and two turns of the tail loop, lanes without entries, partners
in ghost rows. References and bounds are those of the per-kind tests: the oracle for bonds, tests/angle_ref.py and
tests/dihedral_ref.py, 1e-10 of the largest component of the array (tests/test_gpu_parity.py)."""

import math

import numpy as np
import pytest

import angle_cases
import angle_ref
import dihedral_cases
import dihedral_ref
import azplugins_amd as azp
from azplugins_amd import _lib
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

TOL = 1e-10
L, TILT = (9.0, 8.0, 10.0), (0.2, -0.1, 0.15)
# rows: a chain of 12 (0-11), a hub (12) with six arms (13-18), the tail of arm 13 (19), eight particles that belong to
# nothing (20-27) and, as ghost rows, the tails of arms 14-18 (28-32)
CHAIN, HUB, ARMS, FREE = 12, 12, list(range(13, 19)), list(range(20, 28))
N_LOCAL, N_ALL = 28, 33
BATCH = dict(bond=4, angle=3, dihedral=3)   # csrc/*_forces.hip
POTENTIALS = dict(bond=("DoubleWell", "Quartic"), angle=("Harmonic", "CosineSquared"), dihedral=("Periodic", "OPLS"))
PARAMS = {
    "DoubleWell": [dict(r_0=1.0, r_1=1.5, U_1=1.0, U_tilt=0.5), dict(r_0=0.9, r_1=1.3, U_1=2.0, U_tilt=0.0)],
    "Quartic": [dict(k=1434.3, r_0=1.5, b_1=-0.7589, b_2=0.0, U_0=67.2234, sigma=1.0, epsilon=1.0, delta=0.0),
                dict(k=1000.0, r_0=1.6, b_1=-0.5, b_2=0.1, U_0=50.0, sigma=0.9, epsilon=1.2, delta=0.15)],
    "Harmonic": angle_cases.PARAMS, "CosineSquared": angle_cases.PARAMS,
    "Periodic": dihedral_cases.PARAMS["Periodic"], "OPLS": dihedral_cases.PARAMS["OPLS"],
}


def _tail(arm):
    return 19 if arm == 13 else 28 + (arm - 14)


def _positions():
    """Bond lengths in [0.9, 1.1]; the arms leave the hub along +x, +y, +z, -x, -y, -z (jittered), every tail stands 1 rad
    off its arm's axis, so no three members of any group below are collinear. The hub sits in the +x+y+z corner of the
    triclinic box and the chain starts at the -x face: wrapped, the groups straddle the periodic faces."""
    rng = np.random.default_rng(20241018)
    xyz = np.zeros((N_ALL, 3))
    xyz[:CHAIN] = dihedral_cases.random_chain(rng, np.array([-4.2, 0.5, -0.3]), CHAIN)
    xyz[HUB] = (4.3, 3.7, 4.8)
    axes = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]], dtype=np.float64)
    for i, arm in enumerate(ARMS):
        u = axes[i] + 0.1 * rng.normal(size=3)
        u /= np.linalg.norm(u)
        xyz[arm] = xyz[HUB] + rng.uniform(0.9, 1.1) * u
        w = np.cross(u, axes[(i + 1) % 6])
        w /= np.linalg.norm(w)
        xyz[_tail(arm)] = xyz[arm] + rng.uniform(0.9, 1.1) * (math.cos(1.0) * u + math.sin(1.0) * w)
    xyz[FREE] = rng.uniform(-1.0, 1.0, size=(len(FREE), 3)) * 2.0 + np.array([0.0, -2.0, 2.0])
    return dihedral_cases.wrap(xyz, L, TILT)


def _groups(kind):
    """The chain's groups plus a cluster whose hub collects BATCH + 2 table entries; members come in every position."""
    a = ARMS
    if kind == "bond":
        g = [(i, i + 1) for i in range(CHAIN - 1)] + [(HUB, arm) for arm in a[:3]] + [(arm, HUB) for arm in a[3:]]
        g += [(arm, _tail(arm)) for arm in a] + [(a[0], a[1]), (a[2], a[0]), (a[1], a[2]), (a[3], a[1])]
    elif kind == "angle":
        g = angle_ref.chain_angles(0, CHAIN) + [(_tail(arm), arm, HUB) for arm in a[:5]]
        g += [(_tail(a[0]), a[0], a[1]), (a[1], a[0], a[2]), (a[2], a[0], _tail(a[0]))]
    else:
        g = dihedral_ref.chain_dihedrals(0, CHAIN) + [(_tail(a[i]), a[i], HUB, a[i + 1]) for i in range(5)]
    return g, [j % 2 for j in range(len(g))]


def _reference(kind, name, xyz, groups, typeid, oracle):
    """(force (n, 3), energies (n,), virial (n, 6)) of the local rows."""
    if kind == "bond":
        params = np.array([oracle.pack_bond_params(name, p) for p in PARAMS[name]])
        f, bad, v = oracle.bond_forces(name, syn.pos4(xyz), oracle.make_box(L, TILT), np.asarray(groups), np.asarray(typeid, dtype=np.uint32),
                                       params, N=N_LOCAL, virial=True)
        assert bad == 0
        return f[:, :3], f[:, 3], v.T
    ref = angle_ref if kind == "angle" else dihedral_ref
    out = ref.evaluate(name, PARAMS[name], xyz, groups, typeid, L, TILT)
    return out["force"][:N_LOCAL], out["energies"][:N_LOCAL], out["virial"][:N_LOCAL]


def _close(got, want, what):
    """max |got - want| <= 1e-10 max |want|, all finite; prints the figure."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.all(np.isfinite(got)), what
    scale, err = np.abs(want).max(), np.abs(got - want).max()
    print("%s: max deviation %.3e, largest component %.3e" % (what, err, scale))
    assert scale > 0.0 and err <= TOL * scale, "%s: %g > %g" % (what, err, TOL * scale)


@pytest.mark.parametrize("kind", ["bond", "angle", "dihedral"])
def test_outer_loop(kind, oracle):
    import torch

    xyz = _positions()
    groups, typeid = _groups(kind)
    counts = np.bincount(np.asarray(groups).ravel(), minlength=N_ALL)
    B = BATCH[kind]
    # nothing, a batch exactly full, one and two turns of the tail loop -- and no more than two
    assert {0, B, B + 1, B + 2} <= set(counts[:N_LOCAL].tolist()) and counts.max() == counts[HUB] == B + 2
    assert not counts[FREE].any() and counts[N_LOCAL:].sum() >= 4   # partners in ghost rows
    types = ["T0", "T1"]
    snap = azp.Snapshot.from_arrays(xyz, azp.Box(L[0], L[1], L[2], *TILT), **{kind + "s": groups, kind + "_typeid": typeid, kind + "_types": types})
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.state = azp.State(snap, "cuda:0", n_local=N_LOCAL)
    tab = getattr(sim.state, kind + "_table")()
    assert tab["pitch"] == N_LOCAL and tab["width"] == B + 2 and tab["n_%ss" % kind].tolist() == counts[:N_LOCAL].tolist()
    for name in POTENTIALS[kind]:
        f = getattr(getattr(azp, kind), name)()
        for t, p in zip(types, PARAMS[name]):
            f.params[t] = p
        f.compute_virial = True
        f._attach(sim)
        f.compute(0)
        assert f.forces.shape == (N_LOCAL, 3) and f.virials.shape == (N_LOCAL, 6)
        force, energies, virial = _reference(kind, name, xyz, groups, typeid, oracle)
        _close(f.forces, force, name + " forces")
        _close(f.energies, energies, name + " energies")
        for r, label in enumerate(("xx", "xy", "xz", "yy", "yz", "zz")):
            _close(f.virials[:, r], virial[:, r], "%s virial %s" % (name, label))
        # a particle without entries: exact zeros
        assert not f.forces[FREE].any() and not f.energies[FREE].any() and not f.virials[FREE].any()
        # one lane per particle sums its entries in table order whatever the block is: the same bits
        first = (f.force_tensor.clone(), f._virial.clone())
        for bs in (64, 128, 256):
            f.block_size = bs
            f.force_tensor.fill_(float("nan"))
            f._virial.fill_(float("nan"))
            f.compute(0)
            assert _lib.last_launch()["block_size"] == bs
            assert torch.equal(f.force_tensor, first[0]) and torch.equal(f._virial, first[1]), (name, bs)
