"""The step loop of ``Simulation.run`` on the GPU: a run in one piece and the same run in two pieces end in the same
bits on every integration path, with a recorder splitting the fusion every 3 steps, a type updater every 4 and a sort
every 5 (the CPU side, tests/test_step_loop.py, pins the order of the launches; this pins what they compute)."""

import numpy as np
import pytest
import torch

from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

PATHS = ["nve", "bussi", "fire", "langevin"]


def _sim(path):
    """300 particles (a 256-lane workgroup and a ragged one) in DoubleWell chains of 5 behind a planar harmonic barrier:
    two forces, so the net force is summed."""
    import azplugins_amd as azp
    from azplugins_amd import compute, flow, minimize, thermostats
    from azplugins_amd.update import TypeUpdater

    cfg = syn.config_chains(10, 6, 5, 5)
    n = cfg["xyz"].shape[0]
    assert n == 300
    tag = np.arange(n, dtype=np.uint64)
    vel = np.stack([syn.normal(17, tag, c) for c in range(3)], axis=1)
    snap = azp.Snapshot.from_arrays(cfg["xyz"], cfg["L"], typeid=np.arange(n) % 2, types=("A", "B"), bonds=cfg["bonds"],
                                    velocity=vel - vel.mean(axis=0))
    snap.particles.mass[:] = 0.5 + 1.5 * syn.u01(18, tag, 0)
    sim = azp.Simulation(device="cuda:0", seed=5)
    sim.create_state_from_snapshot(snap)
    dw = azp.bond.DoubleWell()
    dw.params["A-A"] = cfg["bond_params"]
    wall = azp.external.PlanarHarmonicBarrier(location=lambda t: 1.5 - 0.01 * t)
    wall.params["A"] = dict(k=50.0, offset=0.0)
    wall.params["B"] = dict(k=20.0, offset=0.25)
    forces, dt = [dw, wall], 0.002
    if path == "fire":
        integ = minimize.FIRE(dt=dt, force_tol=1e-3, angmom_tol=1e-3, energy_tol=1e-7, forces=forces, methods=[azp.ConstantVolume()])
    else:
        method = {"nve": lambda: azp.ConstantVolume(),
                  "bussi": lambda: azp.ConstantVolume(thermostat=thermostats.Bussi(kT=lambda t: 1.0 + 0.01 * t, tau=0.1)),
                  "langevin": lambda: flow.Langevin(filter=azp.All(), kT=1.2, flow_field=flow.ConstantFlow((0.5, 0.0, 0.0)),
                                                    default_gamma=2.0)}[path]()
        integ = azp.Integrator(dt=dt, forces=forces, methods=[method])
    sim.operations.integrator = integ
    sim.operations.tuners[0].trigger_period = 5
    thermo = compute.ThermodynamicQuantities(azp.All())
    rec = compute.ThermodynamicRecorder(thermo, 3)
    for op in (thermo, rec, TypeUpdater(trigger=4, inside_type="B", outside_type="A", lo=-1.0, hi=1.0)):
        sim.operations.add(op)
    return sim, rec


def _by_tag(sim):
    torch.cuda.synchronize()
    st = sim.state
    order = torch.argsort(st.tag[: st.N])
    return {name: getattr(st, name)[: st.N].index_select(0, order).cpu() for name in ("pos", "vel", "image")}


@pytest.mark.parametrize("path", PATHS)
def test_one_run_and_two_runs_end_in_the_same_bits(path):
    ends, tables, sorts = [], [], []
    for pieces in ((12,), (5, 7)):
        sim, rec = _sim(path)
        for steps in pieces:
            sim.run(steps)
        assert sim.timestep == 12
        ends.append(_by_tag(sim))
        tables.append(rec.table)
        sorts.append(sim.operations.tuners[0].num_sorts)
        assert rec.timesteps.tolist() == [3, 6, 9, 12]
    start = _by_tag(_sim(path)[0])
    assert not torch.equal(ends[0]["pos"], start["pos"]) and not torch.equal(ends[0]["vel"], start["vel"])  # (it moved)
    assert sorts == [2, 2]
    for name in ("pos", "vel", "image"):
        assert torch.equal(ends[0][name], ends[1][name]), "%s: %s differs between run(12) and run(5) + run(7)" % (path, name)
    assert tables[0].keys() == tables[1].keys()
    for name in tables[0]:
        np.testing.assert_array_equal(tables[0][name], tables[1][name], err_msg="%s: recorded %s" % (path, name))
    assert np.all(np.isfinite(tables[0]["kinetic_energy"]))
