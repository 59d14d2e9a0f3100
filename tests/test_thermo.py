"""compute.ThermodynamicQuantities / ThermodynamicRecorder without a GPU: the host function that turns a row of sums
into the quantities (degrees-of-freedom rules, pressure, temperature), attachment and filter validation, the
recorder's trigger arithmetic and its rejection at ``run``, and the C ABI of ``azp_thermo_*`` (struct size, argument
errors, the scratch size that the kernel's addition-depth argument rests on)."""

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import azplugins_amd as azp
import thermo_ref as ref
from azplugins_amd import _lib, compute, flow

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _row(n=10.0, p=(1.0, -2.0, 0.5), K=(6.0, 0.1, 0.2, 8.0, 0.3, 10.0), W=(1.0, 0.4, 0.5, 2.0, 0.6, 3.0), U=-7.5, ke_rot=2.25,
         rot_dof=20.0):
    return np.array([n, *p, *K, *W, U, ke_rot, rot_dof, 0.0])


def _same(a, b):
    assert a.keys() == b.keys() == set(compute.THERMO_PROPERTIES)
    for k in a:
        assert np.asarray(a[k]).tolist() == pytest.approx(np.asarray(b[k]).tolist(), rel=1e-15, abs=0.0), k


def test_quantities_all_constant_volume():
    q = compute.thermo_quantities(_row(), 10, 50.0, True, False)
    assert q["num_particles"] == 10 and q["volume"] == 50.0
    assert q["translational_degrees_of_freedom"] == 27.0  # 3 N - 3, as Simulation.kinetic_temperature
    assert q["rotational_degrees_of_freedom"] == 0.0 and q["degrees_of_freedom"] == 27.0
    assert q["translational_kinetic_energy"] == 12.0 and q["kinetic_energy"] == 12.0
    assert q["rotational_kinetic_energy"] == 2.25  # (reported even though it does not count)
    assert q["kinetic_temperature"] == 24.0 / 27.0
    assert q["potential_energy"] == -7.5
    want = ((6.0 + 1.0) / 50.0, (0.1 + 0.4) / 50.0, (0.2 + 0.5) / 50.0, (8.0 + 2.0) / 50.0, (0.3 + 0.6) / 50.0, (10.0 + 3.0) / 50.0)
    assert q["pressure_tensor"] == want  # (K_ab + W_ab) / V
    assert q["pressure"] == (want[0] + want[3] + want[5]) / 3.0
    assert q["linear_momentum"] == (1.0, -2.0, 0.5)
    _same(q, ref.quantities(_row(), 10, 50.0, True, False))


def test_quantities_type_group_constant_volume():
    """A group of 10 out of 40 particles loses its share 3 N_g / N of the center-of-mass degrees of freedom."""
    q = compute.thermo_quantities(_row(), 40, 50.0, True, False)
    assert q["translational_degrees_of_freedom"] == 30.0 - 0.75
    assert q["kinetic_temperature"] == 24.0 / 29.25
    _same(q, ref.quantities(_row(), 40, 50.0, True, False))


@pytest.mark.parametrize("n_global", [10, 40])
def test_quantities_flow_method_or_no_method(n_global):
    """flow.Langevin / flow.Brownian (and no method at all) do not conserve the momentum: 3 N_g."""
    q = compute.thermo_quantities(_row(), n_global, 50.0, False, False)
    assert q["translational_degrees_of_freedom"] == 30.0 and q["kinetic_temperature"] == 24.0 / 30.0
    _same(q, ref.quantities(_row(), n_global, 50.0, False, False))


def test_quantities_rotational_on_and_off():
    on = compute.thermo_quantities(_row(), 10, 50.0, True, True)
    assert on["rotational_degrees_of_freedom"] == 20.0 and on["degrees_of_freedom"] == 47.0
    assert on["kinetic_energy"] == 14.25 and on["kinetic_temperature"] == 28.5 / 47.0
    off = compute.thermo_quantities(_row(), 10, 50.0, True, False)
    assert off["rotational_degrees_of_freedom"] == 0.0 and off["kinetic_energy"] == 12.0
    assert off["rotational_kinetic_energy"] == on["rotational_kinetic_energy"] == 2.25
    _same(on, ref.quantities(_row(), 10, 50.0, True, True))


def test_quantities_zero_degrees_of_freedom():
    """An empty group, and a single particle under ConstantVolume (3 - 3 = 0): temperature 0, no division."""
    empty = compute.thermo_quantities(np.zeros(20), 10, 50.0, True, True)
    assert empty["num_particles"] == 0 and empty["degrees_of_freedom"] == 0.0 and empty["kinetic_temperature"] == 0.0
    assert empty["pressure"] == 0.0
    one = compute.thermo_quantities(_row(n=1.0, rot_dof=0.0), 1, 50.0, True, True)
    assert one["degrees_of_freedom"] == 0.0 and one["kinetic_temperature"] == 0.0
    assert compute.thermo_quantities(_row(n=1.0), 1, 50.0, False, False)["kinetic_temperature"] == 24.0 / 3.0


def test_integrator_flags_follow_the_methods():
    """What the properties pass on: ConstantVolume conserves the momentum, the flow methods and an empty method list do
    not; the rotational flag is the integrator's."""
    field = flow.ConstantFlow(velocity=(0.0, 0.0, 0.0))
    cases = [([azp.ConstantVolume()], True), ([], False), (None, False),
             ([flow.Langevin(filter=azp.All(), kT=1.0, flow_field=field)], False),
             ([flow.Brownian(filter=azp.Type("A"), kT=1.0, flow_field=field)], False)]
    for methods, want in cases:
        for rot in (False, True):
            integ = azp.Integrator(dt=0.001, methods=methods, integrate_rotational_dof=rot)
            assert compute._integrator_flags(integ) == (want, rot), methods
    assert compute._integrator_flags(None) == (False, False)


def test_filter_validation():
    assert compute.ThermodynamicQuantities(azp.All()).filter == azp.All()
    assert compute.ThermodynamicQuantities(azp.Type(["A", "B"])).filter == azp.Type(["B", "A"])
    for bad in (None, ["A"], "A", 3):
        with pytest.raises(azp.AzpError):
            compute.ThermodynamicQuantities(bad)
    with pytest.raises(azp.AzpError):
        compute.ThermodynamicRecorder(compute.VelocityCompute(azp.All()), 10)
    with pytest.raises(azp.AzpError):
        compute.ThermodynamicRecorder(compute.ThermodynamicQuantities(azp.All()), 0)


def test_data_access_error_unattached_and_removed():
    thermo = compute.ThermodynamicQuantities(azp.All())
    for name in compute.THERMO_PROPERTIES:
        with pytest.raises(compute.DataAccessError) as e:
            getattr(thermo, name)
        assert e.value.data_name == name
    sim = azp.Simulation(device="cpu")
    sim.operations.computes.append(thermo)  # in the operations, but the simulation has no state
    with pytest.raises(compute.DataAccessError):
        thermo.pressure
    sim.operations.remove(thermo)
    assert thermo._sim is None
    with pytest.raises(compute.DataAccessError):
        thermo.kinetic_temperature
    other = azp.Simulation(device="cpu")
    other.operations.add(thermo)
    with pytest.raises(azp.AzpError):
        sim.operations.add(thermo)  # already in another simulation's operations


def test_recorder_trigger_arithmetic():
    """run(n) from t0 evaluates the trigger at t0 + 1 ... t0 + n."""
    thermo = compute.ThermodynamicQuantities(azp.All())
    rec = compute.ThermodynamicRecorder(thermo, azp.Periodic(7))
    assert rec.timesteps_in_run(0, 21) == [7, 14, 21]
    assert rec.timesteps_in_run(21, 7) == [28]
    assert rec.timesteps_in_run(0, 6) == [] and rec.timesteps_in_run(7, 6) == []  # (t0 itself is not recorded again)
    assert rec.timesteps_in_run(6, 1) == [7]
    assert compute.ThermodynamicRecorder(thermo, 1).timesteps_in_run(5, 3) == [6, 7, 8]
    assert compute.ThermodynamicRecorder(thermo, azp.Periodic(10, phase=3)).timesteps_in_run(0, 25) == [3, 13, 23]
    assert rec.trigger == azp.Periodic(7) and compute.ThermodynamicRecorder(thermo, 5).trigger == azp.Periodic(5)
    assert rec.timesteps.dtype == np.int64 and rec.timesteps.size == 0
    t = rec.table
    assert set(t) == set(compute.THERMO_PROPERTIES) and t["pressure_tensor"].shape == (0, 6) and t["pressure"].shape == (0,)


def test_operations_writers_and_rejection_at_run():
    sim = azp.Simulation(device="cpu")
    thermo = compute.ThermodynamicQuantities(azp.All())
    rec = compute.ThermodynamicRecorder(thermo, 7)
    assert sim.operations.writers == []
    sim.operations.add(rec)
    sim.operations.add(rec)
    assert sim.operations.writers == [rec] and sim.operations.updaters == [] and list(sim.operations.computes) == []
    # the recorder's compute is not in computes of this simulation: rejected before anything else happens
    with pytest.raises(azp.AzpError, match="not in sim.operations.computes"):
        sim.run(1)
    other = azp.Simulation(device="cpu")
    other.operations.add(thermo)
    with pytest.raises(azp.AzpError, match="not in sim.operations.computes"):
        sim.run(1)
    other.operations.remove(thermo)
    sim.operations.add(thermo)
    with pytest.raises(azp.AzpError, match="integrator is not set"):
        sim.run(1)  # (past the writers' check)
    sim.operations.remove(rec)
    assert sim.operations.writers == []
    with pytest.raises(ValueError):
        sim.operations.remove(rec)


def test_more_than_eight_forces_rejected_at_run():
    sim = azp.Simulation(device="cpu")
    forces = [azp.bond.DoubleWell() for _ in range(9)]
    sim.operations.integrator = azp.Integrator(dt=0.001, forces=forces)
    with pytest.raises(azp.AzpError, match="no state"):
        sim.run(0)  # nine forces alone are fine
    sim.operations.add(compute.ThermodynamicQuantities(azp.All()))
    with pytest.raises(azp.AzpError, match="at most 8 forces"):
        sim.run(0)


def test_abi_thermo_struct_and_constants_match_header():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){printf("%zu %zu %zu %zu %d %d\\n", '
           "sizeof(azp_thermo_args), offsetof(azp_thermo_args, d_virial), offsetof(azp_thermo_args, d_out), "
           "offsetof(azp_thermo_args, n_forces), AZP_THERMO_NSUMS, AZP_THERMO_MAX_FORCES);return 0;}")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        size, off_vir, off_out, off_nf, nsums, max_forces = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    A = _lib.ThermoArgs
    assert size == C.sizeof(A)
    assert (off_vir, off_out, off_nf) == (A.d_virial.offset, A.d_out.offset, A.n_forces.offset)
    assert (nsums, max_forces) == (_lib.THERMO_NSUMS, _lib.THERMO_MAX_FORCES) == (20, 8)
    assert ref.NSUMS == nsums


def test_abi_thermo_argument_errors_and_scratch_size():
    """The argument checks run ahead of any device call. The scratch is one 20-double partial row per workgroup: at most
    2048 rows up to N = 2^24, which with at most 32 particles per lane is what keeps the addition depth under 200."""
    lib = _lib.lib()
    need = C.c_uint64(0)
    vel = (C.c_double * 4)()  # (only its address is looked at)
    fake = C.addressof(vel)

    def args(**kw):
        a = _lib.ThermoArgs()
        a.d_vel = fake
        a.N = 1
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert lib.azp_thermo_scratch_size(C.byref(args()), C.byref(need)) == 0 and need.value == 160
    for n, rows in ((256, 1), (257, 2), (2**19, 2048), (2**19 + 1, 1025), (2**20, 2048), (2**24, 2048), (10007, 40)):
        assert lib.azp_thermo_scratch_size(C.byref(args(N=n)), C.byref(need)) == 0
        assert need.value == rows * 160, n
    a = args(n_forces=9)
    assert lib.azp_thermo_scratch_size(C.byref(a), C.byref(need)) == -1 and lib.azp_thermo_sums(C.byref(a), None) == -1
    a = args(d_vel=None)
    assert lib.azp_thermo_scratch_size(C.byref(a), C.byref(need)) == -1 and lib.azp_thermo_sums(C.byref(a), None) == -1
    for some in (("d_orientation",), ("d_angmom", "d_inertia"), ("d_orientation", "d_inertia")):
        a = args(**{k: fake for k in some})
        assert lib.azp_thermo_sums(C.byref(a), None) == -1, some
    assert lib.azp_thermo_sums(C.byref(args(d_type_mask=fake)), None) == -1  # a mask needs d_pos for the types
    assert lib.azp_thermo_sums(C.byref(args(n_forces=1)), None) == -1  # a listed force array is NULL
    assert lib.azp_thermo_sums(C.byref(args()), None) == -1  # no d_out
    assert lib.azp_thermo_scratch_size(C.byref(args()), None) == -1


def test_reference_terms_and_exact_sums():
    """The test oracle itself: terms of a two-particle system by hand, and fsum against a sum that cancels."""
    vel = np.array([[1.0, 2.0, 3.0, 2.0], [-1.0, 0.5, 0.0, 4.0]])
    f = np.array([[0.0, 0.0, 0.0, 1.5], [0.0, 0.0, 0.0, -0.5]])
    w = np.arange(12.0).reshape(6, 2)
    t = ref.terms(vel, [True, True], [f, f], [w, None], orientation=np.array([[1.0, 0, 0, 0], [1.0, 0, 0, 0]]),
                  angmom=np.array([[0.0, 2.0, 0.0, 4.0], [0.0, 1.0, 1.0, 1.0]]), inertia=np.array([[1.0, 0.0, 2.0], [0.0, 0.0, 0.0]]))
    s, mag = ref.exact(t)
    assert s[0] == 2 and s[1:4].tolist() == [-2.0, 6.0, 6.0]
    assert s[4:10].tolist() == [2 + 4, 4 - 2, 6 + 0, 8 + 1, 12 + 0, 18 + 0]
    assert s[10:16].tolist() == [1.0, 5.0, 9.0, 13.0, 17.0, 21.0] and s[16] == 2.0 and mag[16] == 4.0
    assert s[17] == 0.5 * (1.0 / 1.0) + 0.5 * (4.0 / 2.0) and s[18] == 2 and s[19] == 0
    only_b = ref.exact(ref.terms(vel, [False, True], [f], [w]))[0]
    assert only_b[0] == 1 and only_b[16] == -0.5 and only_b[10] == 1.0 and only_b[17] == 0
    big = np.array([1e16, 1.0, -1e16, 1.0])
    assert ref.exact([big])[0][0] == 2.0 and float(np.sum(big)) != 2.0
