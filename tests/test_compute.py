"""azplugins_amd.compute without a GPU: the numpy reference (tests/velocity_field_ref.py) against the reference's
known answers (tests/golden/compute_cases.json), bin-center coordinates and compact shapes, input validation,
attachment through sim.operations, the Type filter's mask and the ABI struct size."""

import ctypes as C
import itertools
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import azplugins_amd as azp
import velocity_field_ref as ref
from azplugins_amd import _lib
from azplugins_amd.compute import (CartesianVelocityFieldCompute, CylindricalVelocityFieldCompute, DataAccessError,
                                   VelocityCompute)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    with open(os.path.join(ROOT, "tests", "golden", "compute_cases.json")) as f:
        return json.load(f)


def _check(got, want, step):
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    if step.get("exact"):
        np.testing.assert_equal(got, want)
    else:
        np.testing.assert_allclose(got, want, atol=step.get("atol", 0.0))


def test_reference_velocity_compute(cases):
    c = cases["velocity_compute"]
    typeid = np.asarray(c["typeid"])
    for chk in c["checks"]:
        include = None if chk["filter"] == "All" else np.isin(np.asarray(c["types"])[typeid], chk["filter"])
        v = ref.velocities(c["position"], c["velocity"], c["mass"], (0, 0, 0), L=[c["L"]] * 3, include=include)
        np.testing.assert_allclose(v.reshape(3), chk["velocity"])


@pytest.mark.parametrize("name", ["cartesian_basic", "cylindrical_basic"])
def test_reference_basic(cases, name):
    c = cases[name]
    num_bins, lower, upper = None, None, None
    for step in c["steps"]:
        num_bins = step.get("num_bins", num_bins)
        lower = step.get("lower", lower)
        upper = step.get("upper", upper)
        v = ref.velocities(c["position"], c["velocity"], c["mass"], num_bins, lower, upper, cylindrical=c["cls"] == "Cylindrical",
                           L=[c["L"]] * 3)
        _check(v.reshape(ref.compact_shape(num_bins)), step["velocities"], step)


def test_reference_no_particles(cases):
    for c in cases["no_particles"]:
        snap = cases[c["snapshot"]]
        v = ref.velocities(snap["position"], snap["velocity"], snap["mass"], c["num_bins"], c["lower"], c["upper"],
                           cylindrical=True, L=[snap["L"]] * 3, include=np.zeros(2, dtype=bool))
        np.testing.assert_equal(v.reshape(ref.compact_shape(c["num_bins"])), c["velocities"])


def _field_class(name):
    return CartesianVelocityFieldCompute if name == "Cartesian" else CylindricalVelocityFieldCompute


def test_coordinates_and_shapes_golden(cases):
    for c in cases["binning_shape"]:
        f = _field_class(c["cls"])(num_bins=[2, 3, 4], lower_bounds=c["lower"], upper_bounds=c["upper"])
        for step in c["steps"]:
            f.num_bins = step["num_bins"]
            assert f._compact_shape + [3] == step["velocities_shape"]
            coords = f.coordinates
            if step["coordinates"] is None:
                assert coords is None
            else:
                assert list(coords.shape) == step["coordinates_shape"]
                np.testing.assert_allclose(coords, step["coordinates"])


def test_coordinates_every_combination():
    lo, hi = (-1.0, 0.5, 2.0), (3.0, 1.5, 7.0)
    for nb in itertools.product([0, 1, 3], [0, 2], [0, 5]):
        f = CartesianVelocityFieldCompute(num_bins=nb, lower_bounds=lo, upper_bounds=hi)
        binned = [d for d in range(3) if nb[d] > 0]
        coords = f.coordinates
        if not binned:
            assert coords is None
            continue
        centers = [lo[d] + (np.arange(nb[d]) + 0.5) * (hi[d] - lo[d]) / nb[d] for d in binned]
        if len(binned) == 1:
            assert coords.shape == (nb[binned[0]],)
            np.testing.assert_allclose(coords, centers[0])
        else:
            assert coords.shape == tuple(nb[d] for d in binned) + (len(binned),)
            for k, idx in enumerate(itertools.product(*[range(nb[d]) for d in binned])):
                np.testing.assert_allclose(coords[idx], [centers[j][i] for j, i in enumerate(idx)])
        assert tuple(f._compact_shape) + (3,) == ref.compact_shape(nb)


def test_reference_edges_and_ravel():
    # particles exactly on bin edges land in the bin that starts there; the upper bound itself is outside
    L = (10.0, 10.0, 10.0)
    pos = [[-2.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [-3.0, 0.0, 0.0]]
    s, _ = ref.sums(pos, np.ones((5, 3)), np.ones(5), (4, 0, 0), (-2, 0, 0), (2, 0, 0), L=L)
    np.testing.assert_equal(s[:, 0], [1, 1, 1, 0])
    # ravel z + nz (y + ny x)
    s, _ = ref.sums([[0.5, 1.5, 2.5]], [[1, 1, 1]], [2.0], (2, 3, 4), (0, 0, 0), (2, 3, 4), L=L)
    assert s[2 + 4 * (1 + 3 * 0), 0] == 2.0 and s[:, 0].sum() == 2.0
    # wrapping: one box length outside
    s, _ = ref.sums([[11.0, 0.0, 0.0]], [[1, 0, 0]], [1.0], (10, 0, 0), (-5, 0, 0), (5, 0, 0), L=L)
    assert s[6, 0] == 1.0


def test_validation():
    with pytest.raises(azp.AzpError):
        CartesianVelocityFieldCompute(num_bins=(-1, 0, 0), lower_bounds=(0, 0, 0), upper_bounds=(1, 1, 1))
    with pytest.raises(azp.AzpError):
        CartesianVelocityFieldCompute(num_bins=(2, 0, 0), lower_bounds=(1, 0, 0), upper_bounds=(1, 1, 1))
    with pytest.raises(azp.AzpError):
        CylindricalVelocityFieldCompute(num_bins=(2, 0, 0), lower_bounds=(1, 0, 0), upper_bounds=(0.5, 1, 1))
    # a dimension that is not binned ignores its bounds
    CartesianVelocityFieldCompute(num_bins=(2, 0, 0), lower_bounds=(0, 5, 5), upper_bounds=(1, 1, 1))
    with pytest.raises(azp.AzpError):
        CartesianVelocityFieldCompute(num_bins=(2**16, 2**16, 1), lower_bounds=(0, 0, 0), upper_bounds=(1, 1, 1))
    with pytest.raises(azp.AzpError):
        CartesianVelocityFieldCompute(num_bins=(2**15, 2**16, 0), lower_bounds=(0, 0, 0), upper_bounds=(1, 1, 1))  # 2^31
    f = CartesianVelocityFieldCompute(num_bins=(2**15, 2**16 - 1, 0), lower_bounds=(0, 0, 0), upper_bounds=(1, 1, 1))
    assert f.num_bins == (2**15, 2**16 - 1, 0)
    with pytest.raises(azp.AzpError):
        f.num_bins = (2**16, 2**15, 1)
    with pytest.raises(azp.AzpError):
        f.num_bins = (1, -2, 0)
    for cls in (VelocityCompute,):
        with pytest.raises(azp.AzpError, match="MPCD"):
            cls(filter=azp.All(), include_mpcd_particles=True)
    with pytest.raises(azp.AzpError, match="MPCD"):
        CylindricalVelocityFieldCompute(num_bins=(1, 1, 1), lower_bounds=(0, 0, 0), upper_bounds=(1, 1, 1),
                                        include_mpcd_particles=True)
    with pytest.raises(azp.AzpError):
        VelocityCompute(filter="A")


def test_data_access_and_operations():
    v = VelocityCompute()
    assert v.filter is None and v.include_mpcd_particles is False
    f = CartesianVelocityFieldCompute(num_bins=[2, 0, 1], lower_bounds=(-10, -10, -10), upper_bounds=(10, 10, 10))
    np.testing.assert_equal(f.num_bins, (2, 0, 1))
    for obj, name in ((v, "velocity"), (f, "velocities")):
        with pytest.raises(DataAccessError):
            getattr(obj, name)
    assert issubclass(DataAccessError, azp.AzpError)
    sim = azp.Simulation(device="cuda:0", seed=1)
    assert len(sim.operations.computes) == 0
    sim.operations.add(v)
    sim.operations.computes.extend([f])
    assert list(sim.operations.computes) == [v, f]
    assert v._sim is sim and f._sim is sim
    # no state yet: not attached
    with pytest.raises(DataAccessError):
        v.velocity
    sim.operations.add(v)  # adding twice keeps one entry
    assert len(sim.operations.computes) == 2
    sim2 = azp.Simulation(device="cuda:0", seed=1)
    with pytest.raises(azp.AzpError):
        sim2.operations.add(v)
    with pytest.raises(azp.AzpError):
        sim.operations.add(azp.All())
    sim.operations.remove(v)
    assert list(sim.operations.computes) == [f]
    assert v._sim is None
    with pytest.raises(ValueError):
        sim.operations.remove(v)
    sim2.operations.add(v)
    assert v._sim is sim2
    # integrator and tuners are untouched
    assert sim.operations.integrator is None
    assert len(sim.operations.tuners) == 1


def test_type_filter_mask():
    t = azp.Type("B")
    assert t.types == ("B",)
    np.testing.assert_equal(t.mask(["A", "B", "C"]), [0, 1, 0])
    t = azp.Type(["A", "C"])
    m = t.mask(["A", "B", "C"])
    assert m.dtype == np.uint8
    np.testing.assert_equal(m, [1, 0, 1])
    assert azp.Type(("C", "A")) == t and hash(azp.Type(("C", "A"))) == hash(t)
    with pytest.raises(azp.AzpError):
        t.mask(["A", "B"])
    with pytest.raises(azp.AzpError):
        azp.Type([1, 2])
    # integrators keep accepting All only
    with pytest.raises(azp.AzpError):
        azp.ConstantVolume(filter=azp.Type("A"))


def test_abi_velocity_field_struct_size():
    names = ["azp_velocity_field_args", "azp_box"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){' + "".join(
        'printf("%%zu\\n", sizeof(%s));' % n for n in names) + \
        'printf("%zu\\n", offsetof(azp_velocity_field_args, d_type_mask));' + \
        'printf("%zu\\n", offsetof(azp_velocity_field_args, scratch_bytes));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == C.sizeof(_lib.VelocityFieldArgs)
    assert got[1] == C.sizeof(_lib.Box)
    assert got[2] == _lib.VelocityFieldArgs.d_type_mask.offset
    assert got[3] == _lib.VelocityFieldArgs.scratch_bytes.offset


def test_scratch_size_query():
    lib = _lib.lib()
    a = _lib.VelocityFieldArgs()
    a.N = 2**20
    out = C.c_uint64(0)
    _lib.check(lib.azp_velocity_field_scratch_size(C.byref(a), C.byref(out)))
    assert out.value > 0 and out.value % 32 == 0
    a.num_bins[0], a.num_bins[1] = 100, 100
    a.upper[0] = a.upper[1] = 1.0
    _lib.check(lib.azp_velocity_field_scratch_size(C.byref(a), C.byref(out)))
    assert out.value % (10**4 * 32) == 0 and out.value <= max(64 << 20, 10**4 * 32)
    a.num_bins[0], a.num_bins[1], a.num_bins[2] = 2**16, 2**15, 1
    a.upper[2] = 1.0
    assert lib.azp_velocity_field_scratch_size(C.byref(a), C.byref(out)) == -4  # AZP_ERROR_TOO_MANY_BINS
    a.num_bins[0], a.num_bins[1] = 4, 0
    a.upper[0] = a.lower[0]
    assert lib.azp_velocity_field_scratch_size(C.byref(a), C.byref(out)) == -1
