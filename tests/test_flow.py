"""azplugins_amd.flow without a GPU: the reference's flow-field sequences (src/pytest/test_flow.py), the
``_azplugins`` flow objects against their formulas, parameter and filter validation, the driver's rejections, the
C ABI struct layout, and the numpy random stream (tests/flow_ref.py) against the oracle's Philox and DPD draws."""

import ctypes as C
import os
import pickle
import subprocess
import tempfile

import numpy as np
import pytest

import flow_ref as ref
from azplugins_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pickling_check(obj):
    """hoomd.conftest.pickling_check restated: a pickle round trip gives an equal object."""
    other = pickle.loads(pickle.dumps(obj))
    assert other == obj
    assert type(other) is type(obj)


def test_constant_flow_field():
    from azplugins_amd import flow

    U = flow.ConstantFlow(velocity=(1, 0, 0))
    np.testing.assert_array_almost_equal(U.velocity, (1, 0, 0))
    pickling_check(U)
    U.velocity = (1, 2, 3)
    np.testing.assert_array_almost_equal(U.velocity, (1, 2, 3))
    pickling_check(U)
    np.testing.assert_array_almost_equal(U._cpp().velocity, (1, 2, 3))
    pickling_check(U)


def test_parabolic_flow_field():
    from azplugins_amd import flow

    U = flow.ParabolicFlow(mean_velocity=4, separation=10)
    assert U.mean_velocity == 4
    assert U.separation == 10
    pickling_check(U)
    U.mean_velocity = 10
    U.separation = 20
    np.testing.assert_array_almost_equal((U.mean_velocity, U.separation), (10, 20))
    pickling_check(U)
    cpp = U._cpp()
    np.testing.assert_array_almost_equal((cpp.mean_velocity, cpp.separation), (10, 20))
    pickling_check(U)


def test_flow_field_validation():
    from azplugins_amd import flow

    for bad in ((np.nan, 0, 0), (0, np.inf, 0), (1, 2)):
        with pytest.raises(_lib.AzpError):
            flow.ConstantFlow(velocity=bad)
    for sep in (0.0, -1.0, np.nan):
        with pytest.raises(_lib.AzpError):
            flow.ParabolicFlow(mean_velocity=1.0, separation=sep)
    with pytest.raises(_lib.AzpError):
        flow.ParabolicFlow(mean_velocity=np.inf, separation=1.0)
    p = flow.ParabolicFlow(mean_velocity=1.0, separation=1.0)
    with pytest.raises(_lib.AzpError):
        p.separation = 0.0
    assert p.separation == 1.0


def test_cpp_flow_objects_against_formulas():
    m = _lib.ext_module()
    rng = np.random.default_rng(7)
    c = m.ConstantFlow((0.5, -1.25, 3.0))
    assert c.velocity == (0.5, -1.25, 3.0)
    for r in rng.uniform(-5, 5, (10, 3)):
        assert c(tuple(r)) == (0.5, -1.25, 3.0)
    c.velocity = (1.0, 2.0, 3.0)
    assert c((0.0, 0.0, 0.0)) == (1.0, 2.0, 3.0)
    for U, sep in ((4.0, 10.0), (-0.3, 2.5), (1.0, 1e-3)):
        p = m.ParabolicFlow(U, sep)
        # src/ParabolicFlow.h stores Umax = 1.5 U and L = separation / 2
        assert p.Umax == 1.5 * U and p.L == 0.5 * sep
        assert p.mean_velocity == pytest.approx(U, rel=1e-15) and p.separation == sep
        for r in rng.uniform(-sep, sep, (10, 3)):
            yr = r[1] / (0.5 * sep)
            assert p(tuple(r)) == (1.5 * U * (1.0 - yr * yr), 0.0, 0.0)
            got = ref.flow_velocity(("parabolic", U, sep), r[None, :])[0]
            assert tuple(got) == p(tuple(r))
        assert p((0.0, 0.5 * sep, 0.0))[0] == 0.0 and p((0.0, 0.0, 0.0))[0] == 1.5 * U


def test_flow_struct_matches_cpp_object():
    from azplugins_amd import flow

    f = flow.ParabolicFlow(mean_velocity=2.0, separation=3.0)._c()
    assert f.kind == _lib.FLOW_PARABOLIC and tuple(f.p) == (3.0, 1.5, 0.0)
    f = flow.ConstantFlow(velocity=(1.0, -2.0, 0.5))._c()
    assert f.kind == _lib.FLOW_CONSTANT and tuple(f.p) == (1.0, -2.0, 0.5)


def test_method_parameters():
    from azplugins_amd import All, Type, flow

    u = flow.ConstantFlow(velocity=(1, 0, 0))
    lan = flow.Langevin(filter=All(), kT=1.5, flow_field=u, default_gamma=0.0)
    assert lan.gamma["A"] == 0.0 and not lan.noiseless
    lan.gamma["A"] = 2.0
    lan.gamma[("B", "C")] = 3.0
    assert lan.gamma["A"] == 2.0 and lan.gamma["C"] == 3.0 and lan.gamma["D"] == 0.0
    np.testing.assert_array_equal(lan.gamma.table(["A", "B", "D"]), [2.0, 3.0, 0.0])
    with pytest.raises(_lib.AzpError):
        lan.gamma["A"] = -1.0
    with pytest.raises(_lib.AzpError):
        lan.gamma["A"] = np.nan
    assert lan.gamma["A"] == 2.0
    with pytest.raises(_lib.AzpError):
        flow.Langevin(filter=All(), kT=1.0, flow_field=u, default_gamma=-0.5)
    bro = flow.Brownian(filter=Type("A"), kT=lambda t: 1.0 + t, flow_field=u, default_gamma=2.0, noiseless=True)
    assert bro.noiseless and bro._kT(3) == 4.0
    for g in (0.0, -1.0, np.inf):
        with pytest.raises(_lib.AzpError):
            bro.gamma["A"] = g
        with pytest.raises(_lib.AzpError):
            flow.Brownian(filter=All(), kT=1.0, flow_field=u, default_gamma=g)
    for bad_kT in (-1.0, np.nan):
        with pytest.raises(_lib.AzpError):
            flow.Langevin(filter=All(), kT=bad_kT, flow_field=u)
    with pytest.raises(_lib.AzpError):
        flow.Langevin(filter="all", kT=1.0, flow_field=u)
    with pytest.raises(_lib.AzpError):
        flow.Langevin(filter=All(), kT=1.0, flow_field=(1, 0, 0))


class _FakeState:
    types = ["A", "B", "C"]


def _sim_with(methods, rot=False, domain=None):
    import azplugins_amd as azp

    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.state = _FakeState()
    sim.domain = domain
    integ = azp.Integrator(dt=0.005, methods=methods, integrate_rotational_dof=rot)
    return sim, integ


def test_driver_rejections():
    from azplugins_amd import All, ConstantVolume, Type, flow

    u = flow.ConstantFlow(velocity=(1, 0, 0))

    def lan(f):
        return flow.Langevin(filter=f, kT=1.0, flow_field=u)

    def bro(f):
        return flow.Brownian(filter=f, kT=1.0, flow_field=u)

    ok = [[lan(All())], [bro(All())], [lan(Type("A")), bro(Type(["B", "C"]))], [lan(Type("A")), lan(Type("B"))]]
    for methods in ok:
        sim, integ = _sim_with(methods)
        assert sim._check_flow_methods(integ) == methods
    bad = [
        ([lan(All()), ConstantVolume()], {}),                # mixed with NVE
        ([ConstantVolume(), bro(Type("A"))], {}),
        ([lan(Type(["A", "B"])), bro(Type("B"))], {}),       # overlapping filters
        ([lan(All()), bro(Type("A"))], {}),                  # All() not alone
        ([lan(Type("A")), lan(All())], {}),
        ([lan(Type("Z"))], {}),                              # a type the state does not have
        ([lan(All())], dict(rot=True)),                      # rotational degrees of freedom
        ([bro(All())], dict(domain=object())),               # decomposed run
    ]
    for methods, kw in bad:
        sim, integ = _sim_with(methods, **kw)
        with pytest.raises(_lib.AzpError):
            sim._check_flow_methods(integ)
    m = lan(All())
    sim, integ = _sim_with([m, m])
    with pytest.raises(_lib.AzpError):
        sim._check_flow_methods(integ)
    # without flow methods nothing changes
    sim, integ = _sim_with([ConstantVolume()])
    assert sim._check_flow_methods(integ) == []


def test_abi_flow_struct_layout():
    names = ["azp_flow_method_args", "azp_flow", "azp_box"]
    fields = ["d_type_mask", "box", "dt", "kT", "timestep", "seed", "noiseless", "N", "ntypes", "flow", "block_size"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){' + "".join(
        'printf("%%zu\\n", sizeof(%s));' % n for n in names) + "".join(
        'printf("%%zu\\n", offsetof(azp_flow_method_args, %s));' % f for f in fields) + \
        'printf("%zu\\n", offsetof(azp_flow, p));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == C.sizeof(_lib.FlowMethodArgs)
    assert got[1] == C.sizeof(_lib.Flow)
    assert got[2] == C.sizeof(_lib.Box)
    for k, f in enumerate(fields):
        assert got[3 + k] == getattr(_lib.FlowMethodArgs, f).offset, f
    assert got[-1] == _lib.Flow.p.offset


def test_abi_flow_symbols_exported():
    lib = _lib.lib()
    for name in ("azp_integrate_langevin_flow_step_one", "azp_integrate_langevin_flow_step_two",
                 "azp_integrate_langevin_flow_step_two_one", "azp_integrate_brownian_flow_step"):
        assert hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn(None, None) == -1  # AZP_ERROR_INVALID_ARGUMENT, no launch
        a = _lib.FlowMethodArgs()
        assert fn(C.byref(a), None) == 0  # N = 0: nothing to do
        a.N, a.ntypes, a.dt = 4, 1, 0.005
        assert fn(C.byref(a), None) == -1  # no arrays
    assert lib.azp_version() == 2 and _lib.ext_module().azp_version == 2


def test_numpy_philox_matches_oracle(oracle):
    import oracle as o

    rng = np.random.default_rng(11)
    for _ in range(20):
        ctr = rng.integers(0, 2**32, 4, dtype=np.uint64).astype(np.uint32)
        key = rng.integers(0, 2**32, 2, dtype=np.uint64).astype(np.uint32)
        want = np.asarray(o.philox4x32_10(ctr, key), dtype=np.uint32)
        got = np.array([int(x) for x in ref.philox4x32_10(*ctr, *key)], dtype=np.uint32)
        np.testing.assert_array_equal(got, want)
    # vectorised: many counters at once equal the one-at-a-time results
    tags = np.arange(0, 4096 * 977, 977, dtype=np.uint32)
    vec = ref.philox4x32_10(1, tags, 0, 0, np.uint32(0xCA000001), np.uint32(12345))
    for i in (0, 1, 2000, 4095):
        want = np.asarray(o.philox4x32_10(np.array([1, tags[i], 0, 0], dtype=np.uint32),
                                          np.array([0xCA000001, 12345], dtype=np.uint32)), dtype=np.uint32)
        np.testing.assert_array_equal([vec[k][i] for k in range(4)], want)


def test_numpy_stream_reproduces_dpd_draws(oracle):
    """With id = 200 and the counter {0, min tag, max tag, 0} the stream construction is the DPD thermostat's."""
    import oracle as o

    rng = np.random.default_rng(12)
    for seed, ti, tj, ts in zip(rng.integers(0, 2**16, 30), rng.integers(0, 2**20, 30), rng.integers(0, 2**20, 30),
                                rng.integers(0, 2**32, 30)):
        seed, ti, tj, ts = int(seed), int(ti), int(tj), int(ts)
        k0, k1 = ref.key(ref.DPD_ID, seed, ts)
        r = ref.philox4x32_10(0, min(ti, tj), max(ti, tj), 0, k0, k1)
        alpha = -1.0 + 2.0 * ref.u01(np.atleast_1d(r[0]), np.atleast_1d(r[1]))[0]
        assert alpha == o.dpd_alpha(seed, ti, tj, ts)


def test_stream_key_layout():
    assert ref.key(202, 0x1234, 5) == (np.uint32((202 << 24) | 0x1234), np.uint32(5))
    t = (0xAB << 32) | 0xDEADBEEF
    assert ref.key(201, 0x12345, t) == (np.uint32((201 << 24) | (0xAB << 16) | 0x2345), np.uint32(0xDEADBEEF))
    # u01 lies in (0, 1]: the largest draw rounds to 1 (the DPD thermostat's alpha lies in (-1, 1] for the same reason)
    lo = ref.u01(np.array([0], dtype=np.uint32), np.array([0], dtype=np.uint32))[0]
    hi = ref.u01(np.array([0xFFFFFFFF], dtype=np.uint32), np.array([0xFFFFFFFF], dtype=np.uint32))[0]
    assert 0.0 < lo < 1e-15 and hi == 1.0
