"""azplugins_amd.update / .evaporate / .variant without a GPU: the C ABI, parameter validation, triggers, the routing
of ``sim.operations.add`` / ``remove``, ``SphereArea`` against its closed form, and the selection rule of the
evaporator as restated in tests/evaporate_ref.py: that it is a uniform sample, and that its two-phase (decomposed)
form picks what the one-phase form picks."""

import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import evaporate_ref as ref
import azplugins_amd as azp
from azplugins_amd import _lib
from azplugins_amd.evaporate import ParticleEvaporator
from azplugins_amd.update import TypeUpdater
from azplugins_amd.variant import SphereArea

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- C ABI ---------------------------------------------------------------------------------------------------------
def test_abi_type_update_struct_layout():
    names = ["azp_type_update_args", "azp_evaporate_args"]
    fields = ["N", "solvent_type", "evaporated_type", "Nmax", "z_lo", "z_hi", "timestep", "seed", "block_size", "d_scratch",
              "scratch_bytes", "d_counts", "d_keys_out", "d_n_keys_out"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){' + "".join(
        'printf("%%zu\\n", sizeof(%s));' % n for n in names) + "".join(
        'printf("%%zu\\n", offsetof(azp_evaporate_args, %s));' % f for f in fields) + \
        'printf("%zu\\n", offsetof(azp_type_update_args, z_lo));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == C.sizeof(_lib.TypeUpdateArgs)
    assert got[1] == C.sizeof(_lib.EvaporateArgs)
    for k, f in enumerate(fields):
        assert got[2 + k] == getattr(_lib.EvaporateArgs, f).offset, f
    assert got[-1] == _lib.TypeUpdateArgs.z_lo.offset


def test_abi_type_update_symbols_exported():
    lib = _lib.lib()
    for name in ("azp_type_update_region", "azp_evaporate", "azp_evaporate_local_keys", "azp_evaporate_apply_below",
                 "azp_evaporate_scratch_size"):
        assert hasattr(lib, name)
    assert lib.azp_type_update_region(None, None) == -1  # AZP_ERROR_INVALID_ARGUMENT, no launch
    a = _lib.TypeUpdateArgs()
    assert lib.azp_type_update_region(C.byref(a), None) == 0  # N = 0: nothing to do
    a.N, a.z_lo, a.z_hi = 4, -1.0, 1.0
    assert lib.azp_type_update_region(C.byref(a), None) == -1  # no positions
    assert lib.azp_evaporate(None, None) == -1
    assert lib.azp_evaporate_local_keys(None, None) == -1
    assert lib.azp_evaporate_apply_below(None, 0, None) == -1
    e = _lib.EvaporateArgs()
    assert lib.azp_evaporate(C.byref(e), None) == 0
    assert lib.azp_evaporate_apply_below(C.byref(e), 0, None) == 0
    e.N, e.Nmax, e.z_lo, e.z_hi = 4, 2, -1.0, 1.0
    assert lib.azp_evaporate(C.byref(e), None) == -1  # no arrays
    assert lib.azp_evaporate_apply_below(C.byref(e), 0, None) == -1
    # the scratch buffer holds a header, N keys and a power-of-two sort buffer of at least N keys
    for N in (1, 63, 4096, 2**20, 2**20 + 1):
        size = lib.azp_evaporate_scratch_size(N)
        assert size >= 16 * N and size % 8 == 0
        assert size <= 8 * N + 16 * max(N, 2) + 16384


# -- validation (src/TypeUpdater.cc:133-190) -----------------------------------------------------------------------
class _FakeState:
    def __init__(self, types=("A", "B", "C"), L=(10.0, 10.0, 20.0)):
        self.types = list(types)
        self.box = azp.Box(*L)


def _updater(**kw):
    args = dict(trigger=5, inside_type="A", outside_type="B", lo=-2.0, hi=3.0)
    args.update(kw)
    return TypeUpdater(**args)


def test_valid_updater_and_properties():
    u = _updater()
    assert (u.inside_type, u.outside_type, u.lo, u.hi) == ("A", "B", -2.0, 3.0)
    assert u.trigger == azp.Periodic(5)
    assert u._validate(_FakeState()) == (0, 1)
    u.trigger = azp.Periodic(10, phase=3)
    assert u.trigger.period == 10 and u.trigger.phase == 3
    e = ParticleEvaporator(trigger=2, solvent_type="B", evaporated_type="C", lo=-10.0, hi=10.0, Nmax=7)
    assert (e.solvent_type, e.evaporated_type, e.lo, e.hi, e.Nmax) == ("B", "C", -10.0, 10.0, 7)
    assert isinstance(e, TypeUpdater)
    assert e._validate(_FakeState()) == (2, 1)  # (evaporated = the reference's inside type, solvent = outside)
    assert ParticleEvaporator(1, "A", "B", 0.0, 1.0).Nmax is None
    for bad in (-1, 1.5, 2**32 - 1):
        with pytest.raises(azp.AzpError):
            e.Nmax = bad
    with pytest.raises(azp.AzpError):
        e.n_candidates  # no update yet


def test_inside_type_must_exist():
    with pytest.raises(azp.AzpError, match="inside_type"):
        _updater(inside_type="Z")._validate(_FakeState())


def test_outside_type_must_exist():
    with pytest.raises(azp.AzpError, match="outside_type"):
        _updater(outside_type="Z")._validate(_FakeState())
    with pytest.raises(azp.AzpError, match="solvent_type"):
        ParticleEvaporator(1, "Z", "A", 0.0, 1.0)._validate(_FakeState())


def test_types_must_differ():
    with pytest.raises(azp.AzpError, match="cannot match"):
        _updater(inside_type="A", outside_type="A")._validate(_FakeState())


def test_region_must_not_be_inverted():
    for lo, hi in ((1.0, 1.0), (2.0, -2.0), (float("nan"), 1.0)):
        with pytest.raises(azp.AzpError, match="lower z bound"):
            _updater(lo=lo, hi=hi)._validate(_FakeState())


def test_lower_bound_inside_box():
    with pytest.raises(azp.AzpError, match="lower z bound"):
        _updater(lo=-10.5)._validate(_FakeState())
    _updater(lo=-10.0)._validate(_FakeState())  # on the face: allowed


def test_upper_bound_inside_box():
    with pytest.raises(azp.AzpError, match="upper z bound"):
        _updater(hi=10.5)._validate(_FakeState())
    _updater(hi=10.0)._validate(_FakeState())


def test_validation_runs_again_after_setter_or_box_change():
    u, st = _updater(), _FakeState()
    u._validate(st)
    u.hi = 11.0
    with pytest.raises(azp.AzpError):
        u._validate(st)
    u.hi = 3.0
    u._validate(st)
    u.inside_type = "B"
    with pytest.raises(azp.AzpError):
        u._validate(st)
    u.inside_type = "C"
    assert u._validate(st) == (2, 1)
    st.box = azp.Box(10.0, 10.0, 5.0)  # hi = 3 is outside the new box
    with pytest.raises(azp.AzpError):
        u._validate(st)
    st.box = azp.Box(10.0, 10.0, 20.0)
    st.types = ["A", "B"]  # C is gone
    with pytest.raises(azp.AzpError):
        u._validate(st)


# -- triggers and operations ---------------------------------------------------------------------------------------
def test_periodic_firing_pattern():
    p = azp.Periodic(5)
    assert [t for t in range(16) if p(t)] == [0, 5, 10, 15]
    p = azp.Periodic(4, phase=3)
    assert [t for t in range(16) if p(t)] == [3, 7, 11, 15]
    p = azp.Periodic(3, phase=7)  # fires before its phase too: (t - phase) % period == 0
    assert [t for t in range(12) if p(t)] == [1, 4, 7, 10]
    assert azp.Periodic(1)(2**40 + 1)
    assert azp.Periodic(5, 1) == azp.Periodic(5, phase=1) and azp.Periodic(5, 1) != azp.Periodic(5)
    for bad in (0, -1, 2.5, "5"):
        with pytest.raises((azp.AzpError, ValueError, TypeError)):
            azp.Periodic(bad)
    assert _updater(trigger=7).trigger == azp.Periodic(7)


def test_operations_route_updaters_and_computes():
    from azplugins_amd.compute import VelocityCompute

    sim = azp.Simulation(device="cuda:0", seed=1)
    assert sim.operations.updaters == []
    u, e, v = _updater(), ParticleEvaporator(1, "A", "B", 0.0, 1.0, Nmax=3), VelocityCompute()
    sim.operations.add(u)
    sim.operations.add(e)
    sim.operations.add(v)
    sim.operations.add(u)  # adding twice keeps one entry
    assert sim.operations.updaters == [u, e] and list(sim.operations.computes) == [v]
    with pytest.raises(azp.AzpError):
        sim.operations.add(azp.All())  # neither an updater nor a compute
    sim.operations.remove(u)
    assert sim.operations.updaters == [e] and list(sim.operations.computes) == [v]
    with pytest.raises(ValueError):
        sim.operations.remove(u)
    sim.operations.remove(v)
    with pytest.raises(ValueError):
        sim.operations.remove(v)
    assert sim.operations.updaters == [e]
    assert len(sim.operations.tuners) == 1 and sim.operations.integrator is None


def test_updaters_due_follow_the_timestep():
    sim = azp.Simulation(device="cuda:0", seed=1)
    a, b = _updater(trigger=2), _updater(trigger=azp.Periodic(3, phase=1))
    sim.operations.updaters.extend([a, b])
    fired = []
    for t in range(8):
        sim.timestep = t
        fired.append([u is a for u in sim._updaters_due()])
    assert fired == [[True], [False], [True], [], [True, False], [], [True], [False]]


def test_state_has_a_type_generation():
    import inspect

    from azplugins_amd import nlist, state

    assert "type_generation" in inspect.getsource(state.State.__init__)
    for fn in (nlist.Cell.compute, nlist.Cell.allows_speculative_launch):
        assert "type_generation" in inspect.getsource(fn)


# -- SphereArea (src/VariantSphereArea.cc:18-41) -------------------------------------------------------------------
def test_sphere_area():
    R0, alpha = 10.0, 0.5
    v = SphereArea(R0, alpha)
    assert v(0) == R0
    t_end = 4.0 * math.pi * R0 * R0 / alpha  # 2513.27...
    for t in (1, 100, 1256, 2513):
        want = math.sqrt(R0 * R0 - alpha * t / (4.0 * math.pi))
        assert v(t) == pytest.approx(want, rel=1e-15)
        assert v(t) == ref.sphere_area(R0, alpha, t)
        assert 0.0 < v(t) < R0
    assert v(math.ceil(t_end)) == 0.0 and v(10**6) == 0.0
    # exactly at the end: alpha t / (4 pi) = R0^2 with numbers that are exact in binary
    w = SphereArea(2.0, 4.0 * math.pi)
    assert w(3) == 1.0 and w(4) == 0.0 and w(5) == 0.0
    # the area shrinks linearly: 4 pi R(t)^2 = 4 pi R0^2 - alpha t
    assert 4.0 * math.pi * v(1000) ** 2 == pytest.approx(4.0 * math.pi * R0 * R0 - alpha * 1000, rel=1e-14)
    # usable as the location of the spherical barrier
    from azplugins_amd.external import SphericalHarmonicBarrier

    b = SphericalHarmonicBarrier(location=v)
    assert b._location_at(100) == v(100)
    with pytest.raises(azp.AzpError):
        SphereArea(float("nan"), 1.0)


# -- the selection rule --------------------------------------------------------------------------------------------
def test_region_rule_and_faces():
    z = np.array([-3.0, -2.0, 0.0, 3.0, 3.0000001, -2.0000001, 0.0, 0.0])
    t = np.array([0, 1, 1, 1, 0, 0, 2, 0])
    got = ref.type_update_region(z, t, inside=0, outside=1, lo=-2.0, hi=3.0)
    np.testing.assert_array_equal(got, [1, 0, 0, 0, 1, 1, 2, 0])  # faces are inside; type 2 is left alone


def test_key_layout():
    tags = np.array([0, 1, 77, 2**32 - 1], dtype=np.uint32)
    for seed, t in ((5, 0), (0x1FFFF, 12345), (7, (3 << 32) | 9)):
        k = ref.keys(tags, seed, t)
        assert k.dtype == np.uint64
        np.testing.assert_array_equal(k & np.uint64(0xFFFFFFFF), tags)  # the tag: keys are unique
        import flow_ref

        k0, k1 = flow_ref.key(203, seed, t)
        assert int(k0) >> 24 == 203 and int(k0) & 0xFFFF == seed & 0xFFFF and (int(k0) >> 16) & 0xFF == (t >> 32) & 0xFF
        c0 = flow_ref.philox4x32_10(0, tags, 0, 0, k0, k1)[0]
        np.testing.assert_array_equal(k >> np.uint64(32), c0)
    # the high byte of the timestep enters the key
    assert not np.array_equal(ref.keys(tags, 5, 9), ref.keys(tags, 5, (1 << 32) | 9))


def test_pick_counts():
    tags = np.arange(50, dtype=np.uint32)
    for Nmax, want in ((0, 0), (1, 1), (49, 49), (50, 50), (51, 50), (None, 50)):
        assert ref.pick(tags, 3, 10, Nmax).sum() == want
    assert ref.pick(tags[:0], 3, 10, 4).sum() == 0
    # a larger Nmax picks a superset (the smallest keys come first)
    a, b = ref.pick(tags, 3, 10, 5), ref.pick(tags, 3, 10, 9)
    assert np.all(b[a])


def test_selection_is_a_uniform_sample():
    """M = 64 candidates, K = 8, T = 4000 timesteps, seed 5: every call picks exactly K distinct candidates, and each
    candidate's pick count lies within 5 standard deviations of Binomial(T, K / M): mean 500, sigma =
    sqrt(T (K / M) (1 - K / M)) = 20.9. Over 64 candidates the chance of a false alarm is below 1e-4, and with a fixed
    seed the test is deterministic."""
    M, K, T, seed = 64, 8, 4000, 5
    tags = np.arange(100, 100 + M, dtype=np.uint32)
    counts = np.zeros(M, dtype=np.int64)
    for t in range(T):
        picked = ref.pick(tags, seed, t, K)
        assert picked.sum() == K
        counts += picked
    p = K / M
    mean, sigma = T * p, math.sqrt(T * p * (1.0 - p))
    print("pick counts: min %d, max %d, mean %.1f, sigma %.2f" % (counts.min(), counts.max(), mean, sigma))
    assert counts.sum() == T * K
    assert np.all(np.abs(counts - mean) <= 5.0 * sigma), (counts.min(), counts.max())


@pytest.mark.parametrize("ranks", [2, 4, 8])
def test_two_phase_equals_one_phase(ranks):
    rng = np.random.default_rng(20 + ranks)
    N = 5000
    z = rng.uniform(-10.0, 10.0, N)
    typeid = rng.integers(0, 3, N)
    tag = rng.permutation(N).astype(np.uint32)
    x = rng.uniform(-8.0, 8.0, N)
    owner = np.minimum(((x + 8.0) / 16.0 * ranks).astype(int), ranks - 1)  # slabs along x
    owner[rng.random(N) < 0.1] = ranks - 1  # an uneven decomposition; one rank may hold most candidates
    lo, hi, seed = -1.5, 2.0, 11
    cand = ref.candidates(z, typeid, 1, lo, hi)
    M = int(cand.sum())
    assert M > 200  # (so that every Nmax of the list below is a different case)
    for timestep in (0, 17, (1 << 32) + 3):
        for Nmax in (0, 1, 7, 100, M - 1, M, M + 1, None):
            want, M_ref, n_ref = ref.evaporate(z, typeid, tag, 1, 2, lo, hi, Nmax, seed, timestep)
            assert M_ref == M and n_ref == (M if Nmax is None else min(Nmax, M))
            mine = [np.flatnonzero(cand & (owner == r)) for r in range(ranks)]
            offered = [ref.local_keys(tag[i], seed, timestep, Nmax) for i in mine]
            assert all(np.all(np.diff(k.astype(object)) > 0) for k in offered)  # ascending, unique
            if Nmax is not None:
                assert all(k.size <= Nmax for k in offered)
            thr = ref.threshold(offered, Nmax)
            got = typeid.copy()
            for i in mine:
                got[i[ref.apply_below(tag[i], seed, timestep, thr)]] = 2
            np.testing.assert_array_equal(got, want)
