"""azplugins_amd.minimize.FIRE without a GPU: construction and validation, the driver's refusals, the C ABI, and the
numpy restatement (tests/fire_ref.py) on its own on an anisotropic harmonic well."""

import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fire_ref as ref
from azplugins_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fire(**kw):
    from azplugins_amd import minimize

    args = dict(dt=0.005, force_tol=1e-3, angmom_tol=1e-2, energy_tol=1e-7)
    args.update(kw)
    return minimize.FIRE(**args)


# ---------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------
def test_construction_and_defaults():
    import azplugins_amd as azp
    from azplugins_amd import minimize

    assert azp.minimize is minimize and "minimize" in azp.__all__
    f = minimize.FIRE(dt=0.005, force_tol=1e-3, angmom_tol=1e-2, energy_tol=1e-7)
    assert isinstance(f, azp.Integrator)
    assert (f.dt, f.force_tol, f.angmom_tol, f.energy_tol) == (0.005, 1e-3, 1e-2, 1e-7)
    assert (f.min_steps_adapt, f.finc_dt, f.fdec_dt, f.alpha_start, f.fdec_alpha, f.min_steps_conv) == (5, 1.1, 0.5, 0.1, 0.99, 10)
    assert {k: getattr(f, k) for k in ref.DEFAULTS} == ref.DEFAULTS
    assert f.forces == [] and f.methods == [] and f.integrate_rotational_dof is False
    m = azp.ConstantVolume(azp.All())
    g = minimize.FIRE(0.01, 1e-2, 1e-2, 1e-5, False, [], [m], min_steps_adapt=0, finc_dt=1.2, fdec_dt=0.25, alpha_start=0.2,
                      fdec_alpha=0.9, min_steps_conv=0)
    assert g.methods == [m] and (g.min_steps_adapt, g.min_steps_conv) == (0, 0)
    assert (g.finc_dt, g.fdec_dt, g.alpha_start, g.fdec_alpha) == (1.2, 0.25, 0.2, 0.9)
    r = repr(g)
    assert r.startswith("FIRE(") and "dt=0.01" in r and "fdec_alpha=0.9" in r and "min_steps_conv=0" in r
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.operations.integrator = f
    assert sim.dt == 0.005


def test_before_the_first_run():
    f = _fire()
    assert f.converged is False
    assert f.energy == 0.0 and f.force_rms == 0.0
    f.reset()  # (nothing to reset, nothing attached)
    assert f.converged is False


@pytest.mark.parametrize("name", ["dt", "force_tol", "energy_tol", "angmom_tol"])
def test_positive_parameters(name):
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.AzpError, match=name):
            _fire(**{name: bad})


def test_parameter_ranges():
    for bad in (1.0, 0.5, -2.0, float("nan"), float("inf")):
        with pytest.raises(_lib.AzpError, match="finc_dt"):
            _fire(finc_dt=bad)
    for name in ("fdec_dt", "alpha_start", "fdec_alpha"):
        for bad in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
            with pytest.raises(_lib.AzpError, match=name):
                _fire(**{name: bad})
        _fire(**{name: 0.5})
    for name in ("min_steps_adapt", "min_steps_conv"):
        for bad in (-1, 2.5, True, False, float("nan"), float("inf"), "3"):
            with pytest.raises(_lib.AzpError, match=name):
                _fire(**{name: bad})
        assert getattr(_fire(**{name: 0}), name) == 0
        assert getattr(_fire(**{name: 7.0}), name) == 7


class _FakeState:
    types = ["A"]

    def __init__(self, N):
        self.N = N


def _sim_with(fire, N=10, domain=None):
    import azplugins_amd as azp

    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.state = _FakeState(N)
    sim.domain = domain
    sim.operations.integrator = fire
    return sim


def test_driver_refusals():
    import azplugins_amd as azp
    from azplugins_amd import flow, thermostats

    ok = _fire(methods=[azp.ConstantVolume(azp.All())])
    ok._check(_sim_with(ok))  # nothing to object to
    ok = _fire(methods=[azp.ConstantVolume()])
    ok._check(_sim_with(ok))

    def refused(word, methods=None, **kw):
        sim_kw = {k: kw.pop(k) for k in ("N", "domain") if k in kw}
        f = _fire(methods=[azp.ConstantVolume(azp.All())] if methods is None else methods, **kw)
        with pytest.raises(_lib.AzpError, match=word):
            f._check(_sim_with(f, **sim_kw))

    refused("rotational", integrate_rotational_dof=True)
    refused("exactly one ConstantVolume", methods=[])
    refused("exactly one ConstantVolume", methods=[azp.ConstantVolume(), azp.ConstantVolume()])
    refused("exactly one ConstantVolume", methods=[azp.ConstantVolume(thermostat=thermostats.Bussi(kT=1.0, tau=0.5))])
    refused("exactly one ConstantVolume", methods=[flow.Langevin(azp.All(), kT=1.0, flow_field=flow.ConstantFlow((0.0, 0.0, 0.0)))])
    m = azp.ConstantVolume()
    m.filter = azp.Type("A")
    refused("exactly one ConstantVolume", methods=[m])
    refused("decomposed", domain=object())
    refused("no particles", N=0)


# ---------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------
SLOT_NAMES = ["DT", "ALPHA", "KEEP", "MIX", "N_POS", "N_STEPS", "U", "U_PREV", "P", "VV", "FF", "CONVERGED", "NONFINITE"]


def test_abi_fire_struct_layout():
    fields = [f[0] for f in _lib.FireArgs._fields_ if f[0] != "_pad"]
    consts = ["AZP_FIRE_NSTATE", "AZP_FIRE_NSLOTS"] + ["AZP_FIRE_" + n for n in SLOT_NAMES]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){' \
        'printf("%zu\\n", sizeof(azp_fire_args));' + "".join(
            'printf("%%zu\\n", offsetof(azp_fire_args, %s));' % f for f in fields) + "".join(
            'printf("%%d\\n", (int)%s);' % c for c in consts) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == C.sizeof(_lib.FireArgs)
    for k, f in enumerate(fields):
        assert got[1 + k] == getattr(_lib.FireArgs, f).offset, f
    want = [_lib.FIRE_NSTATE, _lib.FIRE_NSLOTS] + [getattr(_lib, "FIRE_" + n) for n in SLOT_NAMES]
    assert got[1 + len(fields):] == want
    # the restatement lays its state out the same way
    assert ref.NSTATE == _lib.FIRE_NSTATE and [s.upper() for s in ref.SLOTS] == SLOT_NAMES
    assert want[2:] == list(range(len(SLOT_NAMES))) and len(SLOT_NAMES) <= ref.NSTATE


def test_abi_fire_symbols_and_arguments():
    import reduction_ref

    lib = _lib.lib()
    need = C.c_uint64(0)
    assert lib.azp_fire_partials_size(0, C.byref(need)) == -1
    assert lib.azp_fire_partials_size(5, None) == -1
    for N in (1, 256, 257, 2048 * 256 + 1, 2**24):
        assert lib.azp_fire_partials_size(N, C.byref(need)) == 0
        assert need.value == 4 * 8 * reduction_ref.shape(N)[1]
    for name in ("azp_fire_measure", "azp_fire_step_two", "azp_fire_advance", "azp_fire_step_one"):
        fn = getattr(lib, name)
        assert fn(None, None) == -1  # AZP_ERROR_INVALID_ARGUMENT, no launch
        a = _lib.FireArgs()
        assert fn(C.byref(a), None) == -1  # N = 0
        a.N = 4
        assert fn(C.byref(a), None) == -1  # no arrays
    # the advance checks its scalars ahead of the launch (the pointers are never followed)
    adv = lib.azp_fire_advance
    buf = (C.c_double * 16)()

    def args(**kw):
        a = _lib.FireArgs()
        a.N, a.dt_max, a.force_tol, a.energy_tol = 4, 0.005, 1e-3, 1e-7
        a.finc_dt, a.fdec_dt, a.alpha_start, a.fdec_alpha, a.min_steps_adapt, a.min_steps_conv = 1.1, 0.5, 0.1, 0.99, 5, 10
        a.d_state = C.addressof(buf)
        a.d_partials = C.addressof(buf)
        a.partials_bytes = 32
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    nan, inf = float("nan"), float("inf")
    bad = [dict(dt_max=0.0), dict(dt_max=-1.0), dict(dt_max=nan), dict(dt_max=inf), dict(force_tol=0.0), dict(force_tol=nan),
           dict(force_tol=inf), dict(energy_tol=0.0), dict(energy_tol=-1e-3), dict(energy_tol=inf), dict(finc_dt=1.0), dict(finc_dt=nan),
           dict(finc_dt=inf), dict(fdec_dt=0.0), dict(fdec_dt=1.0), dict(fdec_dt=nan), dict(alpha_start=0.0), dict(alpha_start=1.0),
           dict(fdec_alpha=0.0), dict(fdec_alpha=1.0), dict(fdec_alpha=nan), dict(partials_bytes=24), dict(partials_bytes=0),
           dict(d_state=None), dict(d_partials=None), dict(N=257, partials_bytes=32)]
    for kw in bad:
        assert adv(C.byref(args(**kw)), None) == -1, kw
    # the passes over the particles refuse a partials buffer that is too small ahead of any launch
    for name in ("azp_fire_measure", "azp_fire_step_two"):
        a = args(d_vel=C.addressof(buf), d_net_force=C.addressof(buf), partials_bytes=24)
        assert getattr(lib, name)(C.byref(a), None) == -1


# ---------------------------------------------------------------------------
# the reference on its own
# ---------------------------------------------------------------------------
WELL_K = np.array([1.0, 4.0, 9.0])
WELL_L = np.array([1000.0, 1000.0, 1000.0])


def well_force(pos):
    """U = 1/2 sum k_c x_c^2: (force, each particle's energy), in a fixed order of operations."""
    f = -(WELL_K * pos)
    e = 0.5 * (((WELL_K[0] * pos[:, 0]) * pos[:, 0] + (WELL_K[1] * pos[:, 1]) * pos[:, 1]) + (WELL_K[2] * pos[:, 2]) * pos[:, 2])
    return f, e


def _well_run(steps=2000, **kw):
    rng = np.random.default_rng(50)
    N = 50
    pos = rng.normal(0.0, 1.0, (N, 3))
    log = []
    out = ref.minimize(well_force, pos, np.zeros((N, 3)), np.ones(N), WELL_L, 0.05, 1e-7, 1e-7, steps,
                       record=lambda k, p, v, s: log.append((dict(s), v.copy())), **kw)
    return out, log, pos


def test_reference_converges_on_the_well():
    (pos, vel, image, s, taken), log, pos0 = _well_run()
    # (it converges after 211 steps: well inside the budget of 2000)
    print("fire_ref on the harmonic well: converged after %d steps, force_rms %.3g" % (taken, ref.force_rms(s, 50)))
    assert s["converged"] == 1.0 and s["nonfinite"] == 0.0 and taken < 2000
    assert ref.force_rms(s, 50) < 1e-7
    assert np.abs(pos).max() < 1e-6 and np.abs(pos0).max() > 1.0
    assert s["u"] / 50 < 1e-12
    dts = np.array([st["dt"] for st, _ in log])
    assert dts.max() <= 0.05  # DT never exceeds dt
    assert dts.max() == 0.05 and dts.min() < 0.05  # and it did adapt both ways
    assert not np.any(image)


def test_nonpositive_power_drops_the_velocities_and_halves_dt():
    _, log, _ = _well_run()
    states = [st for st, _ in log]
    resets = [k for k, st in enumerate(states) if st["p"] <= 0.0 and k > 0]
    assert resets, "the run never met P <= 0 after its first step"
    for k in resets:
        st, before = states[k], states[k - 1]
        assert (st["keep"], st["mix"], st["n_pos"], st["alpha"]) == (0.0, 0.0, 0.0, 0.1)
        assert st["dt"] == before["dt"] * 0.5
    # the first step starts from rest: P = 0 counts as non-positive
    assert states[0]["p"] == 0.0 and states[0]["dt"] == 0.025
    # one step by hand: velocities against the force are dropped, so the step starts from v = (DT / 2) f / m alone
    rng = np.random.default_rng(3)
    pos, mass = rng.normal(size=(7, 3)), rng.uniform(0.5, 2.0, 7)
    f, e = well_force(pos)
    vel = -f
    s = ref.advance(ref.measure(vel, f, e), ref.new_state(0.05), 7, 0.05, 1e-7, 1e-7)
    assert s["p"] < 0.0 and (s["dt"], s["keep"], s["mix"]) == (0.025, 0.0, 0.0)
    p1, v1, _ = ref.step_one(pos, vel, mass, f, np.zeros((7, 3), dtype=np.int32), WELL_L, s)
    np.testing.assert_array_equal(v1, 0.0 * vel + 0.0 * f + (0.0125 * f) * (1.0 / mass)[:, None])
    np.testing.assert_array_equal(p1, pos + 0.025 * v1)


def test_dt_grows_after_min_steps_adapt_and_is_capped():
    s = ref.new_state(0.05)
    s["dt"] = 0.02
    sums = (1.0, 1.0, 1.0, -1.0)  # P > 0
    dts = []
    for _ in range(20):
        s = ref.advance(sums, s, 10, 0.05, 1e-7, 1e-7)
        dts.append(s["dt"])
    assert dts[:5] == [0.02] * 5  # N_POS = 1 .. 5: not above min_steps_adapt
    assert dts[5] == 0.02 * 1.1
    assert math.isclose(s["alpha"], 0.1 * 0.99 ** 15, rel_tol=1e-13)  # (shrunk at the 15 advances with N_POS > 5)
    assert max(dts) == 0.05 and dts[-1] == 0.05
    nxt = ref.advance(sums, s, 10, 0.05, 1e-7, 1e-7)
    assert nxt["keep"] == 1.0 - s["alpha"] and nxt["mix"] == s["alpha"] * 1.0  # (the coefficients use ALPHA before it shrinks)
    # FF == 0 leaves no direction to mix in
    assert ref.advance((0.0, 1.0, 0.0, 0.0), ref.new_state(0.05), 10, 0.05, 1e-7, 1e-7)["mix"] == 0.0


def test_convergence_flag_is_sticky():
    (pos, vel, image, s, taken), _, _ = _well_run()
    assert s["converged"] == 1.0 and (s["keep"], s["mix"]) == (0.0, 0.0)
    # sums that would not converge change nothing any more, and nothing moves
    again = ref.advance((5.0, 1.0, 100.0, 3.0), s, 50, 0.05, 1e-7, 1e-7)
    assert again == s
    p1, v1, i1 = ref.step_one(pos, vel, np.ones(50), well_force(pos)[0], image, WELL_L, s)
    assert p1 is pos and v1 is vel and i1 is image
    v2, sums = ref.step_two(vel, np.ones(50), well_force(pos)[0], well_force(pos)[1], s)
    assert v2 is vel and sums is None
    # the driver's loop, which does not stop, ends in the same place
    (pos_b, vel_b, _, s_b, taken_b), _, _ = _well_run(steps=taken + 40, stop_at_convergence=False)
    assert taken_b == taken + 40 and s_b == s
    np.testing.assert_array_equal(pos_b, pos)
    np.testing.assert_array_equal(vel_b, vel)
    # min_steps_conv holds convergence back, and max(1, 0) = 1 keeps the very first advance from converging on U_PREV = 0
    tiny = (0.0, 0.0, 1e-30, 1e-30)
    assert ref.advance(tiny, ref.new_state(0.05), 50, 0.05, 1e-7, 1e-7, min_steps_conv=0)["converged"] == 0.0
    s1 = dict(ref.new_state(0.05), n_steps=1.0)
    assert ref.advance(tiny, s1, 50, 0.05, 1e-7, 1e-7, min_steps_conv=0)["converged"] == 1.0
    assert ref.advance(tiny, s1, 50, 0.05, 1e-7, 1e-7, min_steps_conv=10)["converged"] == 0.0
    # a non-finite sum is sticky too
    bad = ref.advance((float("nan"), 1.0, 1.0, 1.0), ref.new_state(0.05), 50, 0.05, 1e-7, 1e-7)
    assert bad["nonfinite"] == 1.0 and ref.advance((1.0, 1.0, 1.0, 1.0), bad, 50, 0.05, 1e-7, 1e-7) == bad
