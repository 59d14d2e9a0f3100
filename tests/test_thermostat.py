"""azplugins_amd.thermostats without a GPU: construction and validation, the driver's rejections, the C ABI, and the
numpy restatement (tests/thermostat_ref.py) on its own: its random stream against the vectorised Philox, the Gamma
sampler's moments, the stationary kinetic energy of the Bussi recurrence, and the conserved quantity of MTTK."""

import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import flow_ref
import thermostat_ref as ref
from azplugins_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------
def test_construction():
    import azplugins_amd as azp
    from azplugins_amd import ConstantVolume, thermostats

    assert azp.thermostats is thermostats
    m = ConstantVolume(thermostat=thermostats.Bussi(kT=1.0, tau=0.5))
    assert isinstance(m.thermostat, thermostats.Bussi) and m.thermostat.kT == 1.0 and m.thermostat.tau == 0.5
    assert isinstance(m.filter, azp.All)
    assert thermostats.Bussi(kT=2.0).tau == 0.0
    assert ConstantVolume().thermostat is None and ConstantVolume(thermostat=None).thermostat is None
    m = ConstantVolume(azp.All(), thermostats.MTTK(kT=lambda t: 1.0 + 0.5 * t, tau=1.0))
    assert m.thermostat._kT_at(2) == 2.0
    b = thermostats.Berendsen(kT=1.5, tau=2.0)
    assert (b.kT, b.tau) == (1.5, 2.0)
    assert "Berendsen" in repr(b)


def test_parameter_validation():
    from azplugins_amd import ConstantVolume, thermostats

    for cls in (thermostats.Berendsen, thermostats.Bussi, thermostats.MTTK):
        for kT in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(_lib.AzpError):
                cls(kT=kT, tau=1.0)
        for tau in (-1.0, float("nan"), float("inf")):
            with pytest.raises(_lib.AzpError):
                cls(kT=1.0, tau=tau)
    for cls in (thermostats.Berendsen, thermostats.MTTK):
        with pytest.raises(_lib.AzpError):
            cls(kT=1.0, tau=0.0)
        with pytest.raises(TypeError):
            cls(kT=1.0)  # (tau has a default for Bussi alone)
    t = thermostats.MTTK(kT=1.0, tau=1.0)
    with pytest.raises(_lib.AzpError):
        t.tau = 0.0
    assert t.tau == 1.0
    # a variant that turns non-positive is refused at the step it does
    t.kT = lambda step: 1.0 - step
    assert t._kT_at(0) == 1.0
    with pytest.raises(_lib.AzpError):
        t._kT_at(1)
    with pytest.raises(_lib.AzpError):
        ConstantVolume(thermostat="bussi")


def test_state_before_the_first_run():
    """``energy`` and ``translational_dof`` can be read and set before the thermostat has met a device."""
    from azplugins_amd import thermostats

    for t in (thermostats.Berendsen(kT=1.0, tau=1.0), thermostats.Bussi(kT=1.0)):
        assert t.energy == 0.0
        t.energy = -2.5
        assert t.energy == -2.5
        with pytest.raises(_lib.AzpError):
            t.energy = float("nan")
    m = thermostats.MTTK(kT=1.0, tau=0.5)
    assert m.translational_dof == (0.0, 0.0) and m.energy == 0.0
    m.translational_dof = (0.25, -1.0)
    assert m.translational_dof == (0.25, -1.0)
    with pytest.raises(_lib.AzpError):
        m.energy = 1.0
    with pytest.raises(_lib.AzpError):
        m.translational_dof = (float("inf"), 0.0)


class _FakeState:
    types = ["A"]

    def __init__(self, N):
        self.N = N


def _sim_with(method, N=10, rot=False, domain=None, dt=0.005):
    import azplugins_amd as azp

    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.state = _FakeState(N)
    sim.domain = domain
    return sim, azp.Integrator(dt=dt, methods=[method], integrate_rotational_dof=rot)


def test_driver_rejections():
    from azplugins_amd import ConstantVolume, Type, thermostats

    def method(th=None):
        return ConstantVolume(thermostat=th if th is not None else thermostats.Bussi(kT=1.0, tau=0.5))

    m = method()
    sim, integ = _sim_with(m)
    sim._check_thermostat(integ, m)  # nothing to object to
    m = method(thermostats.Berendsen(kT=1.0, tau=0.005))
    sim, integ = _sim_with(m)
    sim._check_thermostat(integ, m)  # tau == dt is the limit

    def refused(m, word, **kw):
        sim, integ = _sim_with(m, **kw)
        with pytest.raises(_lib.AzpError, match=word):
            sim._check_thermostat(integ, m)

    m = method()
    m.filter = Type("A")
    refused(m, "filter")
    refused(method(), "rotational", rot=True)
    refused(method(), "decomposed", domain=object())
    refused(method(), "fewer than 2 particles", N=1)
    refused(method(thermostats.Berendsen(kT=1.0, tau=0.004)), "below dt")
    # MTTK and Bussi take any positive tau
    for th in (thermostats.MTTK(kT=1.0, tau=0.001), thermostats.Bussi(kT=1.0, tau=0.001)):
        m = method(th)
        sim, integ = _sim_with(m)
        sim._check_thermostat(integ, m)
    th = thermostats.Bussi(kT=1.0, tau=0.5)
    m1, m2 = method(th), method(th)
    refused(m1, "two methods")
    refused(m2, "two methods")
    # handing the thermostat on releases it
    m2.thermostat = None
    sim, integ = _sim_with(m1)
    sim._check_thermostat(integ, m1)


# ---------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------
def test_abi_thermostat_struct_layout():
    fields = [f[0] for f in _lib.ThermostatArgs._fields_ if f[0] != "_pad"]
    consts = ["AZP_THERMOSTAT_BERENDSEN", "AZP_THERMOSTAT_BUSSI", "AZP_THERMOSTAT_MTTK", "AZP_THERMOSTAT_NSTATE",
              "AZP_THERMOSTAT_ALPHA", "AZP_THERMOSTAT_K", "AZP_THERMOSTAT_ENERGY", "AZP_THERMOSTAT_XI", "AZP_THERMOSTAT_ETA",
              "AZP_THERMOSTAT_ATTEMPTS"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){' \
        'printf("%zu\\n", sizeof(azp_thermostat_args));' + "".join(
            'printf("%%zu\\n", offsetof(azp_thermostat_args, %s));' % f for f in fields) + "".join(
            'printf("%%d\\n", (int)%s);' % c for c in consts) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == C.sizeof(_lib.ThermostatArgs)
    for k, f in enumerate(fields):
        assert got[1 + k] == getattr(_lib.ThermostatArgs, f).offset, f
    want = [_lib.THERMOSTAT_BERENDSEN, _lib.THERMOSTAT_BUSSI, _lib.THERMOSTAT_MTTK, _lib.THERMOSTAT_NSTATE,
            _lib.THERMOSTAT_ALPHA, _lib.THERMOSTAT_K, _lib.THERMOSTAT_ENERGY, _lib.THERMOSTAT_XI, _lib.THERMOSTAT_ETA,
            _lib.THERMOSTAT_ATTEMPTS]
    assert got[1 + len(fields):] == want
    assert (ref.BERENDSEN, ref.BUSSI, ref.MTTK) == tuple(want[:3])


def test_abi_thermostat_symbols_and_arguments():
    import reduction_ref

    lib = _lib.lib()
    need = C.c_uint64(0)
    assert lib.azp_thermostat_partials_size(0, C.byref(need)) == -1
    assert lib.azp_thermostat_partials_size(5, None) == -1
    for N in (1, 256, 257, 2048 * 256 + 1, 2**24):
        assert lib.azp_thermostat_partials_size(N, C.byref(need)) == 0
        assert need.value == 8 * reduction_ref.shape(N)[1]
    for name in ("azp_thermostat_kinetic", "azp_thermostat_step_two", "azp_thermostat_advance", "azp_thermostat_step_one"):
        fn = getattr(lib, name)
        assert fn(None, None) == -1  # AZP_ERROR_INVALID_ARGUMENT, no launch
        a = _lib.ThermostatArgs()
        assert fn(C.byref(a), None) == -1  # N = 0
        a.N, a.dt, a.kT, a.tau, a.ndof = 4, 0.005, 1.0, 1.0, 9.0
        assert fn(C.byref(a), None) == -1  # no arrays
    # the advance checks its scalars ahead of the launch (the pointers are never followed)
    adv = lib.azp_thermostat_advance
    buf = (C.c_double * 8)()

    def args(**kw):
        a = _lib.ThermostatArgs()
        a.N, a.dt, a.kT, a.tau, a.ndof, a.kind = 4, 0.005, 1.0, 1.0, 9.0, _lib.THERMOSTAT_BUSSI
        a.d_state = C.addressof(buf)
        a.d_partials = C.addressof(buf)
        a.partials_bytes = 8
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = [dict(kind=3), dict(dt=0.0), dict(kT=0.0), dict(kT=-1.0), dict(ndof=2.0), dict(tau=-1.0),
           dict(kind=_lib.THERMOSTAT_MTTK, tau=0.0), dict(kind=_lib.THERMOSTAT_BERENDSEN, tau=0.004),
           dict(partials_bytes=0), dict(d_state=None), dict(d_partials=None), dict(N=257, partials_bytes=8)]
    for kw in bad:
        assert adv(C.byref(args(**kw)), None) == -1, kw


# ---------------------------------------------------------------------------
# the reference on its own
# ---------------------------------------------------------------------------
def test_stream_matches_vectorised_philox():
    for seed, t in ((0, 0), (7, 12345), (0xFFFF, (0xAB << 32) | 0xDEADBEEF)):
        s = ref.Stream(seed, t)
        k0, k1 = flow_ref.key(ref.THERMOSTAT_ID, seed, t)
        assert (k0 >> 24) == 204
        ks = np.arange(40, dtype=np.uint32)
        r = flow_ref.philox4x32_10(ks, 0, 0, 0, k0, k1)
        want = flow_ref.u01(r[0], r[1])
        got = np.array([s.u01(int(k)) for k in ks])
        np.testing.assert_array_equal(got, want)
        assert np.all((got > 0.0) & (got <= 1.0))
    # a normal is Box-Muller of two consecutive draws
    s = ref.Stream(3, 9)
    assert s.normal(5) == math.sqrt(-2.0 * math.log(s.u01(5))) * math.cos(6.283185307179586 * s.u01(6))


def test_normal_moments():
    n = 20000
    x = np.array([ref.Stream(11, t).normal(0) for t in range(n)])
    assert abs(x.mean()) < 5.0 / math.sqrt(n)
    assert abs(x.var() - 1.0) < 5.0 * math.sqrt(2.0 / n)


@pytest.mark.parametrize("ndof", [3, 93, 3 * 2**20 - 3])
def test_chi_square_moments(ndof):
    """2 Gamma((Nf - 1) / 2) is chi-square with nu = Nf - 1 degrees of freedom: mean nu, variance 2 nu. The sample
    mean has the variance 2 nu / n, the sample variance (mu_4 - sigma^4) / n = (8 nu^2 + 48 nu) / n."""
    n, nu = 6000, ndof - 1
    draws, worst = np.empty(n), 0
    for t in range(n):
        g, attempts = ref.Stream(5, t).gamma(0.5 * nu)
        draws[t] = 2.0 * g
        worst = max(worst, attempts)
    assert worst <= ref.GAMMA_MAX_ATTEMPTS  # the cap is never reached
    assert worst <= 6
    assert np.all(draws > 0.0)
    assert abs(draws.mean() - nu) < 5.0 * math.sqrt(2.0 * nu / n)
    assert abs(draws.var(ddof=1) - 2.0 * nu) < 5.0 * math.sqrt((8.0 * nu * nu + 48.0 * nu) / n)


@pytest.mark.parametrize("tau", [0.0, 0.05])
def test_bussi_recurrence_is_canonical(tau):
    """Without forces K_(n+1) = alpha_n^2 K_n samples the canonical K: mean Kbar = Nf kT / 2, variance Nf kT^2 / 2,
    autocorrelation c = exp(-dt / tau) per step, which inflates the variance of the mean by (1 + c) / (1 - c)."""
    ndof, kT, dt, n = 93.0, 1.5, 0.005, 20000
    Kbar = 0.5 * ndof * kT
    Ks, alphas, state, worst = ref.ideal_gas(ref.BUSSI, Kbar, n, kT, tau, dt, ndof, seed=21)
    assert worst <= ref.GAMMA_MAX_ATTEMPTS
    assert np.all(alphas > 0.0)
    c = math.exp(-dt / tau) if tau > 0.0 else 0.0
    inflate = (1.0 + c) / (1.0 - c)
    var = 0.5 * ndof * kT * kT
    assert abs(Ks[1:].mean() - Kbar) < 5.0 * math.sqrt(var * inflate / n)
    # the energy the thermostat took is what the particles lost
    assert state["energy"] == pytest.approx(Ks[0] - Ks[-1], rel=1e-9, abs=1e-9 * Kbar)
    if tau == 0.0:
        # independent draws: the variance is testable too (mu_4 - sigma^4 of a Gamma(Nf / 2): 2 var^2 (1 + 6 / Nf))
        assert abs(Ks[1:].var(ddof=1) - var) < 5.0 * math.sqrt(2.0 * var * var * (1.0 + 6.0 / ndof) / n)


def test_berendsen_recurrence_and_zero_K():
    ndof, kT, dt, tau = 93.0, 1.5, 0.005, 0.5
    Ks, alphas, state, _ = ref.ideal_gas(ref.BERENDSEN, 10.0, 400, kT, tau, dt, ndof)
    np.testing.assert_allclose(Ks, ref.berendsen_closed(10.0, 400, kT, tau, dt, ndof), rtol=1e-12)
    assert state["energy"] == pytest.approx(Ks[0] - Ks[-1], rel=1e-10)
    # tau == dt reaches Kbar in one step
    Ks, _, _, _ = ref.ideal_gas(ref.BERENDSEN, 10.0, 1, kT, dt, dt, ndof)
    assert Ks[1] == pytest.approx(0.5 * ndof * kT, rel=1e-14)
    # K == 0: Berendsen and Bussi leave everything alone, MTTK still integrates xi and eta
    start = dict(energy=0.25, xi=0.0, eta=0.0)
    for kind in (ref.BERENDSEN, ref.BUSSI):
        alpha, s, attempts = ref.advance(kind, 0.0, start, kT, tau, dt, ndof, 1, 2)
        assert alpha == 1.0 and s == start and attempts == 0
    alpha, s, _ = ref.advance(ref.MTTK, 0.0, start, kT, tau, dt, ndof)
    g0 = -1.0 / (tau * tau)
    assert s["xi"] == pytest.approx(dt * g0, rel=1e-14) and s["eta"] == pytest.approx(0.5 * dt * dt * g0, rel=1e-14)
    assert alpha == pytest.approx(math.exp(-0.5 * dt * dt * g0), rel=1e-14)


def test_mttk_conserves_its_energy_on_oscillators():
    """K + U + energy of thermostatted harmonic oscillators drifts no more than 4 times what K + U of plain velocity
    Verlet drifts over the same steps. The energy error of velocity Verlet scales with (omega dt)^2 of the stiffest
    mode. Linearised about equilibrium the thermostat is an oscillator of its own, xi'' = -(2 / tau^2) xi, so the bound
    is asked where it is not the stiffest mode of the system: sqrt(2) / tau <= sqrt(k_max / m_min) = sqrt(4 / 0.5),
    i.e. tau >= 0.5."""
    rng = np.random.default_rng(31)
    n, steps, dt = 32, 4000, 0.005
    x = rng.normal(0.0, 1.0, (n, 3))
    v = rng.normal(0.0, 1.0, (n, 3))
    m = rng.uniform(0.5, 2.0, n)
    k = rng.uniform(0.5, 4.0, n)
    plain = ref.oscillators(None, x, v, m, k, steps, dt)
    drift_plain = np.abs(plain - plain[0]).max()
    assert 0.0 < drift_plain < 1e-3 * abs(plain[0])
    for kT, tau in ((1.0, 0.5), (2.0, 1.0), (0.5, 2.0)):
        thermo = ref.oscillators(ref.MTTK, x, v, m, k, steps, dt, kT=kT, tau=tau)
        assert np.abs(thermo - thermo[0]).max() <= 4.0 * drift_plain, (kT, tau)
    # and the thermostat does act: the energy of the particles alone changes by far more
    alpha, s, _ = ref.advance(ref.MTTK, 100.0, ref.new_state(), 1.0, 0.5, dt, 93.0)
    assert alpha < 1.0 and s["xi"] > 0.0


@pytest.mark.parametrize("kind", [ref.BERENDSEN, ref.BUSSI, ref.MTTK])
def test_particle_recurrence_and_scalar_recurrence_agree(kind):
    """The recurrence carried per particle in the kernels' arithmetic and the scalar K_(n+1) = alpha_n^2 K_n differ by
    rounding alone, within ``recurrence_rounding``."""
    rng = np.random.default_rng(41)
    n, steps, dt = 32, 200, 0.005
    v, m = rng.normal(size=(n, 3)), rng.uniform(0.5, 2.0, n)
    ndof = 3.0 * n - 3.0
    Ks, alphas, recorded, v_end, state, worst = ref.ideal_gas_particles(kind, v, m, steps, 1.5, 0.2, dt, ndof, seed=3)
    scalar, alphas_s, state_s, _ = ref.ideal_gas(kind, Ks[0], steps, 1.5, 0.2, dt, ndof, seed=3)
    assert worst <= ref.GAMMA_MAX_ATTEMPTS and Ks[0] == ref.kinetic_energy(v, m)
    bound = ref.recurrence_rounding(steps)
    assert 0.0 < np.abs(recorded - scalar[1:]).max() / scalar.max() <= bound
    assert np.abs(Ks - scalar[:-1]).max() <= bound * scalar.max()
    assert np.abs(alphas - alphas_s).max() <= bound
    assert recorded[-1] == ref.recorded_kinetic_energy(v_end, m)
    assert abs(state["energy"] - state_s["energy"]) <= bound * (abs(state_s["energy"]) + scalar.max())
