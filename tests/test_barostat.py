"""azplugins_amd.ConstantPressure without a GPU: construction and the refusals, the C ABI, and the numpy restatement
(tests/barostat_ref.py) on its own: time reversibility, the conserved quantity against plain velocity Verlet in the same
arithmetic, and the couplings."""

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import barostat_ref as ref
from azplugins_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.005


# ---------------------------------------------------------------------------
# public interface
# ---------------------------------------------------------------------------
def test_construction():
    import azplugins_amd as azp
    from azplugins_amd import thermostats, variant

    m = azp.ConstantPressure(azp.All(), S=2.0, tauS=1.5, couple="xyz")
    assert m.S == (2.0, 2.0, 2.0, 0.0, 0.0, 0.0) and m._S_at(7) == (2.0, 2.0, 2.0)
    assert (m.tauS, m.couple, m.thermostat, m.gamma, m.rescale_all) == (1.5, "xyz", None, 0.0, False)
    assert m.box_dof == (True, True, True, False, False, False) and isinstance(m.filter, azp.All)
    assert m._fusable is False
    m = azp.ConstantPressure(filter=azp.All(), S=[1.0, 2.0, 3.0, 0.0, 0.0, 0.0], tauS=1.0, couple="none",
                             thermostat=thermostats.Bussi(kT=1.0, tau=0.5), box_dof=(True, False, True, False, False, False))
    assert m._S_at(0) == (1.0, 2.0, 3.0) and isinstance(m.thermostat, thermostats.Bussi)
    m = azp.ConstantPressure(azp.All(), S=lambda t: 1.0 + 0.5 * t, tauS=1.0, couple="xy")
    assert m._S_at(2) == (2.0, 2.0, 2.0)
    m = azp.ConstantPressure(azp.All(), S=variant.Ramp(1.0, 3.0, 0, 10), tauS=1.0, couple="xy")
    assert m._S_at(5) == (2.0, 2.0, 2.0)
    assert "ConstantPressure" in repr(m)
    assert "ConstantPressure" in azp.__all__


def test_state_before_the_first_run():
    import azplugins_amd as azp

    m = azp.ConstantPressure(azp.All(), S=1.0, tauS=1.0, couple="none")
    assert m.barostat_dof == (0.0, 0.0, 0.0) and m.barostat_energy == 0.0 and m.reference_kT == 0.0
    m.barostat_dof = (0.1, -0.2, 0.3)
    assert m.barostat_dof == (0.1, -0.2, 0.3)
    m.reference_kT = 1.25
    assert m.reference_kT == 1.25
    with pytest.raises(_lib.AzpError, match="finite"):
        m.barostat_dof = (float("nan"), 0.0, 0.0)
    with pytest.raises(_lib.AzpError, match="nu_x, nu_y, nu_z"):
        m.barostat_dof = (0.0, 0.0)
    with pytest.raises(_lib.AzpError, match="reference_kT"):
        m.reference_kT = -1.0


def test_constructor_refusals():
    import azplugins_amd as azp

    def make(**kw):
        args = dict(filter=azp.All(), S=1.0, tauS=1.0, couple="none")
        args.update(kw)
        return azp.ConstantPressure(**args)

    make()
    for kw, word in ((dict(filter=azp.Type("A")), "filter=All"), (dict(gamma=0.1), "Langevin piston"),
                     (dict(box_dof=(True, True, True, True, False, False)), "tilt degrees of freedom"),
                     (dict(box_dof=(True, True, True, False, False, True)), "tilt degrees of freedom"),
                     (dict(box_dof=(True, True, True)), "six flags"), (dict(couple="zx"), "couple must be one of"),
                     (dict(tauS=0.0), "tauS must be > 0"), (dict(tauS=float("nan")), "tauS must be > 0"),
                     (dict(S=[1.0, 1.0, 1.0, 0.0, 0.5, 0.0]), "shear stresses"), (dict(S=[1.0, 2.0, 3.0]), "six values"),
                     (dict(S=float("inf")), "finite"), (dict(thermostat="bussi"), "thermostat must be None or one of")):
        with pytest.raises(_lib.AzpError, match=word):
            make(**kw)
    m = make(S=lambda t: float("nan"))
    with pytest.raises(_lib.AzpError, match="finite"):
        m._S_at(3)


class _FakeState:
    types = ["A"]

    def __init__(self, N, box):
        self.N, self.box = N, box


def test_run_time_refusals():
    import azplugins_amd as azp
    from azplugins_amd import thermostats

    def method(**kw):
        args = dict(filter=azp.All(), S=1.0, tauS=1.0, couple="none")
        args.update(kw)
        return azp.ConstantPressure(**args)

    def check(m, N=10, box=None, rot=False, domain=None, methods=None, forces=(), dt=DT):
        sim = azp.Simulation(device="cuda:0", seed=1)
        sim.state = _FakeState(N, azp.Box(6.0, 7.0, 8.0) if box is None else box)
        sim.domain = domain
        integ = azp.Integrator(dt=dt, forces=list(forces), methods=[m] if methods is None else methods, integrate_rotational_dof=rot)
        m._check(sim, integ)

    def refused(word, m=None, **kw):
        with pytest.raises(_lib.AzpError, match=word):
            check(method() if m is None else m, **kw)

    check(method())  # nothing to object to
    check(method(thermostat=thermostats.MTTK(kT=1.0, tau=0.5)))
    m = method()
    m.filter = azp.Type("A")
    refused("filter=All", m)
    refused("rotational", rot=True)
    refused("decomposed", domain=object())
    refused("fewer than 2 particles", N=1)
    refused("tilted", box=azp.Box(6.0, 7.0, 8.0, xy=0.1))
    refused("not periodic along y", box=azp.Box(6.0, 7.0, 8.0, periodic=(True, False, True)))
    # (a frozen axis need not be periodic)
    check(method(box_dof=(True, False, True, False, False, False)), box=azp.Box(6.0, 7.0, 8.0, periodic=(True, False, True)))
    m = method()
    refused("only method", m, methods=[m, azp.ConstantVolume()])
    refused("only method", m, methods=[m, method()])
    refused("at most 8 forces", forces=[object()] * 9)
    refused("below dt", method(thermostat=thermostats.Berendsen(kT=1.0, tau=0.004)))
    # one thermostat object in two methods: whichever the other holder is
    th = thermostats.Bussi(kT=1.0, tau=0.5)
    m1 = method(thermostat=th)
    cv = azp.ConstantVolume(thermostat=th)
    refused("two methods", m1)
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.state = _FakeState(10, azp.Box(6.0, 7.0, 8.0))
    with pytest.raises(_lib.AzpError, match="two methods"):
        sim._check_thermostat(azp.Integrator(dt=DT, methods=[cv]), cv)
    cv.thermostat = None
    check(m1)


def test_degrees_of_freedom():
    import azplugins_amd as azp
    from azplugins_amd import compute

    m = azp.ConstantPressure(azp.All(), S=1.0, tauS=1.0, couple="none")
    assert compute._integrator_flags(azp.Integrator(dt=DT, methods=[m])) == (True, False)
    q = compute.thermo_quantities([10.0] + [0.0] * 19, 10, 1.0, True, False)
    assert q["translational_degrees_of_freedom"] == 27.0


# ---------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------
def test_abi_barostat_struct_layout():
    fields = [f[0] for f in _lib.BarostatArgs._fields_]
    consts = ["AZP_BAROSTAT_NSTATE", "AZP_BAROSTAT_NU", "AZP_BAROSTAT_ALPHA", "AZP_BAROSTAT_LAMBDA", "AZP_BAROSTAT_B",
              "AZP_BAROSTAT_ALPHA_T", "AZP_BAROSTAT_ENERGY", "AZP_BAROSTAT_V", "AZP_BAROSTAT_P", "AZP_BAROSTAT_NONFINITE",
              "AZP_BAROSTAT_REF_KT", "AZP_BAROSTAT_K", "AZP_BAROSTAT_W", "AZP_BAROSTAT_CLOSE", "AZP_BAROSTAT_OPEN",
              "AZP_BAROSTAT_COUPLE_NONE", "AZP_BAROSTAT_COUPLE_XY", "AZP_BAROSTAT_COUPLE_XZ", "AZP_BAROSTAT_COUPLE_YZ",
              "AZP_BAROSTAT_COUPLE_XYZ", "AZP_THERMO_NSUMS"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){' \
        'printf("%zu\\n", sizeof(azp_barostat_args));' + "".join(
            'printf("%%zu\\n", offsetof(azp_barostat_args, %s));' % f for f in fields) + "".join(
            'printf("%%d\\n", (int)%s);' % c for c in consts) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == C.sizeof(_lib.BarostatArgs)
    for k, f in enumerate(fields):
        assert got[1 + k] == getattr(_lib.BarostatArgs, f).offset, f
    want = [_lib.BAROSTAT_NSTATE, _lib.BAROSTAT_NU, _lib.BAROSTAT_ALPHA, _lib.BAROSTAT_LAMBDA, _lib.BAROSTAT_B, _lib.BAROSTAT_ALPHA_T,
            _lib.BAROSTAT_ENERGY, _lib.BAROSTAT_V, _lib.BAROSTAT_P, _lib.BAROSTAT_NONFINITE, _lib.BAROSTAT_REF_KT, _lib.BAROSTAT_K,
            _lib.BAROSTAT_W, _lib.BAROSTAT_CLOSE, _lib.BAROSTAT_OPEN] + [_lib.BAROSTAT_COUPLE[c] for c in ("none", "xy", "xz", "yz", "xyz")]
    assert got[1 + len(fields):] == want + [_lib.THERMO_NSUMS]
    assert (ref.CLOSE, ref.OPEN) == (_lib.BAROSTAT_CLOSE, _lib.BAROSTAT_OPEN) and ref.COUPLE == _lib.BAROSTAT_COUPLE
    # the slots do not overlap: three each for nu, alpha, lambda, b and P
    slots = [s + k for s in want[1:5] + [want[8]] for k in range(3)] + want[5:8] + want[9:13]
    assert len(set(slots)) == len(slots) and max(slots) < _lib.BAROSTAT_NSTATE


def test_abi_barostat_symbols_and_arguments():
    lib = _lib.lib()
    buf = (C.c_double * 32)()

    def args(**kw):
        a = _lib.BarostatArgs()
        a.N, a.dt, a.tauS, a.ndof, a.box_dof, a.phase = 4, DT, 1.0, 9.0, 7, _lib.BAROSTAT_OPEN
        a.S[:] = (1.0, 1.0, 1.0)
        a.box = _lib.make_box((6.0, 7.0, 8.0))
        for name in ("d_pos", "d_vel", "d_net_force", "d_image", "d_state", "d_sums"):
            setattr(a, name, C.addressof(buf))
        for k, v in kw.items():
            if k == "S":
                a.S[:] = v
            else:
                setattr(a, k, v)
        return a

    # every refusal comes ahead of the launch (the pointers are never followed)
    common = [dict(N=0), dict(dt=0.0), dict(dt=-1.0), dict(d_state=None), dict(box_dof=8),
              dict(box=_lib.make_box((6.0, 7.0, 8.0), tilt=(0.1, 0.0, 0.0))), dict(box=_lib.make_box((6.0, 7.0, 8.0), tilt=(0.0, 0.0, -0.2))),
              dict(box=_lib.make_box((6.0, 7.0, 8.0), periodic=(1, 0, 1))), dict(box=_lib.make_box((6.0, 0.0, 8.0)))]
    per_entry = {
        "azp_barostat_advance": [dict(d_sums=None), dict(tauS=0.0), dict(tauS=-1.0), dict(ndof=2.0), dict(couple=5), dict(phase=0),
                                 dict(phase=4), dict(S=(1.0, float("nan"), 1.0)),
                                 # with a thermostat, what its own advance refuses
                                 dict(d_thermostat_state=C.addressof(buf), thermostat_kind=3, thermostat_kT=1.0, thermostat_tau=1.0),
                                 dict(d_thermostat_state=C.addressof(buf), thermostat_kind=_lib.THERMOSTAT_MTTK, thermostat_kT=0.0,
                                      thermostat_tau=1.0),
                                 dict(d_thermostat_state=C.addressof(buf), thermostat_kind=_lib.THERMOSTAT_MTTK, thermostat_kT=1.0,
                                      thermostat_tau=0.0),
                                 dict(d_thermostat_state=C.addressof(buf), thermostat_kind=_lib.THERMOSTAT_BERENDSEN, thermostat_kT=1.0,
                                      thermostat_tau=0.5 * DT)],
        "azp_barostat_step_one": [dict(d_pos=None), dict(d_vel=None), dict(d_net_force=None)],
        "azp_barostat_step_two": [dict(d_vel=None), dict(d_net_force=None)],
    }
    for name, bad in per_entry.items():
        fn = getattr(lib, name)
        assert fn(None, None) == -1  # AZP_ERROR_INVALID_ARGUMENT, no launch
        assert fn(C.byref(_lib.BarostatArgs()), None) == -1
        for kw in common + bad:
            assert fn(C.byref(args(**kw)), None) == -1, (name, kw)


# ---------------------------------------------------------------------------
# the reference on its own
# ---------------------------------------------------------------------------
def _liquid(**kw):
    pos, vel, L = ref.jittered_lattice(5, 0.8, seed=23)
    return ref.System(pos, vel, L, DT, **kw)


def test_reference_is_time_reversible():
    """100 steps forward, v and nu negated, 100 steps back: positions (minimum image), velocities, box and nu return
    within 1e-10 (measured 4e-13 to 7e-13 with glibc; the margin allows for another libm)."""
    s = _liquid(S=(1.0, 2.0, 3.0), tauS=1.0, couple="none")
    pos0, vel0, L0 = s.pos.copy(), s.vel.copy(), list(s.L)
    s.run(100)
    assert max(abs(x) for x in s.state["nu"]) > 1e-3 and max(abs(a / b - 1.0) for a, b in zip(s.L, L0)) > 1e-4  # it acted
    assert len({round(x, 6) for x in s.L}) == 3  # each axis its own way
    s.vel = -s.vel
    s.state = ref.new_state(nu=[-x for x in s.state["nu"]], ref_kT=s.state["ref_kT"])
    s.run(100)
    d = s.pos - pos0
    d -= np.asarray(L0) * np.rint(d / np.asarray(L0))
    worst = max(np.abs(d).max(), np.abs(s.vel + vel0).max(), max(abs(a - b) for a, b in zip(s.L, L0)),
                max(abs(x) for x in s.state["nu"]))
    print("returned to the start within %.3g" % worst)
    assert worst <= 1e-10


def test_reference_conserves_its_energy():
    """K + U + S V + the barostat's energy drifts at most 1.25 times what K + U of plain velocity Verlet drifts in the same
    arithmetic over the same steps (measured: a ratio of 1.00 to 1.01)."""
    steps, every = 1000, 10
    drift = {}
    for name, kw in (("nve", dict()), ("nph", dict(S=(2.86, 2.86, 2.86), tauS=1.0, couple="xyz"))):
        s = _liquid(**kw)
        E = [s.conserved()]
        for _ in range(steps // every):
            s.run(every)
            E.append(s.conserved())
        E = np.array(E)
        drift[name] = np.abs(E - E[0]).max()
        if name == "nph":
            assert abs(s.volume / np.prod(_liquid().L) - 1.0) > 1e-3  # the box did move
    print("drift of the conserved quantity: NPH %.4g, NVE %.4g, ratio %.3f" % (drift["nph"], drift["nve"], drift["nph"] / drift["nve"]))
    assert drift["nve"] > 0.0
    assert drift["nph"] <= 1.25 * drift["nve"]


def test_reference_couplings():
    def bits(x):
        return np.float64(x).view(np.int64)

    s = _liquid(S=(1.0, 2.0, 3.0), tauS=1.0, couple="xyz")
    s.run(20)
    nu = s.state["nu"]
    assert nu[0] != 0.0 and bits(nu[0]) == bits(nu[1]) == bits(nu[2])
    s = _liquid(S=(1.0, 2.0, 3.0), tauS=1.0, couple="xy")
    s.run(20)
    nu = s.state["nu"]
    assert bits(nu[0]) == bits(nu[1]) and nu[2] != nu[0]
    for frozen in range(3):
        dof = tuple(a != frozen for a in range(3))
        s = _liquid(S=(1.0, 2.0, 3.0), tauS=1.0, couple="none", box_dof=dof)
        L0 = list(s.L)
        s.run(20)
        for a in range(3):
            if a == frozen:
                assert bits(s.state["nu"][a]) == bits(0.0) and bits(s.L[a]) == bits(L0[a])
            else:
                assert s.state["nu"][a] != 0.0 and s.L[a] != L0[a]
    # a frozen axis inside a coupled set: the free ones share the mean of their own G
    s = _liquid(S=(1.0, 2.0, 3.0), tauS=1.0, couple="xyz", box_dof=(True, False, True))
    L0 = list(s.L)
    s.run(5)
    nu = s.state["nu"]
    assert bits(nu[0]) == bits(nu[2]) and nu[0] != 0.0 and bits(nu[1]) == bits(0.0) and bits(s.L[1]) == bits(L0[1])


def test_reference_sinhc_and_advance_identities():
    """s(x) is sinh(x) / x to the last bits for |x| <= 0.1; close|open equals close then open bit for bit; b -> dt and
    lambda, alpha -> 1 for nu = 0."""
    import math

    for x in np.linspace(-0.1, 0.1, 41):
        want = math.sinh(x) / x if x else 1.0
        assert abs(ref.sinhc(float(x)) - want) <= 2.0 ** -52
    assert 0.1 ** 10 / 39916800.0 < 2.0 ** -53  # the first term left out, at the edge of the range
    rng = np.random.default_rng(5)
    row = rng.uniform(0.5, 2.0, 20) * 100.0
    L, S = (6.0, 7.0, 8.0), (1.0, 2.0, 3.0)
    s0 = ref.new_state(nu=(0.1, -0.2, 0.05), ref_kT=1.0)
    both = ref.advance(row, L, S, DT, 1.0, 93.0, "xy", (True, True, True), ref.CLOSE | ref.OPEN, s0)
    two = ref.advance(row, L, S, DT, 1.0, 93.0, "xy", (True, True, True), ref.OPEN,
                      ref.advance(row, L, S, DT, 1.0, 93.0, "xy", (True, True, True), ref.CLOSE, s0))
    for key in ("nu", "alpha", "lam", "b", "energy"):
        assert both[key] == two[key]
    row[[4, 7, 9, 10, 13, 15]] = 0.0
    rest = ref.advance(row, L, (0.0, 0.0, 0.0), DT, 1.0, 93.0, "none", (True, True, True), ref.OPEN, ref.new_state(ref_kT=1.0))
    assert rest["nu"] == (0.0, 0.0, 0.0) and rest["lam"] == (1.0,) * 3 and rest["alpha"] == (1.0,) * 3 and rest["b"] == (DT,) * 3
