"""The step loop of ``Simulation.run`` without a GPU: what it calls, in which order and with which scalars, for every
integration path. The state is a stand-in of CPU tensors, the forces, the writer, the updater, the tuner and the domain
record what is asked of them, and libazp is wrapped so that every entry point that takes a stream is recorded instead of
called. The event logs in ``EXPECTED`` were recorded with this harness from the separate loops that NVE, thermostatted,
FIRE and flow runs had before they shared one; the one loop has to reproduce them exactly."""

import ctypes as C
import warnings

import pytest
import torch

from azplugins_amd import _lib

N = 6
DT = 0.005
PATHS = ["nve", "nve_rot", "nve_domain", "bussi", "fire", "langevin", "langevin_brownian", "nph", "npt_bussi"]
LAMBDA = (1.25, 1.0, 0.8)  # the scale factors every opening barostat advance "computes": the box changes every step


def _kT(log):
    def kT(t):
        log.append("kT(%d)" % t)
        return 1.0 + 0.125 * t

    return kT


def _S(log):
    def S(t):
        log.append("S(%d)" % t)
        return 0.5 + 0.25 * t

    return S


class _State:
    """What the driver and the methods' host code touch of ``State``."""

    def __init__(self):
        from azplugins_amd.state import Box

        f64 = torch.float64
        self.device = torch.device("cpu")
        self.N, self.n_ghost = N, 0
        self.types = ["A", "B"]
        self.box = Box.cube(8.0)
        self.pos = torch.zeros((N, 4), dtype=f64)
        self.vel = torch.zeros((N, 4), dtype=f64)
        self.vel[:, 3] = 1.0
        self.net_force = torch.zeros((N, 4), dtype=f64)
        self.image = torch.zeros((N, 3), dtype=torch.int32)
        self.tag = torch.arange(N, dtype=torch.int32)
        self.orientation = torch.zeros((N, 4), dtype=f64)
        self.angmom = torch.zeros((N, 4), dtype=f64)
        self.inertia = torch.ones((N, 3), dtype=f64)
        self.accel = None
        self.groups = {}
        self.position_generation = self.order_generation = self.type_generation = self.box_generation = 0

    @property
    def n_max(self):
        return self.N + self.n_ghost

    def set_box(self, box):
        """As ``State.set_box``: a box that differs bumps ``box_generation`` and ``position_generation``."""
        if box == self.box:
            return
        self.box = box
        self.box_generation += 1
        self.position_generation += 1


class _Nlist:
    """The neighbor list of the first force: says whether the domain's hooks were wired when it is brought up to date."""

    sort_wanted = False
    reduce_flag = before_rebuild = None

    def __init__(self, log):
        self._log = log

    def compute(self, state):
        self._log.append("nlist.compute wired=%s" % (self.reduce_flag is not None and self.before_rebuild is not None))

    def particles_sorted(self):
        self._log.append("nlist.particles_sorted")


class _Force:
    defer_flag_check = False
    compute_virial = False
    _virial_evaluated = False
    _state = None

    def __init__(self, log, name, with_nlist=False):
        self._log, self._name = log, name
        self.force_tensor = self._force = torch.zeros((N, 4), dtype=torch.float64)
        self._virial = torch.zeros((6, N), dtype=torch.float64)
        self.torque_tensor = torch.zeros((N, 4), dtype=torch.float64)
        if with_nlist:
            self.nlist = _Nlist(log)

    def _attach(self, sim):
        self._state = sim.state

    def compute(self, timestep):
        self._log.append("%s.compute(%d) deferred=%s" % (self._name, timestep, self.defer_flag_check))

    def check_flags(self, wait=True):
        self._log.append("%s.check_flags(wait=%s) deferred=%s" % (self._name, wait, self.defer_flag_check))


class _Tuner:
    last_sort_step = None

    def __init__(self, log, period):
        self._log, self.trigger_period = log, period

    def sort(self, sim):
        self._log.append("sort(%d)" % sim.timestep)
        st = sim.state
        for name in ("pos", "vel", "image"):  # (a sort or a migration replaces the arrays)
            setattr(st, name, getattr(st, name).clone())


class _Domain:
    names = ["pos", "vel", "tag", "image"]

    def __init__(self, log):
        self._log = log

    def all_reduce_flag(self, flag):
        return flag

    def exchange(self, fields):
        self._log.append("exchange(%s)" % ",".join(fields))


class _Lib:
    """libazp with every launch recorded instead of made: host-only calls pass through, an entry point that takes a
    stream returns 0 after its name and the scalars of its argument struct went into the log, marked STALE if the
    struct does not point at the state's arrays of that moment. The barostat's entries also log their phase and the box
    lengths of their struct (a launch with a stale box shows), and an opening advance writes ``LAMBDA`` into the state
    tensor, as the kernel would; the sums pass logs how many forces and virials it was pointed at."""

    state = None

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        real = getattr(self._real, name)
        if name.endswith("_size") or name == "azp_status_string":
            fn = real
        else:
            log = self._log

            def fn(*args):
                a = getattr(args[0], "_obj", None)
                if a is None:  # azp_sum_forces(N, count, ...)
                    log.append("%s N=%d" % (name, args[0]))
                else:
                    st = self.state
                    # (the sums pass of an All() filter reads no positions: its d_pos stays null)
                    arrays = ("vel",) if name == "azp_thermo_sums" else ("pos", "vel", "image", "net_force")
                    stale = any(getattr(a, "d_" + f) != getattr(st, f).data_ptr() for f in arrays if hasattr(a, "d_" + f))
                    extra = ""
                    if name == "azp_thermo_sums":
                        extra = " n_forces=%d virials=%d" % (a.n_forces, sum(1 for k in range(a.n_forces) if a.d_virial[k]))
                    elif name.startswith("azp_barostat_"):
                        extra = " phase=%d L=%r" % (a.phase, tuple(a.box.L))
                        if name == "azp_barostat_advance" and a.phase & _lib.BAROSTAT_OPEN:
                            (C.c_double * 3).from_address(a.d_state + 8 * _lib.BAROSTAT_LAMBDA)[:] = LAMBDA
                    log.append(name + "".join(" %s=%r" % (f, getattr(a, f)) for f in ("timestep", "kT", "dt", "N") if hasattr(a, f))
                               + extra + (" STALE" if stale else ""))
                return 0

        self.__dict__[name] = fn
        return fn


def make_sim(path, monkeypatch, seed=1, writer=3, updater=4, tuner=5):
    """A simulation of ``path`` on the stand-ins; returns it with its event log."""
    import azplugins_amd as azp
    from azplugins_amd import compute, flow, minimize, thermostats, update

    log = []
    recording = _Lib(_lib.lib(), log)
    monkeypatch.setattr(_lib, "lib", lambda: recording)
    monkeypatch.setattr(_lib, "raw_stream", lambda device: 0)

    class Writer(compute._Recorder):
        _compute = compute.VelocityCompute()

        def _record(self, sim, timestep):
            log.append("writer(%d)" % timestep)

    class Updater(update._Updater):
        def _update(self, sim, timestep):
            log.append("updater(%d)" % timestep)

    sim = azp.Simulation(device="cpu", seed=seed)
    sim.state = recording.state = _State()
    forces = [_Force(log, "f0", with_nlist=True), _Force(log, "f1")]
    u = flow.ConstantFlow(velocity=(1, 0, 0))
    rot = path == "nve_rot"
    if path in ("nve", "nve_rot", "nve_domain"):
        methods = [azp.ConstantVolume(azp.All())]
    elif path == "bussi":
        methods = [azp.ConstantVolume(azp.All(), thermostats.Bussi(kT=_kT(log), tau=0.5))]
    elif path == "langevin":
        methods = [flow.Langevin(filter=azp.All(), kT=_kT(log), flow_field=u)]
    elif path == "langevin_brownian":
        methods = [flow.Langevin(filter=azp.Type("A"), kT=_kT(log), flow_field=u),
                   flow.Brownian(filter=azp.Type("B"), kT=2.0, flow_field=u)]
    elif path in ("nph", "npt_bussi"):
        th = thermostats.Bussi(kT=_kT(log), tau=0.5) if path == "npt_bussi" else None
        methods = [azp.ConstantPressure(azp.All(), S=_S(log), tauS=1.0, couple="xyz", thermostat=th)]
    if path == "fire":
        integ = minimize.FIRE(dt=DT, force_tol=1e-3, angmom_tol=1e-3, energy_tol=1e-7, forces=forces,
                              methods=[azp.ConstantVolume(azp.All())])
    else:
        integ = azp.Integrator(dt=DT, forces=forces, methods=methods, integrate_rotational_dof=rot)
    sim.operations.integrator = integ
    sim.operations.tuners[:] = [_Tuner(log, tuner)]
    if path == "nve_domain":
        sim.domain = _Domain(log)
        sim.operations.tuners.clear()  # (as attach_domain does)
    if writer:
        sim.operations.add(Writer._compute)
        sim.operations.add(Writer(writer))
    if updater:
        sim.operations.add(Updater(updater))
    return sim, log


def _events(path, runs, monkeypatch):
    sim, log = make_sim(path, monkeypatch)
    for steps in runs:
        log.append("run(%d)" % steps)
        sim.run(steps)
    log.append("timestep=%d position_generation=%d type_generation=%d"
               % (sim.timestep, sim.state.position_generation, sim.state.type_generation))
    if path in ("nph", "npt_bussi"):
        log.append("box_generation=%d" % sim.state.box_generation)
    return log


SCENARIOS = {"run0": (0,), "run1": (1,), "run7_run5": (7, 5)}


@pytest.mark.parametrize("scenario", sorted(SCENARIOS))
@pytest.mark.parametrize("path", PATHS)
def test_event_log(path, scenario, monkeypatch):
    got = _events(path, SCENARIOS[scenario], monkeypatch)
    want = EXPECTED[path, scenario].strip().split("\n")
    assert not any(e.endswith("STALE") for e in got)  # every launch is pointed at the arrays of its moment
    assert got == want


# ---------------------------------------------------------------------------
# the order of the refusals
# ---------------------------------------------------------------------------
def _computes(log):
    return [e for e in log if ".compute(" in e and not e.startswith("nlist")]


def test_no_methods_and_malformed_methods(monkeypatch):
    import azplugins_amd as azp

    sim, log = make_sim("nve", monkeypatch)
    sim.operations.integrator.methods = []
    sim.run(0)
    sim.run(3)  # (an integrator without methods evaluates the forces and returns)
    assert len(_computes(log)) == 4 and not any(e.startswith("azp_integrate") for e in log) and sim.timestep == 0
    sim, log = make_sim("nve", monkeypatch)
    sim.operations.integrator.methods = [azp.ConstantVolume(), azp.ConstantVolume()]
    sim.run(0)  # a malformed list is refused only when it would have to step
    assert len(_computes(log)) == 2
    with pytest.raises(_lib.AzpError, match="exactly one ConstantVolume"):
        sim.run(1)
    assert len(_computes(log)) == 4 and not any(e.startswith("azp_integrate") for e in log)
    assert not any(f.defer_flag_check for f in sim.operations.integrator.forces)


@pytest.mark.parametrize("path", ["langevin", "fire", "nph", "npt_bussi"])
def test_flow_and_fire_checks_come_first_even_at_zero_steps(path, monkeypatch):
    """(the barostat's refusals too come ahead of the forces, even at ``run(0)``)"""
    sim, log = make_sim(path, monkeypatch)
    sim.operations.integrator.integrate_rotational_dof = True
    with pytest.raises(_lib.AzpError, match="rotational"):
        sim.run(0)
    assert log == []


def test_thermostat_refusals_and_seed_warning_follow_the_first_forces(monkeypatch):
    sim, log = make_sim("bussi", monkeypatch)
    sim.operations.integrator.integrate_rotational_dof = True
    sim.run(0)  # nothing is refused where nothing is stepped
    assert len(_computes(log)) == 2
    with pytest.raises(_lib.AzpError, match="rotational"):
        sim.run(1)
    assert len(_computes(log)) == 4 and not any(e.startswith("azp_thermostat") for e in log)
    # the seed warning: after the forces, ahead of the kinetic pass
    sim, log = make_sim("bussi", monkeypatch, seed=None)
    with warnings.catch_warnings():
        warnings.simplefilter("always")
        monkeypatch.setattr(warnings, "showwarning", lambda message, *a, **k: log.append("warning: %s" % message))
        sim.run(1)
    k = [i for i, e in enumerate(log) if e.startswith("warning")]
    assert len(k) == 1 and "seed" in log[k[0]] and sim.seed == 0
    assert log[k[0] - 1].startswith("azp_sum_forces") and log[k[0] + 1].startswith("azp_thermostat_kinetic")


def test_barostat_refusals_name_it_and_its_seed_warning_follows_the_first_forces(monkeypatch):
    import azplugins_amd as azp

    for path in ("nph", "npt_bussi"):
        sim, log = make_sim(path, monkeypatch)
        sim.operations.integrator.methods.append(azp.ConstantVolume())
        with pytest.raises(_lib.AzpError, match="only method"):
            sim.run(0)
        assert log == []
    # a thermostat's own refusal (held by two methods) comes from the barostat's check: ahead of the forces, at run(0)
    sim, log = make_sim("npt_bussi", monkeypatch)
    other = azp.ConstantVolume(thermostat=sim.operations.integrator.methods[0].thermostat)  # (held weakly: keep it)
    with pytest.raises(_lib.AzpError, match="two methods"):
        sim.run(0)
    assert log == [] and other.thermostat is not None
    # the seed warning: after the forces, ahead of the first sums pass
    sim, log = make_sim("npt_bussi", monkeypatch, seed=None)
    with warnings.catch_warnings():
        warnings.simplefilter("always")
        monkeypatch.setattr(warnings, "showwarning", lambda message, *a, **k: log.append("warning: %s" % message))
        sim.run(0)
        assert not any(e.startswith("warning") for e in log)
        sim.run(1)
    k = [i for i, e in enumerate(log) if e.startswith("warning")]
    assert len(k) == 1 and "seed" in log[k[0]] and sim.seed == 0
    assert log[k[0] - 1].startswith("azp_sum_forces") and not any(e.startswith(("azp_thermo", "azp_barostat")) for e in log[: k[0]])
    assert any(e.startswith("azp_thermo_sums") for e in log[k[0]:])


def test_flow_seed_warning_follows_the_first_forces(monkeypatch):
    sim, log = make_sim("langevin", monkeypatch, seed=None)
    with warnings.catch_warnings():
        warnings.simplefilter("always")
        monkeypatch.setattr(warnings, "showwarning", lambda message, *a, **k: log.append("warning: %s" % message))
        sim.run(0)
        assert not any(e.startswith("warning") for e in log)
        sim.run(1)
    k = [i for i, e in enumerate(log) if e.startswith("warning")]
    assert len(k) == 1 and log[k[0] - 1].startswith("azp_sum_forces")
    assert not any(e.startswith("azp_integrate") for e in log[: k[0]]) and any(e.startswith("azp_integrate") for e in log[k[0]:])
    assert sim.state.accel is not None and sim.state.accel.shape == (N, 4)


def test_domain_is_wired_before_the_first_forces(monkeypatch):
    sim, log = make_sim("nve_domain", monkeypatch)
    sim.run(0)
    assert log[0] == "nlist.compute wired=True"


def test_private_helpers_stay(monkeypatch):
    sim, _ = make_sim("nve_domain", monkeypatch)
    for name in ("_check_thermostat", "_check_flow_methods", "_check_writers", "_updaters_due", "_halo_fields", "_warn_if_seed_unset"):
        assert callable(getattr(sim, name))
    assert sim._halo_fields() == ["pos"]
    assert [type(u).__name__ for u in sim._updaters_due()] == ["Updater"]


# ---------------------------------------------------------------------------
# a run that raises
# ---------------------------------------------------------------------------
class _Boom(Exception):
    pass


@pytest.mark.parametrize("path", PATHS)
def test_a_raising_updater_leaves_no_force_deferring(path, monkeypatch):
    """An updater that raises at step 3: its own exception comes out of ``run`` (the final flag check does not run, so
    it cannot mask it) and no force is left deferring its flag check: a direct ``compute()`` afterwards examines its flag
    at once again."""
    from azplugins_amd import update

    class Raises(update._Updater):
        def _update(self, sim, timestep):
            if timestep == 3:
                raise _Boom("at %d" % timestep)

    sim, log = make_sim(path, monkeypatch)
    sim.operations.add(Raises(1))
    with pytest.raises(_Boom, match="at 3"):
        sim.run(7)
    assert sim.timestep == 3
    forces = sim.operations.integrator.forces
    assert [f.defer_flag_check for f in forces] == [False, False]
    assert "f0.compute(3) deferred=True" in log  # (inside the run the checks were deferred)
    assert not any("check_flags" in e for e in log)


EXPECTED = {
    ('nve', 'run0'): """
run(0)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
timestep=0 position_generation=0 type_generation=0
""",
    ('nve', 'run1'): """
run(1)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
updater(0)
azp_integrate_nve_step_one dt=0.005 N=6
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=1 position_generation=1 type_generation=1
""",
    ('nve', 'run7_run5'): """
run(7)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
updater(0)
azp_integrate_nve_step_one dt=0.005 N=6
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
f0.compute(2) deferred=True
f1.compute(2) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
f0.compute(3) deferred=True
f1.compute(3) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
writer(3)
azp_integrate_nve_step_one dt=0.005 N=6
f0.compute(4) deferred=True
f1.compute(4) deferred=True
azp_sum_forces N=6
updater(4)
azp_integrate_nve_step_two_one dt=0.005 N=6
sort(5)
nlist.particles_sorted
f0.compute(5) deferred=True
f1.compute(5) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
f0.compute(6) deferred=True
f1.compute(6) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
writer(6)
azp_integrate_nve_step_one dt=0.005 N=6
f0.compute(7) deferred=True
f1.compute(7) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
run(5)
f0.compute(7) deferred=False
f1.compute(7) deferred=False
azp_sum_forces N=6
azp_integrate_nve_step_one dt=0.005 N=6
f0.compute(8) deferred=True
f1.compute(8) deferred=True
azp_sum_forces N=6
updater(8)
azp_integrate_nve_step_two_one dt=0.005 N=6
f0.compute(9) deferred=True
f1.compute(9) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
writer(9)
azp_integrate_nve_step_one dt=0.005 N=6
sort(10)
nlist.particles_sorted
f0.compute(10) deferred=True
f1.compute(10) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
f0.compute(11) deferred=True
f1.compute(11) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
f0.compute(12) deferred=True
f1.compute(12) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
writer(12)
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=12 position_generation=12 type_generation=3
""",
    ('nve_rot', 'run0'): """
run(0)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
timestep=0 position_generation=0 type_generation=0
""",
    ('nve_rot', 'run1'): """
run(1)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
updater(0)
azp_integrate_nve_step_one dt=0.005 N=6
azp_integrate_nve_rot_step_one dt=0.005 N=6
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
azp_integrate_nve_rot_step_two dt=0.005 N=6
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=1 position_generation=1 type_generation=1
""",
    ('nve_rot', 'run7_run5'): """
run(7)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
updater(0)
azp_integrate_nve_step_one dt=0.005 N=6
azp_integrate_nve_rot_step_one dt=0.005 N=6
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
azp_integrate_nve_rot_step_two dt=0.005 N=6
azp_integrate_nve_rot_step_one dt=0.005 N=6
f0.compute(2) deferred=True
f1.compute(2) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
azp_integrate_nve_rot_step_two dt=0.005 N=6
azp_integrate_nve_rot_step_one dt=0.005 N=6
f0.compute(3) deferred=True
f1.compute(3) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
azp_integrate_nve_rot_step_two dt=0.005 N=6
writer(3)
azp_integrate_nve_step_one dt=0.005 N=6
azp_integrate_nve_rot_step_one dt=0.005 N=6
f0.compute(4) deferred=True
f1.compute(4) deferred=True
azp_sum_forces N=6
updater(4)
azp_integrate_nve_step_two_one dt=0.005 N=6
azp_integrate_nve_rot_step_two dt=0.005 N=6
azp_integrate_nve_rot_step_one dt=0.005 N=6
sort(5)
nlist.particles_sorted
f0.compute(5) deferred=True
f1.compute(5) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
azp_integrate_nve_rot_step_two dt=0.005 N=6
azp_integrate_nve_rot_step_one dt=0.005 N=6
f0.compute(6) deferred=True
f1.compute(6) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
azp_integrate_nve_rot_step_two dt=0.005 N=6
writer(6)
azp_integrate_nve_step_one dt=0.005 N=6
azp_integrate_nve_rot_step_one dt=0.005 N=6
f0.compute(7) deferred=True
f1.compute(7) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
azp_integrate_nve_rot_step_two dt=0.005 N=6
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
run(5)
f0.compute(7) deferred=False
f1.compute(7) deferred=False
azp_sum_forces N=6
azp_integrate_nve_step_one dt=0.005 N=6
azp_integrate_nve_rot_step_one dt=0.005 N=6
f0.compute(8) deferred=True
f1.compute(8) deferred=True
azp_sum_forces N=6
updater(8)
azp_integrate_nve_step_two_one dt=0.005 N=6
azp_integrate_nve_rot_step_two dt=0.005 N=6
azp_integrate_nve_rot_step_one dt=0.005 N=6
f0.compute(9) deferred=True
f1.compute(9) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
azp_integrate_nve_rot_step_two dt=0.005 N=6
writer(9)
azp_integrate_nve_step_one dt=0.005 N=6
azp_integrate_nve_rot_step_one dt=0.005 N=6
sort(10)
nlist.particles_sorted
f0.compute(10) deferred=True
f1.compute(10) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
azp_integrate_nve_rot_step_two dt=0.005 N=6
azp_integrate_nve_rot_step_one dt=0.005 N=6
f0.compute(11) deferred=True
f1.compute(11) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
azp_integrate_nve_rot_step_two dt=0.005 N=6
azp_integrate_nve_rot_step_one dt=0.005 N=6
f0.compute(12) deferred=True
f1.compute(12) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
azp_integrate_nve_rot_step_two dt=0.005 N=6
writer(12)
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=12 position_generation=12 type_generation=3
""",
    ('nve_domain', 'run0'): """
run(0)
nlist.compute wired=True
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
timestep=0 position_generation=0 type_generation=0
""",
    ('nve_domain', 'run1'): """
run(1)
nlist.compute wired=True
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
updater(0)
azp_integrate_nve_step_one dt=0.005 N=6
exchange(pos)
nlist.compute wired=True
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=1 position_generation=1 type_generation=1
""",
    ('nve_domain', 'run7_run5'): """
run(7)
nlist.compute wired=True
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
updater(0)
azp_integrate_nve_step_one dt=0.005 N=6
exchange(pos)
nlist.compute wired=True
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
exchange(pos)
nlist.compute wired=True
f0.compute(2) deferred=True
f1.compute(2) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
exchange(pos)
nlist.compute wired=True
f0.compute(3) deferred=True
f1.compute(3) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
writer(3)
azp_integrate_nve_step_one dt=0.005 N=6
exchange(pos)
nlist.compute wired=True
f0.compute(4) deferred=True
f1.compute(4) deferred=True
azp_sum_forces N=6
updater(4)
azp_integrate_nve_step_two_one dt=0.005 N=6
exchange(pos)
nlist.compute wired=True
f0.compute(5) deferred=True
f1.compute(5) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
exchange(pos)
nlist.compute wired=True
f0.compute(6) deferred=True
f1.compute(6) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
writer(6)
azp_integrate_nve_step_one dt=0.005 N=6
exchange(pos)
nlist.compute wired=True
f0.compute(7) deferred=True
f1.compute(7) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
run(5)
nlist.compute wired=True
f0.compute(7) deferred=False
f1.compute(7) deferred=False
azp_sum_forces N=6
azp_integrate_nve_step_one dt=0.005 N=6
exchange(pos)
nlist.compute wired=True
f0.compute(8) deferred=True
f1.compute(8) deferred=True
azp_sum_forces N=6
updater(8)
azp_integrate_nve_step_two_one dt=0.005 N=6
exchange(pos)
nlist.compute wired=True
f0.compute(9) deferred=True
f1.compute(9) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
writer(9)
azp_integrate_nve_step_one dt=0.005 N=6
exchange(pos)
nlist.compute wired=True
f0.compute(10) deferred=True
f1.compute(10) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
exchange(pos)
nlist.compute wired=True
f0.compute(11) deferred=True
f1.compute(11) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two_one dt=0.005 N=6
exchange(pos)
nlist.compute wired=True
f0.compute(12) deferred=True
f1.compute(12) deferred=True
azp_sum_forces N=6
azp_integrate_nve_step_two dt=0.005 N=6
writer(12)
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=12 position_generation=12 type_generation=3
""",
    ('bussi', 'run0'): """
run(0)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
timestep=0 position_generation=0 type_generation=0
""",
    ('bussi', 'run1'): """
run(1)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
azp_thermostat_kinetic timestep=0 kT=0.0 dt=0.005 N=6
updater(0)
kT(0)
azp_thermostat_advance timestep=0 kT=1.0 dt=0.005 N=6
azp_thermostat_step_one timestep=0 kT=1.0 dt=0.005 N=6
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
azp_thermostat_step_two timestep=0 kT=1.0 dt=0.005 N=6
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=1 position_generation=1 type_generation=1
""",
    ('bussi', 'run7_run5'): """
run(7)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
azp_thermostat_kinetic timestep=0 kT=0.0 dt=0.005 N=6
updater(0)
kT(0)
azp_thermostat_advance timestep=0 kT=1.0 dt=0.005 N=6
azp_thermostat_step_one timestep=0 kT=1.0 dt=0.005 N=6
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
azp_thermostat_step_two timestep=0 kT=1.0 dt=0.005 N=6
kT(1)
azp_thermostat_advance timestep=1 kT=1.125 dt=0.005 N=6
azp_thermostat_step_one timestep=1 kT=1.125 dt=0.005 N=6
f0.compute(2) deferred=True
f1.compute(2) deferred=True
azp_sum_forces N=6
azp_thermostat_step_two timestep=1 kT=1.125 dt=0.005 N=6
kT(2)
azp_thermostat_advance timestep=2 kT=1.25 dt=0.005 N=6
azp_thermostat_step_one timestep=2 kT=1.25 dt=0.005 N=6
f0.compute(3) deferred=True
f1.compute(3) deferred=True
azp_sum_forces N=6
azp_thermostat_step_two timestep=2 kT=1.25 dt=0.005 N=6
writer(3)
kT(3)
azp_thermostat_advance timestep=3 kT=1.375 dt=0.005 N=6
azp_thermostat_step_one timestep=3 kT=1.375 dt=0.005 N=6
f0.compute(4) deferred=True
f1.compute(4) deferred=True
azp_sum_forces N=6
azp_thermostat_step_two timestep=3 kT=1.375 dt=0.005 N=6
updater(4)
kT(4)
azp_thermostat_advance timestep=4 kT=1.5 dt=0.005 N=6
azp_thermostat_step_one timestep=4 kT=1.5 dt=0.005 N=6
sort(5)
nlist.particles_sorted
f0.compute(5) deferred=True
f1.compute(5) deferred=True
azp_sum_forces N=6
azp_thermostat_step_two timestep=4 kT=1.5 dt=0.005 N=6
kT(5)
azp_thermostat_advance timestep=5 kT=1.625 dt=0.005 N=6
azp_thermostat_step_one timestep=5 kT=1.625 dt=0.005 N=6
f0.compute(6) deferred=True
f1.compute(6) deferred=True
azp_sum_forces N=6
azp_thermostat_step_two timestep=5 kT=1.625 dt=0.005 N=6
writer(6)
kT(6)
azp_thermostat_advance timestep=6 kT=1.75 dt=0.005 N=6
azp_thermostat_step_one timestep=6 kT=1.75 dt=0.005 N=6
f0.compute(7) deferred=True
f1.compute(7) deferred=True
azp_sum_forces N=6
azp_thermostat_step_two timestep=6 kT=1.75 dt=0.005 N=6
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
run(5)
f0.compute(7) deferred=False
f1.compute(7) deferred=False
azp_sum_forces N=6
azp_thermostat_kinetic timestep=0 kT=0.0 dt=0.005 N=6
kT(7)
azp_thermostat_advance timestep=7 kT=1.875 dt=0.005 N=6
azp_thermostat_step_one timestep=7 kT=1.875 dt=0.005 N=6
f0.compute(8) deferred=True
f1.compute(8) deferred=True
azp_sum_forces N=6
azp_thermostat_step_two timestep=7 kT=1.875 dt=0.005 N=6
updater(8)
kT(8)
azp_thermostat_advance timestep=8 kT=2.0 dt=0.005 N=6
azp_thermostat_step_one timestep=8 kT=2.0 dt=0.005 N=6
f0.compute(9) deferred=True
f1.compute(9) deferred=True
azp_sum_forces N=6
azp_thermostat_step_two timestep=8 kT=2.0 dt=0.005 N=6
writer(9)
kT(9)
azp_thermostat_advance timestep=9 kT=2.125 dt=0.005 N=6
azp_thermostat_step_one timestep=9 kT=2.125 dt=0.005 N=6
sort(10)
nlist.particles_sorted
f0.compute(10) deferred=True
f1.compute(10) deferred=True
azp_sum_forces N=6
azp_thermostat_step_two timestep=9 kT=2.125 dt=0.005 N=6
kT(10)
azp_thermostat_advance timestep=10 kT=2.25 dt=0.005 N=6
azp_thermostat_step_one timestep=10 kT=2.25 dt=0.005 N=6
f0.compute(11) deferred=True
f1.compute(11) deferred=True
azp_sum_forces N=6
azp_thermostat_step_two timestep=10 kT=2.25 dt=0.005 N=6
kT(11)
azp_thermostat_advance timestep=11 kT=2.375 dt=0.005 N=6
azp_thermostat_step_one timestep=11 kT=2.375 dt=0.005 N=6
f0.compute(12) deferred=True
f1.compute(12) deferred=True
azp_sum_forces N=6
azp_thermostat_step_two timestep=11 kT=2.375 dt=0.005 N=6
writer(12)
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=12 position_generation=12 type_generation=3
""",
    ('fire', 'run0'): """
run(0)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
timestep=0 position_generation=0 type_generation=0
""",
    ('fire', 'run1'): """
run(1)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
azp_fire_measure N=6
updater(0)
azp_fire_advance N=6
azp_fire_step_one N=6
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
azp_fire_step_two N=6
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=1 position_generation=1 type_generation=1
""",
    ('fire', 'run7_run5'): """
run(7)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
azp_fire_measure N=6
updater(0)
azp_fire_advance N=6
azp_fire_step_one N=6
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
azp_fire_step_two N=6
azp_fire_advance N=6
azp_fire_step_one N=6
f0.compute(2) deferred=True
f1.compute(2) deferred=True
azp_sum_forces N=6
azp_fire_step_two N=6
azp_fire_advance N=6
azp_fire_step_one N=6
f0.compute(3) deferred=True
f1.compute(3) deferred=True
azp_sum_forces N=6
azp_fire_step_two N=6
writer(3)
azp_fire_advance N=6
azp_fire_step_one N=6
f0.compute(4) deferred=True
f1.compute(4) deferred=True
azp_sum_forces N=6
azp_fire_step_two N=6
updater(4)
azp_fire_advance N=6
azp_fire_step_one N=6
sort(5)
nlist.particles_sorted
f0.compute(5) deferred=True
f1.compute(5) deferred=True
azp_sum_forces N=6
azp_fire_step_two N=6
azp_fire_advance N=6
azp_fire_step_one N=6
f0.compute(6) deferred=True
f1.compute(6) deferred=True
azp_sum_forces N=6
azp_fire_step_two N=6
writer(6)
azp_fire_advance N=6
azp_fire_step_one N=6
f0.compute(7) deferred=True
f1.compute(7) deferred=True
azp_sum_forces N=6
azp_fire_step_two N=6
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
run(5)
f0.compute(7) deferred=False
f1.compute(7) deferred=False
azp_sum_forces N=6
azp_fire_measure N=6
azp_fire_advance N=6
azp_fire_step_one N=6
f0.compute(8) deferred=True
f1.compute(8) deferred=True
azp_sum_forces N=6
azp_fire_step_two N=6
updater(8)
azp_fire_advance N=6
azp_fire_step_one N=6
f0.compute(9) deferred=True
f1.compute(9) deferred=True
azp_sum_forces N=6
azp_fire_step_two N=6
writer(9)
azp_fire_advance N=6
azp_fire_step_one N=6
sort(10)
nlist.particles_sorted
f0.compute(10) deferred=True
f1.compute(10) deferred=True
azp_sum_forces N=6
azp_fire_step_two N=6
azp_fire_advance N=6
azp_fire_step_one N=6
f0.compute(11) deferred=True
f1.compute(11) deferred=True
azp_sum_forces N=6
azp_fire_step_two N=6
azp_fire_advance N=6
azp_fire_step_one N=6
f0.compute(12) deferred=True
f1.compute(12) deferred=True
azp_sum_forces N=6
azp_fire_step_two N=6
writer(12)
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=12 position_generation=12 type_generation=3
""",
    ('langevin', 'run0'): """
run(0)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
timestep=0 position_generation=0 type_generation=0
""",
    ('langevin', 'run1'): """
run(1)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
updater(0)
kT(0)
azp_integrate_langevin_flow_step_one timestep=0 kT=1.0 dt=0.005 N=6
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
kT(0)
azp_integrate_langevin_flow_step_two timestep=0 kT=1.0 dt=0.005 N=6
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=1 position_generation=1 type_generation=1
""",
    ('langevin', 'run7_run5'): """
run(7)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
updater(0)
kT(0)
azp_integrate_langevin_flow_step_one timestep=0 kT=1.0 dt=0.005 N=6
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
kT(0)
azp_integrate_langevin_flow_step_two_one timestep=0 kT=1.0 dt=0.005 N=6
f0.compute(2) deferred=True
f1.compute(2) deferred=True
azp_sum_forces N=6
kT(1)
azp_integrate_langevin_flow_step_two_one timestep=1 kT=1.125 dt=0.005 N=6
f0.compute(3) deferred=True
f1.compute(3) deferred=True
azp_sum_forces N=6
kT(2)
azp_integrate_langevin_flow_step_two timestep=2 kT=1.25 dt=0.005 N=6
writer(3)
kT(3)
azp_integrate_langevin_flow_step_one timestep=3 kT=1.375 dt=0.005 N=6
f0.compute(4) deferred=True
f1.compute(4) deferred=True
azp_sum_forces N=6
kT(3)
azp_integrate_langevin_flow_step_two timestep=3 kT=1.375 dt=0.005 N=6
updater(4)
kT(4)
azp_integrate_langevin_flow_step_one timestep=4 kT=1.5 dt=0.005 N=6
sort(5)
nlist.particles_sorted
f0.compute(5) deferred=True
f1.compute(5) deferred=True
azp_sum_forces N=6
kT(4)
azp_integrate_langevin_flow_step_two_one timestep=4 kT=1.5 dt=0.005 N=6
f0.compute(6) deferred=True
f1.compute(6) deferred=True
azp_sum_forces N=6
kT(5)
azp_integrate_langevin_flow_step_two timestep=5 kT=1.625 dt=0.005 N=6
writer(6)
kT(6)
azp_integrate_langevin_flow_step_one timestep=6 kT=1.75 dt=0.005 N=6
f0.compute(7) deferred=True
f1.compute(7) deferred=True
azp_sum_forces N=6
kT(6)
azp_integrate_langevin_flow_step_two timestep=6 kT=1.75 dt=0.005 N=6
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
run(5)
f0.compute(7) deferred=False
f1.compute(7) deferred=False
azp_sum_forces N=6
kT(7)
azp_integrate_langevin_flow_step_one timestep=7 kT=1.875 dt=0.005 N=6
f0.compute(8) deferred=True
f1.compute(8) deferred=True
azp_sum_forces N=6
kT(7)
azp_integrate_langevin_flow_step_two timestep=7 kT=1.875 dt=0.005 N=6
updater(8)
kT(8)
azp_integrate_langevin_flow_step_one timestep=8 kT=2.0 dt=0.005 N=6
f0.compute(9) deferred=True
f1.compute(9) deferred=True
azp_sum_forces N=6
kT(8)
azp_integrate_langevin_flow_step_two timestep=8 kT=2.0 dt=0.005 N=6
writer(9)
kT(9)
azp_integrate_langevin_flow_step_one timestep=9 kT=2.125 dt=0.005 N=6
sort(10)
nlist.particles_sorted
f0.compute(10) deferred=True
f1.compute(10) deferred=True
azp_sum_forces N=6
kT(9)
azp_integrate_langevin_flow_step_two_one timestep=9 kT=2.125 dt=0.005 N=6
f0.compute(11) deferred=True
f1.compute(11) deferred=True
azp_sum_forces N=6
kT(10)
azp_integrate_langevin_flow_step_two_one timestep=10 kT=2.25 dt=0.005 N=6
f0.compute(12) deferred=True
f1.compute(12) deferred=True
azp_sum_forces N=6
kT(11)
azp_integrate_langevin_flow_step_two timestep=11 kT=2.375 dt=0.005 N=6
writer(12)
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=12 position_generation=12 type_generation=3
""",
    ('langevin_brownian', 'run0'): """
run(0)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
timestep=0 position_generation=0 type_generation=0
""",
    ('langevin_brownian', 'run1'): """
run(1)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
updater(0)
kT(0)
azp_integrate_langevin_flow_step_one timestep=0 kT=1.0 dt=0.005 N=6
azp_integrate_brownian_flow_step timestep=0 kT=2.0 dt=0.005 N=6
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
kT(0)
azp_integrate_langevin_flow_step_two timestep=0 kT=1.0 dt=0.005 N=6
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=1 position_generation=1 type_generation=1
""",
    ('langevin_brownian', 'run7_run5'): """
run(7)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
updater(0)
kT(0)
azp_integrate_langevin_flow_step_one timestep=0 kT=1.0 dt=0.005 N=6
azp_integrate_brownian_flow_step timestep=0 kT=2.0 dt=0.005 N=6
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
kT(0)
azp_integrate_langevin_flow_step_two_one timestep=0 kT=1.0 dt=0.005 N=6
azp_integrate_brownian_flow_step timestep=1 kT=2.0 dt=0.005 N=6
f0.compute(2) deferred=True
f1.compute(2) deferred=True
azp_sum_forces N=6
kT(1)
azp_integrate_langevin_flow_step_two_one timestep=1 kT=1.125 dt=0.005 N=6
azp_integrate_brownian_flow_step timestep=2 kT=2.0 dt=0.005 N=6
f0.compute(3) deferred=True
f1.compute(3) deferred=True
azp_sum_forces N=6
kT(2)
azp_integrate_langevin_flow_step_two timestep=2 kT=1.25 dt=0.005 N=6
writer(3)
kT(3)
azp_integrate_langevin_flow_step_one timestep=3 kT=1.375 dt=0.005 N=6
azp_integrate_brownian_flow_step timestep=3 kT=2.0 dt=0.005 N=6
f0.compute(4) deferred=True
f1.compute(4) deferred=True
azp_sum_forces N=6
kT(3)
azp_integrate_langevin_flow_step_two timestep=3 kT=1.375 dt=0.005 N=6
updater(4)
kT(4)
azp_integrate_langevin_flow_step_one timestep=4 kT=1.5 dt=0.005 N=6
azp_integrate_brownian_flow_step timestep=4 kT=2.0 dt=0.005 N=6
sort(5)
nlist.particles_sorted
f0.compute(5) deferred=True
f1.compute(5) deferred=True
azp_sum_forces N=6
kT(4)
azp_integrate_langevin_flow_step_two_one timestep=4 kT=1.5 dt=0.005 N=6
azp_integrate_brownian_flow_step timestep=5 kT=2.0 dt=0.005 N=6
f0.compute(6) deferred=True
f1.compute(6) deferred=True
azp_sum_forces N=6
kT(5)
azp_integrate_langevin_flow_step_two timestep=5 kT=1.625 dt=0.005 N=6
writer(6)
kT(6)
azp_integrate_langevin_flow_step_one timestep=6 kT=1.75 dt=0.005 N=6
azp_integrate_brownian_flow_step timestep=6 kT=2.0 dt=0.005 N=6
f0.compute(7) deferred=True
f1.compute(7) deferred=True
azp_sum_forces N=6
kT(6)
azp_integrate_langevin_flow_step_two timestep=6 kT=1.75 dt=0.005 N=6
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
run(5)
f0.compute(7) deferred=False
f1.compute(7) deferred=False
azp_sum_forces N=6
kT(7)
azp_integrate_langevin_flow_step_one timestep=7 kT=1.875 dt=0.005 N=6
azp_integrate_brownian_flow_step timestep=7 kT=2.0 dt=0.005 N=6
f0.compute(8) deferred=True
f1.compute(8) deferred=True
azp_sum_forces N=6
kT(7)
azp_integrate_langevin_flow_step_two timestep=7 kT=1.875 dt=0.005 N=6
updater(8)
kT(8)
azp_integrate_langevin_flow_step_one timestep=8 kT=2.0 dt=0.005 N=6
azp_integrate_brownian_flow_step timestep=8 kT=2.0 dt=0.005 N=6
f0.compute(9) deferred=True
f1.compute(9) deferred=True
azp_sum_forces N=6
kT(8)
azp_integrate_langevin_flow_step_two timestep=8 kT=2.0 dt=0.005 N=6
writer(9)
kT(9)
azp_integrate_langevin_flow_step_one timestep=9 kT=2.125 dt=0.005 N=6
azp_integrate_brownian_flow_step timestep=9 kT=2.0 dt=0.005 N=6
sort(10)
nlist.particles_sorted
f0.compute(10) deferred=True
f1.compute(10) deferred=True
azp_sum_forces N=6
kT(9)
azp_integrate_langevin_flow_step_two_one timestep=9 kT=2.125 dt=0.005 N=6
azp_integrate_brownian_flow_step timestep=10 kT=2.0 dt=0.005 N=6
f0.compute(11) deferred=True
f1.compute(11) deferred=True
azp_sum_forces N=6
kT(10)
azp_integrate_langevin_flow_step_two_one timestep=10 kT=2.25 dt=0.005 N=6
azp_integrate_brownian_flow_step timestep=11 kT=2.0 dt=0.005 N=6
f0.compute(12) deferred=True
f1.compute(12) deferred=True
azp_sum_forces N=6
kT(11)
azp_integrate_langevin_flow_step_two timestep=11 kT=2.375 dt=0.005 N=6
writer(12)
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=12 position_generation=12 type_generation=3
""",
    ('nph', 'run0'): """
run(0)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
timestep=0 position_generation=0 type_generation=0
box_generation=0
""",
    ('nph', 'run1'): """
run(1)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
updater(0)
azp_thermo_sums N=6 n_forces=2 virials=2
S(0)
azp_barostat_advance timestep=0 dt=0.005 N=6 phase=2 L=(8.0, 8.0, 8.0)
azp_barostat_step_one timestep=0 dt=0.005 N=6 phase=2 L=(10.0, 8.0, 6.4)
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=0 dt=0.005 N=6 phase=2 L=(10.0, 8.0, 6.4)
azp_thermo_sums N=6 n_forces=2 virials=2
S(1)
azp_barostat_advance timestep=1 dt=0.005 N=6 phase=1 L=(10.0, 8.0, 6.4)
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=1 position_generation=2 type_generation=1
box_generation=1
""",
    ('nph', 'run7_run5'): """
run(7)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
updater(0)
azp_thermo_sums N=6 n_forces=2 virials=2
S(0)
azp_barostat_advance timestep=0 dt=0.005 N=6 phase=2 L=(8.0, 8.0, 8.0)
azp_barostat_step_one timestep=0 dt=0.005 N=6 phase=2 L=(10.0, 8.0, 6.4)
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=0 dt=0.005 N=6 phase=2 L=(10.0, 8.0, 6.4)
azp_thermo_sums N=6 n_forces=2 virials=2
S(1)
azp_barostat_advance timestep=1 dt=0.005 N=6 phase=1 L=(10.0, 8.0, 6.4)
S(1)
azp_barostat_advance timestep=1 dt=0.005 N=6 phase=2 L=(10.0, 8.0, 6.4)
azp_barostat_step_one timestep=1 dt=0.005 N=6 phase=2 L=(12.5, 8.0, 5.120000000000001)
f0.compute(2) deferred=True
f1.compute(2) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=1 dt=0.005 N=6 phase=2 L=(12.5, 8.0, 5.120000000000001)
azp_thermo_sums N=6 n_forces=2 virials=2
S(2)
azp_barostat_advance timestep=2 dt=0.005 N=6 phase=1 L=(12.5, 8.0, 5.120000000000001)
S(2)
azp_barostat_advance timestep=2 dt=0.005 N=6 phase=2 L=(12.5, 8.0, 5.120000000000001)
azp_barostat_step_one timestep=2 dt=0.005 N=6 phase=2 L=(15.625, 8.0, 4.096000000000001)
f0.compute(3) deferred=True
f1.compute(3) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=2 dt=0.005 N=6 phase=2 L=(15.625, 8.0, 4.096000000000001)
azp_thermo_sums N=6 n_forces=2 virials=2
S(3)
azp_barostat_advance timestep=3 dt=0.005 N=6 phase=1 L=(15.625, 8.0, 4.096000000000001)
writer(3)
S(3)
azp_barostat_advance timestep=3 dt=0.005 N=6 phase=2 L=(15.625, 8.0, 4.096000000000001)
azp_barostat_step_one timestep=3 dt=0.005 N=6 phase=2 L=(19.53125, 8.0, 3.276800000000001)
f0.compute(4) deferred=True
f1.compute(4) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=3 dt=0.005 N=6 phase=2 L=(19.53125, 8.0, 3.276800000000001)
azp_thermo_sums N=6 n_forces=2 virials=2
S(4)
azp_barostat_advance timestep=4 dt=0.005 N=6 phase=1 L=(19.53125, 8.0, 3.276800000000001)
updater(4)
S(4)
azp_barostat_advance timestep=4 dt=0.005 N=6 phase=2 L=(19.53125, 8.0, 3.276800000000001)
azp_barostat_step_one timestep=4 dt=0.005 N=6 phase=2 L=(24.4140625, 8.0, 2.621440000000001)
sort(5)
nlist.particles_sorted
f0.compute(5) deferred=True
f1.compute(5) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=4 dt=0.005 N=6 phase=2 L=(24.4140625, 8.0, 2.621440000000001)
azp_thermo_sums N=6 n_forces=2 virials=2
S(5)
azp_barostat_advance timestep=5 dt=0.005 N=6 phase=1 L=(24.4140625, 8.0, 2.621440000000001)
S(5)
azp_barostat_advance timestep=5 dt=0.005 N=6 phase=2 L=(24.4140625, 8.0, 2.621440000000001)
azp_barostat_step_one timestep=5 dt=0.005 N=6 phase=2 L=(30.517578125, 8.0, 2.097152000000001)
f0.compute(6) deferred=True
f1.compute(6) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=5 dt=0.005 N=6 phase=2 L=(30.517578125, 8.0, 2.097152000000001)
azp_thermo_sums N=6 n_forces=2 virials=2
S(6)
azp_barostat_advance timestep=6 dt=0.005 N=6 phase=1 L=(30.517578125, 8.0, 2.097152000000001)
writer(6)
S(6)
azp_barostat_advance timestep=6 dt=0.005 N=6 phase=2 L=(30.517578125, 8.0, 2.097152000000001)
azp_barostat_step_one timestep=6 dt=0.005 N=6 phase=2 L=(38.14697265625, 8.0, 1.6777216000000008)
f0.compute(7) deferred=True
f1.compute(7) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=6 dt=0.005 N=6 phase=2 L=(38.14697265625, 8.0, 1.6777216000000008)
azp_thermo_sums N=6 n_forces=2 virials=2
S(7)
azp_barostat_advance timestep=7 dt=0.005 N=6 phase=1 L=(38.14697265625, 8.0, 1.6777216000000008)
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
run(5)
f0.compute(7) deferred=False
f1.compute(7) deferred=False
azp_sum_forces N=6
azp_thermo_sums N=6 n_forces=2 virials=2
S(7)
azp_barostat_advance timestep=7 dt=0.005 N=6 phase=2 L=(38.14697265625, 8.0, 1.6777216000000008)
azp_barostat_step_one timestep=7 dt=0.005 N=6 phase=2 L=(47.6837158203125, 8.0, 1.3421772800000007)
f0.compute(8) deferred=True
f1.compute(8) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=7 dt=0.005 N=6 phase=2 L=(47.6837158203125, 8.0, 1.3421772800000007)
azp_thermo_sums N=6 n_forces=2 virials=2
S(8)
azp_barostat_advance timestep=8 dt=0.005 N=6 phase=1 L=(47.6837158203125, 8.0, 1.3421772800000007)
updater(8)
S(8)
azp_barostat_advance timestep=8 dt=0.005 N=6 phase=2 L=(47.6837158203125, 8.0, 1.3421772800000007)
azp_barostat_step_one timestep=8 dt=0.005 N=6 phase=2 L=(59.604644775390625, 8.0, 1.0737418240000005)
f0.compute(9) deferred=True
f1.compute(9) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=8 dt=0.005 N=6 phase=2 L=(59.604644775390625, 8.0, 1.0737418240000005)
azp_thermo_sums N=6 n_forces=2 virials=2
S(9)
azp_barostat_advance timestep=9 dt=0.005 N=6 phase=1 L=(59.604644775390625, 8.0, 1.0737418240000005)
writer(9)
S(9)
azp_barostat_advance timestep=9 dt=0.005 N=6 phase=2 L=(59.604644775390625, 8.0, 1.0737418240000005)
azp_barostat_step_one timestep=9 dt=0.005 N=6 phase=2 L=(74.50580596923828, 8.0, 0.8589934592000005)
sort(10)
nlist.particles_sorted
f0.compute(10) deferred=True
f1.compute(10) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=9 dt=0.005 N=6 phase=2 L=(74.50580596923828, 8.0, 0.8589934592000005)
azp_thermo_sums N=6 n_forces=2 virials=2
S(10)
azp_barostat_advance timestep=10 dt=0.005 N=6 phase=1 L=(74.50580596923828, 8.0, 0.8589934592000005)
S(10)
azp_barostat_advance timestep=10 dt=0.005 N=6 phase=2 L=(74.50580596923828, 8.0, 0.8589934592000005)
azp_barostat_step_one timestep=10 dt=0.005 N=6 phase=2 L=(93.13225746154785, 8.0, 0.6871947673600004)
f0.compute(11) deferred=True
f1.compute(11) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=10 dt=0.005 N=6 phase=2 L=(93.13225746154785, 8.0, 0.6871947673600004)
azp_thermo_sums N=6 n_forces=2 virials=2
S(11)
azp_barostat_advance timestep=11 dt=0.005 N=6 phase=1 L=(93.13225746154785, 8.0, 0.6871947673600004)
S(11)
azp_barostat_advance timestep=11 dt=0.005 N=6 phase=2 L=(93.13225746154785, 8.0, 0.6871947673600004)
azp_barostat_step_one timestep=11 dt=0.005 N=6 phase=2 L=(116.41532182693481, 8.0, 0.5497558138880003)
f0.compute(12) deferred=True
f1.compute(12) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=11 dt=0.005 N=6 phase=2 L=(116.41532182693481, 8.0, 0.5497558138880003)
azp_thermo_sums N=6 n_forces=2 virials=2
S(12)
azp_barostat_advance timestep=12 dt=0.005 N=6 phase=1 L=(116.41532182693481, 8.0, 0.5497558138880003)
writer(12)
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=12 position_generation=24 type_generation=3
box_generation=12
""",
    ('npt_bussi', 'run0'): """
run(0)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
timestep=0 position_generation=0 type_generation=0
box_generation=0
""",
    ('npt_bussi', 'run1'): """
run(1)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
updater(0)
azp_thermo_sums N=6 n_forces=2 virials=2
S(0)
kT(0)
azp_barostat_advance timestep=0 dt=0.005 N=6 phase=2 L=(8.0, 8.0, 8.0)
azp_barostat_step_one timestep=0 dt=0.005 N=6 phase=2 L=(10.0, 8.0, 6.4)
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=0 dt=0.005 N=6 phase=2 L=(10.0, 8.0, 6.4)
azp_thermo_sums N=6 n_forces=2 virials=2
S(1)
kT(1)
azp_barostat_advance timestep=1 dt=0.005 N=6 phase=1 L=(10.0, 8.0, 6.4)
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=1 position_generation=2 type_generation=1
box_generation=1
""",
    ('npt_bussi', 'run7_run5'): """
run(7)
f0.compute(0) deferred=False
f1.compute(0) deferred=False
azp_sum_forces N=6
updater(0)
azp_thermo_sums N=6 n_forces=2 virials=2
S(0)
kT(0)
azp_barostat_advance timestep=0 dt=0.005 N=6 phase=2 L=(8.0, 8.0, 8.0)
azp_barostat_step_one timestep=0 dt=0.005 N=6 phase=2 L=(10.0, 8.0, 6.4)
f0.compute(1) deferred=True
f1.compute(1) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=0 dt=0.005 N=6 phase=2 L=(10.0, 8.0, 6.4)
azp_thermo_sums N=6 n_forces=2 virials=2
S(1)
kT(1)
azp_barostat_advance timestep=1 dt=0.005 N=6 phase=1 L=(10.0, 8.0, 6.4)
S(1)
kT(1)
azp_barostat_advance timestep=1 dt=0.005 N=6 phase=2 L=(10.0, 8.0, 6.4)
azp_barostat_step_one timestep=1 dt=0.005 N=6 phase=2 L=(12.5, 8.0, 5.120000000000001)
f0.compute(2) deferred=True
f1.compute(2) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=1 dt=0.005 N=6 phase=2 L=(12.5, 8.0, 5.120000000000001)
azp_thermo_sums N=6 n_forces=2 virials=2
S(2)
kT(2)
azp_barostat_advance timestep=2 dt=0.005 N=6 phase=1 L=(12.5, 8.0, 5.120000000000001)
S(2)
kT(2)
azp_barostat_advance timestep=2 dt=0.005 N=6 phase=2 L=(12.5, 8.0, 5.120000000000001)
azp_barostat_step_one timestep=2 dt=0.005 N=6 phase=2 L=(15.625, 8.0, 4.096000000000001)
f0.compute(3) deferred=True
f1.compute(3) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=2 dt=0.005 N=6 phase=2 L=(15.625, 8.0, 4.096000000000001)
azp_thermo_sums N=6 n_forces=2 virials=2
S(3)
kT(3)
azp_barostat_advance timestep=3 dt=0.005 N=6 phase=1 L=(15.625, 8.0, 4.096000000000001)
writer(3)
S(3)
kT(3)
azp_barostat_advance timestep=3 dt=0.005 N=6 phase=2 L=(15.625, 8.0, 4.096000000000001)
azp_barostat_step_one timestep=3 dt=0.005 N=6 phase=2 L=(19.53125, 8.0, 3.276800000000001)
f0.compute(4) deferred=True
f1.compute(4) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=3 dt=0.005 N=6 phase=2 L=(19.53125, 8.0, 3.276800000000001)
azp_thermo_sums N=6 n_forces=2 virials=2
S(4)
kT(4)
azp_barostat_advance timestep=4 dt=0.005 N=6 phase=1 L=(19.53125, 8.0, 3.276800000000001)
updater(4)
S(4)
kT(4)
azp_barostat_advance timestep=4 dt=0.005 N=6 phase=2 L=(19.53125, 8.0, 3.276800000000001)
azp_barostat_step_one timestep=4 dt=0.005 N=6 phase=2 L=(24.4140625, 8.0, 2.621440000000001)
sort(5)
nlist.particles_sorted
f0.compute(5) deferred=True
f1.compute(5) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=4 dt=0.005 N=6 phase=2 L=(24.4140625, 8.0, 2.621440000000001)
azp_thermo_sums N=6 n_forces=2 virials=2
S(5)
kT(5)
azp_barostat_advance timestep=5 dt=0.005 N=6 phase=1 L=(24.4140625, 8.0, 2.621440000000001)
S(5)
kT(5)
azp_barostat_advance timestep=5 dt=0.005 N=6 phase=2 L=(24.4140625, 8.0, 2.621440000000001)
azp_barostat_step_one timestep=5 dt=0.005 N=6 phase=2 L=(30.517578125, 8.0, 2.097152000000001)
f0.compute(6) deferred=True
f1.compute(6) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=5 dt=0.005 N=6 phase=2 L=(30.517578125, 8.0, 2.097152000000001)
azp_thermo_sums N=6 n_forces=2 virials=2
S(6)
kT(6)
azp_barostat_advance timestep=6 dt=0.005 N=6 phase=1 L=(30.517578125, 8.0, 2.097152000000001)
writer(6)
S(6)
kT(6)
azp_barostat_advance timestep=6 dt=0.005 N=6 phase=2 L=(30.517578125, 8.0, 2.097152000000001)
azp_barostat_step_one timestep=6 dt=0.005 N=6 phase=2 L=(38.14697265625, 8.0, 1.6777216000000008)
f0.compute(7) deferred=True
f1.compute(7) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=6 dt=0.005 N=6 phase=2 L=(38.14697265625, 8.0, 1.6777216000000008)
azp_thermo_sums N=6 n_forces=2 virials=2
S(7)
kT(7)
azp_barostat_advance timestep=7 dt=0.005 N=6 phase=1 L=(38.14697265625, 8.0, 1.6777216000000008)
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
run(5)
f0.compute(7) deferred=False
f1.compute(7) deferred=False
azp_sum_forces N=6
azp_thermo_sums N=6 n_forces=2 virials=2
S(7)
kT(7)
azp_barostat_advance timestep=7 dt=0.005 N=6 phase=2 L=(38.14697265625, 8.0, 1.6777216000000008)
azp_barostat_step_one timestep=7 dt=0.005 N=6 phase=2 L=(47.6837158203125, 8.0, 1.3421772800000007)
f0.compute(8) deferred=True
f1.compute(8) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=7 dt=0.005 N=6 phase=2 L=(47.6837158203125, 8.0, 1.3421772800000007)
azp_thermo_sums N=6 n_forces=2 virials=2
S(8)
kT(8)
azp_barostat_advance timestep=8 dt=0.005 N=6 phase=1 L=(47.6837158203125, 8.0, 1.3421772800000007)
updater(8)
S(8)
kT(8)
azp_barostat_advance timestep=8 dt=0.005 N=6 phase=2 L=(47.6837158203125, 8.0, 1.3421772800000007)
azp_barostat_step_one timestep=8 dt=0.005 N=6 phase=2 L=(59.604644775390625, 8.0, 1.0737418240000005)
f0.compute(9) deferred=True
f1.compute(9) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=8 dt=0.005 N=6 phase=2 L=(59.604644775390625, 8.0, 1.0737418240000005)
azp_thermo_sums N=6 n_forces=2 virials=2
S(9)
kT(9)
azp_barostat_advance timestep=9 dt=0.005 N=6 phase=1 L=(59.604644775390625, 8.0, 1.0737418240000005)
writer(9)
S(9)
kT(9)
azp_barostat_advance timestep=9 dt=0.005 N=6 phase=2 L=(59.604644775390625, 8.0, 1.0737418240000005)
azp_barostat_step_one timestep=9 dt=0.005 N=6 phase=2 L=(74.50580596923828, 8.0, 0.8589934592000005)
sort(10)
nlist.particles_sorted
f0.compute(10) deferred=True
f1.compute(10) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=9 dt=0.005 N=6 phase=2 L=(74.50580596923828, 8.0, 0.8589934592000005)
azp_thermo_sums N=6 n_forces=2 virials=2
S(10)
kT(10)
azp_barostat_advance timestep=10 dt=0.005 N=6 phase=1 L=(74.50580596923828, 8.0, 0.8589934592000005)
S(10)
kT(10)
azp_barostat_advance timestep=10 dt=0.005 N=6 phase=2 L=(74.50580596923828, 8.0, 0.8589934592000005)
azp_barostat_step_one timestep=10 dt=0.005 N=6 phase=2 L=(93.13225746154785, 8.0, 0.6871947673600004)
f0.compute(11) deferred=True
f1.compute(11) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=10 dt=0.005 N=6 phase=2 L=(93.13225746154785, 8.0, 0.6871947673600004)
azp_thermo_sums N=6 n_forces=2 virials=2
S(11)
kT(11)
azp_barostat_advance timestep=11 dt=0.005 N=6 phase=1 L=(93.13225746154785, 8.0, 0.6871947673600004)
S(11)
kT(11)
azp_barostat_advance timestep=11 dt=0.005 N=6 phase=2 L=(93.13225746154785, 8.0, 0.6871947673600004)
azp_barostat_step_one timestep=11 dt=0.005 N=6 phase=2 L=(116.41532182693481, 8.0, 0.5497558138880003)
f0.compute(12) deferred=True
f1.compute(12) deferred=True
azp_sum_forces N=6
azp_barostat_step_two timestep=11 dt=0.005 N=6 phase=2 L=(116.41532182693481, 8.0, 0.5497558138880003)
azp_thermo_sums N=6 n_forces=2 virials=2
S(12)
kT(12)
azp_barostat_advance timestep=12 dt=0.005 N=6 phase=1 L=(116.41532182693481, 8.0, 0.5497558138880003)
writer(12)
f0.check_flags(wait=True) deferred=False
f1.check_flags(wait=True) deferred=False
timestep=12 position_generation=24 type_generation=3
box_generation=12
""",
}
