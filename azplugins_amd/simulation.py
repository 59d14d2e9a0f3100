"""The simulation driver: ``hoomd.Simulation``, its operations lists (integrator, computes, updaters, writers, tuners)
and ``hoomd.md.Integrator``, reduced to what this project runs. ``Simulation.run`` attaches the forces to the state,
evaluates them (``run(0)``) and steps: one loop for every integration path (``DESIGN.md`` 4.20), around whatever moves
the particles -- ``methods.ConstantVolume`` (NVE, the dummy integrator of the reference's tests,
src/pytest/test_pair.py:325-327) or its thermostat (``thermostats``), ``methods.ConstantPressure``, ``minimize.FIRE``,
the Langevin / Brownian methods (``methods``, ``flow``) -- with the updaters ahead of each step, the writers after it, the particle sorter and a
domain's halo exchange between the position update and the forces. The methods, the filters and the trigger live in
``methods``, ``filter`` and ``trigger``; their names are re-exported here.
"""

import ctypes as C
import warnings

import numpy as np

from . import _lib
from .filter import All, Type  # noqa: F401 (re-exported, as the names below)
from .methods import Brownian, ConstantPressure, ConstantVolume, Langevin, _check_moves_all, _launch  # noqa: F401
from .state import State
from .trigger import Periodic  # noqa: F401


class Integrator:
    """``hoomd.md.Integrator`` reduced: ``dt``, ``forces``, ``methods``,
    ``integrate_rotational_dof`` (orientations and angular momenta of particles with a
    non-zero moment of inertia are integrated with the net torque, HOOMD's default False).
    ``methods`` holds one ``ConstantVolume``, one ``ConstantPressure``, or one or more of ``methods.Langevin``,
    ``methods.Brownian``, ``flow.Langevin`` and ``flow.Brownian`` with pairwise-disjoint filters (an ``All()`` filter
    stands alone)."""

    def __init__(self, dt, forces=None, methods=None, integrate_rotational_dof=False):
        self.dt = float(dt)
        self.forces = list(forces) if forces is not None else []
        self.methods = list(methods) if methods is not None else []
        self.integrate_rotational_dof = bool(integrate_rotational_dof)


class _Computes(list):
    """``sim.operations.computes``: a list whose members know their simulation (HOOMD attaches an operation when it
    joins the simulation's operations)."""

    def __init__(self, sim):
        super().__init__()
        self._sim = sim

    def _claim(self, op):
        from .compute import _Compute

        if not isinstance(op, _Compute):
            raise _lib.AzpError("sim.operations.computes holds computes (azplugins_amd.compute), got %r" % (op,))
        if op._sim is not None and op._sim is not self._sim and any(c is op for c in op._sim.operations.computes):
            raise _lib.AzpError("%s is already in the operations of another simulation" % type(op).__name__)
        op._sim = self._sim
        return op

    def append(self, op):
        if not any(c is op for c in self):
            super().append(self._claim(op))

    def insert(self, i, op):
        if not any(c is op for c in self):
            super().insert(i, self._claim(op))

    def extend(self, ops):
        for op in ops:
            self.append(op)

    def __iadd__(self, ops):
        self.extend(ops)
        return self

    def remove(self, op):
        for i, c in enumerate(self):
            if c is op:
                del self[i]
                op._sim = None
                return
        raise ValueError("%r is not in sim.operations.computes" % (op,))


class _Operations:
    def __init__(self, sim=None):
        self.integrator = None
        self.computes = _Computes(sim)
        # HOOMD's sim.operations.updaters: run ahead of the integrator's step at the timesteps their trigger fires
        # (azplugins_amd.update.TypeUpdater, azplugins_amd.evaporate.ParticleEvaporator)
        self.updaters = []
        # HOOMD's sim.operations.writers: run after the integrator's step at the timesteps their trigger fires
        # (azplugins_amd.compute.ThermodynamicRecorder, azplugins_amd.compute.RDFRecorder)
        self.writers = []
        # HOOMD puts a ParticleSorter into sim.operations.tuners by default; so does this
        # (remove it from the list, or set trigger_period = 0, to keep the initial order)
        from .sorter import ParticleSorter

        self.tuners = [ParticleSorter(trigger_period=200)]

    def add(self, op):
        """Add an updater, a writer or a compute (``hoomd.Operations.add``); a compute is attached while the simulation
        has a state."""
        from .compute import _Recorder
        from .update import _Updater

        for cls, ops in ((_Updater, self.updaters), (_Recorder, self.writers)):
            if isinstance(op, cls):
                if not any(u is op for u in ops):
                    ops.append(op)
                return
        self.computes.append(op)

    def remove(self, op):
        """Remove an updater, a writer or a compute; reading a removed compute's results raises
        ``compute.DataAccessError``."""
        from .compute import _Recorder
        from .update import _Updater

        for cls, ops, name in ((_Updater, self.updaters, "updaters"), (_Recorder, self.writers, "writers")):
            if isinstance(op, cls):
                for i, u in enumerate(ops):
                    if u is op:
                        del ops[i]
                        return
                raise ValueError("%r is not in sim.operations.%s" % (op, name))
        self.computes.remove(op)


class Simulation:
    def __init__(self, device="cuda:0", seed=None):
        self.device = device
        self.seed = seed
        self.state = None
        self.timestep = 0
        self.operations = _Operations(self)
        self._attached = []
        self.domain = None  # azplugins_amd.domain.DeviceDomain of a decomposed run (attach_domain)

    def attach_domain(self, domain):
        """Domain-decomposed run: ``domain`` (a rebuilt ``DeviceDomain``) owns the particle
        arrays. Every step the ghost rows of the arrays the forces read are exchanged; when
        any rank's distance check asks for a neighbor-list rebuild, all ranks migrate their
        particles and re-select their ghosts first (HOOMD: Communicator::migrateParticles /
        exchangeGhosts ahead of NeighborList::compute). A tilted box is refused: the domain's slabs are Cartesian."""
        if self.state.box.is_triclinic:
            raise _lib.AzpError("attach_domain: %r is tilted -- a domain cuts the box into Cartesian slabs, whose ghost layers "
                                "do not follow a tilted periodic face; run a tilted box on one device" % (self.state.box,))
        for kind, g in self.state.groups.items():
            if g.n and g.tags is None:
                raise _lib.AzpError("attach_domain: a %s needs its topology by tag (State.set_global_%ss) -- the index-based "
                                    "%s table of a single-domain state does not survive a migration"
                                    % ("bonded system" if kind == "bond" else "system with %ss" % kind, kind, kind))
        # every per-particle array that the integrator or a force touches must migrate with the particles
        # (an array left behind keeps its old size and order while N changes under it)
        need = ["pos", "vel", "tag", "image"]
        integ = self.operations.integrator
        if integ is not None:
            for f in integ.forces:
                need += [n for n in getattr(f, "_halo_fields", ()) if n not in need]
            if getattr(integ, "integrate_rotational_dof", False):
                need += ["orientation", "angmom", "inertia"]
        missing = [n for n in need if n not in domain.names]
        if missing:
            raise _lib.AzpError("attach_domain: the domain does not carry %s (DeviceDomain(arrays=...) must hold every array "
                                "the integrator and the forces use)" % ", ".join(missing))
        self.domain = domain
        domain.attach_state(self.state)
        self.operations.tuners.clear()  # the domain keeps its own interior | boundary | ghost order

    def _halo_fields(self):
        names = ["pos"]
        for f in self.operations.integrator.forces:
            for n in getattr(f, "_halo_fields", ()):
                if n not in names and n in self.domain.names:
                    names.append(n)
        return names

    def _wire_domain(self):
        """Point the neighbor lists of the attached forces at the domain's collective hooks."""
        dom = self.domain

        def before_rebuild(state):
            dom.rebuild()
            dom.attach_state(state)

        for f in self.operations.integrator.forces:
            nl = getattr(f, "nlist", None)
            if nl is not None:
                nl.reduce_flag = dom.all_reduce_flag
                nl.before_rebuild = before_rebuild

    def _warn_if_seed_unset(self):
        if self.seed is None:
            warnings.warn("Simulation.seed is not set, using default seed=0", RuntimeWarning)
            self.seed = 0

    def create_state_from_snapshot(self, snapshot):
        self.state = State(snapshot, self.device)
        return self.state

    @property
    def dt(self):
        integ = self.operations.integrator
        return integ.dt if integ is not None else 0.0

    def _attach_all(self):
        integ = self.operations.integrator
        if integ is None:
            raise _lib.AzpError("Simulation.operations.integrator is not set")
        if self.state is None:
            raise _lib.AzpError("Simulation has no state; call create_state_from_snapshot first")
        for f in integ.forces:
            if f not in self._attached or f._state is not self.state:
                f._attach(self)
                if f not in self._attached:
                    self._attached.append(f)
        if self._has_thermo() or self._has_thermo_field() or self._barostat(integ) is not None:
            # (a ThermodynamicQuantities, a ThermodynamicField and a ConstantPressure read the per-particle virials: the
            # virial pass of every force runs every step)
            for f in integ.forces:
                f.compute_virial = True
            for c in self._thermo_computes():
                c._prepare()

    def _thermo_computes(self):
        from .compute import ThermodynamicQuantities

        return [c for c in self.operations.computes if isinstance(c, ThermodynamicQuantities)]

    @staticmethod
    def _barostat(integ):
        """The first ``ConstantPressure`` among the integrator's methods, or None."""
        return next((m for m in integ.methods if isinstance(m, ConstantPressure)), None)

    def _has_thermo(self):
        return bool(self.operations.computes) and bool(self._thermo_computes())

    def _has_thermo_field(self):
        from .compute import ThermodynamicField

        return any(isinstance(c, ThermodynamicField) for c in self.operations.computes)

    def _check_writers(self):
        """A recorder reads its compute through this simulation's state: the compute has to be in ``computes``."""
        for w in self.operations.writers:
            if not any(c is w._compute for c in self.operations.computes):
                raise _lib.AzpError("%s: its %s is not in sim.operations.computes of this simulation"
                                    % (type(w).__name__, type(w._compute).__name__))
        integ = self.operations.integrator
        if integ is not None and len(integ.forces) > _lib.THERMO_MAX_FORCES and (self._has_thermo() or self._has_thermo_field()):
            raise _lib.AzpError("%s sums at most %d forces, the integrator has %d"
                                % ("ThermodynamicQuantities" if self._has_thermo() else "ThermodynamicField",
                                   _lib.THERMO_MAX_FORCES, len(integ.forces)))

    def _writers_due(self):
        return [w for w in self.operations.writers if w.trigger(self.timestep)]

    def _run_writers(self, due):
        for w in due:
            w._record(self, self.timestep)

    def _compute_forces(self):
        import torch

        st = self.state
        forces = self.operations.integrator.forces
        if self.domain is not None:
            # decomposed runs: a neighbor-list rebuild migrates particles (N and every index change). Bring every list
            # up to date BEFORE any force buffer is sized or summed, so that all forces of this step see one order
            seen = []
            for f in forces:
                nl = getattr(f, "nlist", None)
                if nl is not None and all(nl is not s for s in seen):
                    seen.append(nl)
                    nl.compute(st)
            if len(seen) > 1:
                raise _lib.AzpError("decomposed runs support one neighbor list (a second list's rebuild would migrate "
                                    "particles under the first)")
        if len(forces) == 1:
            # a single force: its own array is the net force (no 32 MB zero + add per step)
            forces[0].compute(self.timestep)
            forces[0]._virial_evaluated = bool(forces[0].compute_virial)
            st.net_force = forces[0].force_tensor
            return
        if st.net_force.shape[0] != st.N or any(st.net_force is f.force_tensor for f in forces):
            st.net_force = torch.zeros((st.N, 4), dtype=torch.float64, device=st.device)
        for f in forces:
            f.compute(self.timestep)
            f._virial_evaluated = bool(f.compute_virial)
        # one pass over the forces' arrays (azp_sum_forces) instead of a zero + one read-modify-write per force
        for k0 in range(0, len(forces), 7):
            grp = forces[k0:k0 + 7]
            ptrs = ([st.net_force.data_ptr()] if k0 else []) + [f.force_tensor.data_ptr() for f in grp]
            arr = (C.c_void_p * len(ptrs))(*ptrs)
            _lib.check(_lib.lib().azp_sum_forces(st.N, len(ptrs), arr, st.net_force.data_ptr(), _lib.raw_stream(st.device)), "azp_sum_forces")

    def run(self, steps):
        """``steps`` steps of the integrator's methods (HOOMD IntegratorTwoStep::update): every stepper's step one at the
        step's timestep t, the forces at t + 1, every stepper's step two at t. The one loop of all paths."""
        from .minimize import FIRE

        self._check_writers()
        self._attach_all()
        integ = self.operations.integrator
        st = self.state
        # (refused even where nothing is stepped, and ahead of the forces: what the minimizer and the flow methods cannot do)
        fire = isinstance(integ, FIRE)
        if fire:
            integ._check(self)
        barostat = None if fire else self._barostat(integ)
        if barostat is not None:
            barostat._check(self, integ)
        flow_methods = [] if fire else self._check_flow_methods(integ)
        if self.domain is not None:
            self._wire_domain()
        self._compute_forces()
        if steps == 0 or not integ.methods:
            return
        # what moves the particles, each with the stepper interface: the minimizer, the flow methods, or
        # a ConstantPressure, or the one ConstantVolume (its thermostat where it has one)
        if fire:
            steppers = [integ]
        elif flow_methods:
            steppers = flow_methods
        elif barostat is not None:
            steppers = [barostat]
        elif len(integ.methods) != 1 or not isinstance(integ.methods[0], ConstantVolume):
            raise _lib.AzpError("Integrator.methods must hold exactly one ConstantVolume (all particles); got %r" % (integ.methods,))
        else:
            steppers = [integ.methods[0].thermostat or integ.methods[0]]
        for s in steppers:
            s._begin(self)
        # Inside a run nothing reads the velocities between step two of one step and step one of the next: where the
        # stepper can (_fusable) they are one kernel (same arithmetic, one pass over the arrays). Where a writer is due,
        # the full-step velocities of the previous step have to exist: its step two runs on its own (the same arithmetic,
        # bit for bit), the writer records, and this step starts with a plain step one. An updater that changes types
        # splits the fusion only for kernels that read them (_updaters_split: a flow method filtered by type); one that
        # changes the box (update.BoxResize) splits nothing: its kernel is queued ahead of the fused one, which reads the
        # box in its wrap alone, after step two's half kick
        fusable, updaters_split = steppers[0]._fusable, steppers[0]._updaters_split
        # (a bond force examines the "evaluator rejected its parameters" flag of step k when step k + 1 is queued, and
        # once more after the loop: no host round trip behind every launch)
        deferred = [f for f in integ.forces if hasattr(f, "defer_flag_check")]
        try:
            for f in deferred:
                f.defer_flag_check = True
            for k in range(steps):
                writers = self._writers_due() if k else []
                updaters = self._updaters_due()
                split = k > 0 and bool(not fusable or writers or (updaters_split and any(u._changes_types for u in updaters)))
                if split:
                    for s in steppers:
                        s._step_two(self, self.timestep - 1)
                self._run_writers(writers)  # (the state after self.timestep complete steps)
                self._run_updaters(updaters)
                for s in steppers:
                    s._step_one(self, self.timestep, fused=k > 0 and not split)
                if self.domain is not None:
                    self.domain.exchange(self._halo_fields())  # ghost rows follow their owners' particles
                st.position_generation += 1
                self.timestep += 1
                # re-index the particles between the position update and the force
                # evaluation: every per-particle array that survives the step is permuted,
                # the forces are recomputed in the new order
                # (also when a tile plan could not be compiled from the cells because the members of some tile have drifted
                # apart -- a DPD fluid diffuses a cell width in ~200 steps: sorting now costs 0.5 ms, the list-based rebuilds
                # that would follow until the sorter's next period 2.5 ms each; at most once per 20 steps)
                self._run_tuners(integ)
                self._compute_forces()
            for s in steppers:
                s._step_two(self, self.timestep - 1)
            self._run_writers(self._writers_due())
        finally:
            for f in deferred:
                f.defer_flag_check = False
        for f in deferred:
            f.check_flags(wait=True)

    def _check_thermostat(self, integ, method):
        """What a thermostatted ``ConstantVolume`` cannot do, each refused with its reason."""
        _check_moves_all(method.thermostat._name, "the kinetic energy", method, self, integ)

    def _updaters_due(self):
        return [u for u in self.operations.updaters if u.trigger(self.timestep)]

    def _run_updaters(self, due):
        """The updaters whose trigger fires at this timestep (HOOMD runs its updaters ahead of the integrator's
        step). Where one of them changes particle types (``_Updater._changes_types``), every neighbor list and tile plan
        is rebuilt before the next force evaluation (the reference: notifyParticleSort(), src/TypeUpdater.cc:86-87) --
        whether or not a type really changed, so that nothing is read back from the device."""
        for u in due:
            u._update(self, self.timestep)
        # (an updater that leaves the types alone -- update.BoxResize -- answers for its own generation counters)
        if any(u._changes_types for u in due):
            self.state.type_generation += 1

    def _run_tuners(self, integ):
        lists = [f.nlist for f in integ.forces if getattr(f, "nlist", None) is not None]
        wanted = any(nl.sort_wanted for nl in lists)
        for tuner in self.operations.tuners:
            due = tuner.trigger_period > 0 and self.timestep % tuner.trigger_period == 0
            on_demand = (wanted and tuner.trigger_period > 0
                         and (tuner.last_sort_step is None or self.timestep - tuner.last_sort_step >= 20))
            if (due or on_demand) and self.state.n_ghost == 0:
                tuner.sort(self)
                tuner.last_sort_step = self.timestep
                for nl in lists:
                    nl.particles_sorted()

    def _check_flow_methods(self, integ):
        """The Langevin / Brownian methods of ``integ`` (``flow.*`` and ``methods.Langevin`` / ``methods.Brownian``: one
        family; empty if it has none), after checking that they can run together."""
        from .flow import _FlowMethod
        from .methods import _StochasticMethod

        family = [m for m in integ.methods if isinstance(m, _StochasticMethod)]
        if not family:
            return family
        if len(family) != len(integ.methods):
            raise _lib.AzpError("Integrator.methods: Langevin / Brownian methods (flow.* and methods.*) cannot be mixed with "
                                "other methods, got %r" % (integ.methods,))
        if integ.integrate_rotational_dof and any(isinstance(m, _FlowMethod) for m in family):
            raise _lib.AzpError("flow.Langevin / flow.Brownian do not integrate rotational degrees of freedom "
                                "(integrate_rotational_dof=True); methods.Langevin / methods.Brownian do")
        if self.domain is not None:
            raise _lib.AzpError("Langevin / Brownian methods do not run decomposed (their stored accelerations and torques do "
                                "not migrate)")
        if any(any(m is o for o in family[:k]) for k, m in enumerate(family)):
            raise _lib.AzpError("Integrator.methods holds the same Langevin / Brownian method twice")
        if len(family) > 1 and any(isinstance(m.filter, All) for m in family):
            raise _lib.AzpError("Integrator.methods: a Langevin / Brownian method with filter All() must be the only method")
        seen = set()
        for m in family:
            if isinstance(m.filter, All):
                continue
            m.filter.mask(self.state.types)  # (rejects type names the state does not have)
            overlap = seen & set(m.filter.types)
            if overlap:
                raise _lib.AzpError("Integrator.methods: the filters of the Langevin / Brownian methods overlap (types %s)"
                                    % sorted(overlap))
            seen |= set(m.filter.types)
        return family

    def kinetic_temperature(self):
        """Instantaneous kT = 2 KE / (3 N - 3) (HOOMD ThermodynamicQuantities)."""
        st = self.state
        v = st.vel[: st.N]
        ke = 0.5 * float((v[:, 3] * (v[:, :3] ** 2).sum(dim=1)).sum().item())
        return 2.0 * ke / (3 * st.N - 3)

    def rotational_kinetic_energy(self):
        """sum_k s_k^2 / (2 I_k) over the axes with I_k != 0, s = 1/2 conj(q) p the body-frame
        angular momentum (HOOMD ComputeThermo)."""
        import torch

        st = self.state
        q, p, I = st.orientation[: st.N], st.angmom[: st.N], st.inertia[: st.N]
        qs, qv = q[:, 0:1], q[:, 1:4]
        ps, pv = p[:, 0:1], p[:, 1:4]
        s_v = 0.5 * (qs * pv - ps * qv - torch.linalg.cross(qv, pv))  # vector part of conj(q) p / 2
        ke = torch.where(I != 0.0, s_v * s_v / torch.where(I != 0.0, I, torch.ones_like(I)), torch.zeros_like(I))
        return 0.5 * float(ke.sum().item())

    def thermalize_particle_momenta(self, kT, seed=12345):
        """Maxwell-Boltzmann velocities with zero total momentum."""
        import torch

        from .synthetic import normal

        st = self.state
        tag = np.arange(st.N, dtype=np.uint64)
        m = st.vel[: st.N, 3].cpu().numpy()
        v = np.stack([normal(seed, tag, c) for c in range(3)], axis=1) * np.sqrt(kT / m)[:, None]
        v -= (v * m[:, None]).sum(axis=0) / m.sum()
        st.vel[: st.N, :3] = torch.from_numpy(v).to(st.device)
