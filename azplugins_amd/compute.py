"""Computes: mirror of ``hoomd.azplugins.compute`` (reference ``src/compute.py``) on libazp's velocity-field
kernels (``csrc/velocity_field.hip``).

``VelocityCompute`` is the mass-weighted center-of-mass velocity of a group; ``CartesianVelocityFieldCompute`` and
``CylindricalVelocityFieldCompute`` the mass-averaged velocity in each bin of a 1-, 2- or 3-D grid. A compute is
attached while it is in ``sim.operations.computes`` of a simulation that has a state; its result is computed when
the property is read, on the current state. On a decomposed run (``sim.domain`` set) every rank sums its own rows,
the sums are added over the domain's process group and every rank gets the same result.

``ThermodynamicQuantities`` (``hoomd.md.compute.ThermodynamicQuantities``) is temperature, pressure and the energies
of a group from one deterministic pass over the particles (``csrc/thermo.hip``); ``ThermodynamicRecorder`` appends the
sums of that pass to a device table at the timesteps its trigger fires inside ``Simulation.run``, without a host
synchronisation.

``CartesianThermodynamicField`` / ``CylindricalThermodynamicField`` are the spatial profiles of density, temperature
and (per-atom) stress on the grid of the velocity fields: the particles are keyed by (bin, tag), sorted, and every bin is
summed in a fixed 64-ary tree over its members in tag order (``csrc/thermo_field.hip``; this project's);
``ThermodynamicFieldRecorder`` appends the raw rows to a device table inside ``Simulation.run`` and
``thermo_field_quantities`` turns raw rows into the quantities.

``PressureProfile`` is the pressure tensor in slabs along one axis with every pair's virial spread along the line between
its two particles (the Irving-Kirkwood contour; ``csrc/pressure_profile.hip``; this project's): the pair
and two-body bonded forces are evaluated pair by pair and accumulated as integers; ``PressureProfileRecorder`` appends the
raw rows inside ``Simulation.run`` and ``pressure_profile_quantities`` turns raw rows into the quantities.

``RadialDistributionFunction`` is g(r) between two groups from exact integer pair counts (``csrc/rdf.hip``; not part of
the reference: azplugins had ``analyze.rdf`` in its HOOMD-2 line, the semantics are this project's);
``RDFRecorder`` appends the counts to a device table inside ``Simulation.run`` in the same way.

``BondedDistribution`` is the distribution of the bond lengths, the bending angles or the dihedral angles per group
type, from exact integer counts over the per-particle tables the bonded forces walk (``csrc/bonded_histogram.hip``;
this project's); ``BondedDistributionRecorder`` is its in-run recorder.

``StructureFactor`` is the partial static structure factor S_AB(q) on the reciprocal-lattice vectors of the box, by the
direct sum over the particles in a fixed order (``csrc/structure_factor.hip``; this project's);
``StructureFactorRecorder`` appends the density amplitudes to a device table inside ``Simulation.run``.

``Steinhardt`` is the bond-orientational order q_l of every particle of a group (optionally Lechner and Dellago's
neighbour average) and ``SolidLiquid`` ten Wolde and Frenkel's solid-bond count, from sums of spherical harmonics kept
as integers in units of 2^-40 (``csrc/steinhardt.hip``; this project's); ``SteinhardtRecorder`` and
``SolidLiquidRecorder`` append their summary row to a device table inside ``Simulation.run``.

``Cluster`` is the connected components of the particles of a group closer than ``r_max`` (optionally of those a
``SolidLiquid`` marks solid), labelled by a concurrent union-find on the device (``csrc/cluster.hip``; this project's,
DESIGN 4.29); ``ClusterRecorder`` appends its summary row to a device table inside ``Simulation.run``.

``ClusterProperties`` is the centre, the gyration tensor and the extent of every cluster of a ``Cluster``, from sums over
the cluster labels kept as integers (``csrc/cluster_properties.hip``; this project's);
``ClusterPropertiesRecorder`` appends the number of clusters and the row of the largest one inside ``Simulation.run``.

``MeanSquaredDisplacement`` and ``SelfIntermediateScattering`` measure dynamics: the moments of the displacement of a
group since a time origin (msd, its tensor, the fourth moment, the self part of the van Hove function) and F_s(q, t) on
the vector set of ``StructureFactor``. An origin is the wrapped position and the image of every particle stored BY TAG;
every sum runs in tag order in the reproducible reduction, so a result is bit-identical between two reads and under
the particle sorter (``csrc/displacement.hip``; this project's). ``MeanSquaredDisplacementRecorder`` and
``SelfIntermediateScatteringRecorder`` keep a ring of time origins on the device and write the rows of all of them with
one launch inside ``Simulation.run``; ``average_over_origins`` is their lag average.
``intermediate_scattering_from_amplitudes`` (``StructureFactorRecorder.intermediate_scattering``) is the collective
F(q, t) from the amplitudes that recorder already keeps, on the host.
"""

import ctypes as C
import itertools

import numpy as np

from . import _lib
from .filter import All, Type
from .methods import ConstantPressure, ConstantVolume
from .trigger import Periodic


class DataAccessError(_lib.AzpError):
    """A result was read from a compute that is not attached (``hoomd.error.DataAccessError``)."""

    def __init__(self, data_name):
        super().__init__("%s is not available until the compute is attached to a simulation with a state" % data_name)
        self.data_name = data_name


def _check_filter(filter):
    if filter is not None and not isinstance(filter, (All, Type)):
        raise _lib.AzpError("filter must be None, All() or Type(...), got %r" % (filter,))
    return filter


def _check_mpcd(include_mpcd_particles):
    if include_mpcd_particles:
        raise _lib.AzpError("include_mpcd_particles=True: azplugins_amd has no MPCD particle data")
    return False


class _Compute:
    """What the computes share: attachment through ``sim.operations``, the type masks and the device buffers. A row
    compute has ``_row_width()`` and ``_launch(d_out)``, which queues its kernels with one row of that many 8-byte words
    going to ``d_out``; its properties go through ``_read_row``, its recorder hands ``_launch`` a row of its table."""

    _coordinates = _lib.COORDINATES_CARTESIAN

    def __init__(self, filter, include_mpcd_particles):
        self._filter = _check_filter(filter)
        self._include_mpcd_particles = _check_mpcd(include_mpcd_particles)
        self._sim = None
        self._bufs = None  # key -> (sums, velocity, scratch)
        self._mask = None  # (types, device tensor or None)
        self._masks = None  # (types, mask a, mask b, device): the computes with a second filter
        self._row = None  # the (1, _row_width()) device row of a row compute
        self._scratch = None  # the scratch of its kernels

    @property
    def filter(self):
        return self._filter

    @property
    def include_mpcd_particles(self):
        return self._include_mpcd_particles

    @property
    def _attached(self):
        sim = self._sim
        return sim is not None and sim.state is not None and any(c is self for c in sim.operations.computes)

    def _type_mask(self, st):
        """Device byte mask of the included types, or None for All()."""
        import torch

        if isinstance(self._filter, All):
            return None
        if self._mask is None or self._mask[0] != st.types:
            m = torch.from_numpy(self._filter.mask(st.types)).to(st.device)
            self._mask = (list(st.types), m)
        return self._mask[1]

    def _type_masks(self, st):
        """Device byte masks of ``filter`` and ``filter_b`` (a compute between two groups), None for All()."""
        import torch

        if self._masks is None or self._masks[0] != st.types or self._masks[3] != st.device:
            m = [None if isinstance(f, All) else torch.from_numpy(f.mask(st.types)).to(st.device) for f in (self._filter, self._filter_b)]
            self._masks = (list(st.types), m[0], m[1], st.device)
        return self._masks[1], self._masks[2]

    def _row_buffer(self, width, dtype, attr="_row"):
        """The (1, width) device row kept in ``attr``: reused while device, width and dtype fit, else allocated."""
        import torch

        dev = self._sim.state.device
        dtype = getattr(torch, dtype)
        row = getattr(self, attr)
        if row is None or row.device != dev or row.shape[1] != width or row.dtype != dtype:
            row = torch.empty((1, width), dtype=dtype, device=dev)
            setattr(self, attr, row)
        return row

    def _set_scratch(self, a, size_name, minimum=256):
        """Asks ``size_name`` of libazp for the scratch the call ``a`` needs and points ``a`` at a device buffer of at
        least that many (and ``minimum``) bytes: reused until a call asks for more or the device changes."""
        import torch

        need = C.c_uint64(0)
        _lib.check(getattr(_lib.lib(), size_name)(C.byref(a), C.byref(need)), size_name)
        dev = self._sim.state.device
        if self._scratch is None or self._scratch.numel() < need.value or self._scratch.device != dev:
            self._scratch = torch.empty(max(int(need.value), minimum), dtype=torch.uint8, device=dev)
        a.d_scratch = self._scratch.data_ptr()
        a.scratch_bytes = self._scratch.numel()

    def _read_row(self, name, dtype="int64"):
        """One ``_launch`` on the current state into this compute's own row, which is returned: a (1, ``_row_width()``)
        device tensor. ``name``: the property being read, for ``DataAccessError``."""
        if not self._attached:
            raise DataAccessError(name)
        row = self._row_buffer(self._row_width(), dtype)
        self._launch(row.data_ptr())
        return row

    def _reduce(self, rows):
        """Rows of per-rank words (a (k, row width) device tensor; integer words are the uint64 of the kernels, all below
        2^63) added over the ranks of a decomposed run, as numpy."""
        dom = self._sim.domain
        if dom is not None:
            rows = _all_reduce_sum(dom, rows.clone())
        return rows.cpu().numpy()

    def _velocity_field(self, num_bins, lower, upper, name):
        """Mass-averaged velocity per bin, (bins, 3) float64 numpy, at the simulation's current state."""
        import torch

        if not self._attached:
            raise DataAccessError(name)
        n_bins = _total_bins(num_bins)
        if self._filter is None:
            return np.zeros((n_bins, 3))
        st = self._sim.state
        a = _lib.VelocityFieldArgs()
        a.d_pos = st.pos.data_ptr()
        a.d_vel = st.vel.data_ptr()
        a.N = st.N
        a.coordinates = self._coordinates
        a.box = st.box.to_c()
        for d in range(3):
            a.num_bins[d] = num_bins[d]
            a.lower[d] = lower[d]
            a.upper[d] = upper[d]
        mask = self._type_mask(st)
        a.ntypes = len(st.types)
        a.d_type_mask = mask.data_ptr() if mask is not None else None
        lib = _lib.lib()
        need = C.c_uint64(0)
        _lib.check(lib.azp_velocity_field_scratch_size(C.byref(a), C.byref(need)), "azp_velocity_field_scratch_size")
        bufs = self._bufs
        if bufs is None or bufs[0].shape[0] != n_bins or bufs[2].numel() < need.value:
            # (sized for this bin count and at least this scratch: resized when num_bins or N grows)
            f64 = torch.float64
            bufs = (torch.empty((n_bins, 4), dtype=f64, device=st.device), torch.empty((n_bins, 3), dtype=f64, device=st.device),
                    torch.empty(max(int(need.value), 8), dtype=torch.uint8, device=st.device))
            self._bufs = bufs
        sums, vel, scratch = bufs
        a.d_sums = sums.data_ptr()
        a.d_scratch = scratch.data_ptr()
        a.scratch_bytes = scratch.numel()
        stream = _lib.raw_stream(st.device)
        _lib.check(lib.azp_velocity_field_sums(C.byref(a), stream), "azp_velocity_field_sums")
        dom = self._sim.domain
        if dom is not None:
            sums = _all_reduce_sum(dom, sums)
        _lib.check(lib.azp_velocity_field_normalize(sums.data_ptr(), n_bins, vel.data_ptr(), stream), "azp_velocity_field_normalize")
        return vel.cpu().numpy()


def _all_reduce_sum(dom, sums):
    """Sums of every rank of the domain's group (HOOMD: MPI_Allreduce, src/VelocityFieldCompute.h:236-259)."""
    import torch.distributed as dist

    if dom.world == 1 or not dist.is_initialized():
        return sums
    if dist.get_backend(dom.group) == "gloo":
        # (gloo reduces host tensors, as DeviceDomain.all_reduce_flag)
        host = sums.cpu()
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=dom.group)
        sums.copy_(host)
        return sums
    dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=dom.group)
    return sums


def _total_bins(num_bins):
    n = 1
    for k in num_bins:
        if k > 0:
            n *= k
    return n


class VelocityCompute(_Compute):
    """Center-of-mass velocity of a group (reference ``src/compute.py:17-93``):
    v_cm = sum_i m_i v_i / sum_i m_i over the particles ``filter`` selects (``None``: no particles, velocity 0)."""

    def __init__(self, filter=None, include_mpcd_particles=False):
        super().__init__(filter, include_mpcd_particles)

    @property
    def velocity(self):
        """tuple[float]: center-of-mass velocity of the group."""
        v = self._velocity_field((0, 0, 0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), "velocity")
        return tuple(float(x) for x in v[0])


class VelocityFieldCompute(_Compute):
    """Mass-averaged velocity per bin (reference ``src/compute.py:96-245``). Use a derived type.

    ``num_bins``: bins along each of the three coordinates (0: the coordinate is not binned);
    ``lower_bounds`` / ``upper_bounds``: bounds of each binned coordinate (ignored where the count is 0). Particles
    outside the bounds are not counted. All three may be set after the compute is attached."""

    def __init__(self, num_bins, lower_bounds, upper_bounds, filter=None, include_mpcd_particles=False):
        super().__init__(filter, include_mpcd_particles)
        self.num_bins = num_bins
        self.lower_bounds = lower_bounds
        self.upper_bounds = upper_bounds
        self._check_bounds()

    @property
    def num_bins(self):
        return self._num_bins

    @num_bins.setter
    def num_bins(self, value):
        value = tuple(int(v) for v in value)
        if len(value) != 3:
            raise _lib.AzpError("num_bins needs 3 entries, got %r" % (value,))
        if any(v < 0 for v in value):
            raise _lib.AzpError("num_bins must not be negative, got %r" % (value,))
        if _total_bins(value) > _lib.MAX_BINS:
            raise _lib.AzpError("num_bins %r gives %d bins, more than 2^31 - 1" % (value, _total_bins(value)))
        self._num_bins = value

    @property
    def lower_bounds(self):
        return self._lower_bounds

    @lower_bounds.setter
    def lower_bounds(self, value):
        self._lower_bounds = _three_floats("lower_bounds", value)

    @property
    def upper_bounds(self):
        return self._upper_bounds

    @upper_bounds.setter
    def upper_bounds(self, value):
        self._upper_bounds = _three_floats("upper_bounds", value)

    def _check_bounds(self):
        # (checked at construction and at every computation, not per setter: the bounds are set one at a time)
        for d, (n, lo, hi) in enumerate(zip(self._num_bins, self._lower_bounds, self._upper_bounds)):
            if n > 0 and not hi > lo:
                raise _lib.AzpError("upper_bounds[%d] = %r must be larger than lower_bounds[%d] = %r" % (d, hi, d, lo))

    @property
    def _compact_shape(self):
        return [n for n in self._num_bins if n > 0]

    @property
    def coordinates(self):
        """numpy.ndarray: bin centers (``src/compute.py:206-231``): a 1-D array if one coordinate is binned, an array
        of shape (bins..., dims) if more are, ``None`` if none is."""
        coords = []
        shape = []
        for num, lo, hi in zip(self._num_bins, self._lower_bounds, self._upper_bounds):
            if num > 0:
                x, dx = np.linspace(lo, hi, num, endpoint=False, retstep=True)
                x += 0.5 * dx
                coords.append(x)
                shape.append(num)
        if len(shape) == 0:
            return None
        if len(shape) > 1:
            shape.append(len(shape))
        return np.reshape(list(itertools.product(*coords)), shape)

    @property
    def velocities(self):
        """numpy.ndarray: mass-averaged velocity of each bin, shape (binned dimensions..., 3), or (3,) if nothing is
        binned; 0 in a bin without mass."""
        if not self._attached:
            raise DataAccessError("velocities")
        self._check_bounds()
        v = self._velocity_field(self._num_bins, self._lower_bounds, self._upper_bounds, "velocities")
        return v.reshape(tuple(self._compact_shape) + (3,))


def _three_floats(name, value):
    value = tuple(float(v) for v in value)
    if len(value) != 3:
        raise _lib.AzpError("%s needs 3 entries, got %r" % (name, value))
    return value


class CartesianVelocityFieldCompute(VelocityFieldCompute):
    """Velocity field binned in (x, y, z) (reference ``src/compute.py:248-285``)."""

    _coordinates = _lib.COORDINATES_CARTESIAN


class CylindricalVelocityFieldCompute(VelocityFieldCompute):
    """Velocity field binned in (r, theta, z), 0 <= theta < 2 pi, velocities in the local (r, theta, z) basis
    (reference ``src/compute.py:288-339``)."""

    _coordinates = _lib.COORDINATES_CYLINDRICAL


# ---------------------------------------------------------------------------
# thermodynamic quantities
# ---------------------------------------------------------------------------
THERMO_PROPERTIES = ("num_particles", "volume", "translational_degrees_of_freedom", "rotational_degrees_of_freedom",
                     "degrees_of_freedom", "translational_kinetic_energy", "rotational_kinetic_energy", "kinetic_energy",
                     "potential_energy", "kinetic_temperature", "pressure_tensor", "pressure", "linear_momentum")


def thermo_quantities(sums, n_global, volume, conserves_momentum, rotational):
    """The quantities of ``THERMO_PROPERTIES`` from one row of sums (the 20 slots of ``azp_thermo_sums``, added over the
    ranks of a decomposed run). ``n_global``: particles of the whole system; ``volume``: box volume;
    ``conserves_momentum``: the integration method conserves the linear momentum (``ConstantVolume``), which removes
    the group's share 3 N_g / N_global of the three center-of-mass degrees of freedom; ``rotational``: the integrator
    integrates the rotational degrees of freedom. Plain Python floats in a fixed order: the properties and the
    recorder's table go through here and agree bit for bit."""
    s = [float(x) for x in sums]
    n_g = s[0]
    tdof = 3.0 * n_g
    if conserves_momentum and n_global > 0:
        tdof -= 3.0 * n_g / float(n_global)
    rdof = s[18] if rotational else 0.0
    dof = tdof + rdof
    ke_t = 0.5 * (s[4] + s[7] + s[9])
    ke_r = s[17]
    ke = ke_t + (ke_r if rotational else 0.0)
    p = tuple((s[4 + c] + s[10 + c]) / volume for c in range(6))
    return dict(num_particles=int(n_g), volume=volume, translational_degrees_of_freedom=tdof,
                rotational_degrees_of_freedom=rdof, degrees_of_freedom=dof, translational_kinetic_energy=ke_t,
                rotational_kinetic_energy=ke_r, kinetic_energy=ke, potential_energy=s[16],
                kinetic_temperature=2.0 * ke / dof if dof > 0.0 else 0.0, pressure_tensor=p,
                pressure=(p[0] + p[3] + p[5]) / 3.0, linear_momentum=(s[1], s[2], s[3]))


def _integrator_flags(integ):
    """(conserves_momentum, rotational) of ``thermo_quantities`` for an integrator: ``ConstantVolume`` and
    ``ConstantPressure`` conserve the linear momentum, ``flow.Langevin`` / ``flow.Brownian`` and an integrator without a
    method do not."""
    if integ is None:
        return False, False
    return any(isinstance(m, (ConstantVolume, ConstantPressure)) for m in integ.methods), bool(integ.integrate_rotational_dof)


class ThermodynamicQuantities(_Compute):
    """Thermodynamic properties of a group (``hoomd.md.compute.ThermodynamicQuantities``; D = 3). ``filter``:
    ``All()`` or ``Type(...)``. With K_ab = sum m v_a v_b, W_ab the sum of the per-particle virials and U the sum of
    the per-particle energies of every force of the integrator, over the group's particles, and V the box volume:

    - ``translational_kinetic_energy`` = (K_xx + K_yy + K_zz) / 2, ``rotational_kinetic_energy`` = sum_k s_k^2 / (2 I_k)
      over the axes with I_k != 0 (s = conj(q) p / 2), ``kinetic_energy`` their sum (the rotational part counts only if
      ``integrator.integrate_rotational_dof``), ``potential_energy`` = U;
    - ``translational_degrees_of_freedom`` = 3 N_g - 3 N_g / N_global under ``ConstantVolume`` (it conserves the
      momentum), 3 N_g under ``flow.Langevin`` / ``flow.Brownian`` or without a method;
      ``rotational_degrees_of_freedom`` = the number of non-zero inertia components if
      ``integrator.integrate_rotational_dof``, else 0;
    - ``kinetic_temperature`` = 2 ``kinetic_energy`` / ``degrees_of_freedom`` (0 without degrees of freedom);
    - ``pressure_tensor`` = (K_ab + W_ab) / V in the order xx, xy, xz, yy, yz, zz, ``pressure`` a third of its trace;
    - ``linear_momentum`` = sum m v.

    While a ``ThermodynamicQuantities`` is in ``sim.operations.computes``, ``Simulation.run`` turns ``compute_virial``
    on for every force of the integrator: THE VIRIAL PASS OF THE FORCE KERNELS THEN RUNS EVERY STEP. The pressure is
    available once the forces have been evaluated that way (``sim.run(0)``). At most 8 forces. Every property is
    computed when it is read, from the current state; two reads of the same state agree bit for bit."""

    def __init__(self, filter):
        if not isinstance(filter, (All, Type)):
            raise _lib.AzpError("ThermodynamicQuantities: filter must be All() or Type(...), got %r" % (filter,))
        super().__init__(filter, False)
        self._rotation = None  # (state, any particle has a non-zero moment of inertia)

    # -- one launch ----------------------------------------------------------
    def _forces_evaluated(self):
        """(energies known, virials known) for the forces of the integrator on the current state."""
        sim = self._sim
        integ = sim.operations.integrator
        forces = integ.forces if integ is not None else []
        st = sim.state
        ok = all(f._state is st and f._force is not None and f._force.shape[0] == st.N for f in forces)
        return ok, ok and all(getattr(f, "_virial_evaluated", False) for f in forces)

    def _row_width(self):
        return _lib.THERMO_NSUMS

    def _launch(self, d_out):
        """Queue ``azp_thermo_sums`` for the simulation's current state with the 20 doubles going to ``d_out``."""
        sim = self._sim
        st = sim.state
        integ = sim.operations.integrator
        forces = list(integ.forces) if integ is not None else []
        if len(forces) > _lib.THERMO_MAX_FORCES:
            raise _lib.AzpError("ThermodynamicQuantities sums at most %d forces, the integrator has %d"
                                % (_lib.THERMO_MAX_FORCES, len(forces)))
        a = _lib.ThermoArgs()
        a.d_vel = st.vel.data_ptr()
        a.N = st.N
        mask = self._type_mask(st)
        if mask is not None:
            a.d_pos = st.pos.data_ptr()
            a.d_type_mask = mask.data_ptr()
            a.ntypes = len(st.types)
        if self._forces_evaluated()[0]:
            a.n_forces = len(forces)
            for k, f in enumerate(forces):
                a.d_force[k] = f._force.data_ptr()
                a.d_virial[k] = f._virial.data_ptr() if getattr(f, "_virial_evaluated", False) else None
        if st.N and self._reads_rotation():
            # (a rank without particles has nothing to point at; the kernel zeroes the row)
            a.d_orientation, a.d_angmom, a.d_inertia = st.orientation.data_ptr(), st.angmom.data_ptr(), st.inertia.data_ptr()
        self._set_scratch(a, "azp_thermo_scratch_size", minimum=0)
        a.d_out = d_out
        _lib.check(_lib.lib().azp_thermo_sums(C.byref(a), _lib.raw_stream(st.device)), "azp_thermo_sums")

    def _prepare(self):
        """Called by ``Simulation.run`` ahead of the first step: does any particle have a moment of inertia? Without
        one the three rotational arrays (88 of the pass's bytes per particle) are not read and slots 17 and 18 are the
        zeros they would sum to. One small readback per ``run``, none inside it; a decomposed run always reads them
        (particles migrate between the ranks)."""
        sim = self._sim
        st = sim.state
        self._rotation = (st, bool(sim.domain is not None or st.N == 0 or (st.inertia[: st.N] != 0.0).any().item()))

    def _reads_rotation(self):
        if self._rotation is None or self._rotation[0] is not self._sim.state:
            self._prepare()
        integ = self._sim.operations.integrator
        return self._rotation[1] or bool(integ is not None and integ.integrate_rotational_dof)

    def _context(self, rows):
        """What ``thermo_quantities`` needs beside the rows (a (k, 20) device tensor of per-rank sums): the rows added
        over the ranks, as numpy, and (n_global, volume, conserves_momentum, rotational)."""
        import torch

        sim = self._sim
        st = sim.state
        dom = sim.domain
        host = self._reduce(rows)
        if dom is None:
            n_global = st.N
        elif isinstance(self._filter, All):
            n_global = int(host[0, 0]) if host.shape[0] else 0  # (no particle is created or destroyed during a run)
        else:
            n = _all_reduce_sum(dom, torch.tensor([float(st.N)], dtype=torch.float64, device=st.device))
            n_global = int(n.item())
        box = st.box
        return host, (n_global, box.Lx * box.Ly * box.Lz) + _integrator_flags(sim.operations.integrator)

    def _sums(self):
        """The row of sums of the current state, per rank, as a (1, 20) device tensor."""
        return self._read_row("sums", "float64")

    def _get(self, name):
        if not self._attached:
            raise DataAccessError(name)
        energies, virials = self._forces_evaluated()
        if name == "potential_energy" and not energies:
            raise _lib.AzpError("potential_energy: the forces have not been evaluated on this state; call sim.run(0)")
        if name in ("pressure", "pressure_tensor") and not virials:
            raise _lib.AzpError("%s: the last force evaluation ran without virials; call sim.run(0) with this compute in "
                                "sim.operations.computes" % name)
        host, ctx = self._context(self._sums())
        return thermo_quantities(host[0], *ctx)[name]


def _thermo_property(name):
    return property(lambda self: self._get(name), doc="``%s`` of the group at the current state." % name)


for _name in THERMO_PROPERTIES:
    setattr(ThermodynamicQuantities, _name, _thermo_property(_name))


class _Recorder:
    """What the recorders share: a compute of the same simulation (``_compute``, which the subclass sets), a trigger, and
    a device table of one row per recorded timestep that the compute's kernel writes straight into -- nothing is read
    back and the host never waits. The table grows by doubling; the copy is queued on the stream like everything
    else."""

    _dtype = "float64"

    def __init__(self, trigger):
        self.trigger = trigger if isinstance(trigger, Periodic) else Periodic(trigger)
        self.reset()

    def reset(self):
        """Forget the recorded rows."""
        self._rows = None  # (capacity, row width) device tensor
        self._steps = []
        self._volumes = []  # the volume of the box each row was recorded in (host data: no synchronisation)

    def _row_width(self):
        return self._compute._row_width()

    def _launch_row(self, d_out):
        """Queue the kernels that write one row of the table at ``d_out``."""
        self._compute._launch(d_out)

    def timesteps_in_run(self, t0, n):
        """The timesteps at which ``run(n)`` starting at timestep ``t0`` records: those of t0 + 1 ... t0 + n at which the
        trigger fires."""
        return [t for t in range(int(t0) + 1, int(t0) + int(n) + 1) if self.trigger(t)]

    def _record(self, sim, timestep):
        import torch

        st = sim.state
        k = len(self._steps)
        width = self._row_width()
        rows = self._rows
        if rows is not None and k and rows.shape[1] != width:
            raise _lib.AzpError("%s: the row width changed from %d to %d with rows recorded; call reset() first"
                                % (type(self).__name__, rows.shape[1], width))
        if rows is None or rows.device != st.device or k >= rows.shape[0] or rows.shape[1] != width:
            # (grown by doubling; the copy is queued on the stream like everything else)
            grown = torch.empty((max(64, 2 * k), width), dtype=getattr(torch, self._dtype), device=st.device)
            if k:
                grown[:k].copy_(rows[:k])
            self._rows = rows = grown
        self._launch_row(rows.data_ptr() + k * width * 8)
        self._steps.append(int(timestep))
        self._volumes.append(st.box.volume)  # (an update.BoxResize may change the box before the row is read)

    @property
    def timesteps(self):
        """numpy int64: the timesteps recorded so far."""
        return np.array(self._steps, dtype=np.int64)


class ThermodynamicRecorder(_Recorder):
    """Writer (``sim.operations.writers``) that appends the sums behind ``thermo`` (a ``ThermodynamicQuantities`` in
    ``computes`` of the same simulation) to a device table at the timesteps ``trigger`` (an ``int`` period or a
    ``Periodic``) fires -- the kernel writes straight into row k of the table, nothing is read back and the host never
    waits. In ``run(n)`` starting at timestep t0 the trigger is evaluated at t0 + 1 ... t0 + n; the row of timestep t
    is the state after t complete steps (after step two, with the forces of that configuration). ``Simulation.run``
    runs step two of that step on its own there instead of fused with the next step one: the trajectory is the same
    bit for bit with and without a recorder. ``timesteps`` and ``table`` are read after the run; ``reset()`` forgets the
    recorded rows."""

    def __init__(self, thermo, trigger):
        if not isinstance(thermo, ThermodynamicQuantities):
            raise _lib.AzpError("ThermodynamicRecorder: thermo must be a ThermodynamicQuantities, got %r" % (thermo,))
        self.thermo = self._compute = thermo
        super().__init__(trigger)

    @property
    def table(self):
        """dict of numpy arrays keyed by the property names of ``ThermodynamicQuantities``, one entry per recorded
        timestep (``pressure_tensor``: (rows, 6), ``linear_momentum``: (rows, 3)). On a decomposed run the rows of all
        ranks are added here, in one reduction."""
        k = len(self._steps)
        if k == 0:
            return {name: np.zeros((0,) + ((6,) if name == "pressure_tensor" else (3,) if name == "linear_momentum" else ()),
                                   dtype=np.int64 if name == "num_particles" else np.float64) for name in THERMO_PROPERTIES}
        if not self.thermo._attached:
            raise DataAccessError("table")
        host, ctx = self.thermo._context(self._rows[:k])
        # (each row with the volume of the box it was recorded in, not the box of this moment)
        rows = [thermo_quantities(host[i], ctx[0], self._volumes[i], *ctx[2:]) for i in range(k)]
        return {name: np.array([r[name] for r in rows]) for name in THERMO_PROPERTIES}


# ---------------------------------------------------------------------------
# thermodynamic field
# ---------------------------------------------------------------------------
THERMO_FIELD_PROPERTIES = ("counts", "num_particles", "bin_volumes", "number_density", "mass_density", "velocities",
                           "kinetic_temperature", "pressure_tensor", "pressure", "potential_energy_density", "sums")
_THERMO_FIELD_NEEDS_VOLUME = ("bin_volumes", "number_density", "mass_density", "pressure_tensor", "pressure",
                              "potential_energy_density")
_TENSOR_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))  # xx, xy, xz, yy, yz, zz
RECORDER_MAX_BYTES = 2**30


def thermo_field_quantities(rows, bin_volumes, streaming):
    """The quantities of ``THERMO_FIELD_PROPERTIES`` from raw rows of ``azp_thermo_field_sums``: ``rows`` has shape
    (..., 18 + ntypes) (slots n, M, P, K, W, U, counts per type; added over the ranks of a decomposed run),
    ``bin_volumes`` the shape of ``rows`` without its last axis (or one that broadcasts to it), or ``None``: the
    quantities that divide by a volume are then left out. ``streaming``: ``"subtract"`` (K'_ab = K_ab - P_a P_b / M,
    ``kinetic_temperature`` = tr K' / (3 n - 3), 0 for n < 2) or ``"keep"`` (K' = K, tr K / (3 n), 0 for n = 0). Plain
    numpy in a fixed order: the properties, the recorder's ``table`` and ``mean()`` go through here and agree bit for
    bit."""
    if streaming not in ("subtract", "keep"):
        raise _lib.AzpError("streaming must be 'subtract' or 'keep', got %r" % (streaming,))
    rows = np.asarray(rows, dtype=np.float64)
    if rows.shape[-1] < _lib.THERMO_FIELD_NSUMS:
        raise _lib.AzpError("thermo_field_quantities: a row has at least %d words, got %d" % (_lib.THERMO_FIELD_NSUMS, rows.shape[-1]))
    n, mass = rows[..., 0], rows[..., 1]
    mom, kin, vir, pot = rows[..., 2:5], rows[..., 5:11], rows[..., 11:17], rows[..., 17]
    has_mass = mass > 0.0
    safe_mass = np.where(has_mass, mass, 1.0)
    vel = np.where(has_mass[..., None], mom / safe_mass[..., None], 0.0)
    if streaming == "subtract":
        flow = np.stack([mom[..., a] * mom[..., b] / safe_mass for a, b in _TENSOR_PAIRS], axis=-1)
        kin = kin - np.where(has_mass[..., None], flow, 0.0)
        dof = 3.0 * n - 3.0
        counted = n >= 2.0
    else:
        dof = 3.0 * n
        counted = n >= 1.0
    trace = kin[..., 0] + kin[..., 3] + kin[..., 5]
    out = dict(counts=np.rint(rows[..., _lib.THERMO_FIELD_NSUMS:]).astype(np.int64), num_particles=np.rint(n).astype(np.int64),
               velocities=vel, kinetic_temperature=np.where(counted, trace / np.where(counted, dof, 1.0), 0.0), sums=rows)
    if bin_volumes is not None:
        vol = np.broadcast_to(np.asarray(bin_volumes, dtype=np.float64), n.shape)
        p = (kin + vir) / vol[..., None]
        out.update(bin_volumes=vol, number_density=out["counts"] / vol[..., None], mass_density=mass / vol, pressure_tensor=p,
                   pressure=(p[..., 0] + p[..., 3] + p[..., 5]) / 3.0, potential_energy_density=pot / vol)
    return out


class ThermodynamicField(VelocityFieldCompute):
    """Density, temperature and stress per bin (this project's). Use a derived type.

    ``num_bins`` / ``lower_bounds`` / ``upper_bounds`` / ``coordinates`` are those of ``VelocityFieldCompute``: 0 bins
    means the coordinate is not binned, particles outside the bounds are not counted, ghosts never are. ``filter``:
    ``All()`` or ``Type(...)``. Per bin, with n the particle count, M = sum m, P = sum m v, K_ab = sum m v_a v_b, W_ab the
    sum of the per-particle virials of every force of the integrator, U the sum of the per-particle energies and V_bin
    the volume of the bin:

    - ``counts`` (int64, trailing axis: the state's types; exact), ``num_particles`` = n, ``bin_volumes``,
      ``number_density`` = counts / V_bin per type, ``mass_density`` = M / V_bin;
    - ``velocities`` = P / M, 0 in a bin without mass (``VelocityFieldCompute.velocities``; in the cylindrical field in
      the local (r, theta, z) basis, computed by that compute's kernel);
    - ``streaming="subtract"``: K'_ab = K_ab - P_a P_b / M and ``kinetic_temperature`` = tr K' / (3 n - 3), 0 for
      n < 2; ``"keep"``: K' = K and tr K / (3 n);
    - ``pressure_tensor`` = (K'_ab + W_ab) / V_bin in the order xx, xy, xz, yy, yz, zz, ``pressure`` a third of its
      trace, ``potential_energy_density`` = U / V_bin;
    - ``sums``: the raw row (bins..., 18 + types) of ``azp_thermo_field_sums``.

    THE STRESS IS THE PER-ATOM (IK1) PROFILE: the virial of a pair is shared in halves between its two particles and
    counted in the bins they sit in. It is not the Irving-Kirkwood contour integral (method of planes); the two differ
    where the density varies over the range of the forces. In the cylindrical field P, K and W stay Cartesian.

    V_bin: Cartesian, V_box times the product over the binned axes of width_d / L_d (also in a tilted box);
    cylindrical, (r1^2 - r0^2) / 2 x dtheta x dz with dtheta = 2 pi and dz = Lz where theta / z are not binned -- r must
    be binned, else every property that divides by a volume raises.

    While a ``ThermodynamicField`` is in ``sim.operations.computes``, ``Simulation.run`` turns ``compute_virial`` on for
    every force, as for ``ThermodynamicQuantities``; ``pressure*`` and ``potential_energy_density`` need the forces
    evaluated that way (``sim.run(0)``). At most 8 forces. Every property is computed when it is read. The sum of a bin
    is a fixed 64-ary tree over its members in tag order: two reads of a state, and reads before and after a
    reordering of the rows that carries the tags (``ParticleSorter``), agree bit for bit (single domain)."""

    def __init__(self, num_bins, lower_bounds, upper_bounds, filter=None, streaming="subtract"):
        filter = All() if filter is None else filter
        if not isinstance(filter, (All, Type)):
            raise _lib.AzpError("%s: filter must be All() or Type(...), got %r" % (type(self).__name__, filter))
        super().__init__(num_bins, lower_bounds, upper_bounds, filter, False)
        self.streaming = streaming
        self._keys = None

    @property
    def streaming(self):
        return self._streaming

    @streaming.setter
    def streaming(self, value):
        if value not in ("subtract", "keep"):
            raise _lib.AzpError("streaming must be 'subtract' or 'keep', got %r" % (value,))
        self._streaming = value

    _forces_evaluated = ThermodynamicQuantities._forces_evaluated

    def _row_width(self):
        return _total_bins(self._num_bins) * (_lib.THERMO_FIELD_NSUMS + len(self._sim.state.types))

    def _launch(self, d_out):
        """Queue the key kernel, the sort and ``azp_thermo_field_sums`` for the current state, the row going to
        ``d_out``."""
        import torch

        self._check_bounds()
        sim = self._sim
        st = sim.state
        integ = sim.operations.integrator
        forces = list(integ.forces) if integ is not None else []
        if len(forces) > _lib.THERMO_MAX_FORCES:
            raise _lib.AzpError("%s sums at most %d forces, the integrator has %d"
                                % (type(self).__name__, _lib.THERMO_MAX_FORCES, len(forces)))
        a = _lib.ThermoFieldArgs()
        a.d_pos, a.d_vel, a.d_tag = st.pos.data_ptr(), st.vel.data_ptr(), st.tag.data_ptr()
        a.N = st.N
        a.coordinates = self._coordinates
        a.box = st.box.to_c()
        for d in range(3):
            a.num_bins[d], a.lower[d], a.upper[d] = self._num_bins[d], self._lower_bounds[d], self._upper_bounds[d]
        mask = self._type_mask(st)
        a.ntypes = len(st.types)
        a.d_type_mask = mask.data_ptr() if mask is not None else None
        if self._forces_evaluated()[0]:
            a.n_forces = len(forces)
            for k, f in enumerate(forces):
                a.d_force[k] = f._force.data_ptr()
                a.d_virial[k] = f._virial.data_ptr() if getattr(f, "_virial_evaluated", False) else None
        self._set_scratch(a, "azp_thermo_field_scratch_size")
        a.d_out = d_out
        stream = _lib.raw_stream(st.device)
        if st.N:
            if self._keys is None or self._keys.shape[0] != st.N or self._keys.device != st.device:
                self._keys = torch.empty(st.N, dtype=torch.int64, device=st.device)
            a.d_keys = self._keys.data_ptr()
            _lib.check(_lib.lib().azp_thermo_field_keys(C.byref(a), stream), "azp_thermo_field_keys")
            # (the keys are unique: any sort gives the one order, by bin and then by tag; queued on the stream)
            keys, order = torch.sort(self._keys)
            a.d_sorted_keys, a.d_order = keys.data_ptr(), order.data_ptr()
        _lib.check(_lib.lib().azp_thermo_field_sums(C.byref(a), stream), "azp_thermo_field_sums")

    def _bin_volumes(self, box):
        """Volume of every bin in ``box`` (raveled, float64), or None where it is not defined (no r binning)."""
        raise NotImplementedError

    def _shape_rows(self, host):
        """(k, row width) host rows as (k, bins, 18 + types)."""
        return host.reshape(host.shape[0], _total_bins(self._num_bins), -1)

    def _get(self, name):
        if not self._attached:
            raise DataAccessError(name)
        self._check_bounds()
        energies, virials = self._forces_evaluated()
        if name == "potential_energy_density" and not energies:
            raise _lib.AzpError("%s: the forces have not been evaluated on this state; call sim.run(0)" % name)
        if name in ("pressure", "pressure_tensor") and not virials:
            raise _lib.AzpError("%s: the last force evaluation ran without virials; call sim.run(0) with this compute in "
                                "sim.operations.computes" % name)
        vol = self._bin_volumes(self._sim.state.box)
        if vol is None and name in _THERMO_FIELD_NEEDS_VOLUME:
            raise _lib.AzpError("%s: the volume of a cylindrical bin needs the r coordinate binned" % name)
        shape = tuple(self._compact_shape)
        if name == "bin_volumes":
            return vol.reshape(shape)
        if name == "velocities" and self._coordinates == _lib.COORDINATES_CYLINDRICAL:
            v = self._velocity_field(self._num_bins, self._lower_bounds, self._upper_bounds, name)
            return v.reshape(shape + (3,))
        rows = self._shape_rows(self._reduce(self._read_row(name, "float64")))[0]
        value = thermo_field_quantities(rows, vol, self._streaming)[name]
        return value.reshape(shape + value.shape[1:])


def _thermo_field_property(name):
    return property(lambda self: self._get(name), doc="``%s`` of every bin at the current state." % name)


for _name in THERMO_FIELD_PROPERTIES:
    setattr(ThermodynamicField, _name, _thermo_field_property(_name))


class CartesianThermodynamicField(ThermodynamicField):
    """``ThermodynamicField`` binned in (x, y, z)."""

    _coordinates = _lib.COORDINATES_CARTESIAN

    def _bin_volumes(self, box):
        v = box.volume
        for n, lo, hi, length in zip(self._num_bins, self._lower_bounds, self._upper_bounds, (box.Lx, box.Ly, box.Lz)):
            if n > 0:
                v *= ((hi - lo) / n) / length
        return np.full(_total_bins(self._num_bins), v, dtype=np.float64)


class CylindricalThermodynamicField(ThermodynamicField):
    """``ThermodynamicField`` binned in (r, theta, z), 0 <= theta < 2 pi. The sums stay Cartesian; ``velocities`` is in
    the local (r, theta, z) basis, as ``CylindricalVelocityFieldCompute`` gives it."""

    _coordinates = _lib.COORDINATES_CYLINDRICAL

    def _bin_volumes(self, box):
        nr, nt, nz = self._num_bins
        if nr == 0:
            return None
        edges = np.linspace(self._lower_bounds[0], self._upper_bounds[0], nr + 1)
        area = 0.5 * (edges[1:] ** 2 - edges[:-1] ** 2)
        dtheta = (self._upper_bounds[1] - self._lower_bounds[1]) / nt if nt > 0 else 2.0 * np.pi
        dz = (self._upper_bounds[2] - self._lower_bounds[2]) / nz if nz > 0 else box.Lz
        return np.repeat(area * dtheta * dz, max(nt, 1) * max(nz, 1))


class ThermodynamicFieldRecorder(_Recorder):
    """Writer (``sim.operations.writers``) that appends the raw row of ``field`` (a ``ThermodynamicField`` in
    ``computes`` of the same simulation) to a device table at the timesteps ``trigger`` fires, as
    ``ThermodynamicRecorder`` does: the kernels write row k of the table, nothing is read back, and the trajectory is
    the same bit for bit with and without it. A row is bins x (18 + types) words: a ``_record`` that would grow the table
    beyond 2^30 bytes raises. ``table`` is the dict of ``thermo_field_quantities`` with a leading axis of recorded
    timesteps, every row normalised with the bin volumes of the box it was recorded in (the local-basis ``velocities``
    of a cylindrical field is not in the rows: ``velocities`` is the Cartesian P / M here); ``mean()`` the same
    quantities from the rows SUMMED FIRST and then normalised with the summed volumes (the convention of
    ``average_over_origins``: with ``streaming="subtract"`` the streaming velocity is that of the summed momentum and
    three degrees of freedom are removed once). On a decomposed run the rows of all ranks are added in one reduction."""

    def __init__(self, field, trigger):
        if not isinstance(field, ThermodynamicField):
            raise _lib.AzpError("ThermodynamicFieldRecorder: field must be a ThermodynamicField, got %r" % (field,))
        self.field = self._compute = field
        super().__init__(trigger)

    def reset(self):
        super().reset()
        self._bin_volumes = []  # per row: the bin volumes in the box it was recorded in (host data)

    @staticmethod
    def _grown_bytes(k, capacity, width):
        """Bytes of the table after row k is recorded into a table of ``capacity`` rows of ``width`` words (the base
        class grows it by doubling, to at least 64 rows)."""
        rows = capacity if k < capacity else max(64, 2 * k)
        return rows * width * 8

    def _record(self, sim, timestep):
        k = len(self._steps)
        width = self._row_width()
        fits = self._rows is not None and self._rows.shape[1] == width and self._rows.device == sim.state.device
        need = self._grown_bytes(k, self._rows.shape[0] if fits else 0, width)
        if need > RECORDER_MAX_BYTES:
            raise _lib.AzpError("%s: recording row %d of %d words would grow the table to %d bytes, more than 2^30; record "
                                "fewer bins or reset() more often" % (type(self).__name__, k, width, need))
        super()._record(sim, timestep)
        self._bin_volumes.append(self.field._bin_volumes(sim.state.box))

    def _host_rows(self, name):
        k = len(self._steps)
        if not self.field._attached:
            raise DataAccessError(name)
        rows = self.field._shape_rows(self.field._reduce(self._rows[:k]))
        vol = None if any(v is None for v in self._bin_volumes) else np.array(self._bin_volumes, dtype=np.float64).reshape(k, -1)
        return rows, vol

    def _shaped(self, q, lead):
        shape = lead + tuple(self.field._compact_shape)
        return {name: v.reshape(shape + v.shape[len(lead) + 1:]) for name, v in q.items()}

    @property
    def table(self):
        """dict of numpy arrays keyed by ``THERMO_FIELD_PROPERTIES``, shape (rows, bins..., trailing axis)."""
        k = len(self._steps)
        if k == 0:
            return {}
        rows, vol = self._host_rows("table")
        return self._shaped(thermo_field_quantities(rows, vol, self.field.streaming), (k,))

    def mean(self):
        """dict of the same quantities from the sum of the recorded rows and the sum of their bin volumes."""
        if len(self._steps) == 0:
            return {}
        rows, vol = self._host_rows("mean")
        return self._shaped(thermo_field_quantities(rows.sum(axis=0), None if vol is None else vol.sum(axis=0),
                                                    self.field.streaming), ())


# ---------------------------------------------------------------------------
# radial distribution function
# ---------------------------------------------------------------------------
def _shell_volumes(num_bins, r_max):
    edges = np.linspace(0.0, float(r_max), int(num_bins) + 1)
    return (4.0 * np.pi / 3.0) * (edges[1:] ** 3 - edges[:-1] ** 3)


def _rdf_normalize(counts, n_pairs, volume, r_max):
    counts = np.asarray(counts)
    if n_pairs == 0:
        return np.zeros(counts.shape, dtype=np.float64)
    return counts.astype(np.float64) * (float(volume) / (float(n_pairs) * _shell_volumes(counts.shape[-1], r_max)))


def rdf_from_counts(counts, n_a, n_b, n_ab, volume, r_max):
    """g(r) from ordered pair counts: ``counts[k]`` pairs (i in A, j in B, i != j) in bin k of ``len(counts)`` equal
    bins on [0, r_max), ``n_a`` / ``n_b`` / ``n_ab`` the sizes of A, B and of their intersection, ``volume`` the box
    volume: g[k] = counts[k] V / (n_pairs (4 pi / 3)(r_(k+1)^3 - r_k^3)), n_pairs = n_a n_b - n_ab; zero when n_pairs is
    0. An ideal gas gives 1. The compute, the recorder and the tests all go through here."""
    return _rdf_normalize(counts, int(n_a) * int(n_b) - int(n_ab), volume, r_max)


def perpendicular_widths(box):
    """Distances between opposite faces of ``box`` (a ``state.Box``; HOOMD ``BoxDim.getNearestPlaneDistance``)."""
    return box.nearest_plane_distance


def _check_pair_range(name, box, r_max):
    """What every compute over the pairs closer than ``r_max`` asks of the box (``name``: the class, for the message): a
    3-D box, ``r_max`` at most half the perpendicular width of every periodic axis."""
    widths = perpendicular_widths(box)
    for d in range(3):
        if not widths[d] > 0.0:
            raise _lib.AzpError("%s: a 3-D box is needed (2-D systems are not supported), got %r" % (name, box))
        if box.periodic[d] and r_max > 0.5 * widths[d]:
            raise _lib.AzpError("%s: r_max = %r is larger than half the perpendicular width %r of periodic axis %d: the "
                                "minimum image would not be unique" % (name, r_max, widths[d], d))


def _check_rdf_filter(name, f):
    if not isinstance(f, (All, Type)):
        raise _lib.AzpError("RadialDistributionFunction: %s must be All() or Type(...), got %r" % (name, f))
    return f


class RadialDistributionFunction(_Compute):
    """Radial distribution function g(r) between the groups ``filter_a`` and ``filter_b`` (``All()`` or ``Type(...)``;
    they may overlap) of a 3-D system, on ``num_bins`` equal bins of [0, ``r_max``).

    ``counts[k]`` is the number of ORDERED pairs (i in A, j in B, i != j) whose minimum-image distance r lies in bin k: a
    pair counts iff r^2 < r_max^2 (lower bin edges inclusive, r == r_max excluded), r is the correctly rounded square
    root and k = min(int(r * (num_bins / r_max)), num_bins - 1). The counts are exact integers and two reads of one
    state agree bit for bit. ``rdf`` = ``rdf_from_counts(counts, N_A, N_B, N_AB, V, r_max)``, i.e.
    counts[k] V / (num_pairs (4 pi / 3)(r_(k+1)^3 - r_k^3)) with ``num_pairs`` = N_A N_B - N_AB.

    Refused with ``AzpError``: ``r_max <= 0``, ``num_bins`` outside [1, 8192], a filter that is not ``All()`` or
    ``Type(...)`` (at construction or assignment); ``r_max`` larger than half the smallest perpendicular width of a
    periodic axis of the box (when a property is read: the minimum image would not be unique). ``path``: 0 (default)
    takes the cell-list kernel wherever the box allows it (orthorhombic, at least three cells of width ``r_max`` on
    every periodic axis) and the all-pairs kernel elsewhere, 1 / 2 force one of them; a forced path the box does not
    allow is refused. On a decomposed run each rank counts its own particles against its own particles and ghosts and
    the counts are added over the ranks (every rank gets the same result); ghosts are complete out to the
    decomposition's ``r_ghost`` minus the neighbor-list buffer, a larger ``r_max`` is refused.

    ``exclusions``: the names a neighbor list takes (``nlist.NeighborList``; ``state.EXCLUSIONS``), default none. The
    pairs they name are taken out of the counts again by a second kernel behind the pair pass
    (``azp_rdf_subtract_excluded``): with ``("bond", "1-3", "1-4")`` on chains, what is left is the INTERMOLECULAR g(r)
    plus the intramolecular pairs four or more bonds apart. ``num_pairs`` and with it the normalisation stay as they
    are, so g(r) still tends to 1. ``excluded_pairs`` is the number of ordered pairs taken out. Single-domain states
    only: on a decomposed run a non-empty ``exclusions`` is an ``AzpError`` (a particle that is its own periodic ghost
    sits on two rows, and the exclusion table names one of them).

    Every property is computed when it is read, from the current state."""

    def __init__(self, filter_a, filter_b, r_max, num_bins, exclusions=()):
        from .state import check_exclusions

        super().__init__(_check_rdf_filter("filter_a", filter_a), False)
        self._filter_b = _check_rdf_filter("filter_b", filter_b)
        self.exclusions = tuple(exclusions)
        self._exclusion_kinds = check_exclusions(self.exclusions, "RadialDistributionFunction(exclusions=...)")
        self.r_max = r_max
        self.num_bins = num_bins
        self.path = _lib.RDF_PATH_AUTO

    filter_a = _Compute.filter

    @property
    def filter_b(self):
        return self._filter_b

    @property
    def r_max(self):
        return self._r_max

    @r_max.setter
    def r_max(self, value):
        value = float(value)
        if not (value > 0.0 and np.isfinite(value)):
            raise _lib.AzpError("RadialDistributionFunction: r_max must be positive, got %r" % (value,))
        self._r_max = value

    @property
    def num_bins(self):
        return self._num_bins

    @num_bins.setter
    def num_bins(self, value):
        if isinstance(value, bool) or int(value) != value or int(value) < 1:
            raise _lib.AzpError("RadialDistributionFunction: num_bins must be a positive integer, got %r" % (value,))
        if int(value) > _lib.RDF_MAX_BINS:
            raise _lib.AzpError("RadialDistributionFunction: num_bins = %d is more than the %d bins of AZP_RDF_MAX_BINS"
                                % (value, _lib.RDF_MAX_BINS))
        self._num_bins = int(value)

    @property
    def path(self):
        return self._path

    @path.setter
    def path(self, value):
        if value not in (_lib.RDF_PATH_AUTO, _lib.RDF_PATH_ALL_PAIRS, _lib.RDF_PATH_CELLS):
            raise _lib.AzpError("RadialDistributionFunction: path must be 0 (auto), 1 (all-pairs) or 2 (cells), got %r" % (value,))
        self._path = int(value)

    @property
    def bin_edges(self):
        """numpy.ndarray: the ``num_bins + 1`` edges of the bins."""
        return np.linspace(0.0, self._r_max, self._num_bins + 1)

    @property
    def bin_centers(self):
        e = self.bin_edges
        return 0.5 * (e[1:] + e[:-1])

    # -- one launch ----------------------------------------------------------
    def _row_width(self):
        return self._num_bins + 4

    def _check_box(self, sim):
        _check_pair_range("RadialDistributionFunction", sim.state.box, self._r_max)
        dom = sim.domain
        if dom is not None:
            integ = sim.operations.integrator
            lists = [f.nlist for f in (integ.forces if integ is not None else []) if getattr(f, "nlist", None) is not None]
            buffer = max([float(nl.buffer) for nl in lists], default=0.0)
            if self._r_max > dom.decomp.r_ghost - buffer:
                raise _lib.AzpError("RadialDistributionFunction: r_max = %r is beyond the ghost coverage %r of this decomposed run "
                                    "(r_ghost = %r minus the neighbor-list buffer %r)"
                                    % (self._r_max, dom.decomp.r_ghost - buffer, dom.decomp.r_ghost, buffer))

    def _launch(self, d_out):
        """Queue ``azp_rdf_counts`` for the simulation's current state with the ``num_bins + 4`` words going to ``d_out``."""
        sim = self._sim
        st = sim.state
        self._check_box(sim)
        a = _lib.RdfArgs()
        a.d_pos = st.pos.data_ptr()
        a.N = st.N
        a.n_total = st.n_max
        a.box = st.box.to_c()
        a.ntypes = len(st.types)
        mask_a, mask_b = self._type_masks(st)
        a.d_type_mask_a = mask_a.data_ptr() if mask_a is not None else None
        a.d_type_mask_b = mask_b.data_ptr() if mask_b is not None else None
        a.num_bins = self._num_bins
        a.r_max = self._r_max
        a.scale = self._num_bins / self._r_max
        a.path = self._path
        lib = _lib.lib()
        self._set_scratch(a, "azp_rdf_scratch_size")  # (for this N, box, r_max and path)
        a.d_out = d_out
        kinds = self._exclusion_kinds
        if kinds and sim.domain is not None:
            raise _lib.AzpError("RadialDistributionFunction: exclusions are not supported on a decomposed run (a particle "
                                "that is its own periodic ghost sits on two rows, the exclusion table names one)")
        stream = _lib.raw_stream(st.device)
        _lib.check(lib.azp_rdf_counts(C.byref(a), stream), "azp_rdf_counts")
        if kinds and any(g.n for g in st.groups.values()):
            x = _lib.RdfExclusionArgs()
            x.rdf = a
            n_excl, excl, pitch = st.merged_exclusion_table(kinds)
            x.d_n_excl, x.d_excl, x.excl_pitch = n_excl.data_ptr(), excl.data_ptr(), pitch
            _lib.check(lib.azp_rdf_subtract_excluded(C.byref(x), stream), "azp_rdf_subtract_excluded")

    def _read(self, name):
        return self._reduce(self._read_row(name))[0]

    def _volume(self):
        box = self._sim.state.box
        return box.Lx * box.Ly * box.Lz

    @property
    def counts(self):
        """numpy int64 (num_bins,): ordered pair counts per bin."""
        return self._read("counts")[: self._num_bins].copy()

    @property
    def group_sizes(self):
        """tuple[int]: (N_A, N_B, N_AB), the sizes of the two groups and of their intersection."""
        return tuple(int(x) for x in self._read("group_sizes")[self._num_bins:self._num_bins + 3])

    @property
    def num_pairs(self):
        """int: N_A N_B - N_AB over the owned particles of the whole system."""
        n_a, n_b, n_ab = (int(x) for x in self._read("num_pairs")[self._num_bins:self._num_bins + 3])
        return n_a * n_b - n_ab

    @property
    def excluded_pairs(self):
        """int: the ordered pairs that ``exclusions`` took out of the counts (0 without exclusions)."""
        return int(self._read("excluded_pairs")[self._num_bins + 3])

    @property
    def rdf(self):
        """numpy float64 (num_bins,): g(r) on ``bin_centers``."""
        row = self._read("rdf")
        nb = self._num_bins
        return rdf_from_counts(row[:nb], row[nb], row[nb + 1], row[nb + 2], self._volume(), self._r_max)


class RDFRecorder(_Recorder):
    """Writer (``sim.operations.writers``) that appends the pair counts of ``rdf`` (a ``RadialDistributionFunction`` in
    ``computes`` of the same simulation) to a device table of ``num_bins + 4`` words per row at the timesteps ``trigger``
    (an ``int`` period or a ``Periodic``) fires, as ``ThermodynamicRecorder`` does with its sums: the kernel writes row k
    itself, nothing is read back and the host does not wait; the trajectory is the same bit for bit with and without
    the recorder. Read after the run: ``timesteps``, ``counts`` and ``rdf`` (frames, num_bins) -- each frame normalised
    with its own N_A, N_B and N_AB, which keeps it right while an evaporator changes types -- and ``mean_rdf``, the sum of
    the counts over the sum of the pair numbers. On a decomposed run the whole table is reduced once, when it is read.
    ``reset()`` forgets the recorded frames (needed before ``rdf.num_bins`` changes)."""

    _dtype = "int64"

    def __init__(self, rdf, trigger):
        if not isinstance(rdf, RadialDistributionFunction):
            raise _lib.AzpError("RDFRecorder: rdf must be a RadialDistributionFunction, got %r" % (rdf,))
        self.rdf_compute = self._compute = rdf
        super().__init__(trigger)

    def _table(self, name):
        k = len(self._steps)
        if k == 0:
            return np.zeros((0, self._row_width()), dtype=np.int64)
        if not self.rdf_compute._attached:
            raise DataAccessError(name)
        return self.rdf_compute._reduce(self._rows[:k])

    @property
    def counts(self):
        """numpy int64 (frames, num_bins)."""
        t = self._table("counts")
        return t[:, : t.shape[1] - 4].copy()

    @staticmethod
    def _pairs(t):
        nb = t.shape[1] - 4
        return [int(r[nb]) * int(r[nb + 1]) - int(r[nb + 2]) for r in t]

    @property
    def num_pairs(self):
        """list of int: N_A N_B - N_AB of each frame."""
        return self._pairs(self._table("num_pairs"))

    @property
    def rdf(self):
        """numpy float64 (frames, num_bins): each frame with its own normalisation."""
        t = self._table("rdf")
        nb = t.shape[1] - 4
        c = self.rdf_compute
        if t.shape[0] == 0:
            return np.zeros((0, nb))
        return np.stack([rdf_from_counts(r[:nb], r[nb], r[nb + 1], r[nb + 2], vol, c.r_max) for r, vol in zip(t, self._volumes)])

    @property
    def mean_rdf(self):
        """numpy float64 (num_bins,): sum of the counts of all frames over the sum of their pair numbers."""
        t = self._table("mean_rdf")
        nb = t.shape[1] - 4
        if t.shape[0] == 0:
            return np.zeros(nb)
        c = self.rdf_compute
        vols = self._volumes
        if all(v == vols[0] for v in vols):  # one box throughout: the counts are added as integers
            return _rdf_normalize(t[:, :nb].sum(axis=0), sum(self._pairs(t)), vols[0], c.r_max)
        # frames recorded in different boxes: each frame's counts weighted with its own volume
        weighted = (t[:, :nb].astype(np.float64) * np.array(vols)[:, None]).sum(axis=0)
        return _rdf_normalize(weighted, sum(self._pairs(t)), 1.0, c.r_max)


# ---------------------------------------------------------------------------
# distributions of the bonded coordinates
# ---------------------------------------------------------------------------
def distribution_from_counts(counts, num_groups, bin_width):
    """``counts / (num_groups * bin_width)`` per type (rows of ``counts``), zeros where a type has no groups. The
    compute, the recorder and the tests all go through here."""
    counts = np.asarray(counts, dtype=np.float64)
    n = np.asarray(num_groups, dtype=np.float64).reshape(-1, 1)
    return np.divide(counts, n * float(bin_width), out=np.zeros(counts.shape), where=n > 0)


class BondedDistribution(_Compute):
    """Distributions of the bonded coordinates of a state, one histogram per group type: the bond lengths
    (``kind="bond"``), the lengths of the special pairs (``"pair"``), the bending angles (``"angle"``) or the dihedral
    angles (``"dihedral"``) -- what a tabulated bonded potential (``bond.Table``, ``angle.Table``, ``dihedral.Table``) is
    inverted from. Not part of the reference; the semantics are this project's (``include/azp.h``).

    The coordinate of a group, with the minimum image of the force kernels:

    * bond, pair: ``r`` on ``[r_min, r_max)``, both required, ``0 <= r_min < r_max``; a group outside the range is
      counted in ``outside`` of its type;
    * angle: ``theta = atan2(|dab x dcb|, dab . dcb)`` on [0, pi];
    * dihedral: ``phi = atan2(|b2| (b1 . n2), n1 . n2)`` on [-pi, pi] (IUPAC, as ``dihedral``); ``r_min`` and ``r_max``
      are refused for these two.

    Bin ``k = min(int((x - lo) * (num_bins / (hi - lo))), num_bins - 1)``: lower edges are inclusive, ``theta == pi`` and
    ``phi == pi`` fall into the last bin. ``num_bins`` lies in [1, 8192]. The counts are exact integers (an integer
    histogram in LDS, 64-bit integer atomics: ``csrc/bonded_histogram.hip``) and two reads of one state agree bit for
    bit. The kernel walks the per-particle table the forces walk, on the device: nothing travels to the host but the
    result. On a decomposed run every group is counted by the rank that owns its first member and the rows are added
    over the ranks; every rank gets the same result.

    ``distribution`` is ``counts / (num_groups * bin_width)``: a probability density in the coordinate ITSELF, without
    a Jacobian. A Boltzmann inversion divides by ``r^2`` or ``sin theta`` itself before it takes the logarithm. Its
    integral over the range is the fraction of the groups that lie inside (1 for angles and dihedrals).

    Refused with ``AzpError`` at construction or assignment: an unknown ``kind``, ``num_bins`` outside [1, 8192], a
    missing or empty ``[r_min, r_max)`` for bonds and pairs, ``r_min`` or ``r_max`` for angles and dihedrals. ``path``:
    0 (default) counts in LDS wherever ``n_types * (num_bins + 2)`` words fit into the 64 KiB of a workgroup and with
    global integer atomics elsewhere, 1 / 2 force one of them. Every property is computed when it is read, from the
    current state, and raises ``DataAccessError`` while the compute is not attached."""

    KINDS = {"bond": 2, "pair": 2, "angle": 3, "dihedral": 4}

    def __init__(self, kind, num_bins, r_min=None, r_max=None):
        super().__init__(All(), False)
        if kind not in self.KINDS:
            raise _lib.AzpError("BondedDistribution: kind must be one of %s, got %r" % (sorted(self.KINDS), kind))
        self._kind = kind
        self.num_bins = num_bins
        if self.KINDS[kind] == 2:
            if r_min is None or r_max is None:
                raise _lib.AzpError("BondedDistribution(%r): r_min and r_max are required" % kind)
            lo, hi = float(r_min), float(r_max)
            if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 <= lo < hi):
                raise _lib.AzpError("BondedDistribution(%r): needs finite 0 <= r_min < r_max, got %r, %r" % (kind, r_min, r_max))
        else:
            if r_min is not None or r_max is not None:
                raise _lib.AzpError("BondedDistribution(%r): the range is the whole domain of the angle, r_min and r_max "
                                    "are not accepted" % kind)
            lo, hi = (0.0, np.pi) if kind == "angle" else (-np.pi, np.pi)
        self._range = (lo, hi)
        self.path = _lib.BONDED_HISTOGRAM_PATH_AUTO

    @property
    def kind(self):
        return self._kind

    @property
    def r_min(self):
        return self._range[0] if self.KINDS[self._kind] == 2 else None

    @property
    def r_max(self):
        return self._range[1] if self.KINDS[self._kind] == 2 else None

    @property
    def num_bins(self):
        return self._num_bins

    @num_bins.setter
    def num_bins(self, value):
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= _lib.RDF_MAX_BINS:
            raise _lib.AzpError("BondedDistribution: num_bins must be an integer in [1, %d], got %r" % (_lib.RDF_MAX_BINS, value))
        self._num_bins = int(value)

    @property
    def path(self):
        return self._path

    @path.setter
    def path(self, value):
        if value not in (_lib.BONDED_HISTOGRAM_PATH_AUTO, _lib.BONDED_HISTOGRAM_PATH_LDS, _lib.BONDED_HISTOGRAM_PATH_GLOBAL):
            raise _lib.AzpError("BondedDistribution: path must be 0 (auto), 1 (LDS) or 2 (global atomics), got %r" % (value,))
        self._path = int(value)

    @property
    def bin_edges(self):
        """numpy.ndarray: the ``num_bins + 1`` edges of the bins."""
        return np.linspace(self._range[0], self._range[1], self._num_bins + 1)

    @property
    def bin_centers(self):
        e = self.bin_edges
        return 0.5 * (e[1:] + e[:-1])

    @property
    def bin_width(self):
        return (self._range[1] - self._range[0]) / self._num_bins

    # -- one launch ----------------------------------------------------------
    def _types(self):
        return list(getattr(self._sim.state, self._kind + "_types"))

    def _row_width(self):
        """The uint64 words of one output row: per type counts[num_bins], outside, total (at least one type)."""
        return max(len(self._types()), 1) * (self._num_bins + 2)

    def _launch(self, d_out):
        """Queue ``azp_bonded_histogram`` for the simulation's current state with the ``_row_width()`` words going to
        ``d_out``."""
        st = self._sim.state
        kind = self._kind
        tab = st.group_table(kind)
        a = _lib.BondedHistogramArgs()
        a.d_pos = st.pos.data_ptr()
        a.N = st.N
        a.n_max = st.n_max
        a.box = st.box.to_c()
        a.arity = self.KINDS[kind]
        a.n_types = max(len(self._types()), 1)
        a.d_table = tab["table"].data_ptr()
        a.d_table_pos = tab["bond_pos"].data_ptr() if "bond_pos" in tab else None
        a.d_counts = tab["n_%ss" % kind].data_ptr()
        a.pitch = tab["pitch"]
        a.num_bins = self._num_bins
        a.path = self._path
        if a.arity == 2:
            a.r_min, a.r_max = self._range
        a.d_out = d_out
        _lib.check(_lib.lib().azp_bonded_histogram(C.byref(a), _lib.raw_stream(st.device)), "azp_bonded_histogram")

    def _reduce(self, rows):
        """Rows of per-rank words (a (k, row width) int64 device tensor: the uint64 words of the kernel, all below 2^63)
        added over the ranks of a decomposed run, as numpy int64 of shape (k, n_types, num_bins + 2)."""
        return super()._reduce(rows).reshape(rows.shape[0], -1, self._num_bins + 2)[:, :len(self._types())]

    def _read(self, name):
        return self._reduce(self._read_row(name))[0]

    @property
    def types(self):
        """list of str: the names of the group types, in row order."""
        if not self._attached:
            raise DataAccessError("types")
        return self._types()

    @property
    def counts(self):
        """numpy int64 (n_types, num_bins): the groups of each type per bin."""
        return self._read("counts")[:, :self._num_bins].copy()

    @property
    def outside(self):
        """numpy int64 (n_types,): the groups of each type outside ``[r_min, r_max)`` (bonds and pairs; 0 otherwise)."""
        return self._read("outside")[:, self._num_bins].copy()

    @property
    def num_groups(self):
        """numpy int64 (n_types,): all groups of each type, inside the range or not."""
        return self._read("num_groups")[:, self._num_bins + 1].copy()

    @property
    def distribution(self):
        """numpy float64 (n_types, num_bins): ``counts / (num_groups * bin_width)`` on ``bin_centers``, zeros for a
        type without groups. No Jacobian: the inversion divides by ``r^2`` or ``sin theta`` itself."""
        t = self._read("distribution")
        return distribution_from_counts(t[:, :self._num_bins], t[:, self._num_bins + 1], self.bin_width)


class BondedDistributionRecorder(_Recorder):
    """Writer (``sim.operations.writers``) that appends the histograms of ``dist`` (a ``BondedDistribution`` in
    ``computes`` of the same simulation) to a device table of ``n_types * (num_bins + 2)`` words per row at the
    timesteps ``trigger`` (an ``int`` period or a ``Periodic``) fires, as ``RDFRecorder`` does with its counts: the
    kernel writes row k itself, nothing is read back and the host does not wait; the trajectory is the same bit for
    bit with and without the recorder. Read after the run: ``timesteps``, ``counts`` (frames, n_types, num_bins),
    ``num_groups`` (frames, n_types) and ``mean_distribution`` (n_types, num_bins), the sum of the counts over the sum
    of the group numbers times the bin width. On a decomposed run the whole table is reduced once, when it is read.
    ``reset()`` forgets the recorded frames (needed before ``dist.num_bins`` or the number of group types changes)."""

    _dtype = "int64"

    def __init__(self, dist, trigger):
        if not isinstance(dist, BondedDistribution):
            raise _lib.AzpError("BondedDistributionRecorder: dist must be a BondedDistribution, got %r" % (dist,))
        self.dist = self._compute = dist
        super().__init__(trigger)

    def _table(self, name):
        k = len(self._steps)
        if not self.dist._attached:
            if k == 0:
                return np.zeros((0, 0, self.dist.num_bins + 2), dtype=np.int64)
            raise DataAccessError(name)
        if k == 0:
            return np.zeros((0, len(self.dist._types()), self.dist.num_bins + 2), dtype=np.int64)
        return self.dist._reduce(self._rows[:k])

    @property
    def counts(self):
        """numpy int64 (frames, n_types, num_bins)."""
        return self._table("counts")[:, :, :self.dist.num_bins].copy()

    @property
    def num_groups(self):
        """numpy int64 (frames, n_types)."""
        return self._table("num_groups")[:, :, self.dist.num_bins + 1].copy()

    @property
    def mean_distribution(self):
        """numpy float64 (n_types, num_bins): the counts of all frames over their group numbers and the bin width."""
        t = self._table("mean_distribution")
        nb = self.dist.num_bins
        return distribution_from_counts(t[:, :, :nb].sum(axis=0), t[:, :, nb + 1].sum(axis=0), self.dist.bin_width)


# ---------------------------------------------------------------------------
# static structure factor
# ---------------------------------------------------------------------------
_TWO_PI = 2.0 * np.pi
_SF_MAX_BLOCK = 1 << 24


def reciprocal_vectors(box, m):
    """q(m) = 2 pi H^-T m for integer triples ``m`` (n, 3) in ``box`` (a ``state.Box``), as (n, 3) float64, by forward
    substitution in H^T q' = m: q'_x = h / Lx, q'_y = k / Ly - xy q'_x, q'_z = (l / Lz - xz q'_x) - yz q'_y, q = 2 pi q'."""
    m = np.asarray(m, dtype=np.float64).reshape(-1, 3)
    qx = m[:, 0] / box.Lx
    qy = m[:, 1] / box.Ly - box.xy * qx
    qz = (m[:, 2] / box.Lz - box.xz * qx) - box.yz * qy
    return np.stack([_TWO_PI * qx, _TWO_PI * qy, _TWO_PI * qz], axis=1)


def _sf_code(m):
    m = np.asarray(m, dtype=np.int64) + (1 << 20)
    return ((m[:, 2] << 42) | (m[:, 1] << 21) | m[:, 0]).astype(np.uint64)


def structure_factor_vectors(box, q_max, num_bins, max_vectors_per_bin=None, seed=0):
    """The wavevector set of ``StructureFactor``: (m, bin) with ``m`` (n, 3) int64 and ``bin`` (n,) int64.

    All m = (h, k, l) != 0 with |q(m)|^2 < q_max^2 (|q|^2 = (q_x^2 + q_y^2) + q_z^2 of ``reciprocal_vectors``), one of each
    +-pair (l > 0, or l == 0 and k > 0, or l == k == 0 and h > 0), in lexicographic order of (l, k, h); enumerated over
    |m_k| <= floor(q_max |a_k| / 2 pi). ``bin`` = min(int(|q| num_bins / q_max), num_bins - 1). With
    ``max_vectors_per_bin`` = M every bin keeps the M vectors of smallest key ``synthetic.hash64(seed, code(m), 0)``,
    code = (l + 2^20) 2^42 + (k + 2^20) 2^21 + (h + 2^20), ties to the smaller code. ``AzpError``: a bounding block of more
    than 2^24 triples, more than ``SF_MAX_VECTORS`` vectors after thinning."""
    from .synthetic import hash64

    q_max, num_bins = float(q_max), int(num_bins)
    norms = (box.Lx, box.Ly * np.sqrt(1.0 + box.xy ** 2), box.Lz * np.sqrt(1.0 + box.xz ** 2 + box.yz ** 2))
    M = [int(np.floor(q_max * a / _TWO_PI)) for a in norms]
    block = (2 * M[0] + 1) * (2 * M[1] + 1) * (2 * M[2] + 1)
    if block > _SF_MAX_BLOCK:
        raise _lib.AzpError("StructureFactor: q_max = %r bounds %d integer triples in this box, more than 2^24; lower q_max"
                            % (q_max, block))
    h = np.arange(-M[0], M[0] + 1, dtype=np.int64)
    k = np.arange(-M[1], M[1] + 1, dtype=np.int64)
    kk, hh = (x.ravel() for x in np.meshgrid(k, h, indexing="ij"))
    found, bins = [], []
    for l in range(0, M[2] + 1):  # (the half space has no l < 0)
        m = np.stack([hh, kk, np.full_like(hh, l)], axis=1)
        if l == 0:
            m = m[(kk > 0) | ((kk == 0) & (hh > 0))]
        q = reciprocal_vectors(box, m)
        qsq = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
        keep = qsq < q_max * q_max
        found.append(m[keep])
        bins.append(np.minimum((np.sqrt(qsq[keep]) * num_bins / q_max).astype(np.int64), num_bins - 1))
    m, b = np.concatenate(found), np.concatenate(bins)
    if max_vectors_per_bin is not None and len(m):
        code = _sf_code(m)
        key = hash64(seed, code, 0)
        order = np.lexsort((code, key, b))  # by bin, then key, then code
        first = np.searchsorted(b[order], np.arange(num_bins))  # where each bin starts in that order
        rank = np.arange(len(m)) - first[b[order]]
        keep = np.zeros(len(m), dtype=bool)
        keep[order[rank < int(max_vectors_per_bin)]] = True
        m, b = m[keep], b[keep]
    if len(m) > _lib.SF_MAX_VECTORS:
        raise _lib.AzpError("StructureFactor: %d wavevectors, more than the %d of AZP_SF_MAX_VECTORS; lower q_max or thin the "
                            "set with max_vectors_per_bin" % (len(m), _lib.SF_MAX_VECTORS))
    return m, b


def structure_factor_from_amplitudes(row, n_vectors):
    """S_AB(m) of every vector from one row of ``azp_structure_factor_amplitudes`` (4 n + 4 doubles: Re rho_A, Im rho_A,
    Re rho_B, Im rho_B, then N_A, N_B, N_AB, 0; added over the ranks of a decomposed run):
    S_AB(m) = (Re rho_A Re rho_B + Im rho_A Im rho_B) / sqrt(N_A N_B), i.e. |rho_A|^2 / N_A when B is A; zeros when a
    group is empty. The compute, the recorder and the tests all go through here."""
    row = np.asarray(row, dtype=np.float64)
    n = int(n_vectors)
    n_a, n_b = row[4 * n], row[4 * n + 1]
    if not (n_a > 0.0 and n_b > 0.0):
        return np.zeros(n)
    return (row[:n] * row[2 * n:3 * n] + row[n:2 * n] * row[3 * n:4 * n]) / np.sqrt(n_a * n_b)


def spherical_average(values, bins, num_bins):
    """(mean, count) per |q| bin: the arithmetic mean of ``values`` over the vectors whose ``bins`` entry is k, NaN where
    a bin has no vector, and the number of vectors per bin (int64)."""
    bins = np.asarray(bins, dtype=np.int64)
    count = np.bincount(bins, minlength=int(num_bins)).astype(np.int64)
    total = np.bincount(bins, weights=np.asarray(values, dtype=np.float64), minlength=int(num_bins))
    return np.divide(total, count, out=np.full(int(num_bins), np.nan), where=count > 0), count


def _check_sf_filter(name, f):
    if not isinstance(f, (All, Type)):
        raise _lib.AzpError("StructureFactor: %s must be All() or Type(...), got %r" % (name, f))
    return f


class StructureFactor(_Compute):
    """Partial static structure factor S_AB(q) between the groups ``filter_a`` and ``filter_b`` (``All()`` or
    ``Type(...)``; they may overlap) on the reciprocal-lattice vectors of the box, by the direct sum over the particles
    (``csrc/structure_factor.hip``). Not part of the reference; the semantics are this project's (``include/azp.h``,
    DESIGN 4.27).

    For a 3-D box periodic on all three axes with lattice matrix H (tilts included) the wavevectors are
    q(m) = 2 pi H^-T m, m = (h, k, l) integers, so q . r = 2 pi m . f with f the fractional coordinates. The amplitude of
    a group is rho_G(m) = sum_{j in G} exp(-2 pi i m . f_j) over the owned particles and
    S_AB(m) = Re[rho_A(m) conj(rho_B(m))] / sqrt(N_A N_B) (Ashcroft-Langreth; |rho_A|^2 / N_A for one group; 0 when a
    group is empty). ``vectors`` holds every m != 0 with |q(m)| < ``q_max``, one of each +-pair, ordered by (l, k, h)
    (``structure_factor_vectors``); ``max_vectors_per_bin`` = M thins it to the M vectors of smallest hash per |q| bin
    (deterministic in ``seed``, independent of N and of the ranks). ``structure_factor[k]`` is the arithmetic mean of
    S_AB(m) over the vectors of bin k of ``num_bins`` equal bins on [0, q_max) and NaN where ``vectors_per_bin[k]`` is 0.

    Refused with ``AzpError``: ``q_max <= 0``, ``num_bins`` outside [1, 8192], ``max_vectors_per_bin < 1``, a seed outside
    [0, 2^64), a filter that is not ``All()`` or ``Type(...)`` (at construction or assignment); when a property is
    read: a 2-D or not fully periodic box, an empty vector set (``q_max`` below the smallest |q| of the box), more
    than 2^24 triples to enumerate, more than ``SF_MAX_VECTORS`` = 65,536 vectors. ``path``: 0 (default) takes the
    powers kernel wherever its tables fit and the direct kernel elsewhere, 1 / 2 force one; a forced powers path
    whose tables do not fit is refused. The sums have a fixed order: two reads of one state agree bit for bit. On a
    decomposed run each rank sums its owned particles in the global box and the rows are added over the ranks before
    normalising. The vector list is built on the host, cached on the device, and rebuilt when the box, ``q_max``,
    ``num_bins``, the thinning or the seed changes. Every property is computed when it is read, from the current state."""

    def __init__(self, filter_a, filter_b, q_max, num_bins, max_vectors_per_bin=None, seed=0):
        super().__init__(_check_sf_filter("filter_a", filter_a), False)
        self._filter_b = _check_sf_filter("filter_b", filter_b)
        self.q_max = q_max
        self.num_bins = num_bins
        self.max_vectors_per_bin = max_vectors_per_bin
        self.seed = seed
        self.path = _lib.SF_PATH_AUTO
        self._set = None      # (key, m, bins, device triples, m_max)

    filter_a = _Compute.filter

    @property
    def filter_b(self):
        return self._filter_b

    @property
    def q_max(self):
        return self._q_max

    @q_max.setter
    def q_max(self, value):
        value = float(value)
        if not (value > 0.0 and np.isfinite(value)):
            raise _lib.AzpError("StructureFactor: q_max must be positive, got %r" % (value,))
        self._q_max = value

    @property
    def num_bins(self):
        return self._num_bins

    @num_bins.setter
    def num_bins(self, value):
        if isinstance(value, bool) or int(value) != value or not 1 <= int(value) <= _lib.RDF_MAX_BINS:
            raise _lib.AzpError("StructureFactor: num_bins must be an integer in [1, %d], got %r" % (_lib.RDF_MAX_BINS, value))
        self._num_bins = int(value)

    @property
    def max_vectors_per_bin(self):
        return self._max_per_bin

    @max_vectors_per_bin.setter
    def max_vectors_per_bin(self, value):
        if value is not None and (isinstance(value, bool) or int(value) != value or int(value) < 1):
            raise _lib.AzpError("StructureFactor: max_vectors_per_bin must be None or a positive integer, got %r" % (value,))
        self._max_per_bin = None if value is None else int(value)

    @property
    def seed(self):
        return self._seed

    @seed.setter
    def seed(self, value):
        if isinstance(value, bool) or int(value) != value or not 0 <= int(value) < 1 << 64:
            raise _lib.AzpError("StructureFactor: seed must be an integer in [0, 2^64), got %r" % (value,))
        self._seed = int(value)

    @property
    def path(self):
        return self._path

    @path.setter
    def path(self, value):
        if value not in (_lib.SF_PATH_AUTO, _lib.SF_PATH_DIRECT, _lib.SF_PATH_POWERS):
            raise _lib.AzpError("StructureFactor: path must be 0 (auto), 1 (direct) or 2 (powers), got %r" % (value,))
        self._path = int(value)

    @property
    def bin_edges(self):
        """numpy.ndarray: the ``num_bins + 1`` edges of the |q| bins."""
        return np.linspace(0.0, self._q_max, self._num_bins + 1)

    @property
    def bin_centers(self):
        e = self.bin_edges
        return 0.5 * (e[1:] + e[:-1])

    # -- the vector set --------------------------------------------------------
    def _vector_set(self, name="vectors"):
        """(m, bins, device triples, m_max) for the current box, rebuilt when anything it depends on changed."""
        import torch

        if not self._attached:
            raise DataAccessError(name)
        st = self._sim.state
        box = st.box
        if not (box.Lx > 0.0 and box.Ly > 0.0 and box.Lz > 0.0):
            raise _lib.AzpError("StructureFactor: a 3-D box is needed (2-D systems are not supported), got %r" % (box,))
        if not all(box.periodic):
            raise _lib.AzpError("StructureFactor: the box has to be periodic on all three axes (the wavevectors are those "
                                "of its lattice), got periodic = %r" % (box.periodic,))
        key = (st.box_generation, box._key(), self._q_max, self._num_bins, self._max_per_bin, self._seed, st.device)
        if self._set is None or self._set[0] != key:
            m, bins = structure_factor_vectors(box, self._q_max, self._num_bins, self._max_per_bin, self._seed)
            if len(m) == 0:
                raise _lib.AzpError("StructureFactor: q_max = %r is below the smallest |q| of the box: no wavevector" % (self._q_max,))
            triples = torch.from_numpy(np.ascontiguousarray(m, dtype=np.int32)).to(st.device)
            self._set = (key, m, bins, triples, tuple(int(x) for x in np.abs(m).max(axis=0)))
        return self._set[1:]

    def _row_width(self):
        return 4 * len(self._vector_set()[0]) + 4

    # -- one launch ----------------------------------------------------------
    def _launch(self, d_out):
        """Queue ``azp_structure_factor_amplitudes`` for the simulation's current state with the ``4 n + 4`` doubles
        going to ``d_out``."""
        st = self._sim.state
        m, _, triples, m_max = self._vector_set()
        a = _lib.StructureFactorArgs()
        a.d_pos = st.pos.data_ptr()
        a.N = st.N
        a.ntypes = len(st.types)
        a.box = st.box.to_c()
        mask_a, mask_b = self._type_masks(st)
        a.d_type_mask_a = mask_a.data_ptr() if mask_a is not None else None
        a.d_type_mask_b = mask_b.data_ptr() if mask_b is not None else None
        a.same_groups = 1 if self._filter == self._filter_b else 0
        a.n_vectors = len(m)
        a.d_vectors = triples.data_ptr()
        for d in range(3):
            a.m_max[d] = m_max[d]
        a.path = self._path
        self._set_scratch(a, "azp_structure_factor_scratch_size")  # (for this N, vector count and group pair)
        a.d_out = d_out
        _lib.check(_lib.lib().azp_structure_factor_amplitudes(C.byref(a), _lib.raw_stream(st.device)), "azp_structure_factor_amplitudes")

    def _read(self, name):
        return self._reduce(self._read_row(name, "float64"))[0]

    @property
    def vectors(self):
        """numpy int64 (n, 3): the integer triples m = (h, k, l), ordered by (l, k, h)."""
        return self._vector_set("vectors")[0].copy()

    @property
    def q_vectors(self):
        """numpy float64 (n, 3): q(m) = 2 pi H^-T m."""
        m = self._vector_set("q_vectors")[0]
        return reciprocal_vectors(self._sim.state.box, m)

    @property
    def q(self):
        """numpy float64 (n,): the lengths |q(m)|."""
        m = self._vector_set("q")[0]
        v = reciprocal_vectors(self._sim.state.box, m)
        return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])

    @property
    def vectors_per_bin(self):
        """numpy int64 (num_bins,): the vectors of each |q| bin."""
        return np.bincount(self._vector_set("vectors_per_bin")[1], minlength=self._num_bins).astype(np.int64)

    @property
    def amplitudes(self):
        """numpy complex128 (2, n): rho_A(m) and rho_B(m)."""
        row = self._read("amplitudes")
        n = (len(row) - 4) // 4
        return np.stack([row[:n] + 1j * row[n:2 * n], row[2 * n:3 * n] + 1j * row[3 * n:4 * n]])

    @property
    def group_sizes(self):
        """tuple[int]: (N_A, N_B, N_AB) over the owned particles of the whole system."""
        row = self._read("group_sizes")
        return tuple(int(x) for x in row[-4:-1])

    @property
    def vector_structure_factor(self):
        """numpy float64 (n,): S_AB(m) of every vector."""
        row = self._read("vector_structure_factor")
        return structure_factor_from_amplitudes(row, (len(row) - 4) // 4)

    @property
    def structure_factor(self):
        """numpy float64 (num_bins,): the mean of S_AB(m) over the vectors of each |q| bin, NaN in an empty bin."""
        row = self._read("structure_factor")
        s = structure_factor_from_amplitudes(row, (len(row) - 4) // 4)
        return spherical_average(s, self._vector_set()[1], self._num_bins)[0]


class StructureFactorRecorder(_Recorder):
    """Writer (``sim.operations.writers``) that appends the amplitudes of ``sf`` (a ``StructureFactor`` in ``computes`` of
    the same simulation) to a device table of ``4 n + 4`` doubles per row at the timesteps ``trigger`` (an ``int``
    period or a ``Periodic``) fires, as ``RDFRecorder`` does with its counts: the kernel writes row k itself, nothing
    is read back and the host does not wait; the trajectory is the same bit for bit with and without the recorder.
    Read after the run: ``timesteps``, ``amplitudes`` (frames, 2, n), ``structure_factor`` (frames, num_bins) and
    ``mean_structure_factor`` (num_bins,): S_AB(m) averaged over the frames, then over each bin's vectors. On a
    decomposed run the whole table is reduced once, when it is read. All rows belong to ONE box: the |q| of a fixed m
    changes with the box, so a record in a box different from the first row's (``update.BoxResize``,
    ``ConstantPressure``), like a row width that changes, raises ``AzpError``; ``reset()`` forgets the recorded frames."""

    def __init__(self, sf, trigger):
        if not isinstance(sf, StructureFactor):
            raise _lib.AzpError("StructureFactorRecorder: sf must be a StructureFactor, got %r" % (sf,))
        self.sf = self._compute = sf
        super().__init__(trigger)

    def _record(self, sim, timestep):
        key = sim.state.box._key()
        if self._steps and key != self._box_key:
            raise _lib.AzpError("StructureFactorRecorder: the box changed with rows recorded (the wavevectors of the first "
                                "row are not those of %r); call reset() first" % (sim.state.box,))
        super()._record(sim, timestep)
        self._box_key = key

    def reset(self):
        super().reset()
        self._box_key = None

    def _table(self, name):
        k = len(self._steps)
        if k == 0:
            return np.zeros((0, 4), dtype=np.float64)
        if not self.sf._attached:
            raise DataAccessError(name)
        return self.sf._reduce(self._rows[:k])

    @property
    def amplitudes(self):
        """numpy complex128 (frames, 2, n)."""
        t = self._table("amplitudes")
        n = (t.shape[1] - 4) // 4
        return np.stack([t[:, :n] + 1j * t[:, n:2 * n], t[:, 2 * n:3 * n] + 1j * t[:, 3 * n:4 * n]], axis=1)

    def _per_vector(self, name):
        t = self._table(name)
        n = (t.shape[1] - 4) // 4
        return np.array([structure_factor_from_amplitudes(r, n) for r in t]).reshape(t.shape[0], n)

    @property
    def structure_factor(self):
        """numpy float64 (frames, num_bins): each frame with its own group sizes."""
        s = self._per_vector("structure_factor")
        nb = self.sf.num_bins
        if s.shape[0] == 0:
            return np.zeros((0, nb))
        bins = self.sf._vector_set()[1]
        return np.stack([spherical_average(r, bins, nb)[0] for r in s])

    @property
    def mean_structure_factor(self):
        """numpy float64 (num_bins,): the mean of S_AB(m) over the frames, then over each bin's vectors."""
        s = self._per_vector("mean_structure_factor")
        nb = self.sf.num_bins
        if s.shape[0] == 0:
            return np.full(nb, np.nan)
        return spherical_average(s.mean(axis=0), self.sf._vector_set()[1], nb)[0]

    @property
    def intermediate_scattering(self):
        """``(lags, F)``: the collective intermediate scattering function F_AB(m, tau) of the recorded frames, numpy int64
        (lags,) and float64 (lags, n) (``intermediate_scattering_from_amplitudes`` with each frame's own group sizes)."""
        t = self._table("intermediate_scattering")
        n = (t.shape[1] - 4) // 4
        return intermediate_scattering_from_amplitudes(self.amplitudes, self.timesteps, t[:, 4 * n:4 * n + 2])


# ---------------------------------------------------------------------------
# bond-orientational order
# ---------------------------------------------------------------------------
STEINHARDT_FIXED = float(1 << 40)  # the fixed-point unit of the q_lm words is 2^-40


def steinhardt_norms(l):
    """``[N_l0 .. N_ll]`` with N_lm = sqrt((2l + 1) / (4 pi) (l - m)! / (l + m)!), the normalisation of the orthonormal
    Y_lm: the ratio of the factorials exactly, then one division and one square root in double. The kernel gets these
    numbers in its arguments and the test reference uses the same ones."""
    import math
    from fractions import Fraction

    l = int(l)
    return [math.sqrt(float(Fraction((2 * l + 1) * math.factorial(l - m), math.factorial(l + m))) / (4.0 * math.pi))
            for m in range(l + 1)]


def steinhardt_words(l):
    """``(words, offsets)``: the int64 a particle owns for the terms ``l`` and where each term starts; component m of a
    term sits at ``offset + 2 m`` (Re) and ``offset + 2 m + 1`` (Im)."""
    offsets, words = [], 0
    for x in l:
        offsets.append(words)
        words += 2 * (int(x) + 1)
    return words, offsets


def steinhardt_summary_width(n_terms, num_bins):
    return 4 + int(n_terms) * (1 + int(num_bins)) + _lib.STEINHARDT_CONNECTION_BINS


def steinhardt_summary(row, n_terms, num_bins):
    """The summary row of ``azp_steinhardt_compute`` (int64) as a dict: ``num_particles`` (N_G), ``num_with_neighbors``,
    ``sum_neighbors``, ``num_solid``, ``order_sums`` (n_terms exact integers, units of 2^-40), ``order`` (the group mean
    per l: order_sums 2^-40 / N_G, 0 for an empty group), ``histogram`` (n_terms, num_bins) and
    ``connection_histogram`` (33,)."""
    row = np.asarray(row)
    n_terms, num_bins = int(n_terms), int(num_bins)
    if row.ndim != 1 or row.shape[0] != steinhardt_summary_width(n_terms, num_bins):
        raise _lib.AzpError("steinhardt_summary: a row of %d words is expected for %d terms and %d bins, got shape %r"
                            % (steinhardt_summary_width(n_terms, num_bins), n_terms, num_bins, row.shape))
    n_g = int(row[0])
    sums = [int(x) for x in row[4:4 + n_terms]]
    h0 = 4 + n_terms
    h1 = h0 + n_terms * num_bins
    return dict(num_particles=n_g, num_with_neighbors=int(row[1]), sum_neighbors=int(row[2]), num_solid=int(row[3]),
                order_sums=sums, order=np.array([s / STEINHARDT_FIXED / n_g if n_g else 0.0 for s in sums]),
                histogram=row[h0:h1].reshape(n_terms, num_bins).astype(np.int64),
                connection_histogram=row[h1:].astype(np.int64))


def _check_l(name, l, single):
    if isinstance(l, (int, np.integer)) and not isinstance(l, bool):
        l = (l,)
    elif single:
        raise _lib.AzpError("%s: l must be one integer, got %r" % (name, l))
    try:
        l = tuple(l)
    except TypeError:
        raise _lib.AzpError("%s: l must be an integer or a sequence of integers, got %r" % (name, l))
    if not 1 <= len(l) <= _lib.STEINHARDT_MAX_TERMS:
        raise _lib.AzpError("%s: l must hold 1 to %d values, got %r" % (name, _lib.STEINHARDT_MAX_TERMS, l))
    for x in l:
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 1 <= int(x) <= _lib.STEINHARDT_MAX_L:
            raise _lib.AzpError("%s: every l must be an integer in 1 .. %d, got %r" % (name, _lib.STEINHARDT_MAX_L, x))
    l = tuple(int(x) for x in l)
    if len(set(l)) != len(l):
        raise _lib.AzpError("%s: l holds a value twice: %r" % (name, l))
    return l


class _BondOrder(_Compute):
    """What ``Steinhardt`` and ``SolidLiquid`` share: one call of ``azp_steinhardt_compute`` per read, the per-particle
    device buffers it fills and the summary row."""

    _flags = 0
    _q_threshold = 0.0
    _solid_threshold = 0

    def __init__(self, filter, l, r_max, num_bins, single):
        name = type(self).__name__
        if not isinstance(filter, (All, Type)):
            raise _lib.AzpError("%s: filter must be All() or Type(...), got %r" % (name, filter))
        super().__init__(filter, False)
        self._l = _check_l(name, l, single)
        try:
            r_max = float(r_max)
        except (TypeError, ValueError):
            raise _lib.AzpError("%s: r_max must be a number, got %r" % (name, r_max))
        if not (r_max > 0.0 and np.isfinite(r_max)):
            raise _lib.AzpError("%s: r_max must be positive, got %r" % (name, r_max))
        self._r_max = r_max
        if isinstance(num_bins, bool) or int(num_bins) != num_bins or not 1 <= int(num_bins) <= _lib.STEINHARDT_MAX_BINS:
            raise _lib.AzpError("%s: num_bins must be an integer in 1 .. %d, got %r" % (name, _lib.STEINHARDT_MAX_BINS, num_bins))
        self._num_bins = int(num_bins)
        self.path = _lib.STEINHARDT_PATH_AUTO
        self._out = None      # (N, device, dict of per-particle tensors)

    @property
    def l(self):
        return self._l

    @property
    def r_max(self):
        return self._r_max

    @property
    def path(self):
        """0 (default): the cell-list kernels wherever the box allows them (orthorhombic, at least three cells of width
        ``r_max`` on every periodic axis), the all-pairs kernels elsewhere; 1 / 2 force one of them."""
        return self._path

    @path.setter
    def path(self, value):
        if value not in (_lib.STEINHARDT_PATH_AUTO, _lib.STEINHARDT_PATH_ALL_PAIRS, _lib.STEINHARDT_PATH_CELLS):
            raise _lib.AzpError("%s: path must be 0 (auto), 1 (all-pairs) or 2 (cells), got %r" % (type(self).__name__, value))
        self._path = int(value)

    def _row_width(self):
        return steinhardt_summary_width(len(self._l), self._num_bins)

    def _check_box(self, sim):
        name = type(self).__name__
        if sim.domain is not None:
            raise _lib.AzpError("%s: decomposed runs are not supported (the second pass would need the q_lm of the ghost "
                                "particles)" % name)
        _check_pair_range(name, sim.state.box, self._r_max)

    def _args(self, st):
        a = _lib.SteinhardtArgs()
        a.N = st.N
        a.ntypes = len(st.types)
        a.box = st.box.to_c()
        a.r_max = self._r_max
        a.q_threshold = self._q_threshold
        a.solid_threshold = self._solid_threshold
        a.n_terms = len(self._l)
        for t, l in enumerate(self._l):
            a.l[t] = l
            for m, v in enumerate(steinhardt_norms(l)):
                a.norm[t][m] = v
        a.flags = self._flags
        a.path = self._path
        a.num_bins = self._num_bins
        return a

    def _launch(self, d_out):
        """Queue ``azp_steinhardt_compute`` for the simulation's current state with the summary row going to ``d_out``;
        the per-particle results go to this compute's own buffers."""
        import torch

        sim = self._sim
        st = sim.state
        self._check_box(sim)
        a = self._args(st)
        if st.N > _lib.STEINHARDT_MAX_N:
            raise _lib.AzpError("%s: %d particles are more than the %d the fixed-point sums are sized for"
                                % (type(self).__name__, st.N, _lib.STEINHARDT_MAX_N))
        a.d_pos = st.pos.data_ptr()
        mask = self._type_mask(st)
        a.d_type_mask = mask.data_ptr() if mask is not None else None
        words = steinhardt_words(self._l)[0]
        if self._out is None or self._out[0] != st.N or self._out[1] != st.device:
            def buf(shape, dtype):
                return torch.empty(shape, dtype=dtype, device=st.device)

            n = max(st.N, 1)
            self._out = (st.N, st.device, dict(
                num_neighbors=buf((n,), torch.int32), words=buf((n, words), torch.int64),
                order=buf((n, len(self._l)), torch.float64),
                avg_words=buf((n, words), torch.int64) if self._flags & _lib.STEINHARDT_AVERAGE else None,
                num_connections=buf((n,), torch.int32) if self._flags & _lib.STEINHARDT_CONNECTIONS else None))
        out = self._out[2]
        a.d_num_neighbors = out["num_neighbors"].data_ptr()
        a.d_words = out["words"].data_ptr()
        a.d_order = out["order"].data_ptr()
        a.d_avg_words = out["avg_words"].data_ptr() if out["avg_words"] is not None else None
        a.d_num_connections = out["num_connections"].data_ptr() if out["num_connections"] is not None else None
        self._set_scratch(a, "azp_steinhardt_scratch_size")
        a.d_summary = d_out
        _lib.check(_lib.lib().azp_steinhardt_compute(C.byref(a), _lib.raw_stream(st.device)), "azp_steinhardt_compute")

    def _read(self, name):
        """One call on the current state, then ``name`` as numpy: ``summary`` (the row), ``num_neighbors``, ``qlm`` (the
        fixed-point words S, (N, words) int64), ``qlm_average`` (T), ``order`` (N, len(l)) or ``num_connections``."""
        row = self._read_row(name)
        if name == "summary":
            return row.cpu().numpy()[0]
        key = {"qlm": "words", "qlm_average": "avg_words"}.get(name, name)
        t = self._out[2].get(key)
        if t is None:
            raise _lib.AzpError("%s: %s is not computed by this compute" % (type(self).__name__, name))
        return t[: self._sim.state.N].cpu().numpy()

    def _summary(self, name="summary"):
        if not self._attached:
            raise DataAccessError(name)
        return steinhardt_summary(self._read("summary"), len(self._l), self._num_bins)

    @property
    def num_neighbors(self):
        """numpy int32 (N,): N_b per row, 0 outside the group."""
        return self._read("num_neighbors")

    @property
    def num_particles(self):
        """int: the size of the group."""
        return self._summary("num_particles")["num_particles"]


class Steinhardt(_BondOrder):
    """Steinhardt's bond-orientational order parameters q_l of the particles selected by ``filter`` (``All()`` or
    ``Type(...)``) of a 3-D system, for ``l`` = one integer or up to 4 distinct ones in 1 .. 12 (freud's
    ``order.Steinhardt``; semantics: DESIGN 4.28). The neighbours of a particle are the particles of the group closer
    than ``r_max`` (minimum image, ``rsq < r_max^2`` as ``RadialDistributionFunction``); q_lm(i) is the mean of
    Y_lm over its bonds and q_l(i) = sqrt(4 pi / (2l + 1) sum_m |q_lm|^2). ``average=True`` gives Lechner and Dellago's
    form: q_lm averaged over the particle and its neighbours before the norm is taken.

    The sums over the bonds are kept as integers in units of 2^-40 (``_read("qlm")``), so they do not depend on the
    order of summation: two reads of one state agree bit for bit, on either path, before and after the particle sorter.

    ``num_neighbors`` (N,), ``particle_order`` (N, len(l)), row order like ``Force.forces``, rows outside the group 0;
    ``order`` the group mean per l; ``histogram`` (len(l), num_bins) of ``particle_order`` over the group on [0, 1] with
    ``bin_edges``. Every property is computed when it is read, from the current state. Refused with ``AzpError``: a
    bad ``l``, ``r_max <= 0``, ``num_bins`` outside 1 .. 1024, a filter that is not ``All()`` or ``Type(...)``; when
    read: ``r_max`` above half a periodic perpendicular width, a forced ``path`` the box does not allow, a decomposed
    run."""

    def __init__(self, filter, l, r_max, average=False, num_bins=100):
        super().__init__(filter, l, r_max, num_bins, single=False)
        self._average = bool(average)
        self._flags = _lib.STEINHARDT_AVERAGE if self._average else 0

    @property
    def average(self):
        return self._average

    @property
    def num_bins(self):
        return self._num_bins

    @property
    def bin_edges(self):
        """numpy.ndarray: the ``num_bins + 1`` edges of the histogram's bins on [0, 1]."""
        return np.linspace(0.0, 1.0, self._num_bins + 1)

    @property
    def particle_order(self):
        """numpy float64 (N, len(l)): q_l per row (the neighbour-averaged one with ``average=True``)."""
        return self._read("order")

    @property
    def order(self):
        """numpy float64 (len(l),): the mean of ``particle_order`` over the group, from the summary row."""
        return self._summary("order")["order"]

    @property
    def histogram(self):
        """numpy int64 (len(l), num_bins)."""
        return self._summary("histogram")["histogram"]


class SolidLiquid(_BondOrder):
    """ten Wolde and Frenkel's solid-bond count for one ``l`` (freud's ``order.SolidLiquid`` without the clusters;
    DESIGN 4.28): the bond between neighbours i and j is solid iff the normalised product
    d(i, j) = Re sum_m q_lm(i) conj(q_lm(j)) / (|q(i)| |q(j)|) exceeds ``q_threshold``; ``num_connections`` (N,) counts a
    particle's solid bonds and the particle is ``solid`` iff that is at least ``solid_threshold``. ``num_solid`` and
    ``connection_histogram`` (33 words, the last for 32 and more) come from the summary row. Refused with ``AzpError``:
    what ``Steinhardt`` refuses, an ``l`` that is not one integer, a ``q_threshold`` outside [-1, 1], a
    ``solid_threshold`` that is not a positive integer."""

    _flags = _lib.STEINHARDT_CONNECTIONS

    def __init__(self, filter, l, r_max, q_threshold, solid_threshold):
        super().__init__(filter, l, r_max, 1, single=True)
        try:
            q = float(q_threshold)
        except (TypeError, ValueError):
            raise _lib.AzpError("SolidLiquid: q_threshold must be a number, got %r" % (q_threshold,))
        if not -1.0 <= q <= 1.0:
            raise _lib.AzpError("SolidLiquid: q_threshold must lie in [-1, 1], got %r" % (q_threshold,))
        if (isinstance(solid_threshold, bool) or not isinstance(solid_threshold, (int, np.integer))
                or not 1 <= int(solid_threshold) < (1 << 31)):
            raise _lib.AzpError("SolidLiquid: solid_threshold must be a positive integer, got %r" % (solid_threshold,))
        self._q_threshold = q
        self._solid_threshold = int(solid_threshold)

    @property
    def q_threshold(self):
        return self._q_threshold

    @property
    def solid_threshold(self):
        return self._solid_threshold

    @property
    def num_connections(self):
        """numpy int32 (N,): solid bonds per row, 0 outside the group."""
        return self._read("num_connections")

    @property
    def solid(self):
        """numpy bool (N,): in the group and ``num_connections >= solid_threshold``."""
        return self._read("num_connections") >= self._solid_threshold  # (a row outside the group has none, the threshold is >= 1)

    @property
    def num_solid(self):
        return self._summary("num_solid")["num_solid"]

    @property
    def connection_histogram(self):
        """numpy int64 (33,): particles of the group by ``num_connections``, the last word for 32 and more."""
        return self._summary("connection_histogram")["connection_histogram"]


class _BondOrderRecorder(_Recorder):
    """The summary row of a ``Steinhardt`` or a ``SolidLiquid`` appended to a device table at the timesteps the trigger
    fires inside ``Simulation.run``, as ``RDFRecorder`` does with its counts: the last kernel of the call writes row k
    itself, nothing is read back, the host does not wait, and the trajectory is the same bit for bit with and without
    the recorder."""

    _dtype = "int64"
    _kind = _BondOrder

    def __init__(self, compute, trigger):
        if not isinstance(compute, self._kind):
            raise _lib.AzpError("%s: a %s is expected, got %r" % (type(self).__name__, self._kind.__name__, compute))
        self._compute = compute
        super().__init__(trigger)

    def _table(self):
        c = self._compute
        k = len(self._steps)
        rows = self._rows[:k].cpu().numpy() if k else np.zeros((0, self._row_width()), dtype=np.int64)
        return [steinhardt_summary(r, len(c.l), c._num_bins) for r in rows]

    @property
    def num_particles(self):
        """numpy int64 (frames,): the size of the group."""
        return np.array([r["num_particles"] for r in self._table()], dtype=np.int64)


class SteinhardtRecorder(_BondOrderRecorder):
    """Writer (``sim.operations.writers``) for a ``Steinhardt`` in ``computes`` of the same simulation. Read after the
    run: ``timesteps``, ``order`` (frames, len(l)), ``histogram`` (frames, len(l), num_bins), ``num_particles``;
    ``reset()`` forgets the frames."""

    _kind = Steinhardt

    def __init__(self, steinhardt, trigger):
        super().__init__(steinhardt, trigger)
        self.steinhardt = steinhardt

    @property
    def order(self):
        t = self._table()
        return np.array([r["order"] for r in t]).reshape(len(t), len(self._compute.l))

    @property
    def histogram(self):
        t = self._table()
        c = self._compute
        return np.array([r["histogram"] for r in t], dtype=np.int64).reshape(len(t), len(c.l), c.num_bins)


class SolidLiquidRecorder(_BondOrderRecorder):
    """Writer (``sim.operations.writers``) for a ``SolidLiquid`` in ``computes`` of the same simulation. Read after the
    run: ``timesteps``, ``num_solid`` (frames,), ``connection_histogram`` (frames, 33), ``num_particles``; ``reset()``
    forgets the frames."""

    _kind = SolidLiquid

    def __init__(self, solid_liquid, trigger):
        super().__init__(solid_liquid, trigger)
        self.solid_liquid = solid_liquid

    @property
    def num_solid(self):
        return np.array([r["num_solid"] for r in self._table()], dtype=np.int64)

    @property
    def connection_histogram(self):
        t = self._table()
        return np.array([r["connection_histogram"] for r in t], dtype=np.int64).reshape(len(t), _lib.STEINHARDT_CONNECTION_BINS)


# ---------------------------------------------------------------------------
# clusters
# ---------------------------------------------------------------------------
def cluster_summary_width(size_bins):
    return 6 + int(size_bins)


def cluster_summary(row, size_bins):
    """The summary row of ``azp_cluster_compute`` (int64) as a dict: ``num_particles`` (N_G), ``num_clusters``,
    ``largest_cluster_size``, ``largest_cluster_key`` (-1 for an empty group), ``sum_size_squared``, ``num_edges`` and
    ``size_histogram`` (size_bins,): clusters of size s at s - 1, the last word for ``size_bins`` and more."""
    row = np.asarray(row)
    size_bins = int(size_bins)
    if row.ndim != 1 or row.shape[0] != cluster_summary_width(size_bins):
        raise _lib.AzpError("cluster_summary: a row of %d words is expected for %d bins, got shape %r"
                            % (cluster_summary_width(size_bins), size_bins, row.shape))
    return dict(num_particles=int(row[0]), num_clusters=int(row[1]), largest_cluster_size=int(row[2]),
                largest_cluster_key=int(row[3]), sum_size_squared=int(row[4]), num_edges=int(row[5]),
                size_histogram=row[6:].astype(np.int64))


def cluster_indices(keys, sizes):
    """freud's ``cluster_idx`` from the per-row ``cluster_keys`` and ``cluster_sizes``: int64 (N,), 0 for the rows of the
    largest cluster, 1 for the next and so on, clusters of one size in ascending order of their key, -1 for a row
    outside the group (key ``CLUSTER_NONE``)."""
    keys = np.asarray(keys).astype(np.int64).reshape(-1)
    sizes = np.asarray(sizes).astype(np.int64).reshape(-1)
    if keys.shape != sizes.shape:
        raise _lib.AzpError("cluster_indices: keys and sizes differ in shape: %r and %r" % (keys.shape, sizes.shape))
    idx = np.full(keys.shape, -1, dtype=np.int64)
    inside = keys != _lib.CLUSTER_NONE
    if inside.any():
        uniq, first, inverse = np.unique(keys[inside], return_index=True, return_inverse=True)
        order = np.lexsort((uniq, -sizes[inside][first]))  # by size, largest first, then by key
        rank = np.empty(order.shape[0], dtype=np.int64)
        rank[order] = np.arange(order.shape[0])
        idx[inside] = rank[inverse.reshape(-1)]
    return idx


class Cluster(_Compute):
    """The connected components of the particles selected by ``filter`` (``All()`` or ``Type(...)``) of a 3-D system,
    two particles being joined where they are closer than ``r_max`` (minimum image, ``rsq < r_max^2`` as
    ``RadialDistributionFunction`` and ``Steinhardt``); freud's ``cluster.Cluster`` on the device (semantics:
    ``include/azp.h`` "clusters"). A particle without a neighbour is a cluster of one.

    ``solid`` (a ``SolidLiquid`` in ``computes`` of the same simulation) restricts the group to the particles it marks
    solid: every read first queues the ``SolidLiquid``'s own call and hands its ``num_connections`` buffer and its
    ``solid_threshold`` to the kernel, nothing goes through the host. The largest cluster is then ten Wolde and
    Frenkel's nucleus. ``r_max`` is the cluster's own and may differ from the one that defines the solid bonds.

    Per row, in row order like ``Force.forces``: ``cluster_keys`` (uint32: the smallest tag of the row's cluster,
    ``CLUSTER_NONE`` outside the group -- a label that survives the particle sorter), ``cluster_sizes`` (uint32, 0
    outside the group), ``cluster_idx`` (freud's numbering from the two, see ``cluster_indices``). From the summary
    row: ``num_particles``, ``num_clusters``, ``largest_cluster_size``, ``largest_cluster_key``, ``num_edges``,
    ``mean_cluster_size`` (number average), ``weight_average_cluster_size`` (sum of size^2 over the number of
    particles) and ``size_histogram`` (``size_bins`` words, the last for ``size_bins`` and more). All are exact integers or
    quotients of two: two reads, the two paths and a sorted state agree bit for bit. Every property is computed when
    it is read, from the current state. Refused with ``AzpError``: a filter that is not ``All()`` or ``Type(...)``,
    ``r_max <= 0``, ``size_bins`` outside 1 .. 1024, a ``solid`` that is not a ``SolidLiquid``; when read: ``r_max`` above
    half a periodic perpendicular width, a forced ``path`` the box does not allow, a decomposed run, a ``solid`` of
    another simulation."""

    def __init__(self, filter, r_max, solid=None, size_bins=64):
        if not isinstance(filter, (All, Type)):
            raise _lib.AzpError("Cluster: filter must be All() or Type(...), got %r" % (filter,))
        super().__init__(filter, False)
        try:
            r_max = float(r_max)
        except (TypeError, ValueError):
            raise _lib.AzpError("Cluster: r_max must be a number, got %r" % (r_max,))
        if not (r_max > 0.0 and np.isfinite(r_max)):
            raise _lib.AzpError("Cluster: r_max must be positive, got %r" % (r_max,))
        self._r_max = r_max
        if solid is not None and not isinstance(solid, SolidLiquid):
            raise _lib.AzpError("Cluster: solid must be a SolidLiquid or None, got %r" % (solid,))
        self._solid = solid
        if (isinstance(size_bins, bool) or not isinstance(size_bins, (int, np.integer))
                or not 1 <= int(size_bins) <= _lib.CLUSTER_MAX_BINS):
            raise _lib.AzpError("Cluster: size_bins must be an integer in 1 .. %d, got %r" % (_lib.CLUSTER_MAX_BINS, size_bins))
        self._size_bins = int(size_bins)
        self.path = _lib.CLUSTER_PATH_AUTO
        self._stages = 0      # (tools/cluster_probe.py: 1 and 2 stop the call early, for timing)
        self._out = None      # (N, device, keys, sizes)
        self._solid_row = None
        self._want_rep = False  # (a ClusterProperties asks for the representative rows: allocated on request)
        self._rep = None

    @property
    def r_max(self):
        return self._r_max

    @property
    def solid(self):
        return self._solid

    @property
    def size_bins(self):
        return self._size_bins

    @property
    def path(self):
        """0 (default): the cell-list kernels wherever the box allows them (orthorhombic, at least three cells of width
        ``r_max`` on every periodic axis), the all-pairs kernels elsewhere; 1 / 2 force one of them."""
        return self._path

    @path.setter
    def path(self, value):
        if isinstance(value, bool) or value not in (_lib.CLUSTER_PATH_AUTO, _lib.CLUSTER_PATH_ALL_PAIRS, _lib.CLUSTER_PATH_CELLS):
            raise _lib.AzpError("Cluster: path must be 0 (auto), 1 (all-pairs) or 2 (cells), got %r" % (value,))
        self._path = int(value)

    def _row_width(self):
        return cluster_summary_width(self._size_bins)

    def _check_box(self, sim):
        if sim.domain is not None:
            raise _lib.AzpError("Cluster: decomposed runs are not supported (a cluster may span ranks)")
        _check_pair_range("Cluster", sim.state.box, self._r_max)

    def _launch(self, d_out):
        """Queue ``azp_cluster_compute`` for the simulation's current state with the summary row going to ``d_out``
        (after the ``SolidLiquid``'s own call where ``solid`` is set); keys and sizes go to this compute's buffers."""
        import torch

        sim = self._sim
        st = sim.state
        self._check_box(sim)
        if st.N > _lib.CLUSTER_MAX_N:
            raise _lib.AzpError("Cluster: %d particles are more than the %d the 32-bit slots are sized for" % (st.N, _lib.CLUSTER_MAX_N))
        solid = self._solid
        if solid is not None and (solid._sim is not sim or not solid._attached):
            raise _lib.AzpError("Cluster: solid must be in sim.operations.computes of the same simulation")
        a = _lib.ClusterArgs()
        a.N = st.N
        a.ntypes = len(st.types)
        a.box = st.box.to_c()
        a.r_max = self._r_max
        a.path = self._path
        a.stages = self._stages
        a.size_bins = self._size_bins
        a.d_pos = st.pos.data_ptr()
        a.d_tag = st.tag.data_ptr()
        mask = self._type_mask(st)
        a.d_type_mask = mask.data_ptr() if mask is not None else None
        # (every refusal of the cluster's own comes before the SolidLiquid's launch)
        self._set_scratch(a, "azp_cluster_scratch_size")
        if solid is not None:
            solid._launch(self._row_buffer(solid._row_width(), "int64", "_solid_row").data_ptr())
            a.d_member = solid._out[2]["num_connections"].data_ptr()
            a.member_min = solid.solid_threshold
        if self._out is None or self._out[0] != st.N or self._out[1] != st.device:
            n = max(st.N, 1)
            self._out = (st.N, st.device, torch.empty((n,), dtype=torch.int32, device=st.device),
                         torch.empty((n,), dtype=torch.int32, device=st.device))
        a.d_cluster_key = self._out[2].data_ptr()
        a.d_cluster_size = self._out[3].data_ptr()
        if self._want_rep:
            if self._rep is None or self._rep.shape[0] != max(st.N, 1) or self._rep.device != st.device:
                self._rep = torch.empty((max(st.N, 1),), dtype=torch.int32, device=st.device)
            a.d_cluster_rep = self._rep.data_ptr()
        a.d_summary = d_out
        _lib.check(_lib.lib().azp_cluster_compute(C.byref(a), _lib.raw_stream(st.device)), "azp_cluster_compute")

    def _read(self, name):
        """One call on the current state, then ``name`` as numpy: ``summary`` (the row), ``cluster_keys`` or
        ``cluster_sizes`` (uint32), or ``both`` (keys, sizes) of that one call."""
        row = self._read_row(name)
        if name == "summary":
            return row.cpu().numpy()[0]
        keys, sizes = (t[: self._sim.state.N].cpu().numpy().view(np.uint32) for t in self._out[2:])
        return {"cluster_keys": keys, "cluster_sizes": sizes, "both": (keys, sizes)}[name]

    def _summary(self, name="summary"):
        if not self._attached:
            raise DataAccessError(name)
        return cluster_summary(self._read("summary"), self._size_bins)

    @property
    def cluster_keys(self):
        """numpy uint32 (N,): the smallest tag of the row's cluster, ``CLUSTER_NONE`` outside the group."""
        return self._read("cluster_keys")

    @property
    def cluster_sizes(self):
        """numpy uint32 (N,): the size of the row's cluster, 0 outside the group."""
        return self._read("cluster_sizes")

    @property
    def cluster_idx(self):
        """numpy int64 (N,): ``cluster_indices`` of the keys and sizes of one call."""
        return cluster_indices(*self._read("both"))

    @property
    def num_particles(self):
        """int: the size of the group."""
        return self._summary("num_particles")["num_particles"]

    @property
    def num_clusters(self):
        return self._summary("num_clusters")["num_clusters"]

    @property
    def largest_cluster_size(self):
        return self._summary("largest_cluster_size")["largest_cluster_size"]

    @property
    def largest_cluster_key(self):
        """int: the key of the largest cluster (the smallest key among equals), -1 for an empty group."""
        return self._summary("largest_cluster_key")["largest_cluster_key"]

    @property
    def num_edges(self):
        """int: pairs of the group closer than ``r_max``, each counted once."""
        return self._summary("num_edges")["num_edges"]

    @property
    def mean_cluster_size(self):
        """float: particles per cluster (the number average), 0 for an empty group."""
        s = self._summary("mean_cluster_size")
        return s["num_particles"] / s["num_clusters"] if s["num_clusters"] else 0.0

    @property
    def weight_average_cluster_size(self):
        """float: sum of size^2 over the number of particles, 0 for an empty group."""
        s = self._summary("weight_average_cluster_size")
        return s["sum_size_squared"] / s["num_particles"] if s["num_particles"] else 0.0

    @property
    def size_histogram(self):
        """numpy int64 (size_bins,): clusters of size s at s - 1, the last word for ``size_bins`` and more."""
        return self._summary("size_histogram")["size_histogram"]


class ClusterRecorder(_Recorder):
    """Writer (``sim.operations.writers``) for a ``Cluster`` in ``computes`` of the same simulation: its summary row
    appended to a device table at the timesteps the trigger fires inside ``Simulation.run``, as ``SolidLiquidRecorder``
    does -- the call's last kernels write row k themselves, nothing is read back, the host does not wait, and the
    trajectory is the same bit for bit with and without the recorder. Read after the run: ``timesteps``,
    ``num_particles``, ``num_clusters``, ``largest_cluster_size``, ``num_edges``, ``weight_average_cluster_size``
    (frames,) and ``size_histogram`` (frames, size_bins); ``reset()`` forgets the frames."""

    _dtype = "int64"

    def __init__(self, cluster, trigger):
        if not isinstance(cluster, Cluster):
            raise _lib.AzpError("ClusterRecorder: a Cluster is expected, got %r" % (cluster,))
        self.cluster = self._compute = cluster
        super().__init__(trigger)

    def _table(self):
        k = len(self._steps)
        return self._rows[:k].cpu().numpy() if k else np.zeros((0, self._row_width()), dtype=np.int64)

    @property
    def num_particles(self):
        return self._table()[:, 0].copy()

    @property
    def num_clusters(self):
        return self._table()[:, 1].copy()

    @property
    def largest_cluster_size(self):
        return self._table()[:, 2].copy()

    @property
    def num_edges(self):
        return self._table()[:, 5].copy()

    @property
    def weight_average_cluster_size(self):
        t = self._table()
        return np.divide(t[:, 4], t[:, 0], out=np.zeros(t.shape[0]), where=t[:, 0] != 0)

    @property
    def size_histogram(self):
        return self._table()[:, 6:].copy()


# ---------------------------------------------------------------------------
# cluster properties
# ---------------------------------------------------------------------------
def _gyration_matrix(words):
    """(..., 6) words xx, xy, xz, yy, yz, zz -> (..., 3, 3) symmetric."""
    w = np.asarray(words, dtype=np.float64)
    return w[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(w.shape[:-1] + (3, 3))


def _properties_row(row):
    """One table row of ``azp_cluster_properties`` (16 float64) as a dict."""
    return dict(key=int(row[0]), size=int(row[1]), center=row[2:5].copy(), gyration=_gyration_matrix(row[5:11]),
                radius_of_gyration=float(np.sqrt(max(row[11], 0.0))), compact=bool(row[12] != 0.0), extent=row[13:16].copy())


def cluster_properties_table(table, summary):
    """The table and the summary of ``azp_cluster_properties`` (float64, (rows >= summary[0], 16) and (20,)) as a dict of
    numpy arrays in freud's order of the clusters -- descending size, then ascending key: ``keys`` (C,) int64, ``sizes``
    (C,) int64, ``centers`` (C, 3), ``gyrations`` (C, 3, 3), ``radii_of_gyration`` (C,), ``compact`` (C,) bool,
    ``extents`` (C, 3); and ``num_clusters``, ``num_particles``, ``shift`` and ``largest`` (the summary's row as a dict,
    key -1 where there is no cluster)."""
    table = np.asarray(table, dtype=np.float64)
    summary = np.asarray(summary, dtype=np.float64).reshape(-1)
    if summary.shape[0] != _lib.CLUSTER_PROPERTIES_SUMMARY or table.ndim != 2 or table.shape[1] != _lib.CLUSTER_PROPERTIES_ROW:
        raise _lib.AzpError("cluster_properties_table: a (rows, %d) table and a summary of %d words are expected, got %r and %r"
                            % (_lib.CLUSTER_PROPERTIES_ROW, _lib.CLUSTER_PROPERTIES_SUMMARY, table.shape, summary.shape))
    rows = int(summary[0])
    if rows > table.shape[0]:
        raise _lib.AzpError("cluster_properties_table: the summary counts %d rows, the table has %d" % (rows, table.shape[0]))
    t = table[:rows]
    t = t[np.lexsort((t[:, 0], -t[:, 1]))]  # by size, largest first, then by key
    return dict(num_clusters=rows, num_particles=int(summary[1]), shift=int(summary[2]),
                keys=t[:, 0].astype(np.int64), sizes=t[:, 1].astype(np.int64), centers=t[:, 2:5].copy(),
                gyrations=_gyration_matrix(t[:, 5:11]), radii_of_gyration=np.sqrt(np.maximum(t[:, 11], 0.0)),
                compact=t[:, 12] != 0.0, extents=t[:, 13:16].copy(), largest=_properties_row(summary[4:]))


class ClusterProperties(_Compute):
    """The centre and the gyration tensor of every cluster of ``cluster`` (a ``Cluster`` in ``computes`` of the same
    simulation) with at least ``min_size`` particles; freud's ``cluster.ClusterProperties`` on the device, every
    particle with weight 1 (semantics: ``include/azp.h`` "cluster properties"). Every read queues the
    ``Cluster``'s own call and then ``azp_cluster_properties`` on its per-row keys, sizes and representative rows;
    nothing goes through the host.

    A cluster is unwrapped about the circular mean of its fractional coordinates. ``compact`` is True where it extends
    over less than half the box on every periodic axis; its centre and tensor are then exact. For any other cluster
    (one that wraps round the box is never compact) the same formulas are evaluated: reproducible, but what they mean is
    the caller's business. All sums are integers in units of 2^-``shift``: two reads, the two paths of the ``Cluster`` and
    a sorted state give the same bits per key.

    In freud's order of the clusters (descending size, then ascending key; with ``min_size == 1`` index k is
    ``cluster_idx == k``): ``keys``, ``sizes`` (C,), ``centers`` (C, 3), ``gyrations`` (C, 3, 3), ``radii_of_gyration``
    (C,), ``compact`` (C,) bool, ``extents`` (C, 3) fractional, ``principal_moments`` (C, 3) descending,
    ``relative_shape_anisotropy`` (C,); ``num_clusters``; ``largest``, a dict of the largest cluster's row. Refused with
    ``AzpError``: a ``cluster`` that is not a ``Cluster``, a ``min_size`` that is not an integer >= 1; when read: not
    attached, a ``Cluster`` of another simulation, a decomposed run."""

    def __init__(self, cluster, min_size=1):
        if not isinstance(cluster, Cluster):
            raise _lib.AzpError("ClusterProperties: cluster must be a Cluster, got %r" % (cluster,))
        if isinstance(min_size, bool) or not isinstance(min_size, (int, np.integer)) or not 1 <= int(min_size) < (1 << 32):
            raise _lib.AzpError("ClusterProperties: min_size must be an integer >= 1, got %r" % (min_size,))
        super().__init__(None, False)
        self._cluster = cluster
        self._min_size = int(min_size)
        self._cluster_row = None
        self._table = None
        self._own_only = False  # (tools/cluster_properties_probe.py: the properties call alone, on the labels of the last call)

    @property
    def cluster(self):
        return self._cluster

    @property
    def min_size(self):
        return self._min_size

    def _row_width(self):
        return _lib.CLUSTER_PROPERTIES_SUMMARY

    def _launch(self, d_out):
        """Queue the ``Cluster``'s call and ``azp_cluster_properties`` for the simulation's current state with the summary
        going to ``d_out``; the table goes to this compute's own buffer."""
        import torch

        sim = self._sim
        if sim.domain is not None:
            raise _lib.AzpError("ClusterProperties: decomposed runs are not supported (a cluster may span ranks)")
        cl = self._cluster
        if cl._sim is not sim or not cl._attached:
            raise _lib.AzpError("ClusterProperties: cluster must be in sim.operations.computes of the same simulation")
        st = sim.state
        a = _lib.ClusterPropertiesArgs()
        a.N = st.N
        a.min_size = self._min_size
        a.box = st.box.to_c()
        a.d_pos = st.pos.data_ptr()
        # (every refusal of this compute's own comes before the Cluster's launch)
        self._set_scratch(a, "azp_cluster_properties_scratch_size")
        if self._own_only:
            if cl._rep is None or cl._out is None or cl._out[0] != st.N or cl._rep.device != st.device:
                raise _lib.AzpError("ClusterProperties: the properties call alone needs the labels of an earlier whole call on this state")
        else:
            cl._want_rep = True  # (for this call only: a Cluster read on its own writes no representative rows)
            try:
                cl._launch(self._row_buffer(cl._row_width(), "int64", "_cluster_row").data_ptr())
            finally:
                cl._want_rep = False
        rows = max(st.N // self._min_size, 1)
        if self._table is None or self._table.shape[0] != rows or self._table.device != st.device:
            self._table = torch.empty((rows, _lib.CLUSTER_PROPERTIES_ROW), dtype=torch.float64, device=st.device)
        a.d_cluster_rep = cl._rep.data_ptr()
        a.d_cluster_key = cl._out[2].data_ptr()
        a.d_cluster_size = cl._out[3].data_ptr()
        a.d_table = self._table.data_ptr()
        a.d_summary = d_out
        _lib.check(_lib.lib().azp_cluster_properties(C.byref(a), _lib.raw_stream(st.device)), "azp_cluster_properties")

    def _read(self, name="table"):
        """One call on the current state: ``cluster_properties_table`` of its table and summary."""
        row = self._read_row(name, "float64").cpu().numpy()[0]
        return cluster_properties_table(self._table[: int(row[0])].cpu().numpy(), row)

    @property
    def num_clusters(self):
        return int(self._read_row("num_clusters", "float64").cpu().numpy()[0, 0])

    @property
    def keys(self):
        """numpy int64 (C,): the clusters' keys (``Cluster.cluster_keys``)."""
        return self._read("keys")["keys"]

    @property
    def sizes(self):
        return self._read("sizes")["sizes"]

    @property
    def centers(self):
        """numpy float64 (C, 3): the mean position of the unwrapped cluster, wrapped into the box."""
        return self._read("centers")["centers"]

    @property
    def gyrations(self):
        """numpy float64 (C, 3, 3): the covariance of the positions of the unwrapped cluster."""
        return self._read("gyrations")["gyrations"]

    @property
    def radii_of_gyration(self):
        return self._read("radii_of_gyration")["radii_of_gyration"]

    @property
    def compact(self):
        return self._read("compact")["compact"]

    @property
    def extents(self):
        """numpy float64 (C, 3): the extent of the unwrapped cluster along each lattice vector, as a fraction of it."""
        return self._read("extents")["extents"]

    @property
    def principal_moments(self):
        """numpy float64 (C, 3): the eigenvalues of ``gyrations``, descending."""
        g = self._read("principal_moments")["gyrations"]
        return np.linalg.eigvalsh(g)[:, ::-1] if g.shape[0] else np.zeros((0, 3))

    @property
    def relative_shape_anisotropy(self):
        """numpy float64 (C,): 1 - 3 (l1 l2 + l2 l3 + l3 l1) / (l1 + l2 + l3)^2 of the principal moments, 0 where Rg^2 = 0."""
        g = self._read("relative_shape_anisotropy")["gyrations"]
        if not g.shape[0]:
            return np.zeros(0)
        lam = np.linalg.eigvalsh(g)
        tr = lam.sum(axis=1)
        pairs = lam[:, 0] * lam[:, 1] + lam[:, 1] * lam[:, 2] + lam[:, 2] * lam[:, 0]
        return np.where(tr > 0.0, 1.0 - 3.0 * np.divide(pairs, tr * tr, out=np.zeros_like(tr), where=tr > 0.0), 0.0)

    @property
    def largest(self):
        """dict: ``key`` (-1 where there is no cluster), ``size``, ``center``, ``gyration``, ``radius_of_gyration``,
        ``compact``, ``extent`` of the largest cluster (among equal sizes the smallest key)."""
        return _properties_row(self._read_row("largest", "float64").cpu().numpy()[0, 4:])


class ClusterPropertiesRecorder(_Recorder):
    """Writer (``sim.operations.writers``) for a ``ClusterProperties`` in ``computes`` of the same simulation: its summary
    (20 float64: the number of clusters and the row of the largest one) appended to a device table at the timesteps the
    trigger fires inside ``Simulation.run`` -- the call's last kernel writes row k itself, nothing is read back, the host
    does not wait, and the trajectory is the same bit for bit with and without the recorder. Read after the run:
    ``timesteps``, ``num_clusters``, ``largest_cluster_size``, ``largest_cluster_key`` (frames,), ``largest_center``
    (frames, 3), ``largest_gyration`` (frames, 3, 3), ``largest_radius_of_gyration``, ``largest_compact`` (frames,);
    ``reset()`` forgets the frames."""

    def __init__(self, props, trigger):
        if not isinstance(props, ClusterProperties):
            raise _lib.AzpError("ClusterPropertiesRecorder: a ClusterProperties is expected, got %r" % (props,))
        self.props = self._compute = props
        super().__init__(trigger)

    def _table(self):
        k = len(self._steps)
        return self._rows[:k].cpu().numpy() if k else np.zeros((0, self._row_width()))

    @property
    def num_clusters(self):
        return self._table()[:, 0].astype(np.int64)

    @property
    def largest_cluster_size(self):
        return self._table()[:, 5].astype(np.int64)

    @property
    def largest_cluster_key(self):
        return self._table()[:, 4].astype(np.int64)

    @property
    def largest_center(self):
        return self._table()[:, 6:9].copy()

    @property
    def largest_gyration(self):
        return _gyration_matrix(self._table()[:, 9:15])

    @property
    def largest_radius_of_gyration(self):
        return np.sqrt(np.maximum(self._table()[:, 15], 0.0))

    @property
    def largest_compact(self):
        return self._table()[:, 16] != 0.0


# ---------------------------------------------------------------------------
# displacements between two times: mean squared displacement, self scattering
# ---------------------------------------------------------------------------
def average_over_origins(steps, origin_steps, rows):
    """The lag average behind the recorders of this section: ``steps`` (R,) the timestep of every recorded row,
    ``origin_steps`` (R, K) the timestep of the origin that slot held when the row was recorded (negative: the slot was
    not filled), ``rows`` (R, K, W) the SUMS of every (row, slot). Returns ``(lags, samples, sums)``: the distinct lags
    ``steps[r] - origin_steps[r, s]`` of the filled pairs in ascending order, how many pairs have each lag, and the rows
    of equal lag added, (lags, W), in the dtype of ``rows`` -- sums are added first, the caller normalises afterwards, so
    that pairs with different group sizes weigh by their particles. Pure host code."""
    steps = np.asarray(steps, dtype=np.int64).reshape(-1)
    origin_steps = np.asarray(origin_steps, dtype=np.int64)
    rows = np.asarray(rows)
    if origin_steps.ndim != 2 or rows.ndim != 3 or origin_steps.shape[0] != len(steps) or rows.shape[:2] != origin_steps.shape:
        raise _lib.AzpError("average_over_origins: steps (R,), origin_steps (R, K) and rows (R, K, W) are expected, got %r, %r and %r"
                            % (steps.shape, origin_steps.shape, rows.shape))
    filled = origin_steps >= 0
    lag = (steps[:, None] - origin_steps)[filled]
    lags = np.unique(lag)
    where = np.searchsorted(lags, lag)
    sums = np.zeros((len(lags), rows.shape[2]), dtype=rows.dtype)
    np.add.at(sums, where, rows[filled])
    return lags, np.bincount(where, minlength=len(lags)).astype(np.int64), sums


def displacement_moments(sums):
    """The properties of ``MeanSquaredDisplacement`` from the 12 doubles of ``azp_displacement_moments`` (N_g, S_x, S_y,
    S_z, S_xx, S_yy, S_zz, S_xy, S_xz, S_yz, S_4, 0; leading axes are kept): a dict of ``num_particles``,
    ``mean_displacement`` (.., 3), ``msd``, ``msd_components`` (.., 3), ``msd_tensor`` (.., 3, 3), ``msd_drift_removed``,
    ``fourth_moment`` and ``non_gaussian`` = 3 <d^4> / (5 <d^2>^2) - 1 (NaN where ``msd`` is 0). An empty group gives
    zeros. The compute, the recorders and the tests all go through here."""
    s = np.asarray(sums, dtype=np.float64)
    n = s[..., 0]
    inv = np.divide(1.0, n, out=np.zeros_like(n), where=n > 0.0)
    mean = s[..., 1:4] * inv[..., None]
    comp = s[..., 4:7] * inv[..., None]
    msd = ((s[..., 4] + s[..., 5]) + s[..., 6]) * inv
    xy, xz, yz = (s[..., 7 + c] * inv for c in range(3))
    tensor = np.stack([np.stack([comp[..., 0], xy, xz], axis=-1), np.stack([xy, comp[..., 1], yz], axis=-1),
                       np.stack([xz, yz, comp[..., 2]], axis=-1)], axis=-2)
    fourth = s[..., 10] * inv
    ngp = np.full(np.shape(msd), np.nan)
    np.divide(3.0 * fourth, 5.0 * msd * msd, out=ngp, where=msd != 0.0)
    ngp = np.where(msd != 0.0, ngp - 1.0, np.nan)
    return {"num_particles": np.asarray(n).astype(np.int64), "mean_displacement": mean, "msd": msd, "msd_components": comp,
            "msd_tensor": tensor, "msd_drift_removed": msd - ((mean[..., 0] ** 2 + mean[..., 1] ** 2) + mean[..., 2] ** 2),
            "fourth_moment": fourth, "non_gaussian": ngp}


def van_hove_from_counts(counts, n_g, r_max):
    """The self part of the van Hove function from the integer histogram of |d|: counts / (N_g x shell volume), so that
    sum_k van_hove[k] V_k = 1 - outside / N_g; zeros for an empty group. Leading axes are kept."""
    counts = np.asarray(counts, dtype=np.float64)
    nb = counts.shape[-1]
    n_g = np.asarray(n_g, dtype=np.float64)[..., None]
    if nb == 0:
        return np.zeros(counts.shape)
    return np.divide(counts, n_g * _shell_volumes(nb, r_max), out=np.zeros(counts.shape), where=n_g > 0.0)


def self_scattering_from_row(row, n_vectors):
    """(Re rho_s / N_g, Im rho_s / N_g) per vector from rows of ``azp_self_scattering`` (2 n + 2 doubles: Re[n], Im[n],
    N_g, bad_tags; leading axes are kept); zeros for an empty group."""
    row = np.asarray(row, dtype=np.float64)
    n = int(n_vectors)
    n_g = row[..., 2 * n:2 * n + 1]
    inv = np.divide(1.0, n_g, out=np.zeros_like(n_g), where=n_g > 0.0)
    return row[..., :n] * inv, row[..., n:2 * n] * inv


def intermediate_scattering_from_amplitudes(amplitudes, timesteps, group_sizes=None):
    """The collective intermediate scattering function from density amplitudes of several times (what
    ``StructureFactorRecorder.amplitudes`` holds: complex (frames, 2, n), rho_A and rho_B) and their ``timesteps``:
    ``(lags, F)`` with F (lags, n),

        F(m, tau) = <Re[rho_A(m, t + tau) conj(rho_B(m, t))]>_t / sqrt(N_A N_B)

    over all pairs of frames t + tau >= t, every frame serving as a time origin, with the lag averaging of
    ``average_over_origins``: the products of equal lag are added, then divided by the added sqrt(N_A(t + tau) N_B(t)).
    ``group_sizes``: (N_A, N_B) or one pair per frame (frames, 2); None leaves the mean product unnormalised. F(m, 0) is
    the static S_AB(m) averaged over the frames. Host code: the collective counterpart of F_s costs no kernel."""
    amp = np.asarray(amplitudes, dtype=np.complex128)
    steps = np.asarray(timesteps, dtype=np.int64).reshape(-1)
    if amp.ndim != 3 or amp.shape[1] != 2 or amp.shape[0] != len(steps):
        raise _lib.AzpError("intermediate_scattering_from_amplitudes: amplitudes must be (frames, 2, n) with one timestep per "
                            "frame, got %r and %d timesteps" % (amp.shape, len(steps)))
    frames, n = amp.shape[0], amp.shape[2]
    if group_sizes is None:
        sizes = np.ones((frames, 2))
    else:
        sizes = np.broadcast_to(np.asarray(group_sizes, dtype=np.float64), (frames, 2))
    origin_steps = np.where(steps[None, :] <= steps[:, None], steps[None, :], -1)  # (row r, origin s): s no later than r
    rows = np.zeros((frames, frames, n + 1))
    for r in range(frames):
        rows[r, :, :n] = (amp[r, 0][None, :] * np.conj(amp[:, 1])).real
        rows[r, :, n] = np.sqrt(sizes[r, 0] * sizes[:, 1])
    lags, _, sums = average_over_origins(steps, origin_steps, rows)
    norm = sums[:, n:]
    return lags, np.divide(sums[:, :n], norm, out=np.zeros((len(lags), n)), where=norm > 0.0)


class _TwoTimeCompute(_Compute):
    """What ``MeanSquaredDisplacement`` and ``SelfIntermediateScattering`` share: the time origin (wrapped positions and
    images BY TAG, ``csrc/displacement.hip``), the reverse-tag table and the refusals."""

    _needs_periodic = False

    def __init__(self, filter):
        name = type(self).__name__
        if not isinstance(filter, (All, Type)):
            raise _lib.AzpError("%s: filter must be All() or Type(...), got %r" % (name, filter))
        super().__init__(filter, False)
        self._origin = None  # (state, box key, timestep, positions (1, N, 4), images (1, N, 3))
        self._rtag = None    # (state, order generation, N, device tensor)

    def _state(self, name):
        """The state, after the refusals that every read and every record makes."""
        if not self._attached:
            raise DataAccessError(name)
        cls = type(self).__name__
        sim = self._sim
        if sim.domain is not None:
            raise _lib.AzpError("%s: decomposed runs are not supported (an origin is stored by tag on one device)" % cls)
        box = sim.state.box
        if not (box.Lx > 0.0 and box.Ly > 0.0 and box.Lz > 0.0):
            raise _lib.AzpError("%s: a 3-D box is needed (2-D systems are not supported), got %r" % (cls, box))
        if self._needs_periodic and not all(box.periodic):
            raise _lib.AzpError("%s: the box has to be periodic on all three axes (the wavevectors are those of its lattice), "
                                "got periodic = %r" % (cls, box.periodic))
        return sim.state

    def _reverse_tags(self, st):
        """(device table rtag[tag[i]] = i, stale): cached on (state, order_generation, N); a stale table is rebuilt by the
        next ``_scatter`` call, which the caller makes."""
        import torch

        c = self._rtag
        if c is not None and c[0] is st and c[1] == st.order_generation and c[2] == st.N and c[3].device == st.device:
            return c[3], False
        self._rtag = (st, st.order_generation, st.N, torch.empty(max(st.N, 1), dtype=torch.int32, device=st.device))
        return self._rtag[3], True

    def _scatter(self, st, pos0=None, image0=None, slot=0):
        """Queue ``azp_displacement_origin``: the current state into slot ``slot`` of the store (``pos0`` (K, N, 4),
        ``image0`` (K, N, 3); None: no origin is taken) and, where it is stale, the reverse-tag table. Returns the table."""
        rtag, stale = self._reverse_tags(st)
        if pos0 is None and not stale:
            return rtag
        a = _lib.DisplacementOriginArgs()
        a.d_pos, a.d_image, a.d_tag, a.N = st.pos.data_ptr(), st.image.data_ptr(), st.tag.data_ptr(), st.N
        a.slot, a.n_slots = int(slot), 1 if pos0 is None else pos0.shape[0]
        a.build_rtag = 1 if stale else 0
        if pos0 is not None:
            a.d_origin_pos, a.d_origin_image = pos0.data_ptr(), image0.data_ptr()
        a.d_rtag = rtag.data_ptr()
        _lib.check(_lib.lib().azp_displacement_origin(C.byref(a), _lib.raw_stream(st.device)), "azp_displacement_origin")
        return rtag

    @staticmethod
    def _store(st, n_slots):
        import torch

        return (torch.empty((n_slots, max(st.N, 1), 4), dtype=torch.float64, device=st.device),
                torch.empty((n_slots, max(st.N, 1), 3), dtype=torch.int32, device=st.device))

    def set_origin(self):
        """Take the time origin from the current state: the wrapped position and the image of every particle, by tag."""
        st = self._state("set_origin")
        o = self._origin
        if o is None or o[0] is not st or o[3].shape[1] != max(st.N, 1) or o[3].device != st.device:
            pos0, image0 = self._store(st, 1)
        else:
            pos0, image0 = o[3], o[4]
        self._scatter(st, pos0, image0, 0)
        self._origin = (st, st.box._key(), int(self._sim.timestep), pos0, image0)

    @property
    def origin_timestep(self):
        """The timestep the origin was taken at; None without an origin (none taken yet, or the state was replaced)."""
        o = self._origin
        if o is None or self._sim is None or o[0] is not self._sim.state:
            return None
        return o[2]

    def _check_box(self, st, key, what="the origin"):
        if key != st.box._key():
            raise _lib.AzpError("%s: the box changed since %s was taken (%r now): a displacement across a box change is not "
                                "defined here; take a new origin (set_origin(), or reset() of the recorder)"
                                % (type(self).__name__, what, st.box))

    def _current_origin(self, name):
        """(state, origin positions, origin images): the origin is taken now if there is none for this state."""
        st = self._state(name)
        if self._origin is None or self._origin[0] is not st:
            self.set_origin()
        o = self._origin
        self._check_box(st, o[1])
        return st, o[3], o[4]

    def _args(self, st, pos0, image0, n_origins, active):
        a = _lib.DisplacementArgs()
        a.d_pos, a.d_image, a.d_tag, a.N = st.pos.data_ptr(), st.image.data_ptr(), st.tag.data_ptr(), st.N
        a.d_rtag = self._scatter(st).data_ptr()
        a.ntypes = len(st.types)
        a.box = st.box.to_c()
        mask = self._type_mask(st)
        a.d_type_mask = mask.data_ptr() if mask is not None else None
        a.d_origin_pos, a.d_origin_image = pos0.data_ptr(), image0.data_ptr()
        a.n_origins, a.active_mask = int(n_origins), int(active)
        return a

    def _launch(self, d_out):
        """One row against this compute's own origin."""
        st, pos0, image0 = self._current_origin("row")
        self._launch_slots(d_out, st, pos0, image0, 1, 1)

    @staticmethod
    def _refuse_bad_tags(name, bad):
        if np.any(np.asarray(bad) != 0):
            raise _lib.AzpError("%s: %d tag slot(s) without a particle: the tags of the state are not a permutation of "
                                "0 .. N-1 (a tag >= N, a duplicate)" % (name, int(np.max(bad))))


class MeanSquaredDisplacement(_TwoTimeCompute):
    """Mean squared displacement of a group since a time origin, with the moments around it, by one deterministic pass
    over the particles (``csrc/displacement.hip``). Not part of the reference (freud's ``msd.MSD`` is the model in
    spirit); the semantics are this project's (``include/azp.h``).

    ``set_origin()`` stores the wrapped position r0 and the image n0 of every particle BY TAG; it is also taken by the
    first read without one, and dropped when the state is replaced. The displacement of a particle is
    d = (r - r0) + H (n - n0) with the images subtracted as integers first, H the lattice matrix of the box. A particle
    belongs to the group (``filter``: ``All()`` or ``Type(...)``) by its CURRENT type. Properties, computed when read:
    ``num_particles`` N_g, ``mean_displacement`` <d>, ``msd`` <|d|^2>, ``msd_components``, ``msd_tensor`` <d_a d_b>,
    ``msd_drift_removed`` = msd - |<d>|^2, ``fourth_moment`` <|d|^4>, ``non_gaussian`` = 3 <d^4> / (5 <d^2>^2) - 1 (NaN
    where msd is 0), with ``num_bins`` > 0 the self part of the van Hove function on [0, ``r_max``):
    ``van_hove_counts``, ``outside``, ``van_hove`` = counts / (N_g x shell volume), ``bin_edges``, ``bin_centers``; and
    ``displacements`` (N, 3) by tag, of every particle. An empty group gives zeros.

    All sums run in TAG order in the reproducible reduction of ``csrc/azp_reduce.hpp``: two reads agree bit for bit, a
    ``ParticleSorter.sort`` between them changes no bit, and ``tests/reduction_ref.tree_sum`` over the terms in tag
    order reproduces them. Refused with ``AzpError``: a filter that is not ``All()`` or ``Type(...)``, ``num_bins``
    outside [0, 8192], ``num_bins`` > 0 without a positive ``r_max`` (at construction); when read: a decomposed run, a
    2-D box, a box other than the origin's ("take a new origin"), tags that are not a permutation of 0 .. N-1."""

    def __init__(self, filter=None, num_bins=0, r_max=None):
        super().__init__(All() if filter is None else filter)
        if isinstance(num_bins, bool) or int(num_bins) != num_bins or not 0 <= int(num_bins) <= _lib.RDF_MAX_BINS:
            raise _lib.AzpError("MeanSquaredDisplacement: num_bins must be an integer in [0, %d], got %r" % (_lib.RDF_MAX_BINS, num_bins))
        self._num_bins = int(num_bins)
        if self._num_bins and (r_max is None or not (float(r_max) > 0.0 and np.isfinite(float(r_max)))):
            raise _lib.AzpError("MeanSquaredDisplacement: num_bins = %d needs a positive r_max, got %r" % (self._num_bins, r_max))
        self._r_max = None if r_max is None else float(r_max)
        self._disp = None

    @property
    def num_bins(self):
        return self._num_bins

    @property
    def r_max(self):
        return self._r_max

    @property
    def bin_edges(self):
        """numpy.ndarray: the ``num_bins + 1`` edges of the |d| bins."""
        return np.linspace(0.0, self._r_max or 0.0, self._num_bins + 1)

    @property
    def bin_centers(self):
        e = self.bin_edges
        return 0.5 * (e[1:] + e[:-1])

    def _row_width(self):
        return _lib.DISPLACEMENT_NSUMS + 2 + self._num_bins

    def _launch_slots(self, d_out, st, pos0, image0, n_origins, active, d_displacements=None):
        """Queue ``azp_displacement_moments``: ``n_origins`` rows of ``_row_width()`` words to ``d_out``, one per slot of the
        store (``pos0``, ``image0``); a slot whose bit in ``active`` is clear gives zeros."""
        a = self._args(st, pos0, image0, n_origins, active)
        a.num_bins = self._num_bins
        a.r_max = self._r_max if self._num_bins else 0.0
        a.d_displacements = d_displacements
        self._set_scratch(a, "azp_displacement_moments_scratch_size")
        a.d_out = d_out
        _lib.check(_lib.lib().azp_displacement_moments(C.byref(a), _lib.raw_stream(st.device)), "azp_displacement_moments")

    def _read(self, name):
        """The row of the current state against the origin as int64 numpy (the first 12 words are doubles)."""
        row = self._read_row(name, "int64").cpu().numpy()[0]
        self._refuse_bad_tags("MeanSquaredDisplacement", row[_lib.DISPLACEMENT_NSUMS])
        return row

    def _moments(self, name):
        return displacement_moments(self._read(name)[:_lib.DISPLACEMENT_NSUMS].view(np.float64))[name]

    @property
    def num_particles(self):
        return int(self._moments("num_particles"))

    @property
    def msd(self):
        return float(self._moments("msd"))

    @property
    def msd_drift_removed(self):
        return float(self._moments("msd_drift_removed"))

    @property
    def fourth_moment(self):
        return float(self._moments("fourth_moment"))

    @property
    def non_gaussian(self):
        return float(self._moments("non_gaussian"))

    @property
    def mean_displacement(self):
        return self._moments("mean_displacement")

    @property
    def msd_components(self):
        return self._moments("msd_components")

    @property
    def msd_tensor(self):
        return self._moments("msd_tensor")

    @property
    def van_hove_counts(self):
        """numpy int64 (num_bins,): particles of the group with |d| in each bin."""
        return self._read("van_hove_counts")[_lib.DISPLACEMENT_NSUMS + 2:].copy()

    @property
    def outside(self):
        """int: particles of the group with |d| >= r_max."""
        return int(self._read("outside")[_lib.DISPLACEMENT_NSUMS + 1])

    @property
    def van_hove(self):
        row = self._read("van_hove")
        return van_hove_from_counts(row[_lib.DISPLACEMENT_NSUMS + 2:], row[:1].view(np.float64)[0], self._r_max)

    @property
    def displacements(self):
        """numpy float64 (N, 3): d of EVERY particle (in the group or not), indexed by tag."""
        import torch

        st, pos0, image0 = self._current_origin("displacements")
        if self._disp is None or self._disp.shape[0] != max(st.N, 1) or self._disp.device != st.device:
            self._disp = torch.empty((max(st.N, 1), 3), dtype=torch.float64, device=st.device)
        row = self._row_buffer(self._row_width(), "int64")
        self._launch_slots(row.data_ptr(), st, pos0, image0, 1, 1, self._disp.data_ptr())
        self._refuse_bad_tags("MeanSquaredDisplacement", row.cpu().numpy()[0, _lib.DISPLACEMENT_NSUMS])
        return self._disp[: st.N].cpu().numpy()


class SelfIntermediateScattering(_TwoTimeCompute):
    """Self intermediate scattering function F_s(q, t) of a group since a time origin on the reciprocal-lattice vectors
    of the box (``csrc/displacement.hip``; this project's): rho_s(m) = sum_j exp(-2 pi i m . (f_j - f0_j))
    over the group, f the fractional coordinates of the wrapped positions -- on the reciprocal lattice the images drop
    out exactly. The vector set, its thinning and the |q| bins are those of ``StructureFactor`` with the same arguments
    (``structure_factor_vectors``). ``set_origin()``, ``origin_timestep`` as ``MeanSquaredDisplacement``. Properties,
    computed when read: ``vectors``, ``q``, ``vectors_per_bin``, ``num_particles``, ``vector_scattering`` = Re rho_s / N_g,
    ``scattering`` (its mean per |q| bin, NaN in an empty bin) and ``imaginary`` (the mean of Im rho_s / N_g per bin: the
    odd part, which shows a drift). The sums run in tag order in a fixed shape: bit-identical between two reads and
    under a sort. Refused as ``StructureFactor`` refuses its arguments; when read: a decomposed run, a 2-D or not fully
    periodic box, a box other than the origin's, an empty vector set, tags that are not a permutation."""

    _needs_periodic = True

    def __init__(self, filter, q_max, num_bins, max_vectors_per_bin=None, seed=0):
        super().__init__(filter)
        try:  # (the argument checks of StructureFactor, which also keeps the values)
            self._sf = StructureFactor(filter, filter, q_max, num_bins, max_vectors_per_bin, seed)
        except _lib.AzpError as e:
            raise _lib.AzpError(str(e).replace("StructureFactor", "SelfIntermediateScattering")) from None
        self._set = None

    q_max = property(lambda self: self._sf.q_max)
    num_bins = property(lambda self: self._sf.num_bins)
    max_vectors_per_bin = property(lambda self: self._sf.max_vectors_per_bin)
    seed = property(lambda self: self._sf.seed)
    bin_edges = property(lambda self: self._sf.bin_edges)
    bin_centers = property(lambda self: self._sf.bin_centers)

    def _vector_set(self, name="vectors"):
        """(m, bins, device triples) for the current box, rebuilt when the box changed."""
        import torch

        st = self._state(name)
        sf = self._sf
        key = (st.box._key(), st.device)
        if self._set is None or self._set[0] != key:
            m, bins = structure_factor_vectors(st.box, sf.q_max, sf.num_bins, sf.max_vectors_per_bin, sf.seed)
            if len(m) == 0:
                raise _lib.AzpError("SelfIntermediateScattering: q_max = %r is below the smallest |q| of the box: no wavevector" % (sf.q_max,))
            self._set = (key, m, bins, torch.from_numpy(np.ascontiguousarray(m, dtype=np.int32)).to(st.device))
        return self._set[1:]

    def _row_width(self):
        return 2 * len(self._vector_set()[0]) + 2

    def _launch_slots(self, d_out, st, pos0, image0, n_origins, active):
        """Queue ``azp_self_scattering``: ``n_origins`` rows of ``2 n + 2`` doubles to ``d_out``."""
        m, _, triples = self._vector_set()
        a = self._args(st, pos0, image0, n_origins, active)
        a.n_vectors = len(m)
        a.d_vectors = triples.data_ptr()
        self._set_scratch(a, "azp_self_scattering_scratch_size")
        a.d_out = d_out
        _lib.check(_lib.lib().azp_self_scattering(C.byref(a), _lib.raw_stream(st.device)), "azp_self_scattering")

    def _read(self, name):
        row = self._read_row(name, "float64").cpu().numpy()[0]
        self._refuse_bad_tags("SelfIntermediateScattering", row[-1])
        return row

    @property
    def vectors(self):
        """numpy int64 (n, 3): the integer triples m = (h, k, l), ordered by (l, k, h)."""
        return self._vector_set("vectors")[0].copy()

    @property
    def q(self):
        """numpy float64 (n,): the lengths |q(m)|."""
        v = reciprocal_vectors(self._sim.state.box, self._vector_set("q")[0])
        return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])

    @property
    def vectors_per_bin(self):
        return np.bincount(self._vector_set("vectors_per_bin")[1], minlength=self.num_bins).astype(np.int64)

    @property
    def num_particles(self):
        return int(self._read("num_particles")[-2])

    @property
    def vector_scattering(self):
        """numpy float64 (n,): Re rho_s(m) / N_g of every vector."""
        row = self._read("vector_scattering")
        return self_scattering_from_row(row, (len(row) - 2) // 2)[0]

    def _binned(self, name, part):
        row = self._read(name)
        return spherical_average(self_scattering_from_row(row, (len(row) - 2) // 2)[part], self._vector_set()[1], self.num_bins)[0]

    @property
    def scattering(self):
        """numpy float64 (num_bins,): F_s per |q| bin, the mean of Re rho_s / N_g over the bin's vectors (NaN: none)."""
        return self._binned("scattering", 0)

    @property
    def imaginary(self):
        """numpy float64 (num_bins,): the mean of Im rho_s / N_g per |q| bin (zero without a drift)."""
        return self._binned("imaginary", 1)


class _TwoTimeRecorder(_Recorder):
    """The recorders of this section: a ring of ``origins`` = K <= 64 time origins on the device, filled by the recorder.
    The first firing, and then every ``origin_every``-th firing (None: no further one), first scatters the current
    state into slot (origins taken so far) mod K, overwriting the oldest; then ONE launch writes the rows of all K slots
    into row k of the table (K x the compute's row width; a slot not yet filled gives zeros). Which origin timestep each
    slot held at each row is host data like the timesteps: nothing is read back, the host never waits, and the
    trajectory is the same bit for bit with and without the recorder. An origin taken and compared in the same firing
    is lag 0. All rows and origins belong to ONE box and one state: a record in another box raises ``AzpError``;
    ``reset()`` forgets rows and origins."""

    def __init__(self, compute, trigger, origins=1, origin_every=None):
        name = type(self).__name__
        if isinstance(origins, bool) or int(origins) != origins or not 1 <= int(origins) <= _lib.DISPLACEMENT_MAX_ORIGINS:
            raise _lib.AzpError("%s: origins must be an integer in [1, %d], got %r" % (name, _lib.DISPLACEMENT_MAX_ORIGINS, origins))
        if origin_every is not None and (isinstance(origin_every, bool) or int(origin_every) != origin_every or int(origin_every) < 1):
            raise _lib.AzpError("%s: origin_every must be None or a positive integer, got %r" % (name, origin_every))
        self._compute = compute
        self.origins = int(origins)
        self.origin_every = None if origin_every is None else int(origin_every)
        super().__init__(trigger)

    def reset(self):
        super().reset()
        self._ring = None           # (state, box key, positions (K, N, 4), images (K, N, 3))
        self._slot_steps = [-1] * getattr(self, "origins", 1)
        self._taken = 0
        self._origin_steps = []     # per row: the origin timestep of every slot (-1: not filled)

    def _row_width(self):
        return self.origins * self._compute._row_width()

    def _record(self, sim, timestep):
        c = self._compute
        name = type(self).__name__
        st = c._state(name)
        if self._ring is not None and (self._ring[0] is not st or self._ring[2].shape[1] != max(st.N, 1)):
            raise _lib.AzpError("%s: the state was replaced with rows recorded; call reset() first" % name)
        if self._ring is not None and self._ring[1] != st.box._key():
            raise _lib.AzpError("%s: the box changed with rows recorded (%r now): the origins of the ring belong to another "
                                "box; call reset() first" % (name, st.box))
        if self._ring is None:
            self._ring = (st, st.box._key()) + c._store(st, self.origins)
        k = len(self._steps)
        if k == 0 or (self.origin_every is not None and k % self.origin_every == 0):
            slot = self._taken % self.origins
            c._scatter(st, self._ring[2], self._ring[3], slot)
            self._slot_steps[slot] = int(timestep)
            self._taken += 1
        super()._record(sim, timestep)
        self._origin_steps.append(list(self._slot_steps))

    def _launch_row(self, d_out):
        st = self._ring[0]
        active = sum(1 << s for s, t in enumerate(self._slot_steps) if t >= 0)
        self._compute._launch_slots(d_out, st, self._ring[2], self._ring[3], self.origins, active)

    @property
    def origin_timesteps(self):
        """numpy int64 (rows, origins): the timestep of the origin every slot held at every row, -1 where not filled."""
        return np.array(self._origin_steps, dtype=np.int64).reshape(len(self._steps), self.origins)

    def _host_rows(self, dtype):
        """The table as numpy (rows, origins, row width of the compute) in ``dtype`` (8-byte words)."""
        k = len(self._steps)
        w = self._compute._row_width() if k else 0
        if k == 0:
            return np.zeros((0, self.origins, w), dtype=dtype)
        return self._rows[:k].cpu().numpy().view(dtype).reshape(k, self.origins, w)

    def _lag_sums(self, rows):
        return average_over_origins(self._steps, self.origin_timesteps, rows)

    @property
    def lags(self):
        """numpy int64: the distinct lags (row timestep - origin timestep) recorded, ascending."""
        return self._lag_sums(np.zeros((len(self._steps), self.origins, 0)))[0]

    @property
    def samples_per_lag(self):
        """numpy int64: the (row, slot) pairs behind every lag."""
        return self._lag_sums(np.zeros((len(self._steps), self.origins, 0)))[1]


class MeanSquaredDisplacementRecorder(_TwoTimeRecorder):
    """Writer (``sim.operations.writers``) for a ``MeanSquaredDisplacement`` in ``computes`` of the same simulation, with
    a ring of ``origins`` time origins (see ``_TwoTimeRecorder`` for the ring, ``origin_every`` and the guarantees).
    Read after the run: ``timesteps``, ``origin_timesteps``, ``table`` (per row and slot the properties of the compute;
    an unfilled slot gives zeros, NaN for ``non_gaussian``) and the lag averages ``lags``, ``samples_per_lag``, ``msd``,
    ``msd_components``, ``non_gaussian`` and ``van_hove`` (lags, num_bins): over all (row, slot) pairs of equal lag the
    SUMS are added and then normalised (``average_over_origins``)."""

    def __init__(self, msd, trigger, origins=1, origin_every=None):
        if not isinstance(msd, MeanSquaredDisplacement):
            raise _lib.AzpError("MeanSquaredDisplacementRecorder: msd must be a MeanSquaredDisplacement, got %r" % (msd,))
        self.msd_compute = msd
        super().__init__(msd, trigger, origins, origin_every)

    def _words(self):
        rows = self._host_rows(np.int64)
        self._compute._refuse_bad_tags("MeanSquaredDisplacementRecorder", rows[..., _lib.DISPLACEMENT_NSUMS] if rows.size else 0)
        return rows

    @property
    def table(self):
        """dict of numpy arrays (rows, origins, ...) keyed by the property names of ``MeanSquaredDisplacement``."""
        rows = self._words()
        ns = _lib.DISPLACEMENT_NSUMS
        sums = np.ascontiguousarray(rows[..., :ns]).view(np.float64)
        out = displacement_moments(sums)
        out["van_hove_counts"] = rows[..., ns + 2:].copy()
        out["outside"] = rows[..., ns + 1].copy()
        out["van_hove"] = van_hove_from_counts(rows[..., ns + 2:], sums[..., 0], self._compute.r_max)
        return out

    def _averaged(self):
        rows = self._words()
        ns = _lib.DISPLACEMENT_NSUMS
        _, _, sums = self._lag_sums(np.ascontiguousarray(rows[..., :ns]).view(np.float64))
        _, _, words = self._lag_sums(rows[..., ns:])
        return sums, words

    @property
    def msd(self):
        """numpy float64 (lags,): the sums of |d|^2 of equal lag added, over the added N_g."""
        return displacement_moments(self._averaged()[0])["msd"]

    @property
    def msd_components(self):
        return displacement_moments(self._averaged()[0])["msd_components"]

    @property
    def non_gaussian(self):
        return displacement_moments(self._averaged()[0])["non_gaussian"]

    @property
    def van_hove(self):
        sums, words = self._averaged()
        return van_hove_from_counts(words[:, 2:], sums[:, 0], self._compute.r_max)


class SelfIntermediateScatteringRecorder(_TwoTimeRecorder):
    """Writer (``sim.operations.writers``) for a ``SelfIntermediateScattering`` in ``computes`` of the same simulation,
    with a ring of ``origins`` time origins (see ``_TwoTimeRecorder``). Read after the run: ``timesteps``,
    ``origin_timesteps``, ``table`` (``num_particles`` (rows, origins), ``vector_scattering`` and ``vector_imaginary``
    (rows, origins, n)) and the lag averages ``lags``, ``samples_per_lag``, ``vector_scattering_per_lag`` (lags, n) and
    ``scattering`` (lags, num_bins): Re rho_s of equal lag added over the added N_g, then the mean over each bin's
    vectors."""

    def __init__(self, fs, trigger, origins=1, origin_every=None):
        if not isinstance(fs, SelfIntermediateScattering):
            raise _lib.AzpError("SelfIntermediateScatteringRecorder: fs must be a SelfIntermediateScattering, got %r" % (fs,))
        self.fs = fs
        super().__init__(fs, trigger, origins, origin_every)

    def _words(self):
        rows = self._host_rows(np.float64)
        self._compute._refuse_bad_tags("SelfIntermediateScatteringRecorder", rows[..., -1] if rows.size else 0)
        return rows

    @property
    def table(self):
        rows = self._words()
        n = (rows.shape[2] - 2) // 2 if rows.shape[2] else 0
        re, im = self_scattering_from_row(rows, n) if rows.shape[2] else (rows, rows)
        return {"num_particles": rows[..., 2 * n].astype(np.int64) if rows.shape[2] else np.zeros(rows.shape[:2], dtype=np.int64),
                "vector_scattering": re, "vector_imaginary": im}

    @property
    def vector_scattering_per_lag(self):
        rows = self._words()
        _, _, sums = self._lag_sums(rows)
        n = (sums.shape[1] - 2) // 2 if sums.shape[1] else 0
        return self_scattering_from_row(sums, n)[0] if sums.shape[1] else sums

    @property
    def scattering(self):
        """numpy float64 (lags, num_bins): F_s(|q|, lag), NaN in a bin without vectors."""
        per = self.vector_scattering_per_lag
        nb = self.fs.num_bins
        if per.shape[0] == 0:
            return np.zeros((0, nb))
        bins = self.fs._vector_set()[1]
        return np.stack([spherical_average(r, bins, nb)[0] for r in per])


# ---------------------------------------------------------------------------
# pressure profile (Irving-Kirkwood contour)
# ---------------------------------------------------------------------------
PRESSURE_PROFILE_PROPERTIES = ("configurational_pressure_tensor", "kinetic_pressure_tensor", "pressure_tensor", "normal_pressure",
                               "tangential_pressure", "bin_volumes", "num_pairs", "num_terms", "overflow")
_AXES = {"x": 0, "y": 1, "z": 2}
_DIAGONAL = (0, 3, 5)  # xx, yy, zz among xx, xy, xz, yy, yz, zz


def pressure_profile_shift(n_particles, max_term):
    """The shift of ``azp_pressure_profile_args`` for N particles: terms are kept in units of 2^-shift, the largest
    shift (at most 52) at which ``max_term * 2^shift * 2^pair_bits <= 2^63``, ``pair_bits = ceil(log2 N) + 8`` -- the sum
    of a word cannot wrap while fewer than 2^pair_bits pairs are evaluated. Returns ``(shift, pair_bits)``; ``AzpError``
    where ``max_term`` leaves no shift >= 0."""
    max_term = float(max_term)
    if not (max_term > 0.0 and np.isfinite(max_term)):
        raise _lib.AzpError("PressureProfile: max_term must be positive and finite, got %r" % (max_term,))
    pair_bits = max(int(n_particles) - 1, 1).bit_length() + 8
    m = int(np.ceil(np.log2(max_term)))
    while 2.0 ** m < max_term:  # (log2 rounded down at a power of two's neighbour)
        m += 1
    shift = min(52, 63 - pair_bits - m)
    if shift < 0:
        raise _lib.AzpError("PressureProfile: max_term = %r is too large for %d particles (no integer scale is left)"
                            % (max_term, n_particles))
    return shift, pair_bits


def pressure_profile_quantities(row, kinetic_rows, bin_volumes, axis, bin_width, streaming="subtract", interfaces=2, shift=None):
    """The quantities of ``compute.PressureProfile`` from raw rows. ``row``: (..., 6 bins + 4) int64 of
    ``azp_pressure_profile_*`` (a sum of rows where ``shift`` is given: the shift word of a sum is meaningless);
    ``kinetic_rows``: (..., bins, 18 + types) raw rows of ``azp_thermo_field_sums`` on the same bins (their W slots are
    not read); ``bin_volumes``: (..., bins) or one that broadcasts; ``axis``: 0, 1, 2; ``bin_width``: the width of a bin
    along the axis. Returns a dict: ``configurational_pressure_tensor`` = sums 2^-shift / V_k, ``kinetic_pressure_tensor``
    = K'_ab / V_k (``streaming`` as ``thermo_field_quantities``), ``pressure_tensor`` their sum (all (..., bins, 6), xx,
    xy, xz, yy, yz, zz), ``normal_pressure`` the axis' diagonal component, ``tangential_pressure`` the mean of the other
    two, ``surface_tension`` = (1 / interfaces) sum_k (P_N - P_T)_k bin_width, ``bin_volumes``, ``num_pairs``,
    ``num_terms`` and ``overflow``. Plain numpy in a fixed order: the properties and the recorder go through here."""
    if axis not in (0, 1, 2):
        raise _lib.AzpError("pressure_profile_quantities: axis must be 0, 1 or 2, got %r" % (axis,))
    if isinstance(interfaces, bool) or int(interfaces) != interfaces or int(interfaces) < 1:
        raise _lib.AzpError("pressure_profile_quantities: interfaces must be a positive integer, got %r" % (interfaces,))
    row = np.asarray(row, dtype=np.int64)
    if row.shape[-1] < 10 or (row.shape[-1] - 4) % 6:
        raise _lib.AzpError("pressure_profile_quantities: a row has 6 bins + 4 words, got %d" % row.shape[-1])
    nb = (row.shape[-1] - 4) // 6
    if shift is None:
        shift = row[..., -1]
    scale = np.ldexp(1.0, -np.asarray(shift, dtype=np.int64))
    sums = row[..., : 6 * nb].reshape(row.shape[:-1] + (nb, 6)).astype(np.float64) * np.asarray(scale)[..., None, None]
    kin = np.asarray(kinetic_rows, dtype=np.float64).copy()
    if kin.shape[-2] != nb:
        raise _lib.AzpError("pressure_profile_quantities: %d kinetic rows for %d bins" % (kin.shape[-2], nb))
    kin[..., 11:17] = 0.0  # (the field's W is the per-atom virial: not this compute's)
    vol = np.broadcast_to(np.asarray(bin_volumes, dtype=np.float64), sums.shape[:-1])
    p_conf = sums / vol[..., None]
    p_kin = thermo_field_quantities(kin, vol, streaming)["pressure_tensor"]
    p = p_kin + p_conf
    others = [d for d in range(3) if d != axis]
    p_n = p[..., _DIAGONAL[axis]]
    p_t = 0.5 * (p[..., _DIAGONAL[others[0]]] + p[..., _DIAGONAL[others[1]]])
    gamma = ((p_n - p_t) * np.asarray(bin_width, dtype=np.float64)[..., None]).sum(axis=-1) / float(interfaces)
    return dict(configurational_pressure_tensor=p_conf, kinetic_pressure_tensor=p_kin, pressure_tensor=p, normal_pressure=p_n,
                tangential_pressure=p_t, surface_tension=gamma, bin_volumes=vol, num_pairs=row[..., -4].copy(),
                num_terms=row[..., -3].copy(), overflow=row[..., -2].copy())


def _pressure_profile_force(f):
    """How ``PressureProfile`` takes the force ``f``: ``("pair", libazp entry, evaluator)``, ``("bond" | "pair group",
    evaluator)`` for the bonds and special pairs, ``None`` for a one-body force; ``AzpError`` for the others."""
    from . import angle, bond, dihedral, external, pair, special_pair, wall

    name = type(f).__name__
    if isinstance(f, pair.DPDGeneralWeight):
        raise _lib.AzpError("PressureProfile: %s is a thermostat: its pair force depends on the velocities and on random "
                            "numbers, which the contour integral of a configuration does not hold" % name)
    if isinstance(f, pair.TwoPatchMorse):
        raise _lib.AzpError("PressureProfile: %s is anisotropic: its force is not along the line between the particles" % name)
    if isinstance(f, (angle.Angle, dihedral.Dihedral)):
        raise _lib.AzpError("PressureProfile: %s is a many-body force: its contour is not a single segment (out of scope)" % name)
    pairs = {pair.PerturbedLennardJones: "perturbed_lennard_jones", pair.Hertz: "hertz", pair.ExpandedYukawa: "expanded_yukawa",
             pair.Colloid: "colloid", pair.DPDConservativeGeneralWeight: "dpd_conservative", pair.Table: "table"}
    names = {pair.Table: "PairTable", bond.Table: "BondTable", special_pair.LJ: "SpecialPairLJ"}
    for cls, entry in pairs.items():
        if type(f) is cls:
            return ("pair", "azp_pressure_profile_pairs_" + entry, _lib.PP_EVALUATORS[names.get(cls, cls.__name__)])
    for cls in (bond.DoubleWell, bond.Quartic, bond.Table, special_pair.LJ):
        if type(f) is cls:
            return ("group", f._kind, _lib.PP_EVALUATORS[names.get(cls, cls.__name__)])
    if isinstance(f, (external.HarmonicBarrier, wall._WallPotential)):
        return None
    raise _lib.AzpError("PressureProfile: %s is not a force this compute knows how to spread over a contour" % name)


class _KineticField(ThermodynamicField):
    """The ``CartesianThermodynamicField`` a ``PressureProfile`` owns: counts, M, P and K on its bins; no force is read."""

    _coordinates = _lib.COORDINATES_CARTESIAN

    def _forces_evaluated(self):
        return False, False


class PressureProfile(_Compute):
    """The pressure tensor along one Cartesian axis by the Irving-Kirkwood contour (this project's):
    ``num_bins`` equal slabs on [``lower``, ``upper``) along ``axis`` ("x", "y" or "z"; default range: the whole box
    length). The virial of every pair is spread along the straight line between the two particles: a slab receives the
    fraction of the line's extent along the axis that lies in it. Unlike the per-atom profile of
    ``ThermodynamicField`` its normal component is constant across a flat interface at equilibrium, and
    ``surface_tension`` is the mechanical route, gamma = (1 / interfaces) sum_k (P_N - P_T)_k delta.

    ``forces``: the forces that count, default every force of the integrator. The isotropic pair potentials
    (``Colloid``, ``ExpandedYukawa``, ``Hertz``, ``PerturbedLennardJones``, ``DPDConservativeGeneralWeight``,
    ``pair.Table``; with their ``r_cut``, ``r_on`` and ``mode``, less the pairs their neighbor list's ``exclusions``
    name) and the two-body bonded forces (``bond.DoubleWell``, ``bond.Quartic``, ``bond.Table``, ``special_pair.LJ``) are
    evaluated pair by pair with the evaluators the force kernels use; barriers and walls are one-body and skipped; the
    DPD thermostat, ``TwoPatchMorse``, angles, dihedrals and anything else are refused with an ``AzpError``. The forces
    themselves are not read: ``compute_virial`` is neither needed nor turned on, but the forces must be attached
    (``sim.run(0)``).

    Pairs, weights and integer accumulation are stated in ``include/azp.h`` ("pressure profile"). A term of magnitude
    ``max_term`` or more (two particles nearly on top of each other) is not added but counted in ``overflow``; reading a
    profile then raises and names ``max_term``, as it does when more pairs were evaluated than the integer scale was
    chosen for (2^(ceil(log2 N) + 8)). The raw row is the same bits between two reads, between the paths, under the
    particle sorter and with or without a recorder.

    The range wraps (bin indices modulo ``num_bins``) where ``lower`` and ``upper`` are both left None and the axis is
    periodic; then a tilt that shears the axis (xy, xz for "x"; yz for "y") is refused. With explicit bounds the parts of
    a line outside the range are dropped. V_k = V_box delta / L_axis. The kinetic part K'_ab / V_k and the counts come
    from a ``CartesianThermodynamicField`` on the same bins that this compute owns (``All()``, the same
    ``streaming``). ``path``: 0 automatic, 1 all-pairs (any box), 2 cells (orthorhombic, three cells of the largest
    ``r_cut`` on every periodic axis), as ``RadialDistributionFunction.path``. Single-domain states only: a pair that
    straddles two ranks would need its line cut at the boundary. At most 8 forces in the integrator (the owned field's
    limit)."""

    def __init__(self, axis, num_bins, forces=None, lower=None, upper=None, streaming="subtract", max_term=1024.0):
        super().__init__(All(), False)
        if axis not in _AXES:
            raise _lib.AzpError("PressureProfile: axis must be 'x', 'y' or 'z', got %r" % (axis,))
        self._axis = _AXES[axis]
        if isinstance(num_bins, bool) or int(num_bins) != num_bins or not 1 <= int(num_bins) <= _lib.PRESSURE_PROFILE_MAX_BINS:
            raise _lib.AzpError("PressureProfile: num_bins must be an integer in [1, %d], got %r"
                                % (_lib.PRESSURE_PROFILE_MAX_BINS, num_bins))
        self._num_bins = int(num_bins)
        if (lower is None) != (upper is None):
            raise _lib.AzpError("PressureProfile: give both lower and upper, or neither")
        if lower is not None:
            lower, upper = float(lower), float(upper)
            if not (np.isfinite(lower) and np.isfinite(upper) and upper > lower):
                raise _lib.AzpError("PressureProfile: upper = %r must be larger than lower = %r" % (upper, lower))
        self._lower, self._upper = lower, upper
        if streaming not in ("subtract", "keep"):
            raise _lib.AzpError("streaming must be 'subtract' or 'keep', got %r" % (streaming,))
        self._streaming = streaming
        pressure_profile_shift(2, max_term)
        self._max_term = float(max_term)
        self.forces = None if forces is None else list(forces)
        if self.forces is not None:
            for f in self.forces:
                _pressure_profile_force(f)
        self.path = _lib.RDF_PATH_AUTO
        bins = [0, 0, 0]
        bins[self._axis] = self._num_bins
        self._field = _KineticField(bins, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), All(), streaming)

    axis = property(lambda self: "xyz"[self._axis])
    num_bins = property(lambda self: self._num_bins)
    streaming = property(lambda self: self._streaming)
    max_term = property(lambda self: self._max_term)

    @property
    def path(self):
        return self._path

    @path.setter
    def path(self, value):
        if value not in (_lib.RDF_PATH_AUTO, _lib.RDF_PATH_ALL_PAIRS, _lib.RDF_PATH_CELLS):
            raise _lib.AzpError("PressureProfile: path must be 0 (auto), 1 (all-pairs) or 2 (cells), got %r" % (value,))
        self._path = int(value)

    def _range(self, box):
        """(lower, upper, wrap) in ``box``."""
        length = (box.Lx, box.Ly, box.Lz)[self._axis]
        if self._lower is None:
            return -0.5 * length, 0.5 * length, bool(box.periodic[self._axis])
        return self._lower, self._upper, False

    def _edges(self):
        if self._lower is None and not self._attached:
            raise DataAccessError("bin_edges")
        lo, hi, _ = self._range(self._sim.state.box) if self._lower is None else (self._lower, self._upper, False)
        return np.linspace(lo, hi, self._num_bins + 1)

    @property
    def bin_edges(self):
        """numpy.ndarray: the ``num_bins + 1`` edges of the slabs (of the current box where the range is the default)."""
        return self._edges()

    @property
    def bin_centers(self):
        e = self._edges()
        return 0.5 * (e[1:] + e[:-1])

    def _bin_width(self, box):
        lo, hi, _ = self._range(box)
        return (hi - lo) / self._num_bins

    def _bin_volumes(self, box):
        length = (box.Lx, box.Ly, box.Lz)[self._axis]
        return np.full(self._num_bins, box.volume * (self._bin_width(box) / length), dtype=np.float64)

    # -- one launch ----------------------------------------------------------
    def _kinetic_width(self):
        return self._num_bins * (_lib.THERMO_FIELD_NSUMS + len(self._sim.state.types))

    def _row_width(self):
        """6 bins + 4 integer words, then the kinetic field's row (float64 bits in the same 8-byte words)."""
        return 6 * self._num_bins + 4 + self._kinetic_width()

    def _forces(self):
        integ = self._sim.operations.integrator
        forces = self.forces if self.forces is not None else (list(integ.forces) if integ is not None else [])
        out = []
        for f in forces:
            how = _pressure_profile_force(f)
            if how is not None:
                if f._state is not self._sim.state:
                    raise _lib.AzpError("PressureProfile: %s is not attached to this simulation's state; call sim.run(0)"
                                        % type(f).__name__)
                out.append((f, how))
        return out

    def _launch(self, d_out):
        """Queue the kernels of every force and the kinetic field for the current state, the row going to ``d_out``."""
        sim = self._sim
        st = sim.state
        if sim.domain is not None:
            raise _lib.AzpError("PressureProfile: decomposed runs are not supported (the line of a pair that straddles two "
                                "ranks would have to be cut at the boundary)")
        box = st.box
        lo, hi, wrap = self._range(box)
        if wrap and ((self._axis == 0 and (box.xy != 0.0 or box.xz != 0.0)) or (self._axis == 1 and box.yz != 0.0)):
            raise _lib.AzpError("PressureProfile: axis %r of %r is sheared by a tilt: its slabs are not periodic images of "
                                "themselves; profile along z, or give lower and upper" % ("xyz"[self._axis], box))
        shift, _ = pressure_profile_shift(st.N, self._max_term)
        a = _lib.PressureProfileArgs()
        a.d_pos, a.d_tag = st.pos.data_ptr(), st.tag.data_ptr()
        a.N = st.N
        a.ntypes = len(st.types)
        a.box = box.to_c()
        a.axis, a.num_bins = self._axis, self._num_bins
        a.lower = lo
        a.scale = self._num_bins / (hi - lo)
        a.max_term = self._max_term
        a.wrap, a.shift = int(wrap), shift
        a.path = self._path
        a.d_out = d_out
        lib = _lib.lib()
        stream = _lib.raw_stream(st.device)
        forces = self._forces()
        _lib.check(lib.azp_pressure_profile_begin(C.byref(a), stream), "azp_pressure_profile_begin")
        for f, how in forces:
            if f._tables is None:
                f._build_tables()
            if how[0] == "pair":
                r_max = float(np.max(f._r_cut_matrix()))
                if not r_max > 0.0:
                    continue
                _check_pair_range("PressureProfile (%s)" % type(f).__name__, box, r_max)
                a.d_rcutsq, a.d_ronsq = f._tables["rcutsq"].data_ptr(), f._tables["ronsq"].data_ptr()
                a.r_max = r_max
                a.shift_mode = {"none": 0, "shift": 1, "xplor": 2}[f.mode]
                params = f._tables["params"].data_ptr()
                if self._path == _lib.RDF_PATH_CELLS and box.is_triclinic:
                    raise _lib.AzpError("PressureProfile: path 2 (cells) needs an orthorhombic box, got %r" % (box,))
                self._set_scratch(a, "azp_pressure_profile_scratch_size")
                _lib.check(getattr(lib, how[1])(C.byref(a), params, stream), how[1])
                kinds = f.nlist._exclusion_kinds
                if kinds and any(g.n for g in st.groups.values()):
                    x = _lib.PressureProfileListArgs()
                    x.profile = a
                    n_excl, excl, pitch = st.merged_exclusion_table(kinds)
                    x.d_table, x.d_counts, x.pitch = excl.data_ptr(), n_excl.data_ptr(), pitch
                    x.evaluator, x.sign = how[2], -1
                    _lib.check(lib.azp_pressure_profile_listed(C.byref(x), params, stream), "azp_pressure_profile_listed")
            else:
                kind = how[1]
                if not st.groups[kind].n:
                    continue
                tab = st.group_table(kind)
                x = _lib.PressureProfileListArgs()
                x.profile = a
                x.profile.d_rcutsq = x.profile.d_ronsq = None
                x.profile.shift_mode = 0
                x.d_table, x.d_counts, x.pitch = tab["table"].data_ptr(), tab["n_%ss" % kind].data_ptr(), tab["pitch"]
                x.n_types = max(len(f._types()), 1)
                x.evaluator, x.sign = how[2], 1
                _lib.check(lib.azp_pressure_profile_listed(C.byref(x), f._tables.data_ptr(), stream), "azp_pressure_profile_listed")
        field = self._field
        field._sim = sim
        lower, upper = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
        lower[self._axis], upper[self._axis] = lo, hi
        field.lower_bounds, field.upper_bounds = lower, upper
        field._launch(d_out + (6 * self._num_bins + 4) * 8)

    # -- results -------------------------------------------------------------
    def _split(self, host):
        """(k, row width) int64 host rows as the integer rows and the kinetic rows (k, bins, 18 + types)."""
        n = 6 * self._num_bins + 4
        return host[:, :n], np.ascontiguousarray(host[:, n:]).view(np.float64).reshape(host.shape[0], self._num_bins, -1)

    def _check_rows(self, rows, n_particles, what):
        """Raise where a row cannot be trusted: refused terms, or more pairs than the scale was chosen for."""
        for r, n in zip(rows, n_particles):
            _, pair_bits = pressure_profile_shift(n, self._max_term)
            if int(r[-2]) != 0:
                raise _lib.AzpError("PressureProfile.%s: %d terms were not finite or reached max_term = %r and were left out "
                                    "(particles nearly on top of each other?); raise max_term" % (what, int(r[-2]), self._max_term))
            if int(r[-4]) >= 2 ** pair_bits:
                raise _lib.AzpError("PressureProfile.%s: %d pairs were evaluated, the integer scale chosen from max_term = %r "
                                    "holds fewer than 2^%d; lower max_term" % (what, int(r[-4]), self._max_term, pair_bits))

    def _read(self, name):
        return self._read_row(name).cpu().numpy()

    @property
    def row(self):
        """numpy int64 (6 num_bins + 4,): the raw integer row (bins x {xx, xy, xz, yy, yz, zz} in units of 2^-shift, then
        pairs evaluated, terms added, terms refused, shift)."""
        return self._split(self._read("row"))[0][0].copy()

    def _get(self, name, interfaces=2):
        host = self._read(name)
        box = self._sim.state.box
        ints, kin = self._split(host)
        if name not in ("num_pairs", "num_terms", "overflow"):
            self._check_rows(ints, [self._sim.state.N], name)
        q = pressure_profile_quantities(ints[0], kin[0], self._bin_volumes(box), self._axis, self._bin_width(box), self._streaming,
                                        interfaces)
        v = q[name]
        return int(v) if name in ("num_pairs", "num_terms", "overflow") else v

    def surface_tension(self, interfaces=2):
        """float: (1 / ``interfaces``) sum_k (P_N - P_T)_k delta; a slab of liquid in a periodic box has two interfaces."""
        return float(self._get("surface_tension", interfaces))


def _pressure_profile_property(name):
    return property(lambda self: self._get(name), doc="``%s`` at the current state (``pressure_profile_quantities``)." % name)


for _name in PRESSURE_PROFILE_PROPERTIES:
    setattr(PressureProfile, _name, _pressure_profile_property(_name))


class PressureProfileRecorder(_Recorder):
    """Writer (``sim.operations.writers``) that appends the raw row of ``profile`` (a ``PressureProfile`` in ``computes``
    of the same simulation: the integer row and the kinetic field's row) to a device table at the timesteps ``trigger``
    fires, as ``ThermodynamicFieldRecorder`` does: the kernels write row k of the table, nothing is read back, and the
    trajectory is the same bit for bit with and without it. ``rows`` are the integer rows, ``table`` the dict of
    ``pressure_profile_quantities`` with a leading axis of recorded timesteps, every row with the bin volumes of the box
    it was recorded in; ``mean()`` the same quantities from the rows SUMMED and normalised with the summed volumes."""

    _dtype = "int64"

    def __init__(self, profile, trigger):
        if not isinstance(profile, PressureProfile):
            raise _lib.AzpError("PressureProfileRecorder: profile must be a PressureProfile, got %r" % (profile,))
        self.profile = self._compute = profile
        super().__init__(trigger)

    def reset(self):
        super().reset()
        self._bin_volumes = []  # per row, host data: the bin volumes, the bin width and N when it was recorded
        self._bin_widths = []
        self._n = []

    def _record(self, sim, timestep):
        k = len(self._steps)
        width = self._row_width()
        need = ThermodynamicFieldRecorder._grown_bytes(k, self._rows.shape[0] if self._rows is not None and self._rows.shape[1] == width
                                                       else 0, width)
        if need > RECORDER_MAX_BYTES:
            raise _lib.AzpError("%s: recording row %d of %d words would grow the table to %d bytes, more than 2^30; record "
                                "fewer bins or reset() more often" % (type(self).__name__, k, width, need))
        super()._record(sim, timestep)
        box = sim.state.box
        self._bin_volumes.append(self.profile._bin_volumes(box))
        self._bin_widths.append(self.profile._bin_width(box))
        self._n.append(sim.state.N)

    def _host(self, name):
        k = len(self._steps)
        if not self.profile._attached:
            raise DataAccessError(name)
        ints, kin = self.profile._split(self._rows[:k].cpu().numpy())
        return ints, kin

    @property
    def rows(self):
        """numpy int64 (rows, 6 num_bins + 4): the raw integer rows."""
        if len(self._steps) == 0:
            return np.zeros((0, 6 * self.profile.num_bins + 4), dtype=np.int64)
        return self._host("rows")[0].copy()

    def table(self, interfaces=2):
        """dict of numpy arrays, one leading entry per recorded timestep."""
        if len(self._steps) == 0:
            return {}
        ints, kin = self._host("table")
        p = self.profile
        p._check_rows(ints, self._n, "table")
        return pressure_profile_quantities(ints, kin, np.array(self._bin_volumes), p._axis, np.array(self._bin_widths), p.streaming,
                                           interfaces)

    def mean(self, interfaces=2):
        """dict of the same quantities from the sum of the recorded rows and the sum of their bin volumes (the bin width
        is the mean of the recorded widths)."""
        if len(self._steps) == 0:
            return {}
        ints, kin = self._host("mean")
        p = self.profile
        p._check_rows(ints, self._n, "mean")
        if np.any(ints[:, -1] != ints[0, -1]):
            raise _lib.AzpError("PressureProfileRecorder.mean: the rows were recorded with different integer scales (the number "
                                "of particles changed); use table()")
        return pressure_profile_quantities(ints.sum(axis=0), kin.sum(axis=0), np.array(self._bin_volumes).sum(axis=0), p._axis,
                                           np.mean(self._bin_widths), p.streaming, interfaces, shift=int(ints[0, -1]))


__all__ = ["PressureProfile", "PressureProfileRecorder", "pressure_profile_quantities", "pressure_profile_shift",
           "MeanSquaredDisplacement", "MeanSquaredDisplacementRecorder", "SelfIntermediateScattering",
           "SelfIntermediateScatteringRecorder", "average_over_origins", "displacement_moments",
           "intermediate_scattering_from_amplitudes", "self_scattering_from_row", "van_hove_from_counts",
           "BondedDistribution", "BondedDistributionRecorder", "CartesianVelocityFieldCompute", "Cluster", "ClusterProperties",
           "ClusterPropertiesRecorder", "ClusterRecorder", "cluster_properties_table",
           "CylindricalVelocityFieldCompute", "DataAccessError", "RDFRecorder", "cluster_indices", "cluster_summary", "distribution_from_counts",
           "RadialDistributionFunction", "SolidLiquid", "SolidLiquidRecorder", "Steinhardt", "SteinhardtRecorder",
           "StructureFactor", "StructureFactorRecorder", "ThermodynamicQuantities",
           "ThermodynamicRecorder", "VelocityCompute", "VelocityFieldCompute", "perpendicular_widths", "rdf_from_counts",
           "reciprocal_vectors", "spherical_average", "steinhardt_norms", "steinhardt_summary", "steinhardt_words",
           "structure_factor_from_amplitudes", "structure_factor_vectors", "thermo_quantities"]
