"""Computes: mirror of ``hoomd.azplugins.compute`` (reference ``src/compute.py``) on libazp's velocity-field
kernels (``csrc/velocity_field.hip``).

``VelocityCompute`` is the mass-weighted center-of-mass velocity of a group; ``CartesianVelocityFieldCompute`` and
``CylindricalVelocityFieldCompute`` the mass-averaged velocity in each bin of a 1-, 2- or 3-D grid. A compute is
attached while it is in ``sim.operations.computes`` of a simulation that has a state; its result is computed when
the property is read, on the current state. On a decomposed run (``sim.domain`` set) every rank sums its own rows,
the sums are added over the domain's process group and every rank gets the same result.
"""

import ctypes as C
import itertools

import numpy as np

from . import _lib
from .simulation import All, Type


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
    """What the two compute classes share: attachment through ``sim.operations`` and the device buffers."""

    _coordinates = _lib.COORDINATES_CARTESIAN

    def __init__(self, filter, include_mpcd_particles):
        self._filter = _check_filter(filter)
        self._include_mpcd_particles = _check_mpcd(include_mpcd_particles)
        self._sim = None
        self._bufs = None  # key -> (sums, velocity, scratch)
        self._mask = None  # (types, device tensor or None)

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


__all__ = ["CartesianVelocityFieldCompute", "CylindricalVelocityFieldCompute", "DataAccessError", "VelocityCompute",
           "VelocityFieldCompute"]
