"""``hoomd.azplugins.update``: ``TypeUpdater`` flips particles between two types by a slab in z
(src/TypeUpdater.{h,cc}, HOOMD-2-era code restated for the v5-style interface). The pass over the particles runs in
libazp (csrc/type_update.hip); ``Simulation.run`` calls the updaters of ``sim.operations.updaters`` ahead of the
integrator's step, as HOOMD does, and has every neighbor list rebuilt before the next force evaluation.

``BoxResize`` is ``hoomd.update.BoxResize`` (the reference has no box-resize code): the box follows a ``variant.box``
object, the particles are rescaled and wrapped in libazp (csrc/box_resize.hip), and ``State.box_generation`` tells the
neighbor lists, the steppers and the recorders."""

import ctypes as C
import math

from . import _lib
from .filter import All, Type
from .trigger import Periodic


class _Updater:
    """Base of what ``sim.operations.updaters`` holds: a ``trigger`` and ``_update(sim, timestep)``.
    ``_changes_types``: the updater may rewrite types in pos.w, so ``Simulation.run`` bumps ``State.type_generation``
    behind it (every neighbor list and tile plan is rebuilt) and a stepper that reads types does not fuse across it."""

    _changes_types = True

    def __init__(self, trigger):
        self.trigger = trigger

    @property
    def trigger(self):
        return self._trigger

    @trigger.setter
    def trigger(self, trigger):
        self._trigger = trigger if isinstance(trigger, Periodic) else Periodic(trigger)

    def _update(self, sim, timestep):
        raise NotImplementedError


class TypeUpdater(_Updater):
    """Particles of ``inside_type`` or ``outside_type`` get ``inside_type`` while ``lo <= z <= hi`` and
    ``outside_type`` elsewhere (a particle on a face is inside, src/TypeUpdater.cc:107); other types are left alone.
    ``trigger``: an ``int`` period or a ``Periodic``. The types are type names. In a decomposed run every rank
    updates its own particles."""

    _name = "TypeUpdater"
    _inside_word, _outside_word = "inside_type", "outside_type"

    def __init__(self, trigger, inside_type, outside_type, lo, hi):
        super().__init__(trigger)
        self._inside_type, self._outside_type = inside_type, outside_type
        self._lo, self._hi = float(lo), float(hi)
        self._checked = None

    def _set(self, name, value):
        setattr(self, name, value)
        self._checked = None  # (validated again at the next update)

    inside_type = property(lambda self: self._inside_type, lambda self, t: self._set("_inside_type", t))
    outside_type = property(lambda self: self._outside_type, lambda self, t: self._set("_outside_type", t))
    lo = property(lambda self: self._lo, lambda self, z: self._set("_lo", float(z)))
    hi = property(lambda self: self._hi, lambda self, z: self._set("_hi", float(z)))

    def _validate(self, state):
        """src/TypeUpdater.cc:133-190 (checkTypes, checkRegion): at the first update, and again after a setter or
        when the types or the box of the state changed. Returns the two type indices."""
        key = (tuple(state.types), state.box.Lz)
        if self._checked is not None and self._checked[0] == key:
            return self._checked[1]
        for word, t in ((self._inside_word, self._inside_type), (self._outside_word, self._outside_type)):
            if t not in state.types:
                raise _lib.AzpError("%s: %s %r is not a particle type of the state (types %s)"
                                    % (self._name, word, t, list(state.types)))
        if self._inside_type == self._outside_type:
            raise _lib.AzpError("%s: %s and %s (%r) cannot match" % (self._name, self._inside_word, self._outside_word,
                                                                     self._inside_type))
        if not (math.isfinite(self._lo) and math.isfinite(self._hi)) or self._lo >= self._hi:
            raise _lib.AzpError("%s: lower z bound %r >= upper z bound %r" % (self._name, self._lo, self._hi))
        half = 0.5 * state.box.Lz
        if self._lo < -half:
            raise _lib.AzpError("%s: lower z bound %r lies outside the simulation box (%r)" % (self._name, self._lo, -half))
        if self._hi > half:
            raise _lib.AzpError("%s: upper z bound %r lies outside the simulation box (%r)" % (self._name, self._hi, half))
        ids = (state.types.index(self._inside_type), state.types.index(self._outside_type))
        self._checked = (key, ids)
        return ids

    def _update(self, sim, timestep):
        st = sim.state
        inside, outside = self._validate(st)
        a = _lib.TypeUpdateArgs()
        a.d_pos = st.pos.data_ptr()
        a.N = st.N
        a.inside_type, a.outside_type = inside, outside
        a.z_lo, a.z_hi = self._lo, self._hi
        _lib.check(_lib.lib().azp_type_update_region(C.byref(a), _lib.raw_stream(st.device)), "azp_type_update_region")


def box_resize_matrix(old, new):
    """M = H_new H_old^-1 for two ``state.Box`` (H: the lattice vectors as columns, upper triangular), as the six
    float64 ``(M00, M01, M02, M11, M12, M22)`` that ``azp_box_resize`` takes: r' = M r keeps the fractional coordinates
    of r. Written out from the closed form of the inverse of an upper-triangular H, so that an axis that does not
    change has its 1 and its 0s exactly."""
    sx, sy, sz = new.Lx / old.Lx, new.Ly / old.Ly, new.Lz / old.Lz
    return (sx, new.xy * sy - old.xy * sx, (old.xy * old.yz - old.xz) * sx - old.yz * (new.xy * sy) + new.xz * sz,
            sy, new.yz * sz - old.yz * sy,
            sz)


class BoxResize(_Updater):
    """``hoomd.update.BoxResize``: at the timesteps ``trigger`` fires the box becomes ``box(timestep)`` (``box``: a
    ``variant.box`` object -- ``Constant``, ``Interpolate``, ``InverseVolumeRamp`` -- or any callable of the timestep that
    returns a ``state.Box``), and the particles of ``filter`` (``All()``, default, or ``Type(...)``) are mapped affinely
    from the old box to the new one: their fractional coordinates stay. The other particles keep their positions. Every
    particle is then wrapped into the new box, its image counters following (one launch of ``azp_box_resize``,
    csrc/box_resize.hip). Velocities are not scaled (HOOMD does not scale them either).

    Where the box at a timestep equals the state's box nothing happens: no launch, no generation bump, no neighbor-list
    rebuild. Otherwise ``State.box_generation`` moves, so every neighbor list is rebuilt at the next force evaluation
    and the steppers wrap with the new box. A box too narrow for the list radius is refused there, by the cell grid of
    that rebuild -- the particles have already been scaled by then.

    ``BoxResize.update(state, box, filter=All())`` does the same once, between runs, with ``box`` a ``state.Box``.

    Refused: a decomposed run (the domain's slabs are cut once), periodic flags that differ from the state's, an edge
    that is not positive and finite, a ``Type`` filter naming a type the state lacks. Out of scope: flipping a sheared
    box, 2-D boxes, scaling velocities."""

    _name = "BoxResize"
    _changes_types = False

    def __init__(self, trigger, box, filter=None):
        super().__init__(trigger)
        if not callable(box):
            raise _lib.AzpError("BoxResize: box must be a variant.box object (a callable of the timestep that returns a Box), "
                                "got %r; for one resize between runs call BoxResize.update(state, box)" % (box,))
        self.box = box
        self.filter = _check_filter(filter)
        self._mask = None

    def _update(self, sim, timestep):
        if sim.domain is not None:
            raise _lib.AzpError("BoxResize does not run decomposed: the domain's slabs are cut once, for the box of that moment")
        st = sim.state
        key = (tuple(st.types), self.filter, str(st.device))
        if self._mask is None or self._mask[0] != key:
            self._mask = (key, _device_mask(st, self.filter))
        _resize(st, self.box(timestep), self._mask[1])

    @staticmethod
    def update(state, box, filter=None):
        """Resize ``state`` to ``box`` (a ``state.Box``) once, as one update of a ``BoxResize`` would."""
        if state.n_ghost:
            raise _lib.AzpError("BoxResize.update: the state belongs to a decomposed run (it has ghost rows): the domain's "
                                "slabs are cut once, for the box of that moment")
        _resize(state, box, _device_mask(state, _check_filter(filter)))


def _check_filter(filter):
    if filter is None:
        return All()
    if not isinstance(filter, (All, Type)):
        raise _lib.AzpError("BoxResize: filter must be All() or Type(...), got %r" % (filter,))
    return filter


def _device_mask(st, filter):
    """The filter's byte per type on the state's device; None for ``All()``. (``Type.mask`` refuses a type the state lacks.)"""
    import torch

    if isinstance(filter, All):
        return None
    return torch.from_numpy(filter.mask(st.types)).to(st.device)


def _resize(st, box, mask):
    from .state import Box

    old, new = st.box, Box.from_box(box)
    if new.periodic != old.periodic:
        raise _lib.AzpError("BoxResize: the periodic flags %r of the new box differ from the state's %r: a resize cannot "
                            "change them" % (new.periodic, old.periodic))
    for name in ("Lx", "Ly", "Lz"):
        if not (math.isfinite(getattr(new, name)) and getattr(new, name) > 0.0):
            raise _lib.AzpError("BoxResize: edge %s = %r of the new box is not positive and finite (%r)" % (name, getattr(new, name), new))
        if not getattr(old, name) > 0.0:
            raise _lib.AzpError("BoxResize: edge %s = %r of the state's box is not positive: 2-D boxes are not supported"
                                % (name, getattr(old, name)))
    for name in ("xy", "xz", "yz"):
        if not math.isfinite(getattr(new, name)):
            raise _lib.AzpError("BoxResize: tilt factor %s = %r of the new box is not finite" % (name, getattr(new, name)))
    if new == old:
        return
    a = _lib.BoxResizeArgs()
    a.d_pos = st.pos.data_ptr()
    a.d_image = st.image.data_ptr()
    a.d_type_mask = mask.data_ptr() if mask is not None else None
    a.N = st.N
    a.ntypes = len(st.types)
    a.M[:] = box_resize_matrix(old, new)
    a.box = new.to_c()
    _lib.check(_lib.lib().azp_box_resize(C.byref(a), _lib.raw_stream(st.device)), "azp_box_resize")
    st.set_box(new)
