"""``hoomd.azplugins.update``: ``TypeUpdater`` flips particles between two types by a slab in z
(src/TypeUpdater.{h,cc}, HOOMD-2-era code restated for the v5-style interface). The pass over the particles runs in
libazp (csrc/type_update.hip); ``Simulation.run`` calls the updaters of ``sim.operations.updaters`` ahead of the
integrator's step, as HOOMD does, and has every neighbor list rebuilt before the next force evaluation."""

import ctypes as C
import math

from . import _lib
from .simulation import Periodic


class _Updater:
    """Base of what ``sim.operations.updaters`` holds: a ``trigger`` and ``_update(sim, timestep)``."""

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
