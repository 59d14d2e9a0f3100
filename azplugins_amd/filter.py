"""Particle filters under the names of ``hoomd.filter``: ``All`` and ``Type``."""

import numpy as np

from . import _lib


class All:
    """``hoomd.filter.All``: every particle. The only filter the NVE kernels implement."""

    def __eq__(self, other):
        return isinstance(other, All)

    def __hash__(self):
        return hash("All")


class Type:
    """``hoomd.filter.Type``: the particles of the named types. ``types`` is one type name or an iterable of type
    names. Computes and the flow methods (``flow.Langevin``, ``flow.Brownian``) accept it; ``ConstantVolume``
    integrates all particles (``All`` only)."""

    def __init__(self, types):
        if isinstance(types, str):
            types = [types]
        self.types = tuple(types)
        if not all(isinstance(t, str) for t in self.types):
            raise _lib.AzpError("Type: type names must be strings, got %r" % (types,))

    def mask(self, type_names):
        """One byte per type of ``type_names`` (the state's types): 1 if the type is selected."""
        missing = [t for t in self.types if t not in type_names]
        if missing:
            raise _lib.AzpError("Type filter names %s, which the state does not have (types %s)" % (missing, list(type_names)))
        return np.array([1 if t in self.types else 0 for t in type_names], dtype=np.uint8)

    def __eq__(self, other):
        return isinstance(other, Type) and set(self.types) == set(other.types)

    def __hash__(self):
        return hash(("Type", frozenset(self.types)))

    def __repr__(self):
        return "Type(%r)" % (list(self.types),)
