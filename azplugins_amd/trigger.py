"""Triggers under the names of ``hoomd.trigger``: ``Periodic``."""

from . import _lib


class Periodic:
    """``hoomd.trigger.Periodic``: fires at the timesteps t with ``(t - phase) % period == 0``."""

    def __init__(self, period, phase=0):
        if isinstance(period, bool) or int(period) != period or int(period) < 1:
            raise _lib.AzpError("Periodic: period must be a positive integer, got %r" % (period,))
        if isinstance(phase, bool) or int(phase) != phase:
            raise _lib.AzpError("Periodic: phase must be an integer, got %r" % (phase,))
        self.period, self.phase = int(period), int(phase)

    def __call__(self, timestep):
        return (int(timestep) - self.phase) % self.period == 0

    def __eq__(self, other):
        return isinstance(other, Periodic) and (other.period, other.phase) == (self.period, self.phase)

    def __hash__(self):
        return hash(("Periodic", self.period, self.phase))

    def __repr__(self):
        return "Periodic(period=%d, phase=%d)" % (self.period, self.phase)
