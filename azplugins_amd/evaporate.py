"""``hoomd.azplugins.evaporate``: ``ParticleEvaporator`` turns up to ``Nmax`` randomly chosen solvent particles inside
a slab in z into a non-interacting "evaporated" type every time its trigger fires (src/ParticleEvaporator.{h,cc},
HOOMD-2-era code restated for the v5-style interface). The work runs in libazp (csrc/type_update.hip).

Which particles are picked: every candidate gets a 64-bit key from a counter-based random stream of its tag, the
timestep and the seed, and the ``min(Nmax, M)`` candidates with the smallest keys go (include/azp.h). The reference
shuffles candidate *indices* on the host instead; the rule here gives every subset the same probability as well,
and does not depend on how the particles are indexed or decomposed."""

import ctypes as C

import numpy as np

from . import _lib
from .update import TypeUpdater


class ParticleEvaporator(TypeUpdater):
    """``trigger``: an ``int`` period or a ``Periodic``. ``solvent_type`` / ``evaporated_type``: type names.
    ``lo`` / ``hi``: the slab (faces included). ``Nmax``: the most particles evaporated per update, ``None`` for no
    limit. The random stream takes the low 16 bits of ``Simulation.seed``.

    ``n_candidates`` / ``n_evaporated`` describe the last update; reading them waits for the device. In a decomposed
    run they count over all ranks when ``Nmax`` is set, and over this rank's particles when it is ``None`` (no
    collective runs then)."""

    _name = "ParticleEvaporator"
    # (the reference's evaporator is its TypeUpdater with outside = solvent and inside = evaporated,
    # src/ParticleEvaporator.cc:190, :216)
    _inside_word, _outside_word = "evaporated_type", "solvent_type"

    def __init__(self, trigger, solvent_type, evaporated_type, lo, hi, Nmax=None):
        super().__init__(trigger, inside_type=evaporated_type, outside_type=solvent_type, lo=lo, hi=hi)
        self.Nmax = Nmax
        self._scratch = None
        self._counts = None       # device tensor [M, picked] of the last update, or the host pair once known
        self._out = None          # decomposed runs: [n_keys, M, 0] and the message of keys

    solvent_type = TypeUpdater.outside_type
    evaporated_type = TypeUpdater.inside_type

    @property
    def Nmax(self):
        return self._Nmax

    @Nmax.setter
    def Nmax(self, Nmax):
        if Nmax is not None:
            if int(Nmax) != Nmax or not 0 <= int(Nmax) < _lib.EVAPORATE_NO_LIMIT:
                raise _lib.AzpError("ParticleEvaporator: Nmax must be None or an integer in [0, 2^32 - 1), got %r" % (Nmax,))
            Nmax = int(Nmax)
        self._Nmax = Nmax

    def _host_counts(self):
        if self._counts is None:
            raise _lib.AzpError("ParticleEvaporator: no update has run yet")
        if not isinstance(self._counts, tuple):
            m, k = self._counts.cpu().numpy().view(np.uint32).tolist()  # (the one host wait of an evaporator)
            self._counts = (int(m), int(k))
        return self._counts

    @property
    def n_candidates(self):
        """Solvent particles inside the slab at the last update."""
        return self._host_counts()[0]

    @property
    def n_evaporated(self):
        """Particles the last update turned into the evaporated type."""
        return self._host_counts()[1]

    def _args(self, sim, timestep):
        import torch

        st = sim.state
        evaporated, solvent = self._validate(st)
        sim._warn_if_seed_unset()
        a = _lib.EvaporateArgs()
        a.d_pos = st.pos.data_ptr()
        a.d_tag = st.tag.data_ptr()
        a.N = st.N
        a.solvent_type, a.evaporated_type = solvent, evaporated
        a.Nmax = _lib.EVAPORATE_NO_LIMIT if self._Nmax is None else self._Nmax
        a.z_lo, a.z_hi = self._lo, self._hi
        a.timestep = int(timestep)
        a.seed = int(sim.seed) & 0xFFFF
        if self._Nmax is not None:
            need = int(_lib.lib().azp_evaporate_scratch_size(st.N))
            if self._scratch is None or self._scratch.numel() < need or self._scratch.device != st.device:
                self._scratch = torch.empty(need, dtype=torch.uint8, device=st.device)
            a.d_scratch, a.scratch_bytes = self._scratch.data_ptr(), self._scratch.numel()
        # (a fresh pair of words per update: the previous pair may not have been read yet)
        self._counts = torch.empty(2, dtype=torch.int32, device=st.device)
        a.d_counts = self._counts.data_ptr()
        return a

    def _update(self, sim, timestep):
        a = self._args(sim, timestep)
        stream = _lib.raw_stream(sim.state.device)
        if sim.domain is None or self._Nmax is None:
            _lib.check(_lib.lib().azp_evaporate(C.byref(a), stream), "azp_evaporate")
            return
        self._update_decomposed(sim, a, stream)

    def _update_decomposed(self, sim, a, stream):
        """Every rank offers its ``Nmax`` smallest keys; the ``Nmax``-th smallest of all of them is the threshold."""
        import torch

        st, cap = sim.state, self._Nmax
        if self._out is None or self._out[1].numel() != cap + 2 or self._out[1].device != st.device:
            self._out = (torch.zeros(3, dtype=torch.int32, device=st.device),
                         torch.zeros(cap + 2, dtype=torch.int64, device=st.device))
        head, msg = self._out
        a.d_n_keys_out, a.d_counts = head.data_ptr(), head.data_ptr() + 4
        a.d_keys_out = msg.data_ptr() + 16
        _lib.check(_lib.lib().azp_evaporate_local_keys(C.byref(a), stream), "azp_evaporate_local_keys")
        msg[:2] = head[:2]  # [number of keys, local candidates]
        rows = sim.domain.all_gather_rows(msg).cpu().numpy()
        keys = np.concatenate([r[2:2 + int(r[0])] for r in rows]).view(np.uint64)
        total = int(rows[:, 1].sum())
        threshold = int(np.partition(keys, cap - 1)[cap - 1]) if (cap and keys.size >= cap) else 0xFFFFFFFFFFFFFFFF
        a.d_counts = None
        if cap:
            _lib.check(_lib.lib().azp_evaporate_apply_below(C.byref(a), threshold, stream), "azp_evaporate_apply_below")
        self._counts = (total, min(cap, total))
