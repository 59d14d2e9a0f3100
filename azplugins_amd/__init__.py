"""azplugins_amd -- MI355X-native force-compute hot path of azplugins.

``pair`` / ``bond`` / ``external`` / ``compute`` / ``flow`` / ``update`` / ``evaporate`` / ``variant`` mirror ``hoomd.azplugins.pair`` /
``.bond`` / ``.external`` / ``.compute`` / ``.flow`` / ``.update`` / ``.evaporate`` / ``.variant`` (class names, parameters, modes); ``wall``
holds the reference's legacy wall potentials (LJ 9-3, colloid) with geometries defined by this project; ``angle`` holds harmonic,
cosine-squared and tabulated bending with HOOMD's ``md.angle`` conventions and ``dihedral`` periodic, OPLS and tabulated torsions under ``md.dihedral``'s
names and ``special_pair`` the Lennard-Jones special pair under ``md.special_pair``'s (the reference has no angle, dihedral or special-pair code); ``update.BoxResize`` with the box variants of ``variant.box`` and the scalar
variants of ``variant`` follows ``hoomd.update.BoxResize`` / ``hoomd.variant`` (the reference has no box-resize code either); ``thermostats`` holds the Berendsen, Bussi and MTTK thermostats of ``ConstantVolume``
under ``hoomd.md.methods.thermostats``' names, ``ConstantPressure`` a Martyna-Tobias-Klein barostat under ``hoomd.md.methods.ConstantPressure``'s, ``Langevin`` / ``Brownian`` (``methods``) Langevin and Brownian dynamics with rotation under ``hoomd.md.methods``' names and ``minimize`` the FIRE energy minimizer under ``hoomd.md.minimize``'s. The compute path is libazp.so (hand-written
HIP for gfx950, C ABI in ``include/azp.h``); there is no CPU fallback. ``compute.BondedDistribution`` (this project's) is the distribution of the bond lengths,
bending angles or dihedral angles per group type that the tabulated bonded potentials are inverted from.
"""

from . import _lib, angle, bond, compute, dihedral, evaporate, external, flow, methods, minimize, nlist, pair, sorter, special_pair, synthetic, thermostats, tune, update, variant, wall
from ._lib import AzpError
from .simulation import All, Brownian, ConstantPressure, ConstantVolume, Integrator, Langevin, Periodic, Simulation, Type
from .sorter import ParticleSorter
from .state import (Box, Snapshot, State, bonded_two_particle_snapshot, lattice_snapshot, two_particle_snapshot)

__version__ = "0.1.0"

__all__ = ["All", "AzpError", "Box", "Brownian", "ParticleSorter", "ConstantPressure", "ConstantVolume", "Integrator", "Langevin", "Periodic", "Simulation", "Snapshot", "State", "Type", "angle", "bond", "compute", "dihedral",
           "evaporate", "external", "flow", "methods", "minimize", "nlist", "pair", "special_pair", "synthetic", "thermostats", "tune", "update", "variant", "wall", "two_particle_snapshot", "bonded_two_particle_snapshot",
           "lattice_snapshot"]
