"""Host snapshot and device state: the minimal stand-in for the HOOMD-blue
objects the reference's force classes are attached to (``hoomd.Snapshot``,
``hoomd.State`` / ``ParticleData``). Device memory is held in torch tensors
(plumbing only); the layouts are HOOMD's:

* ``pos``   (n_max, 4) float64: x, y, z, type index in the low 32 bits of w
* ``vel``   (n_max, 4) float64: vx, vy, vz, mass
* ``orientation`` (n_max, 4) float64 quaternion, scalar part first
* ``tag``   (n_max,) uint32 (stored as int32 bit pattern)
* ``angmom`` (n_max, 4) float64 angular-momentum quaternion, ``inertia`` (n_max, 3) principal moments
* ``accel`` (n_max, 4) float64 ax, ay, az, 0: ``None`` until a ``flow.Langevin`` or ``methods.Langevin`` run creates it
* ``langevin_torque`` (n_max, 4) float64 body-frame bx, by, bz, 0: ``None`` until a ``methods.Langevin`` run with rotation creates it
"""

import math

import numpy as np

from . import _lib
from .synthetic import pos4 as _pos4


class Box:
    """Triclinic periodic box centred on the origin (HOOMD ``BoxDim``)."""

    def __init__(self, Lx, Ly=None, Lz=None, xy=0.0, xz=0.0, yz=0.0, periodic=(True, True, True)):
        self.Lx = float(Lx)
        self.Ly = float(Lx if Ly is None else Ly)
        self.Lz = float(Lx if Lz is None else Lz)
        self.xy, self.xz, self.yz = float(xy), float(xz), float(yz)
        self.periodic = tuple(bool(p) for p in periodic)

    @classmethod
    def cube(cls, L):
        return cls(L, L, L)

    @classmethod
    def from_box(cls, box):
        if isinstance(box, Box):
            return box
        box = list(box)
        if len(box) == 3:
            return cls(*box)
        return cls(*box[:6])

    @property
    def L(self):
        return np.array([self.Lx, self.Ly, self.Lz])

    @property
    def is_triclinic(self):
        return self.xy != 0.0 or self.xz != 0.0 or self.yz != 0.0

    @property
    def nearest_plane_distance(self):
        """Distances between opposite faces of the box (HOOMD ``BoxDim.getNearestPlaneDistance``): the widths of the
        box perpendicular to its yz, xz and xy faces."""
        t = self.xy * self.yz - self.xz
        return (self.Lx / math.sqrt(1.0 + self.xy * self.xy + t * t), self.Ly / math.sqrt(1.0 + self.yz * self.yz), self.Lz)

    @property
    def volume(self):
        return self.Lx * self.Ly * self.Lz

    def _key(self):
        return (self.Lx, self.Ly, self.Lz, self.xy, self.xz, self.yz, self.periodic)

    def __eq__(self, other):
        """Equal in all six numbers and the periodic flags."""
        return isinstance(other, Box) and other._key() == self._key()

    def __ne__(self, other):
        return not self == other

    __hash__ = object.__hash__  # (a box is mutable: hashed by identity, as before it had an __eq__)

    def to_c(self):
        key = self._key()
        if getattr(self, "_c_key", None) != key:  # (called for every launch: build the struct once per box)
            self._c = _lib.make_box(key[:3], key[3:6], [int(p) for p in self.periodic])
            self._c_key = key
        return self._c

    def __repr__(self):
        return "Box(Lx=%g, Ly=%g, Lz=%g, xy=%g, xz=%g, yz=%g)" % (self.Lx, self.Ly, self.Lz, self.xy, self.xz, self.yz)


class _Particles:
    def __init__(self):
        self._N = 0
        self.types = ["A"]
        self._alloc(0)

    def _alloc(self, n):
        self.position = np.zeros((n, 3))
        self.typeid = np.zeros(n, dtype=np.uint32)
        self.orientation = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (n, 1))
        self.velocity = np.zeros((n, 3))
        self.mass = np.ones(n)
        self.moment_inertia = np.zeros((n, 3))
        self.angmom = np.zeros((n, 4))
        self.tag = np.arange(n, dtype=np.uint32)

    @property
    def N(self):
        return self._N

    @N.setter
    def N(self, n):
        self._N = int(n)
        self._alloc(self._N)


# The group kinds and the number of members of one group of each. "pair" is HOOMD's special pair (``Snapshot.pairs``):
# two particles that carry an interaction of their own (``special_pair``), e.g. the scaled 1-4 pairs of an OPLS chain.
ARITY = dict(bond=2, angle=3, dihedral=4, pair=2)
KINDS = tuple(ARITY)


class _Groups:
    """The bonds, angles, dihedrals or special pairs of a snapshot: ``N`` groups of ``arity`` members each."""

    def __init__(self, arity):
        self._arity = arity
        self.types = []
        self.N = 0

    @property
    def N(self):
        return self._N

    @N.setter
    def N(self, n):
        self._N = int(n)
        self.group = np.zeros((self._N, self._arity), dtype=np.uint32)
        self.typeid = np.zeros(self._N, dtype=np.uint32)


class _Configuration:
    def __init__(self):
        self.box = Box(1.0)
        self.dimensions = 3


class Snapshot:
    """Host-side system description with ``hoomd.Snapshot``'s attribute names
    (``particles.N/position/typeid/types/orientation/velocity/mass``,
    ``bonds.N/group/typeid/types``, ``angles.N/group/typeid/types`` with members ``a, b, c`` and ``b`` the vertex,
    ``dihedrals.N/group/typeid/types`` with members ``a, b, c, d`` along the chain, ``pairs.N/group/typeid/types``: the
    special pairs, ``configuration.box``)."""

    def __init__(self):
        self.particles = _Particles()
        self.bonds = _Groups(2)
        self.angles = _Groups(3)
        self.dihedrals = _Groups(4)
        self.pairs = _Groups(2)
        self.configuration = _Configuration()

    @classmethod
    def from_arrays(cls, xyz, box, typeid=None, types=("A",), orientation=None, velocity=None, tag=None, bonds=None,
                    bond_typeid=None, bond_types=("A-A",), moment_inertia=None, angmom=None, angles=None, angle_typeid=None,
                    angle_types=("A-A-A",), dihedrals=None, dihedral_typeid=None, dihedral_types=("A-A-A-A",), pairs=None,
                    pair_typeid=None, pair_types=("A-A",)):
        s = cls()
        xyz = np.asarray(xyz, dtype=np.float64)
        s.particles.N = xyz.shape[0]
        s.particles.position[:] = xyz
        s.particles.types = list(types)
        if typeid is not None:
            s.particles.typeid[:] = typeid
        if orientation is not None:
            s.particles.orientation[:] = orientation
        if velocity is not None:
            s.particles.velocity[:] = velocity
        if tag is not None:
            s.particles.tag[:] = tag
        if moment_inertia is not None:
            s.particles.moment_inertia[:] = moment_inertia
        if angmom is not None:
            s.particles.angmom[:] = angmom
        s.configuration.box = Box.from_box(box)
        for kind, members, tid, names in (("bond", bonds, bond_typeid, bond_types), ("angle", angles, angle_typeid, angle_types),
                                          ("dihedral", dihedrals, dihedral_typeid, dihedral_types),
                                          ("pair", pairs, pair_typeid, pair_types)):
            if members is not None:
                g = getattr(s, kind + "s")
                members = np.asarray(members, dtype=np.uint32).reshape(-1, ARITY[kind])
                g.N = members.shape[0]
                g.group[:] = members
                g.types = list(names)
                if tid is not None:
                    g.typeid[:] = tid
        return s


def two_particle_snapshot(particle_types=("A",), d=1.0, L=20.0):
    """HOOMD conftest's ``two_particle_snapshot_factory`` restated: two particles
    at (-d/2, 0, 0) and (+d/2, 0, 0) in a cubic box (used by every 2-particle
    reference test, e.g. src/pytest/test_pair.py:319-321)."""
    s = Snapshot()
    s.particles.N = 2
    s.particles.types = list(particle_types)
    s.particles.position[:] = [[-d / 2.0, 0.0, 0.0], [d / 2.0, 0.0, 0.0]]
    s.configuration.box = Box.cube(L)
    return s


def bonded_two_particle_snapshot(bond_types=None, **kwargs):
    """src/conftest.py:10-24 restated: one bond [0, 1] of type "A-A"."""
    s = two_particle_snapshot(**kwargs)
    s.bonds.N = 1
    s.bonds.types = list(bond_types) if bond_types is not None else ["A-A"]
    s.bonds.group[0] = [0, 1]
    return s


def lattice_snapshot(particle_types=("A",), n=10, a=0.6):
    """HOOMD conftest's ``lattice_snapshot_factory`` restated: n^3 simple cubic,
    box n*a (src/pytest/test_pair_dpd.py:15)."""
    s = Snapshot()
    s.particles.N = n**3
    s.particles.types = list(particle_types)
    g = (np.arange(n) + 0.5) * a - 0.5 * n * a
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    s.particles.position[:] = np.stack([X.ravel(), Y.ravel(), Z.ravel()], axis=1)
    s.configuration.box = Box.cube(n * a)
    return s


# what a rank says when a group it must evaluate has a member that is neither local nor a ghost there
_MISSING_MEMBER = {
    2: "a bonded partner of a local particle is neither local nor a ghost on this rank: the ghost shell (r_cut + buffer) is "
       "narrower than a bond",
    3: "a member of an angle with a local particle is neither local nor a ghost on this rank: the ghost shell (r_cut + "
       "buffer) is narrower than two bond lengths",
    4: "a member of a dihedral with a local particle is neither local nor a ghost on this rank: the ghost shell (r_cut + "
       "buffer) is narrower than three bond lengths",
    "pair": "a member of a special pair with a local particle is neither local nor a ghost on this rank: the ghost shell "
            "(r_cut + buffer) is narrower than the pair (a 1-4 pair spans up to three bond lengths)",
}


def localize_groups(tag, n_local, tags, typeid, arity, kind=None):
    """The groups of a global topology (``tags``: rows of ``arity`` particle tags -- bonds, angles a, b, c with the vertex
    in the middle, dihedrals a, b, c, d) that one rank of a decomposed run evaluates, as index rows over its rows
    (``tag``: the tags of its local rows [0, n_local) followed by its ghost rows): every group with at least one LOCAL
    member. All its members must be on the rank, as locals or ghosts: the far end of a group is ``arity - 1`` bonds away
    from a local end (``kind``: names the kind in the error where the arity does not, "pair"). Returns (group uint32
    (n, arity), typeid)."""
    tag = np.asarray(tag, dtype=np.int64)
    tags = np.asarray(tags, dtype=np.int64).reshape(-1, arity)
    n_glob = int(max(tags.max() + 1 if tags.size else 0, tag.max() + 1 if tag.size else 0))
    rtag = np.full(n_glob + 1, -1, dtype=np.int64)
    # (a particle can sit on a rank more than once: as a local and as its own periodic ghost; the lowest row wins
    # -- local before ghost -- and the groups are evaluated with the minimum image)
    rtag[tag[::-1]] = np.arange(tag.size - 1, -1, -1)
    idx = rtag[tags]
    mine = np.any((idx >= 0) & (idx < n_local), axis=1)
    if np.any(mine & np.any(idx < 0, axis=1)):
        raise _lib.AzpError(_MISSING_MEMBER.get(kind, _MISSING_MEMBER[arity]))
    return idx[mine].astype(np.uint32).reshape(-1, arity), np.asarray(typeid, dtype=np.uint32)[mine]


def build_group_table(group, typeid, n_local, kind):
    """The per-particle table the bonded kernel walks, from the group members (``group``: integer tensor (n, arity),
    ``typeid``: integer tensor (n,); any device, CPU included). ``kind``: "bond", "angle", "dihedral" or "pair" (the
    arities 2, 3 and 4 still name the first three). Particle-major: entry ``s`` of local particle ``i`` is
    ``table[s, i]``, for ``s < counts[i]``; only members with index ``< n_local`` get entries (a ghost member gets its
    rows on its owner's rank), unused slots are zero. One stable sort fixes the entry order inside a particle, and with it
    the order of the kernel's sums: angles and dihedrals by group index; bonds, as HOOMD's ``BondData::getGPUTable``,
    those in which the particle is the first member before those in which it is the second, each by bond index.

    The words of an entry, the only thing that differs between the kinds:

    * bond and pair: (partner, type), and the particle's position in the bond in a plane of its own, ``bond_pos``
      (HOOMD's layout);
    * angle: (the two other members in angle order, type, position 0 / 1 / 2), 16 bytes;
    * dihedral: (the three other members in dihedral order, type in the low 30 bits | position 0 .. 3 in the top two).

    Returns ``table`` int32 (width, n_local, words), the counts int32 (n_local,) under ``n_bonds`` / ``n_angles`` /
    ``n_dihedrals`` / ``n_pairs``, ``pitch`` = n_local, ``width`` >= 1, and for bonds and pairs ``bond_pos`` int32
    (width, n_local)."""
    import torch

    if not isinstance(kind, str):
        kind = {2: "bond", 3: "angle", 4: "dihedral"}[int(kind)]
    arity = ARITY[kind]
    N = int(n_local)
    dev = group.device
    g = group.reshape(-1, arity).to(torch.int64)
    n = g.shape[0]
    # one candidate entry per (group, member), group-major -- member-major for bonds
    cols = list(range(arity))
    member = g.reshape(-1)
    others = torch.stack([g[:, cols[:k] + cols[k + 1:]] for k in cols], dim=1).reshape(-1, arity - 1)
    which = torch.arange(arity, dtype=torch.int64, device=dev).repeat(n)
    gtype = typeid.to(torch.int64).reshape(-1).repeat_interleave(arity)
    if arity == 2:
        major = torch.arange(2 * n, device=dev).reshape(n, 2).t().reshape(-1)
        member, others, which, gtype = member[major], others[major], which[major], gtype[major]
    keep = member < N
    member, others, which, gtype = member[keep], others[keep], which[keep], gtype[keep]
    counts = torch.bincount(member, minlength=N)[:N] if member.numel() else torch.zeros(N, dtype=torch.int64, device=dev)
    width = max(int(counts.max().item()) if (N and member.numel()) else 0, 1)
    if arity == 2:
        words = [others[:, 0], gtype]
    elif arity == 3:
        words = [others[:, 0], others[:, 1], gtype, which]
    else:
        word = gtype | (which << 30)
        words = [others[:, 0], others[:, 1], others[:, 2], torch.where(word >= 2 ** 31, word - 2 ** 32, word)]  # (the bits of a uint32)
    table = torch.zeros((width, N, len(words)), dtype=torch.int32, device=dev)
    out = {"table": table, "n_%ss" % kind: counts.to(torch.int32), "pitch": N, "width": width}
    if arity == 2:
        out["bond_pos"] = torch.zeros((width, N), dtype=torch.int32, device=dev)
    if member.numel():
        order = torch.sort(member, stable=True).indices
        m = member[order]
        start = torch.cumsum(counts, 0) - counts
        slot = torch.arange(m.numel(), device=dev) - start[m]
        table[slot, m] = torch.stack(words, dim=1)[order].to(torch.int32)
        if arity == 2:
            out["bond_pos"][slot, m] = which[order].to(torch.int32)
    return out


def localize_bonds(tag, n_local, bond_tags, bond_typeid):
    return localize_groups(tag, n_local, bond_tags, bond_typeid, 2)


def localize_angles(tag, n_local, angle_tags, angle_typeid):
    return localize_groups(tag, n_local, angle_tags, angle_typeid, 3)


def localize_dihedrals(tag, n_local, dihedral_tags, dihedral_typeid):
    return localize_groups(tag, n_local, dihedral_tags, dihedral_typeid, 4)


def build_angle_table(group, typeid, n_local):
    return build_group_table(group, typeid, n_local, 3)


def build_dihedral_table(group, typeid, n_local):
    return build_group_table(group, typeid, n_local, 4)


# Neighbor-list exclusions (HOOMD ``md.nlist`` ``exclusions``). What each name excludes:
#   "bond"          both members of every bond;
#   "angle"         the first and the last member of every angle;
#   "dihedral"      the first and the last member of every dihedral;
#   "special_pair"  both members of every special pair;
#   "1-3"           (a, c) for every walk a - b - c over bonds with a != c;
#   "1-4"           (a, d) for every walk a - b - c - d over bonds with a != c, b != d and a != d.
# Walks, not shortest paths: in a ring of four the 1-4 walks end on a bonded neighbor. The names of EXCLUSIONS_WITHOUT_EFFECT
# are HOOMD's for things this project does not have: accepted, they exclude nothing.
EXCLUSIONS = ("bond", "angle", "dihedral", "special_pair", "1-3", "1-4")
EXCLUSIONS_WITHOUT_EFFECT = ("body", "constraint", "meshbond")


def check_exclusions(names, who="exclusions"):
    """``names`` as a tuple of the names of ``EXCLUSIONS`` in that order, each once; ``AzpError`` for any name that is
    neither one of them nor one of ``EXCLUSIONS_WITHOUT_EFFECT``."""
    if isinstance(names, str):
        names = (names,)
    names = tuple(names)
    for n in names:
        if n not in EXCLUSIONS and n not in EXCLUSIONS_WITHOUT_EFFECT:
            raise _lib.AzpError("%s: unknown name %r (known: %s; accepted without effect: %s)"
                                % (who, n, ", ".join(EXCLUSIONS), ", ".join(EXCLUSIONS_WITHOUT_EFFECT)))
    return tuple(n for n in EXCLUSIONS if n in names)


def _bond_walks(bonds, n_ids):
    """Every walk a - b - c over ``bonds`` (int64 (n, 2)) with a != c as three tensors, with the lookup
    ``neighbors(x) -> (repeat, y)`` that made them: for every entry of ``x`` its bonded neighbors ``y``, entry ``k`` of
    ``x`` standing ``repeat``-ed in front of each of them."""
    import torch

    dev = bonds.device
    src = torch.cat([bonds[:, 0], bonds[:, 1]])
    dst = torch.cat([bonds[:, 1], bonds[:, 0]])
    order = torch.sort(src, stable=True).indices
    dst = dst[order]
    deg = torch.bincount(src, minlength=n_ids)
    start = torch.cumsum(deg, 0) - deg

    def neighbors(x):
        d = deg[x]
        rep = torch.repeat_interleave(torch.arange(x.numel(), device=dev), d)
        first = torch.cumsum(d, 0) - d
        within = torch.arange(rep.numel(), device=dev) - first[rep]
        return rep, dst[start[x][rep] + within]

    a, b = torch.cat([bonds[:, 0], bonds[:, 1]]), torch.cat([bonds[:, 1], bonds[:, 0]])
    rep, c = neighbors(b)
    a, b = a[rep], b[rep]
    keep = a != c
    return a[keep], b[keep], c[keep], neighbors


def excluded_pairs(kinds, members):
    """The ordered pairs (i, j) that the exclusion names ``kinds`` (``check_exclusions``' form) name, as an int64
    tensor (m, 2): symmetric ((j, i) is there with (i, j)), sorted by (i, j), free of duplicates and of pairs with
    i == j. ``members``: kind ("bond", "angle", "dihedral", "pair") -> integer tensor (n, arity) of non-negative
    particle ids (row indices or tags; any device, CPU included), a missing kind has no groups. torch only: two sorts
    and the joins of the bond walks, no loop over groups."""
    import torch

    have = {k: v.reshape(-1, ARITY[k]).to(torch.int64) for k, v in members.items() if v is not None and v.numel()}
    dev = next(iter(have.values())).device if have else "cpu"
    ends = []
    for name, kind in (("bond", "bond"), ("angle", "angle"), ("dihedral", "dihedral"), ("special_pair", "pair")):
        if name in kinds and kind in have:
            ends.append(have[kind][:, [0, ARITY[kind] - 1]])
    if ("1-3" in kinds or "1-4" in kinds) and "bond" in have:
        bonds = have["bond"]
        a, b, c, neighbors = _bond_walks(bonds, int(bonds.max().item()) + 1)
        if "1-3" in kinds:
            ends.append(torch.stack([a, c], dim=1))
        if "1-4" in kinds:
            rep, d = neighbors(c)
            a, b = a[rep], b[rep]
            keep = (b != d) & (a != d)
            ends.append(torch.stack([a[keep], d[keep]], dim=1))
    if not ends:
        return torch.zeros((0, 2), dtype=torch.int64, device=dev)
    p = torch.cat(ends)
    p = torch.cat([p, p.flip(1)])
    p = p[p[:, 0] != p[:, 1]]
    if not p.numel():
        return p
    base = int(p.max().item()) + 1
    key = torch.unique(p[:, 0] * base + p[:, 1])  # (sorted; ids are below 2^31, the key below 2^62)
    return torch.stack([key // base, key % base], dim=1)


def localize_pairs(pairs, tag, n_local):
    """Excluded pairs by particle TAG (``excluded_pairs`` of a global topology) as pairs of row indices on one rank of
    a decomposed run (``tag``: integer tensor, the tags of its local rows [0, n_local) and then of its ghost rows): the
    pairs whose first member is a local row and whose second member is on the rank at all. A pair whose partner is
    not on the rank is DROPPED, not an error: that partner is farther away than the ghost shell, which is at least the
    list radius wide. A particle that is on the rank twice (a local and its own periodic ghost) is its lowest row, as
    in ``localize_groups``. Sorted by (i, j)."""
    import torch

    tag = tag.reshape(-1).to(torch.int64)
    if not pairs.numel() or not tag.numel():
        return pairs[:0]
    n_ids = int(max(pairs.max().item(), tag.max().item())) + 1
    missing = tag.numel()
    row = torch.full((n_ids,), missing, dtype=torch.int64, device=tag.device)
    row.scatter_reduce_(0, tag, torch.arange(tag.numel(), dtype=torch.int64, device=tag.device), "amin")
    ij = row[pairs.to(tag.device)]
    ij = ij[(ij[:, 0] < int(n_local)) & (ij[:, 1] < missing)]
    if not ij.numel():
        return ij
    key = torch.unique(ij[:, 0] * (missing + 1) + ij[:, 1])
    return torch.stack([key // (missing + 1), key % (missing + 1)], dim=1)


def build_exclusion_table(pairs, n_local):
    """The table the neighbor-list kernels and the RDF read, from ordered pairs of row indices sorted by (i, j)
    (``excluded_pairs``, ``localize_pairs``): ``(n_excl int32 (n_local,), excl int32 (width, n_local), pitch)`` with
    entry ``s`` of row ``i`` at ``excl[s, i]`` for ``s < n_excl[i]``, ascending in ``s``; rows for the local particles
    only (a pair whose first member is a ghost row has no entry), unused slots zero, ``width`` >= 1, ``pitch`` = n_local."""
    import torch

    N = int(n_local)
    dev = pairs.device
    pairs = pairs[pairs[:, 0] < N]
    i, j = pairs[:, 0], pairs[:, 1]
    counts = torch.bincount(i, minlength=N)[:N] if i.numel() else torch.zeros(N, dtype=torch.int64, device=dev)
    width = max(int(counts.max().item()) if (N and i.numel()) else 0, 1)
    excl = torch.zeros((width, N), dtype=torch.int32, device=dev)
    if i.numel():
        start = torch.cumsum(counts, 0) - counts
        excl[torch.arange(i.numel(), device=dev) - start[i], i] = j.to(torch.int32)
    return counts.to(torch.int32), excl, N


class GroupStore:
    """The bonds, the angles, the dihedrals or the special pairs of a ``State`` (``State.groups[kind]``): type names, type ids and the
    members as indices over the state's rows.

    The members live in two places: a host array (HOOMD's snapshot layout, uint32 (n, arity)) and a device tensor (int64
    (n, arity)). Whoever writes one invalidates the other; the copy across happens when the other one is asked for -- the
    particle sorter re-indexes a million bonds on the device and the table is built there, so inside a run nothing
    travels (a sort used to cost two 8 MB transfers and two numpy passes, ~20 ms of idle GPU). Either write also drops
    the cached table.

    Decomposed runs (``set_global``): the whole topology by particle TAG, replicated on every rank (HOOMD's BondData
    migrates its groups with their members; a static topology of 12 B per bond can simply be everywhere). The
    index-based members are rebuilt from it whenever particles migrate (``relocalize``)."""

    def __init__(self, kind, groups, device):
        self.kind, self.arity, self.device = kind, ARITY[kind], device
        self.types = list(groups.types)
        self.group = groups.group
        self.typeid = np.ascontiguousarray(groups.typeid, dtype=np.uint32)
        self.tags = None
        self.tags_typeid = None

    # counts every write to the members (either setter; with them a sort, ``set_global``, ``relocalize``): what
    # ``State.exclusion_table`` keys its cache on
    version = 0

    @property
    def group(self):
        if self._host is None:
            import torch

            self._host = self._dev.to(torch.int32).cpu().numpy().view(np.uint32).reshape(-1, self.arity)
        return self._host

    @group.setter
    def group(self, group):
        self._host = np.ascontiguousarray(group, dtype=np.uint32).reshape(-1, self.arity)
        self._dev = None
        self._table = None
        self.version += 1

    @property
    def n(self):
        return int((self._host if self._host is not None else self._dev).shape[0])

    def group_device(self):
        """The members as an int64 (n, arity) tensor on the state's device."""
        if self._dev is None:
            import torch

            self._dev = torch.from_numpy(self._host.astype(np.int64)).to(self.device).reshape(-1, self.arity)
        return self._dev

    def set_group_device(self, group):
        self._dev = group.reshape(-1, self.arity)
        self._host = None
        self._table = None
        self.version += 1

    def reindex(self, inv):
        """The particles were permuted: row ``i`` is now row ``inv[i]`` (on the device, and the result stays there)."""
        if self.n:
            self.set_group_device(inv[self.group_device()])

    def set_global(self, tags, typeid, types, tag, n_local):
        """The groups of the WHOLE system as rows of particle tags; ``relocalize`` turns them into this rank's."""
        self.tags = np.ascontiguousarray(tags, dtype=np.int64).reshape(-1, self.arity)
        self.tags_typeid = np.ascontiguousarray(typeid, dtype=np.uint32)
        self.types = list(types)
        self.relocalize(tag, n_local)

    def relocalize(self, tag, n_local):
        """(Re)build the members -- index rows over local + ghost rows -- from the tags now on this rank
        (``localize_groups``): every group with at least one LOCAL member (a group is evaluated by the rank(s) owning a
        member), all its members on the rank (``AzpError`` if one is missing)."""
        self.group, self.typeid = localize_groups(tag, n_local, self.tags, self.tags_typeid, self.arity, self.kind)

    def table(self, n_local):
        """``build_group_table`` on the state's device, kept until the members change (a sort, a migration). Built
        there with one stable sort: numpy's scatter-add took 0.14 s for the 10^6 bonds of C3."""
        if self._table is None:
            import torch

            tid = torch.from_numpy(self.typeid.astype(np.int64)).to(self.device)
            self._table = build_group_table(self.group_device(), tid, n_local, self.kind)
        return self._table


class State:
    """Device-resident particle data (HOOMD ``ParticleData`` + ``BondData``)."""

    def __init__(self, snapshot, device, n_local=None):
        """``n_local``: in a domain-decomposed run the snapshot lists this rank's
        local particles first and its ghosts after them; forces are computed
        for the first ``n_local`` only."""
        import torch

        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.AzpError("azplugins_amd states live on an MI355X (device 'cuda:N'); there is no CPU path")
        p = snapshot.particles
        self.N = p.N if n_local is None else int(n_local)
        self.n_ghost = p.N - self.N
        self.types = list(p.types)
        self._box = Box.from_box(snapshot.configuration.box)
        f64 = torch.float64
        self.pos = torch.from_numpy(_pos4(p.position, p.typeid)).to(self.device)
        vel = np.zeros((p.N, 4))
        vel[:, :3] = p.velocity
        vel[:, 3] = p.mass
        self.vel = torch.from_numpy(vel).to(self.device)
        self.orientation = torch.from_numpy(np.ascontiguousarray(p.orientation, dtype=np.float64)).to(self.device)
        self.tag = torch.from_numpy(np.ascontiguousarray(p.tag, dtype=np.uint32).view(np.int32)).to(self.device)
        # rotational degrees of freedom (HOOMD ParticleData: angmom Scalar4, moment_inertia Scalar3)
        self.angmom = torch.from_numpy(np.ascontiguousarray(p.angmom, dtype=np.float64)).to(self.device)
        self.inertia = torch.from_numpy(np.ascontiguousarray(p.moment_inertia, dtype=np.float64)).to(self.device)
        self.net_force = torch.zeros((self.N, 4), dtype=f64, device=self.device)
        self.image = torch.zeros((p.N, 3), dtype=torch.int32, device=self.device)
        # (n_max, 4) accelerations of the Langevin methods (HOOMD ParticleData accelerations): created by their first
        # run as F_net / m, then carried from step two to the next step one
        self.accel = None
        # (n_max, 4) body-frame Langevin torques b_x, b_y, b_z, 0 of methods.Langevin with rotation: created
        # by its first run as zeros, then carried from step two to the next step one
        self.langevin_torque = None
        # bonds, angles (members a, b, c with b the vertex) and dihedrals (members a, b, c, d): one GroupStore each,
        # also reachable as bond_group, n_bonds, bond_table(), set_global_bonds(), ... (the delegations below the class)
        # (special pairs under the kind "pair": pair_group, n_pairs, pair_table(), set_global_pairs(), ...)
        self.groups = {kind: GroupStore(kind, getattr(snapshot, kind + "s"), self.device) for kind in KINDS}
        self._exclusions = None       # (key, table) of the last exclusion_table() that was not bond-only
        self.position_generation = 0  # bumped whenever positions change
        self.order_generation = 0     # bumped whenever the particles are re-indexed (sort, migration)
        self.type_generation = 0      # bumped whenever an updater may have changed the types in pos.w
        self.box_generation = 0       # bumped whenever the box changes (set_box): cell grids and image shifts are stale

    @property
    def n_max(self):
        return self.N + self.n_ghost

    @property
    def box(self):
        """The simulation box. Assigning one (or ``set_box``) that differs from the current box in an edge, a tilt factor
        or a periodic flag bumps ``box_generation`` and ``position_generation``: neighbor lists are rebuilt and the
        steppers wrap with the new box from the next step on. The particles are NOT moved (``update.BoxResize`` scales
        them); the box object itself is treated as immutable -- change the box by assigning a new one."""
        return self._box

    @box.setter
    def box(self, box):
        self.set_box(box)

    def set_box(self, box):
        """HOOMD ``State.set_box``: see ``box``. A box equal to the current one changes nothing."""
        box = Box.from_box(box)
        if box == self._box:
            return
        self._box = box
        self.box_generation += 1
        self.position_generation += 1

    @property
    def typeid_host(self):
        return self.pos[: self.N, 3].cpu().numpy().view(np.int64).astype(np.int64) & 0xFFFFFFFF

    def _row_tags(self):
        return self.tag[: self.n_max].cpu().numpy().view(np.uint32).astype(np.int64)

    def set_global(self, kind, tags, typeid, types):
        """Domain-decomposed runs: the bonds, angles or dihedrals of the WHOLE system by particle tag, replicated on
        every rank (``GroupStore.set_global``); localized at once and again after every migration (``relocalize``)."""
        self.groups[kind].set_global(tags, typeid, types, self._row_tags(), self.N)

    def relocalize(self, kind):
        self.groups[kind].relocalize(self._row_tags(), self.N)

    def group_table(self, kind):
        """The per-particle table of one kind (``build_group_table``). ``bond_table()`` is HOOMD's
        ``BondData::getGPUTable``: column-major entries (partner index, bond type), the particle's position in the
        bond, and the per-particle bond count."""
        return self.groups[kind].table(self.N)

    def exclusion_table(self, kinds=("bond",)):
        """Neighbor-list exclusions (HOOMD's ``exclusions``; the default is HOOMD's ``('bond',)``): one merged table
        ``(n_excl int32[N], excl int32[width, N], pitch)`` for the names in ``kinds`` (``EXCLUSIONS`` above the
        ``GroupStore``; an unknown name is an ``AzpError``). Rows for the local particles only.

        ``("bond",)`` alone is the partner column of the bond table, in that table's order, as it always was. Every
        other choice is built with torch on the state's device (``excluded_pairs``, ``build_exclusion_table``):
        symmetric, ascending inside a row, free of duplicates and of self-entries. On a decomposed run the pairs come
        from the global topology by tag (``GroupStore.tags``: a 1-3 pair whose middle bead is a ghost belongs to no
        group of this rank) and are localized with ``localize_pairs``. The table is kept until a group store is written
        or the particles are re-indexed."""
        kinds = check_exclusions(kinds, "exclusion_table")
        if kinds == ("bond",):
            t = self.bond_table()
            return t["n_bonds"], t["table"][:, :, 0].contiguous(), t["pitch"]
        return self.merged_exclusion_table(kinds)

    def merged_exclusion_table(self, kinds):
        """``exclusion_table`` in its merged form for every choice of names, ``("bond",)`` alone included (the RDF
        subtracts what the table names: a bond listed twice must come up once)."""
        kinds = check_exclusions(kinds, "exclusion_table")
        key = (kinds, tuple(g.version for g in self.groups.values()), self.order_generation, self.N, self.n_max)
        if self._exclusions is None or self._exclusions[0] != key:
            by_tag = any(g.tags is not None for g in self.groups.values())
            if by_tag:
                import torch

                members = {kind: torch.from_numpy(g.tags).to(self.device) for kind, g in self.groups.items() if g.tags is not None}
                pairs = localize_pairs(excluded_pairs(kinds, members), self.tag[: self.n_max], self.N)
            else:
                pairs = excluded_pairs(kinds, {kind: g.group_device() for kind, g in self.groups.items() if g.n})
            self._exclusions = (key, build_exclusion_table(pairs.to(self.device), self.N))
        return self._exclusions[1]

    def drop_exclusion_table(self):
        """Forget the kept ``exclusion_table`` (the rows were re-indexed by somebody who does not bump a counter)."""
        self._exclusions = None


def _delegate(kind):
    """The names the three kinds had before there was a ``GroupStore``: ``bond_group``, ``n_bonds``, ``bond_types``,
    ``bond_typeid``, ``bond_tags``, ``bond_tags_typeid``, ``bond_group_device()``, ``set_bond_group_device()``,
    ``set_global_bonds()``, ``relocalize_bonds()``, ``bond_table()`` and their angle, dihedral and (special) pair
    counterparts."""
    def attribute(name):
        return property(lambda self: getattr(self.groups[kind], name), lambda self, value: setattr(self.groups[kind], name, value))

    for name in ("group", "types", "typeid", "tags", "tags_typeid"):
        setattr(State, "%s_%s" % (kind, name), attribute(name))
    setattr(State, "n_%ss" % kind, property(lambda self: self.groups[kind].n))
    setattr(State, "%s_group_device" % kind, lambda self: self.groups[kind].group_device())
    setattr(State, "set_%s_group_device" % kind, lambda self, group: self.groups[kind].set_group_device(group))
    setattr(State, "set_global_%ss" % kind, lambda self, tags, typeid, types: self.set_global(kind, tags, typeid, types))
    setattr(State, "relocalize_%ss" % kind, lambda self: self.relocalize(kind))
    setattr(State, "%s_table" % kind, lambda self: self.group_table(kind))


for _kind in KINDS:
    _delegate(_kind)
