"""Reference for the neighbor-list exclusions (``azplugins_amd.state.EXCLUSIONS``), in plain Python over adjacency sets
and explicit walks, written from the definitions and not from the torch builder:

* ``"bond"``: both members of every bond; ``"special_pair"``: both members of every special pair;
* ``"angle"`` / ``"dihedral"``: the first and the last member of every angle / dihedral;
* ``"1-3"``: (a, c) for every walk a - b - c over bonds with a != c;
* ``"1-4"``: (a, d) for every walk a - b - c - d over bonds with a != c, b != d and a != d.

A pair is unordered, never (i, i), and counts once however many groups or walks name it."""

import numpy as np

OPTIONS = ("bond", "angle", "dihedral", "special_pair", "1-3", "1-4")


def _rows(groups, arity):
    if groups is None:
        return []
    return [tuple(int(x) for x in g) for g in np.asarray(groups, dtype=np.int64).reshape(-1, arity)]


def _adjacency(bonds):
    adj = {}
    for a, b in bonds:
        adj.setdefault(a, set()).add(b)
        adj.setdefault(b, set()).add(a)
    return adj


def pair_sets(bonds=None, angles=None, dihedrals=None, pairs=None):
    """option -> set of unordered pairs (lo, hi)."""
    bonds, angles, dihedrals, pairs = _rows(bonds, 2), _rows(angles, 3), _rows(dihedrals, 4), _rows(pairs, 2)
    out = {name: set() for name in OPTIONS}

    def add(name, i, j):
        if i != j:
            out[name].add((min(i, j), max(i, j)))

    for a, b in bonds:
        add("bond", a, b)
    for a, b in pairs:
        add("special_pair", a, b)
    for g in angles:
        add("angle", g[0], g[2])
    for g in dihedrals:
        add("dihedral", g[0], g[3])
    adj = _adjacency(bonds)
    for a in adj:
        for b in adj[a]:
            for c in adj[b]:
                if c == a:
                    continue
                add("1-3", a, c)
                for d in adj[c]:
                    if d == b or d == a:
                        continue
                    add("1-4", a, d)
    return out


def pair_set(options, **topology):
    """The union of the sets of ``options``."""
    sets = pair_sets(**topology)
    out = set()
    for name in options:
        out |= sets[name]
    return out


def table(pairs, N):
    """(n_excl uint32[N], excl uint32[N, width]) from a set of unordered pairs: the form ``oracle.build_nlist`` and
    ``nlist_ref.all_pairs_rows`` take; rows ascending, for the particles below N."""
    partners = [set() for _ in range(N)]
    for i, j in pairs:
        if i < N:
            partners[i].add(j)
        if j < N:
            partners[j].add(i)
    n_excl = np.array([len(p) for p in partners], dtype=np.uint32)
    excl = np.zeros((N, max(int(n_excl.max()) if N else 0, 1)), dtype=np.uint32)
    for i, p in enumerate(partners):
        excl[i, :len(p)] = sorted(p)
    return n_excl, excl


def chain_bonds(n_chains, length, first=0):
    """Bonds of ``n_chains`` linear chains of ``length`` beads laid out from particle ``first``."""
    return np.array([(first + c * length + k, first + c * length + k + 1) for c in range(n_chains) for k in range(length - 1)],
                    dtype=np.int64).reshape(-1, 2)


def star_bonds(n_stars, arms, first=0):
    """Bonds of ``n_stars`` stars of one centre and ``arms`` one-bead arms laid out from particle ``first``."""
    return np.array([(first + s * (arms + 1), first + s * (arms + 1) + 1 + k) for s in range(n_stars) for k in range(arms)],
                    dtype=np.int64).reshape(-1, 2)
