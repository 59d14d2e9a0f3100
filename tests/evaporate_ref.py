"""numpy restatement of the type updater and the particle evaporator (csrc/type_update.hip, include/azp.h) and of
``variant.SphereArea``, on host arrays: z (N,), typeid (N,), tag (N,) uint32."""

import math

import numpy as np

import flow_ref

EVAPORATOR_ID = 203  # src/RNGIdentifiers.h
NO_THRESHOLD = np.uint64(0xFFFFFFFFFFFFFFFF)


def in_slab(z, lo, hi):
    """A particle on a face is inside."""
    z = np.asarray(z, dtype=np.float64)
    return ~((z > hi) | (z < lo))


def type_update_region(z, typeid, inside, outside, lo, hi):
    """The new type ids: rows of type inside / outside get inside in the slab, outside elsewhere."""
    typeid = np.asarray(typeid).copy()
    ours = (typeid == inside) | (typeid == outside)
    typeid[ours] = np.where(in_slab(z, lo, hi)[ours], inside, outside)
    return typeid


def candidates(z, typeid, solvent, lo, hi):
    return (np.asarray(typeid) == solvent) & in_slab(z, lo, hi)


def keys(tag, seed, timestep):
    """u64 key of every tag: c0 << 32 | tag, c0 the first Philox word of counter {0, tag, 0, 0}."""
    tag = np.asarray(tag, dtype=np.uint32).reshape(-1)
    k0, k1 = flow_ref.key(EVAPORATOR_ID, seed, timestep)
    c0 = flow_ref.philox4x32_10(0, tag, 0, 0, k0, k1)[0]
    return (c0.astype(np.uint64) << np.uint64(32)) | tag.astype(np.uint64)


def _limit(Nmax, M):
    return M if Nmax is None else min(int(Nmax), M)


def pick(tag, seed, timestep, Nmax):
    """Boolean mask over the candidates' ``tag``: the min(Nmax, M) with the smallest keys (Nmax None: all)."""
    tag = np.asarray(tag, dtype=np.uint32).reshape(-1)
    K = _limit(Nmax, tag.size)
    out = np.zeros(tag.size, dtype=bool)
    out[np.argsort(keys(tag, seed, timestep), kind="stable")[:K]] = True
    return out


def evaporate(z, typeid, tag, solvent, evaporated, lo, hi, Nmax, seed, timestep):
    """Returns (new type ids, M, number picked)."""
    typeid = np.asarray(typeid).copy()
    cand = np.flatnonzero(candidates(z, typeid, solvent, lo, hi))
    picked = cand[pick(np.asarray(tag)[cand], seed, timestep, Nmax)]
    typeid[picked] = evaporated
    return typeid, cand.size, picked.size


def local_keys(tag, seed, timestep, Nmax):
    """Phase one on one rank: its min(Nmax, M) smallest keys, ascending."""
    k = np.sort(keys(tag, seed, timestep))
    return k[:_limit(Nmax, k.size)]


def threshold(gathered, Nmax):
    """Phase two: the Nmax-th smallest of the ranks' keys; with fewer than Nmax keys in all, every candidate goes."""
    allk = np.sort(np.concatenate([np.asarray(g, dtype=np.uint64) for g in gathered]))
    if Nmax is None or allk.size < Nmax:
        return NO_THRESHOLD
    if Nmax == 0:
        return None  # nothing is picked
    return allk[Nmax - 1]


def apply_below(tag, seed, timestep, thr):
    """Boolean mask over one rank's candidates: key <= threshold."""
    if thr is None:
        return np.zeros(np.asarray(tag).size, dtype=bool)
    return keys(tag, seed, timestep) <= thr


def sphere_area(R0, alpha, timestep):
    drsq = alpha / (4.0 * math.pi) * timestep
    return 0.0 if drsq >= R0 * R0 else math.sqrt(R0 * R0 - drsq)
