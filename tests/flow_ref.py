"""numpy restatement of the flow module's integration methods (csrc/flow_methods.hip, include/azp.h): the flow
fields, the per-particle random stream (a vectorised Philox4x32-10) and one step of each scheme, on host arrays.

pos (N, 3), vel (N, 3), mass (N,), accel (N, 3), force (N, 3), image (N, 3) int, tag (N,) uint32, typeid (N,).
``sel`` is a boolean mask of the particles a method integrates; the others are returned unchanged."""

import numpy as np

import box_ref

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)
LANGEVIN_ID, BROWNIAN_ID, DPD_ID = 202, 201, 200


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (broadcast): returns the four output words as uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, dtype=np.uint32) for x in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    c0, c1, c2, c3, k0, k1 = (x.copy() for x in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = M0 * c0.astype(np.uint64)
        p1 = M1 * c2.astype(np.uint64)
        hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & MASK32).astype(np.uint32)
        hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & MASK32).astype(np.uint32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        with np.errstate(over="ignore"):  # (the key schedule wraps modulo 2^32)
            k0 = k0 + W0
            k1 = k1 + W1
    return c0, c1, c2, c3


def key(rng_id, seed, timestep):
    t = int(timestep)
    k0 = (rng_id << 24) | (((t >> 32) & 0xFF) << 16) | (int(seed) & 0xFFFF)
    return np.uint32(k0), np.uint32(t & 0xFFFFFFFF)


def u01(c0, c1):
    """(u64 >> 11) 2^-53 + 2^-54 of u64 = c0 << 32 | c1."""
    u = (c0.astype(np.uint64) << np.uint64(32)) | c1.astype(np.uint64)
    return (u >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) + (0.5 / 9007199254740992.0)


def uniform3(rng_id, seed, tag, timestep, c):
    """(N, 3) draws uniform(-c, c) (c: scalar or per particle) = -c + 2 c u01 with counter {k, tag, 0, 0}, k = 0, 1, 2."""
    k0, k1 = key(rng_id, seed, timestep)
    tag = np.asarray(tag, dtype=np.uint32).reshape(-1)
    c = np.broadcast_to(np.asarray(c, dtype=np.float64), tag.shape)
    out = np.empty((tag.size, 3))
    for k in range(3):
        r = philox4x32_10(np.uint32(k), tag, 0, 0, k0, k1)
        out[:, k] = -c + 2.0 * c * u01(r[0], r[1])
    return out


def flow_velocity(flow, pos):
    """flow = ("constant", (Ux, Uy, Uz)) or ("parabolic", mean_velocity, separation)."""
    pos = np.asarray(pos, dtype=np.float64)
    u = np.zeros_like(pos)
    if flow[0] == "constant":
        u[:] = np.asarray(flow[1], dtype=np.float64)
    else:
        Umax, L = 1.5 * float(flow[1]), 0.5 * float(flow[2])
        yr = pos[:, 1] / L
        u[:, 0] = Umax * (1.0 - yr * yr)
    return u


def wrap(pos, image, L, tilt=(0.0, 0.0, 0.0), periodic=(1, 1, 1)):
    """Box of edges L centred on the origin, one shift per axis (wrap_into_box): tests/box_ref.py."""
    return box_ref.wrap(pos, image, L, tilt, periodic)


def langevin_step_one(pos, vel, accel, image, L, dt, sel, tilt=(0.0, 0.0, 0.0), periodic=(1, 1, 1)):
    hdt = 0.5 * dt
    p = pos + (vel + hdt * accel) * dt
    p, im = wrap(p, image, L, tilt, periodic)
    v = vel + hdt * accel
    return (np.where(sel[:, None], p, pos), np.where(sel[:, None], v, vel), np.where(sel[:, None], im, image))


def langevin_step_two(pos, vel, mass, accel, force, tag, gamma, kT, dt, seed, timestep, flow, noiseless, sel):
    """gamma: per particle. Returns (vel, accel)."""
    u = flow_velocity(flow, pos)
    c = np.sqrt(6.0 * gamma * kT / dt)
    if noiseless:
        c = np.zeros_like(c)
    R = uniform3(LANGEVIN_ID, seed, tag, timestep, c)
    bd = R - gamma[:, None] * (vel - u)
    minv = 1.0 / mass
    a = (force + bd) * minv[:, None]
    v = vel + (0.5 * dt) * a
    return np.where(sel[:, None], v, vel), np.where(sel[:, None], a, accel)


def brownian_step(pos, image, force, tag, gamma, kT, dt, seed, timestep, flow, noiseless, L, sel, tilt=(0.0, 0.0, 0.0),
                  periodic=(1, 1, 1)):
    u = flow_velocity(flow, pos)
    c = np.sqrt(6.0 * gamma * kT / dt)
    if noiseless:
        c = np.zeros_like(c)
    R = uniform3(BROWNIAN_ID, seed, tag, timestep, c)
    p = pos + (u + (force + R) / gamma[:, None]) * dt
    p, im = wrap(p, image, L, tilt, periodic)
    return np.where(sel[:, None], p, pos), np.where(sel[:, None], im, image)
