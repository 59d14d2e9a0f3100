"""numpy restatement of methods.Langevin / methods.Brownian (include/azp.h: azp_langevin_args), written from
the scheme's text: quaternion algebra from its definition (no shortcut formulas shared with the kernel), the NO_SQUISH
free rotations, and the rotational halves of both methods. The translation is flow_ref's at a zero constant flow.

q (N, 4) orientation, scalar first; p (N, 4) angular-momentum quaternion; I (N, 3) principal moments; tau (N, 3) net
torque, space frame; b (N, 3) the stored body-frame Langevin torque; gamma_r (N, 3) per particle and body axis; ``sel``
is a boolean mask of the particles a method integrates, the others are returned unchanged."""

import numpy as np

import flow_ref

ZERO_FLOW = ("constant", (0.0, 0.0, 0.0))


def qmul(a, b):
    """Hamilton product of quaternion arrays (N, 4), scalar first: (a0 b0 - a.b, a0 b + b0 a + a x b)."""
    a0, a1, a2, a3 = a.T
    b0, b1, b2, b3 = b.T
    out = np.empty(np.broadcast_shapes(a.shape, b.shape))
    out[:, 0] = a0 * b0 - (a1 * b1 + a2 * b2 + a3 * b3)
    out[:, 1] = a0 * b1 + b0 * a1 + (a2 * b3 - a3 * b2)
    out[:, 2] = a0 * b2 + b0 * a2 + (a3 * b1 - a1 * b3)
    out[:, 3] = a0 * b3 + b0 * a3 + (a1 * b2 - a2 * b1)
    return out


def conj(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def pure(v):
    """(0, v)."""
    return np.concatenate([np.zeros((v.shape[0], 1)), v], axis=1)


def rotate(q, v):
    """vec(q (0, v) conj(q))."""
    return qmul(qmul(q, pure(v)), conj(q))[:, 1:]


def body(q, tau):
    """rotate(conj(q), tau) (no torque anywhere: zeros, without the arithmetic)."""
    return rotate(conj(q), tau) if np.any(tau) else np.zeros_like(tau)


def body_angmom(q, p):
    """S = vec(1/2 conj(q) p)."""
    return 0.5 * qmul(conj(q), p)[:, 1:]


def rot_draws(rng_id, seed, tag, timestep, c):
    """(N, 3) draws 3, 4, 5 of the key (rng_id, timestep, seed), counter {k, tag, 0, 0}: -c_k + 2 c_k u01; c (N, 3)."""
    k0, k1 = flow_ref.key(rng_id, seed, timestep)
    tag = np.asarray(tag, dtype=np.uint32).reshape(-1)
    out = np.empty((tag.size, 3))
    for k in range(3):
        if not np.any(c[:, k]):  # (-0 + 2 0 u01 = 0: a draw that no row uses is not made)
            out[:, k] = 0.0
            continue
        r = flow_ref.philox4x32_10(np.uint32(k + 3), tag, 0, 0, k0, k1)
        out[:, k] = -c[:, k] + 2.0 * c[:, k] * flow_ref.u01(r[0], r[1])
    return out


def kick(q, p, T, dt):
    """p += dt q (0, T): this project's half kick."""
    return p + dt * qmul(q, pure(T))


# P_k q of the NO_SQUISH scheme (Miller et al., J. Chem. Phys. 116, 8649): P_1 q = (-q1, q0, q3, -q2),
# P_2 q = (-q2, -q3, q0, q1), P_3 q = (-q3, q2, -q1, q0)
PERM = {1: ([1, 0, 3, 2], [-1, 1, 1, -1]), 2: ([2, 3, 0, 1], [-1, -1, 1, 1]), 3: ([3, 2, 1, 0], [-1, 1, -1, 1])}


def free_rotation(k, p, q, Ik, dt):
    """exp(dt L_k) on the rows with Ik != 0: zeta = dt p . P_k q / (4 I_k); (p, q) <- cos(zeta) (p, q) + sin(zeta) (P_k p, P_k q)."""
    if not np.any(Ik):
        return p, q
    idx, sign = PERM[k]
    Pq, Pp = q[:, idx] * np.array(sign, dtype=np.float64), p[:, idx] * np.array(sign, dtype=np.float64)
    on = Ik != 0.0
    zeta = dt * np.sum(p * Pq, axis=1) / (4.0 * np.where(on, Ik, 1.0))
    c, s = np.cos(zeta)[:, None], np.sin(zeta)[:, None]
    return np.where(on[:, None], c * p + s * Pp, p), np.where(on[:, None], c * q + s * Pq, q)


def free_rotations(p, q, I, dt):
    """Axes 3, 2, 1, 2, 3 (half, half, full, half, half), then q renormalised."""
    for k, h in ((3, 0.5), (2, 0.5), (1, 1.0), (2, 0.5), (3, 0.5)):
        p, q = free_rotation(k, p, q, I[:, k - 1], h * dt)
    return p, q / np.linalg.norm(q, axis=1)[:, None]


def _coeff(gamma_r, kT, dt):
    return np.sqrt(6.0 * gamma_r * kT / dt)


def langevin_rot_step_two(q, p, I, tau, tag, gamma_r, kT, dt, seed, timestep, sel):
    """Returns (p, b): b_k = R_k - gamma_r,k S_k / I_k on the axes with I_k != 0 (else 0); T = body(tau) + b, zeroed where
    I_k == 0; p += dt q (0, T)."""
    on = I != 0.0
    R = rot_draws(flow_ref.LANGEVIN_ID, seed, tag, timestep, _coeff(gamma_r, kT, dt))
    S = body_angmom(q, p)
    b = np.where(on, R - gamma_r * S / np.where(on, I, 1.0), 0.0)
    T = np.where(on, body(q, tau) + b, 0.0)
    return np.where(sel[:, None], kick(q, p, T, dt), p), b


def langevin_rot_step_one(q, p, I, tau, b, dt, sel):
    """Returns (q, p): T = body(tau) + b stored; p += dt q (0, T); free rotations; q renormalised."""
    T = np.where(I != 0.0, body(q, tau) + b, 0.0)
    pn, qn = free_rotations(kick(q, p, T, dt), q, I, dt)
    return np.where(sel[:, None], qn, q), np.where(sel[:, None], pn, p)


def brownian_rot_step(q, I, tau, tag, gamma_r, kT, dt, seed, timestep, sel):
    """Returns q: dtheta_k = (body(tau)_k + R_k) dt / gamma_r,k on the axes with I_k != 0; q <- normalize(q exp(dtheta / 2));
    rows with |dtheta| = 0 keep q."""
    on = I != 0.0
    R = rot_draws(flow_ref.BROWNIAN_ID, seed, tag, timestep, _coeff(gamma_r, kT, dt))
    dth = np.where(on, (body(q, tau) + R) * dt / gamma_r, 0.0)
    th = np.linalg.norm(dth, axis=1)
    moved = th > 0.0
    safe = np.where(moved, th, 1.0)
    e = np.concatenate([np.cos(0.5 * th)[:, None], (np.sin(0.5 * th) / safe)[:, None] * dth], axis=1)
    qn = qmul(q, e)
    qn /= np.linalg.norm(qn, axis=1)[:, None]
    return np.where((sel & moved)[:, None], qn, q)


# ---------------------------------------------------------------------------
# whole steps on a host state h: dict with pos, vel, mass, accel, image, tag (translation, as flow_ref) and, with
# ``rot``, q, p, I, b. force / torque: (N, 3) at the positions of the moment
# ---------------------------------------------------------------------------
def langevin_step_one(h, torque, L, dt, sel, rot):
    h = dict(h)
    h["pos"], h["vel"], h["image"] = flow_ref.langevin_step_one(h["pos"], h["vel"], h["accel"], h["image"], L, dt, sel)
    if rot:
        h["q"], h["p"] = langevin_rot_step_one(h["q"], h["p"], h["I"], torque, h["b"], dt, sel)
    return h


def langevin_step_two(h, force, torque, gamma, gamma_r, kT, dt, seed, timestep, sel, rot):
    h = dict(h)
    h["vel"], h["accel"] = flow_ref.langevin_step_two(h["pos"], h["vel"], h["mass"], h["accel"], force, h["tag"], gamma, kT, dt,
                                                      seed, timestep, ZERO_FLOW, False, sel)
    if rot:
        p, b = langevin_rot_step_two(h["q"], h["p"], h["I"], torque, h["tag"], gamma_r, kT, dt, seed, timestep, sel)
        h["p"], h["b"] = p, np.where(sel[:, None], b, h["b"])
    return h


def brownian_step(h, force, torque, gamma, gamma_r, kT, dt, seed, timestep, L, sel, rot):
    h = dict(h)
    h["pos"], h["image"] = flow_ref.brownian_step(h["pos"], h["image"], force, h["tag"], gamma, kT, dt, seed, timestep, ZERO_FLOW,
                                                  False, L, sel)
    if rot:
        h["q"] = brownian_rot_step(h["q"], h["I"], torque, h["tag"], gamma_r, kT, dt, seed, timestep, sel)
    return h
