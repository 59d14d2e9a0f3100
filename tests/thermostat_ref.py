"""numpy / plain-Python restatement of the thermostats of ``ConstantVolume`` (csrc/thermostat.hip, include/azp.h,
DESIGN.md 4.18): the kinetic terms and the two integration halves bit for bit, the random stream, and the scalar map
(K, state, t) -> alpha of Berendsen, Bussi and MTTK in Python floats with ``math``'s functions.

vel (N, 3), mass (N,), force (N, 3), pos (N, 3), image (N, 3) int. A thermostat's state is the dict
``dict(energy=, xi=, eta=)``."""

import math

import numpy as np

import flow_ref
import reduction_ref

BERENDSEN, BUSSI, MTTK = 0, 1, 2
THERMOSTAT_ID = 204
GAMMA_MAX_ATTEMPTS = 32

# Largest relative deviation of the device's alpha (and xi, eta, energy) from this restatement that the tests allow:
# 8 times the largest deviation measured on the MI355X over the grid of tests/test_gpu_thermostat.py.
# Measured: 0.0. Over all 50,688 cases of the grid (46,080 of them Bussi) alpha, xi, eta, energy and the number of
# Gamma attempts came out bit for bit as here: the device library's exp / log / cos / sqrt returned what the host's
# did for every argument met. So ALPHA_REL is 0 and the tests hold the advance, and with it whole runs, to bit
# equality: a run without forces is compared with ``ideal_gas_particles``, the recurrence carried in the arithmetic
# the kernels define (every velocity scaled, K re-summed in the device's order), which leaves no rounding to allow for.
# The scalar form K_(n+1) = alpha_n^2 K_n (``ideal_gas``) differs from that by rounding alone, bounded by
# ``recurrence_rounding(steps)``.
ALPHA_REL_MEASURED = 0.0
ALPHA_REL = 8 * ALPHA_REL_MEASURED


# ---------------------------------------------------------------------------
# the per-particle arithmetic, bit for bit
# ---------------------------------------------------------------------------
def kinetic_terms(vel, mass):
    """0.5 * (((m vx) vx + (m vy) vy) + (m vz) vz) per particle."""
    vel, m = np.asarray(vel, dtype=np.float64), np.asarray(mass, dtype=np.float64)
    return 0.5 * ((((m * vel[:, 0]) * vel[:, 0]) + ((m * vel[:, 1]) * vel[:, 1])) + ((m * vel[:, 2]) * vel[:, 2]))


def kinetic_energy(vel, mass):
    """K in the order of the device's two-stage sum."""
    return float(reduction_ref.tree_sum(kinetic_terms(vel, mass)))


def step_two(vel, mass, force, dt):
    """v + ((dt / 2) f) (1 / m)."""
    hdt = 0.5 * dt
    minv = 1.0 / np.asarray(mass, dtype=np.float64)
    return vel + (hdt * force) * minv[:, None]


def step_one(pos, vel, mass, force, image, L, dt, alpha, tilt=(0.0, 0.0, 0.0), periodic=(1, 1, 1)):
    """v = alpha v; v += ((dt / 2) f) (1 / m); x += dt v; wrap. Returns (pos, vel, image)."""
    v = step_two(alpha * vel, mass, force, dt)
    p, im = flow_ref.wrap(pos + dt * v, image, L, tilt, periodic)
    return p, v, im


# ---------------------------------------------------------------------------
# random stream
# ---------------------------------------------------------------------------
def _philox(c0, k0, k1):
    """Philox4x32-10 of the counter {c0, 0, 0, 0} in Python integers: the first two output words."""
    c1 = c2 = c3 = 0
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1


class Stream:
    """The draws of one step: key (204, seed, t) in the flow methods' layout, counter {k, 0, 0, 0} for draw k."""

    def __init__(self, seed, timestep):
        k0, k1 = flow_ref.key(THERMOSTAT_ID, seed, timestep)
        self.k0, self.k1 = int(k0), int(k1)

    def u01(self, k):
        c0, c1 = _philox(k, self.k0, self.k1)
        return float(((c0 << 32) | c1) >> 11) * (1.0 / 9007199254740992.0) + (0.5 / 9007199254740992.0)

    def normal(self, k):
        """Box-Muller from the draws k and k + 1."""
        ua, ub = self.u01(k), self.u01(k + 1)
        return math.sqrt(-2.0 * math.log(ua)) * math.cos(6.283185307179586 * ub)

    def gamma(self, shape):
        """Gamma(shape, 1), shape >= 1, by Marsaglia and Tsang: (value, attempts taken). After GAMMA_MAX_ATTEMPTS
        rejections the value is d (a guard that the tests never reach)."""
        d = shape - 1.0 / 3.0
        c = 1.0 / math.sqrt(9.0 * d)
        for j in range(GAMMA_MAX_ATTEMPTS):
            x = self.normal(2 + 3 * j)
            u = self.u01(4 + 3 * j)
            t = 1.0 + c * x
            v = (t * t) * t
            if v > 0.0 and math.log(u) < ((0.5 * (x * x) + d) - d * v) + d * math.log(v):
                return d * v, j + 1
        return d, GAMMA_MAX_ATTEMPTS + 1


# ---------------------------------------------------------------------------
# the thermostats
# ---------------------------------------------------------------------------
def new_state():
    return dict(energy=0.0, xi=0.0, eta=0.0)


def mttk_g(K, ndof, kT, tau):
    return ((2.0 * K) / (ndof * kT) - 1.0) / (tau * tau)


def mttk_energy(xi, eta, ndof, kT, tau):
    return (ndof * kT) * (0.5 * ((tau * tau) * (xi * xi)) + eta)


def advance(kind, K, state, kT, tau, dt, ndof, seed=0, timestep=0):
    """One advance at the start of step ``timestep``: (alpha, new state, Gamma attempts). ``state`` is not changed."""
    s = dict(state)
    attempts = 0
    alpha = 1.0
    if kind == MTTK:
        hdt = 0.5 * dt
        xi = s["xi"] + hdt * mttk_g(K, ndof, kT, tau)
        alpha = math.exp(-(xi * dt))
        s["eta"] = s["eta"] + xi * dt
        s["xi"] = xi + hdt * mttk_g((alpha * alpha) * K, ndof, kT, tau)
        s["energy"] = mttk_energy(s["xi"], s["eta"], ndof, kT, tau)
    elif K > 0.0:
        if kind == BERENDSEN:
            Kbar = 0.5 * (ndof * kT)
            alpha = math.sqrt(1.0 + (dt / tau) * (Kbar / K - 1.0))
        else:
            rng = Stream(seed, timestep)
            c = math.exp(-(dt / tau)) if tau > 0.0 else 0.0
            R1 = rng.normal(0)
            g, attempts = rng.gamma(0.5 * (ndof - 1.0))
            S = 2.0 * g
            w = (1.0 - c) * (0.5 * kT)
            r = math.sqrt(c * K) + R1 * math.sqrt(w)
            alpha = math.sqrt((r * r + w * S) / K)
        s["energy"] = s["energy"] + (K - (alpha * alpha) * K)
    return alpha, s, attempts


def ideal_gas(kind, K0, steps, kT, tau, dt, ndof, seed=0, t0=0, state=None):
    """The recurrence K_(n+1) = alpha_n^2 K_n of particles without forces: (K_0 .. K_steps, alphas, final state, largest
    number of Gamma attempts). kT: a float or a callable of the timestep."""
    s = new_state() if state is None else dict(state)
    Ks, alphas, worst = [float(K0)], [], 0
    for n in range(steps):
        kTn = float(kT(t0 + n)) if callable(kT) else kT
        alpha, s, attempts = advance(kind, Ks[-1], s, kTn, tau, dt, ndof, seed, t0 + n)
        alphas.append(alpha)
        Ks.append((alpha * alpha) * Ks[-1])
        worst = max(worst, attempts)
    return np.array(Ks), np.array(alphas), s, worst


def recorded_kinetic_energy(vel, mass):
    """``kinetic_energy`` of ``compute.ThermodynamicQuantities`` bit for bit: 0.5 ((S_xx + S_yy) + S_zz) with
    S_aa the device's two-stage sum of (m v_a) v_a (csrc/thermo.hip)."""
    vel, m = np.asarray(vel, dtype=np.float64), np.asarray(mass, dtype=np.float64)
    S = [float(reduction_ref.tree_sum((m * vel[:, a]) * vel[:, a])) for a in range(3)]
    return 0.5 * ((S[0] + S[1]) + S[2])


def ideal_gas_particles(kind, vel, mass, steps, kT, tau, dt, ndof, seed=0, t0=0, state=None):
    """The recurrence of particles without forces carried in the arithmetic the kernels define: K_n is the two-stage sum
    over the velocities, every velocity is scaled by alpha_n, and both half kicks add (dt / 2) 0 / m. Returns (the K
    each advance saw, K_0 .. K_(steps-1); alphas; the recorder's kinetic energy after each step, steps of them; the
    final velocities; the final state; the largest number of Gamma attempts)."""
    v = np.array(vel, dtype=np.float64)
    zero = np.zeros_like(v)
    s = new_state() if state is None else dict(state)
    Ks, alphas, recorded, worst = [], [], [], 0
    for n in range(steps):
        kTn = float(kT(t0 + n)) if callable(kT) else kT
        Ks.append(kinetic_energy(v, mass))
        alpha, s, attempts = advance(kind, Ks[-1], s, kTn, tau, dt, ndof, seed, t0 + n)
        alphas.append(alpha)
        v = step_two(step_two(alpha * v, mass, zero, dt), mass, zero, dt)
        recorded.append(recorded_kinetic_energy(v, mass))
        worst = max(worst, attempts)
    return np.array(Ks), np.array(alphas), np.array(recorded), v, s, worst


def recurrence_rounding(steps):
    """Bound on the relative difference between K carried per particle and the scalar recurrence K_(n+1) = alpha_n^2
    K_n after ``steps`` steps, from the number format alone. Per step the per-particle form rounds alpha v once (two
    ulp in the squared term), the term three more times, and a term then passes through at most 17 additions of the
    two-stage sum at the sizes used here (1 in the lane, 6 + 3 in the workgroup, 1 + 6 in the fold); the scalar form
    rounds twice: 24 ulp of 2^-53, and one more set of 24 for the recorder's own sum. The differences feed back through
    alpha with a factor below one (every thermostat pulls K towards Kbar), so they add at most linearly."""
    return (steps + 1) * 24 * 2.0 ** -53


def berendsen_closed(K0, steps, kT, tau, dt, ndof):
    """Berendsen without forces in closed form: K_(n+1) = K_n + (dt / tau)(Kbar - K_n), so
    K_n = Kbar + (K_0 - Kbar)(1 - dt / tau)^n."""
    Kbar = 0.5 * ndof * kT
    return Kbar + (K0 - Kbar) * (1.0 - dt / tau) ** np.arange(steps + 1)


def oscillators(kind, x, v, mass, k, steps, dt, kT=1.0, tau=0.5, ndof=None):
    """Velocity Verlet of independent harmonic oscillators (force -k x), thermostatted as the driver does (advance,
    scaled step one, forces, step two), or plain with ``kind`` None. Returns K + U (+ the thermostat's energy) after
    every step, the start included."""
    x, v = np.array(x, dtype=np.float64), np.array(v, dtype=np.float64)
    m = np.asarray(mass, dtype=np.float64)[:, None]
    kk = np.asarray(k, dtype=np.float64)[:, None]
    ndof = float(x.size) if ndof is None else ndof
    s = new_state()

    def total():
        return float((0.5 * m * v * v).sum() + (0.5 * kk * x * x).sum()) + s["energy"]

    out = [total()]
    f = -kk * x
    for n in range(steps):
        if kind is not None:
            alpha, s, _ = advance(kind, float((0.5 * m * v * v).sum()), s, kT, tau, dt, ndof, 0, n)
            v = alpha * v
        v = v + (0.5 * dt) * f / m
        x = x + dt * v
        f = -kk * x
        v = v + (0.5 * dt) * f / m
        out.append(total())
    return np.array(out)
