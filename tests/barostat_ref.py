"""numpy / plain-Python restatement of ``ConstantPressure`` (csrc/barostat.hip, include/azp.h): step one
and step two bit for bit, the advance in Python floats with ``math``'s ``exp``, the sums it reads in the order of the
device's two-stage sum, the thermostat through ``thermostat_ref.advance``, and a whole step of a small system with an
all-pairs truncated Lennard-Jones force for the tests that need no GPU.

vel (N, 3), mass (N,), force (N, 3), pos (N, 3), image (N, 3) int, L the three box lengths. The barostat's state is the
dict of ``new_state``; ``advance`` returns a new one with everything the device writes."""

import math

import numpy as np

import flow_ref
import reduction_ref
import thermo_ref
import thermostat_ref

CLOSE, OPEN = 1, 2
COUPLE = {"none": 0, "xy": 1, "xz": 2, "yz": 3, "xyz": 4}
_COUPLED_AXES = {"none": (), "xy": (0, 1), "xz": (0, 2), "yz": (1, 2), "xyz": (0, 1, 2)}
KAA, WAA = (4, 7, 9), (10, 13, 15)  # slots of azp_thermo_sums

# Largest relative deviation of the device's advance (nu, alpha, lambda, b, alpha_T, energy, each relative to the magnitude of
# its terms) from this restatement that the tests allow: 8 times the largest deviation measured on the MI355X over the
# grid of tests/test_gpu_barostat.py.
# Measured: 2.21e-16, over 25,920 cases. nu, the energy, K, V, W and P came out bit for bit as here (they pass through no
# library function); alpha, lambda, b and alpha_T differed in at most the last bit: the device library's exp is one ulp
# off the host's for some arguments, and an ulp is at most 2^-52 = 2.22e-16 of the result. That bound of the measured
# value is what is recorded.
BARO_REL_MEASURED = 2.0 ** -52
BARO_REL = 8 * BARO_REL_MEASURED


# ---------------------------------------------------------------------------
# the per-particle arithmetic, bit for bit
# ---------------------------------------------------------------------------
def step_one(pos, vel, mass, force, image, L_new, dt, alpha, lam, b, alpha_T=1.0):
    """c_a = alpha_T alpha_a; v_a = c_a v_a; v += ((dt / 2) f) (1 / m); r_a = lambda_a r_a + b_a v_a; wrap into the box
    of edges ``L_new``. Returns (pos, vel, image)."""
    c = np.array([alpha_T * alpha[0], alpha_T * alpha[1], alpha_T * alpha[2]])
    v = thermostat_ref.step_two(c[None, :] * vel, mass, force, dt)
    r = np.asarray(lam, dtype=np.float64)[None, :] * pos + np.asarray(b, dtype=np.float64)[None, :] * v
    p, im = flow_ref.wrap(r, image, L_new)
    return p, v, im


def step_two(vel, mass, force, dt, alpha):
    """v += ((dt / 2) f) (1 / m); v_a = alpha_a v_a."""
    return np.asarray(alpha, dtype=np.float64)[None, :] * thermostat_ref.step_two(vel, mass, force, dt)


def sums(vel, mass, force=None, energy=None, virial=None):
    """The row of ``azp_thermo_sums`` over all particles, bit for bit: ``force`` (N, 3) and ``energy`` (N,) of the one
    force, ``virial`` its (6, N) per-particle virials; all None: no force."""
    vel4 = np.c_[np.asarray(vel, dtype=np.float64), np.asarray(mass, dtype=np.float64)]
    forces, virials = (), ()
    if force is not None:
        forces = (np.c_[force, energy],)
        virials = (virial,)
    terms = thermo_ref.particle_terms(vel4, np.ones(vel4.shape[0], dtype=bool), forces, virials)
    return reduction_ref.tree_sum(terms)


# ---------------------------------------------------------------------------
# the advance
# ---------------------------------------------------------------------------
def new_state(nu=(0.0, 0.0, 0.0), ref_kT=0.0):
    return dict(nu=tuple(float(x) for x in nu), ref_kT=float(ref_kT))


def sinhc(x):
    x2 = x * x
    return 1.0 + x2 * (1.0 / 6.0 + x2 * (1.0 / 120.0 + x2 * (1.0 / 5040.0 + x2 * (1.0 / 362880.0))))


def advance(row, L, S, dt, tauS, ndof, couple, box_dof, phase, state, thermostat=None):
    """One ``azp_barostat_advance``. ``row``: the 20 sums; ``S``: three floats; ``couple``: a key of ``COUPLE``;
    ``box_dof``: three flags; ``thermostat``: None or dict(kind, kT, tau, seed, timestep, state) with ``state`` a
    ``thermostat_ref`` state. Returns the new state: nu, ref_kT, energy, K, V, W, P (3), G (3) and, after an open phase,
    alpha, lam, b (3 each), alpha_T and ``thermostat_state``. ``state`` is not changed."""
    row = [float(x) for x in row]
    Kaa = [row[k] for k in KAA]
    Waa = [row[k] for k in WAA]
    K = 0.5 * ((Kaa[0] + Kaa[1]) + Kaa[2])
    V = (L[0] * L[1]) * L[2]
    out = dict(state)
    if thermostat is not None:
        kT = thermostat["kT"]
    else:
        kT = state["ref_kT"]
        if not kT > 0.0:
            kT = (2.0 * K) / ndof
            out["ref_kT"] = kT
    W = ((ndof + 3.0) * kT) * (tauS * tauS)
    two_k = (2.0 * K) / ndof
    free = [bool(f) for f in box_dof[:3]]
    G = [(((Kaa[a] + Waa[a]) - V * S[a]) + two_k) / W if free[a] else 0.0 for a in range(3)]
    axes = _COUPLED_AXES[couple]
    n = float(sum(1 for a in axes if free[a]))
    if axes and n:
        total = 0.0
        for a in axes:
            total = total + G[a]
        mean = total / n
        for a in axes:
            if free[a]:
                G[a] = mean
    hdt = 0.5 * dt
    nu = list(state["nu"])
    for _ in range((1 if phase & CLOSE else 0) + (1 if phase & OPEN else 0)):
        nu = [nu[a] + hdt * G[a] if free[a] else 0.0 for a in range(3)]
    if phase & OPEN:
        trace = (nu[0] + nu[1]) + nu[2]
        share = trace / ndof
        out["alpha"] = tuple(math.exp(-((nu[a] + share) * hdt)) for a in range(3))
        out["lam"] = tuple(math.exp(nu[a] * dt) for a in range(3))
        out["b"] = tuple((dt * math.exp(nu[a] * hdt)) * sinhc(nu[a] * hdt) for a in range(3))
        out["alpha_T"] = 1.0
        if thermostat is not None:
            t = thermostat
            out["alpha_T"], out["thermostat_state"], _ = thermostat_ref.advance(t["kind"], K, t["state"], t["kT"], t["tau"], dt, ndof,
                                                                                t.get("seed", 0), t.get("timestep", 0))
    out.update(nu=tuple(nu), energy=(0.5 * W) * ((nu[0] * nu[0] + nu[1] * nu[1]) + nu[2] * nu[2]), K=K, V=V, W=W, G=tuple(G),
               P=tuple((Kaa[a] + Waa[a]) / V for a in range(3)))
    return out


# ---------------------------------------------------------------------------
# a small system for the tests without a GPU
# ---------------------------------------------------------------------------
def lj(pos, L, r_cut=2.5):
    """All-pairs Lennard-Jones (epsilon = sigma = 1), truncated and shifted at ``r_cut``, minimum image in the
    orthorhombic box ``L``: (force (N, 3), energy per particle (N,), virial per particle (6, N) in the order xx, xy, xz,
    yy, yz, zz with W_ab = 1/2 sum_j r_a f_b)."""
    pos, L = np.asarray(pos, dtype=np.float64), np.asarray(L, dtype=np.float64)
    d = pos[:, None, :] - pos[None, :, :]
    d -= L * np.rint(d / L)
    r2 = (d * d).sum(axis=2)
    np.fill_diagonal(r2, np.inf)
    inside = r2 < r_cut * r_cut
    inv2 = np.where(inside, 1.0 / r2, 0.0)
    inv6 = inv2 * inv2 * inv2
    f_over_r = 24.0 * inv2 * inv6 * (2.0 * inv6 - 1.0)
    shift = 4.0 * (r_cut ** -12 - r_cut ** -6)
    e = np.where(inside, 4.0 * inv6 * (inv6 - 1.0) - shift, 0.0)
    fij = f_over_r[:, :, None] * d
    force = fij.sum(axis=1)
    virial = np.array([0.5 * (d[:, :, a] * fij[:, :, b]).sum(axis=1) for a, b in thermo_ref.ORDER])
    return force, 0.5 * e.sum(axis=1), virial


def jittered_lattice(n, rho, seed, kT=1.0):
    """n^3 particles of unit mass on a simple cubic lattice at density ``rho``, each displaced by up to 5 % of the
    spacing, with Maxwell-Boltzmann velocities of zero total momentum: (pos, vel, L)."""
    rng = np.random.default_rng(seed)
    a = rho ** (-1.0 / 3.0)
    g = (np.arange(n) + 0.5) * a - 0.5 * n * a
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) + rng.uniform(-0.05, 0.05, (n ** 3, 3)) * a
    vel = rng.normal(0.0, math.sqrt(kT), (n ** 3, 3))
    vel -= vel.mean(axis=0)
    return pos, vel, np.array([n * a] * 3)


class System:
    """Positions, velocities and box of unit-mass LJ particles under the barostat, stepped as the driver does: the first
    step of ``run`` opens from a sums pass of the state as it stands; every step is open, box, step one, forces, step
    two, sums, close. ``S`` None: plain velocity Verlet (NVE) in the same arithmetic."""

    def __init__(self, pos, vel, L, dt, S=None, tauS=1.0, couple="none", box_dof=(True, True, True), state=None):
        self.pos, self.vel, self.L = np.array(pos, dtype=np.float64), np.array(vel, dtype=np.float64), [float(x) for x in L]
        self.N = self.pos.shape[0]
        self.mass = np.ones(self.N)
        self.image = np.zeros((self.N, 3), dtype=np.int64)
        self.dt, self.S, self.tauS, self.couple, self.box_dof = dt, S, tauS, couple, tuple(box_dof)
        self.ndof = 3.0 * self.N - 3.0
        self.state = new_state() if state is None else dict(state)
        self.force, self.energy, self.virial = lj(self.pos, self.L)

    def row(self):
        return sums(self.vel, self.mass, self.force, self.energy, self.virial)

    def _advance(self, row, phase):
        self.state = advance(row, self.L, self.S, self.dt, self.tauS, self.ndof, self.couple, self.box_dof, phase, self.state)

    def run(self, steps):
        one = (1.0, 1.0, 1.0)
        row = self.row()
        for _ in range(steps):
            if self.S is None:
                alpha, lam, b = one, one, (self.dt,) * 3
            else:
                self._advance(row, OPEN)
                alpha, lam, b = self.state["alpha"], self.state["lam"], self.state["b"]
                self.L = [lam[a] * self.L[a] for a in range(3)]
            self.pos, self.vel, self.image = step_one(self.pos, self.vel, self.mass, self.force, self.image, self.L, self.dt,
                                                      alpha, lam, b)
            self.force, self.energy, self.virial = lj(self.pos, self.L)
            self.vel = step_two(self.vel, self.mass, self.force, self.dt, alpha)
            row = self.row()
            if self.S is not None:
                self._advance(row, CLOSE)

    @property
    def volume(self):
        return (self.L[0] * self.L[1]) * self.L[2]

    def conserved(self):
        """K + U + S V + the barostat's energy (hydrostatic S), or K + U without a barostat."""
        row = self.row()
        e = 0.5 * ((row[4] + row[7]) + row[9]) + row[16]
        if self.S is not None:
            e += self.S[0] * self.volume + self.state.get("energy", 0.0)
        return float(e)


def ideal_gas(vel, mass, L, steps, S, dt, tauS, couple="none", box_dof=(True, True, True), thermostat=None, seed=0, t0=0,
              state=None):
    """Particles without forces under the barostat, carried in the arithmetic the kernels define (the sums re-summed in
    the device's order every step; both half kicks add (dt / 2) 0 / m). ``thermostat``: None or dict(kind, kT, tau) with
    ``kT`` a float or a callable of the timestep. Returns (K after every step, V after every step, the final velocities,
    the final L, the final barostat state, the final thermostat state or None)."""
    v = np.array(vel, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    zero = np.zeros_like(v)
    L = [float(x) for x in L]
    ndof = 3.0 * v.shape[0] - 3.0
    s = new_state() if state is None else dict(state)
    ts = thermostat_ref.new_state() if thermostat is not None else None

    def th(t):
        if thermostat is None:
            return None
        kT = thermostat["kT"]
        return dict(kind=thermostat["kind"], kT=float(kT(t)) if callable(kT) else kT, tau=thermostat["tau"], seed=seed, timestep=t,
                    state=ts)

    Ks, Vs = [], []
    row = sums(v, mass)
    for n in range(steps):
        s = advance(row, L, S, dt, tauS, ndof, couple, box_dof, OPEN, s, th(t0 + n))
        if thermostat is not None:
            ts = s["thermostat_state"]
        L = [s["lam"][a] * L[a] for a in range(3)]
        c = np.array([s["alpha_T"] * s["alpha"][a] for a in range(3)])
        v = thermostat_ref.step_two(c[None, :] * v, mass, zero, dt)
        v = step_two(v, mass, zero, dt, s["alpha"])
        row = sums(v, mass)
        s = advance(row, L, S, dt, tauS, ndof, couple, box_dof, CLOSE, s, th(t0 + n + 1))
        Ks.append(s["K"])
        Vs.append(s["V"])
    return np.array(Ks), np.array(Vs), v, L, s, ts
