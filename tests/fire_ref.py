"""numpy / plain-Python restatement of ``minimize.FIRE`` (csrc/fire.hip, include/azp.h): the four sums in
the device's order, the measure pass, step two, the advance and step one, and a ``minimize`` loop that drives them with a
host force function.

vel (N, 3), mass (N,), force (N, 3), energy (N,) (each particle's share of the potential energy, ``net_force.w``),
pos (N, 3), image (N, 3) int. The control state is a dict keyed by the lower-case names of the AZP_FIRE_* slots."""

import math

import numpy as np

import flow_ref
import reduction_ref

SLOTS = ("dt", "alpha", "keep", "mix", "n_pos", "n_steps", "u", "u_prev", "p", "vv", "ff", "converged", "nonfinite")
NSTATE = 16
DEFAULTS = dict(min_steps_adapt=5, finc_dt=1.1, fdec_dt=0.5, alpha_start=0.1, fdec_alpha=0.99, min_steps_conv=10)

# Largest relative deviation of the device's MIX from this restatement that the tests allow: 8 times the largest
# deviation measured on the MI355X over the grid of tests/test_gpu_fire.py (advance_grid).
# Measured on the MI355X (gfx950): 0.0. Over all 11,684 cases of the grid MIX, and every other slot of the state, came
# out bit for bit as here: the advance uses + * / sqrt min alone, which the device rounds correctly as the host does. So
# ADVANCE_REL is 0 and the tests hold the advance, and with it whole trajectories, to bit equality. DT, ALPHA, KEEP, the
# counters and the flags have to match bit for bit regardless of this constant.
ADVANCE_REL_MEASURED = 0.0
ADVANCE_REL = 8 * ADVANCE_REL_MEASURED


def new_state(dt, alpha_start=DEFAULTS["alpha_start"]):
    s = dict.fromkeys(SLOTS, 0.0)
    s.update(dt=float(dt), alpha=float(alpha_start), keep=1.0)
    return s


def to_array(state):
    """The state as the device lays it out (AZP_FIRE_NSTATE doubles, unused slots 0)."""
    out = np.zeros(NSTATE)
    for k, name in enumerate(SLOTS):
        out[k] = state[name]
    return out


def from_array(arr):
    return {name: float(arr[k]) for k, name in enumerate(SLOTS)}


# ---------------------------------------------------------------------------
# the sums
# ---------------------------------------------------------------------------
def terms(vel, force, energy):
    """The per-particle terms of P, VV, FF, U, (4, N), each in the order the header states."""
    v, f = np.asarray(vel, dtype=np.float64), np.asarray(force, dtype=np.float64)
    return np.stack([((f[:, 0] * v[:, 0]) + (f[:, 1] * v[:, 1])) + (f[:, 2] * v[:, 2]),
                     ((v[:, 0] * v[:, 0]) + (v[:, 1] * v[:, 1])) + (v[:, 2] * v[:, 2]),
                     ((f[:, 0] * f[:, 0]) + (f[:, 1] * f[:, 1])) + (f[:, 2] * f[:, 2]),
                     np.asarray(energy, dtype=np.float64)])


def measure(vel, force, energy):
    """(P, VV, FF, U) in the order of the device's two-stage sum, the four slots summed independently."""
    with np.errstate(invalid="ignore", over="ignore"):
        return tuple(float(x) for x in reduction_ref.tree_sum(terms(vel, force, energy)))


def step_two(vel, mass, force, energy, state):
    """v + ((DT / 2) f) (1 / m) and the sums of the new v; untouched, with sums None, when a flag is set."""
    if state["converged"] or state["nonfinite"]:
        return vel, None
    hdt = 0.5 * state["dt"]
    minv = 1.0 / np.asarray(mass, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = vel + (hdt * force) * minv[:, None]
    return v, measure(v, force, energy)


def advance(sums, state, N, dt_max, force_tol, energy_tol, min_steps_adapt=5, finc_dt=1.1, fdec_dt=0.5, alpha_start=0.1,
            fdec_alpha=0.99, min_steps_conv=10):
    """One advance on the sums (P, VV, FF, U): the new state (``state`` is not changed)."""
    s = dict(state)
    if s["converged"] or s["nonfinite"]:
        return s
    P, VV, FF, U = (float(x) for x in sums)
    if not all(math.isfinite(x) for x in (P, VV, FF, U)):
        s.update(nonfinite=1.0, keep=0.0, mix=0.0)
        return s
    s.update(p=P, vv=VV, ff=FF, u=U)
    n = float(N)
    if s["n_steps"] >= max(1, min_steps_conv) and math.sqrt(FF / (3.0 * n)) < force_tol and abs(U - s["u_prev"]) / n < energy_tol:
        s.update(converged=1.0, keep=0.0, mix=0.0)
        return s
    dt, alpha, n_pos = s["dt"], s["alpha"], s["n_pos"]
    keep = 1.0 - alpha
    mix = alpha * (math.sqrt(VV) / math.sqrt(FF)) if FF > 0.0 else 0.0
    if P > 0.0:
        n_pos = n_pos + 1.0
        if n_pos > min_steps_adapt:
            dt = min(dt * finc_dt, dt_max)
            alpha = alpha * fdec_alpha
    else:
        dt, alpha, n_pos, keep, mix = dt * fdec_dt, alpha_start, 0.0, 0.0, 0.0
    s.update(dt=dt, alpha=alpha, keep=keep, mix=mix, n_pos=n_pos, u_prev=U, n_steps=s["n_steps"] + 1.0)
    return s


def step_one(pos, vel, mass, force, image, L, state, tilt=(0.0, 0.0, 0.0), periodic=(1, 1, 1)):
    """v = (KEEP v) + (MIX f); v += ((DT / 2) f) (1 / m); x += DT v; wrap. Returns (pos, vel, image); untouched when a
    flag is set."""
    if state["converged"] or state["nonfinite"]:
        return pos, vel, image
    dt = state["dt"]
    hdt = 0.5 * dt
    minv = 1.0 / np.asarray(mass, dtype=np.float64)
    v = (state["keep"] * vel) + (state["mix"] * force)
    v = v + (hdt * force) * minv[:, None]
    p, im = flow_ref.wrap(pos + dt * v, image, L, tilt, periodic)
    return p, v, im


def force_rms(state, N):
    return math.sqrt(state["ff"] / (3.0 * N))


def minimize(force_fn, pos, vel, mass, L, dt, force_tol, energy_tol, steps, image=None, state=None, record=None, **params):
    """Drives the four passes as the driver does: measure, then per step advance, step one, forces, step two.
    ``force_fn(pos)`` returns (force (N, 3), energy (N,)). Stops after ``steps`` steps or at convergence, whichever
    comes first (``stop_at_convergence``: the device's loop goes on and moves nothing). ``record(k, pos, vel, state)``
    is called after step two of step k (0-based). Returns (pos, vel, image, state, steps taken)."""
    stop = params.pop("stop_at_convergence", True)
    pos, vel = np.array(pos, dtype=np.float64), np.array(vel, dtype=np.float64)
    N = pos.shape[0]
    image = np.zeros((N, 3), dtype=np.int32) if image is None else np.array(image)
    s = new_state(dt, params.get("alpha_start", DEFAULTS["alpha_start"])) if state is None else dict(state)
    f, e = force_fn(pos)
    sums = measure(vel, f, e)
    taken = 0
    for k in range(steps):
        s = advance(sums, s, N, dt, force_tol, energy_tol, **params)
        if stop and (s["converged"] or s["nonfinite"]):
            break
        pos, vel, image = step_one(pos, vel, mass, f, image, L, s)
        f, e = force_fn(pos)
        vel, new = step_two(vel, mass, f, e, s)
        sums = new if new is not None else sums
        taken = k + 1
        if record is not None:
            record(k, pos, vel, s)
    return pos, vel, image, s, taken
