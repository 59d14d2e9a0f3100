"""``wrap_with_image`` (csrc/azp_device.hpp) through every kernel that moves particles, in tilted and partly periodic
boxes, against tests/box_ref.py: the seven entry points of SETUPS below, called through the C ABI with the seeded moves of
tests/box_cases.py -- every shift combination a box allows at least 20 times, no end point within 1e-9 (fractional) of a
face, so that the kernel (whose tilted shifts are FMAs) and numpy (a product and a sum) must take the same branch.

Per kernel and box: the image counters equal the reference exactly; rows that were not shifted hold what the
orthorhombic test of that kernel pins (the bits for the thermostat and FIRE, tests/test_gpu_flow.py's ``_assert_close``
for the flow methods, 1e-11 as in test_nve_steps_match_oracle for NVE); every row agrees within BOUND; and, without the
reference's wrap, the unwrapped position is the pre-wrap position within BOUND and the periodic fractional coordinates
lie in [-0.5, 0.5).

BOUND = 3.6e-15 absolute per component: a tilted shift is one FMA in the kernel and a multiply plus an add in numpy, at
most 1 ulp of the result apart per shift, and x takes at most three shifts. Coordinates stay below 16 before the wrap
and below 8 after it in these boxes, so that is 4 ulp of a wrapped coordinate, 4 * 8.9e-16, or 2 ulp of the largest
pre-wrap one. Where the arithmetic before the wrap contracts as well (NVE and the flow methods: x + dt v is one FMA)
the same budget has to hold that rounding too. Measured on the MI355X (profiles/box_wrap.md): 0 for the thermostat and
FIRE wherever the products Lz yz, Lz xz, Ly xy are exact, 8.9e-16 in tilt_xy_slab, at most 1.8e-15 for NVE and the flow
methods; in tilt3_inexact, which has a bound of its own (BOUND_OF), 1.8e-15 and 2.7e-15."""

import ctypes as C

import numpy as np
import pytest

import box_cases
import box_ref
import fire_ref
import flow_ref
import test_gpu_fire as tfire
import test_gpu_flow as tflow
import test_gpu_thermostat as tthermo
import thermostat_ref
from azplugins_amd import _lib
from box_cases import BOXES

pytestmark = pytest.mark.gpu

BOUND = 3.6e-15
# tilt3_inexact: all three products round, and the intermediate x lies above 8 for some rows, where 1 ulp is 1.8e-15: four
# roundings (three shifts, and x + dt v where that is an FMA) of that size. (In the other boxes at most one product rounds.)
BOUND_OF = {b: BOUND for b in BOXES}
BOUND_OF["tilt3_inexact"] = 4 * float(np.spacing(8.0))
ULP_HALF = float(np.spacing(0.5))
DT = 0.05  # displacements of up to 0.45 of an edge: velocities of up to about 70
NVE_UNSHIFTED = 1e-11  # what test_nve_steps_match_oracle holds the positions to


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _call(name, a):
    _lib.check(getattr(_lib.lib(), name)(C.byref(a), _lib.raw_stream("cuda:0")), name)


def _type_w(typeid):
    return np.asarray(typeid).astype(np.int64).view(np.float64)


def _host(tensors, names):
    import torch

    torch.cuda.synchronize()
    return {k: tensors[k].cpu().numpy().copy() for k in names}


class _Setup:
    """One kernel on one set of moves: ``launch(cbox, entries, with_image)`` runs the entries in turn on fresh device
    arrays and returns the host copies (pos and vel with their w); ``reference(tilt, periodic)`` the numpy result (pos
    (N, 3), vel (N, 3), image, accel or None). ``selected``: the rows the kernel integrates."""

    exact = False  # the arithmetic before the wrap is pinned bit for bit by the kernel's orthorhombic test
    entries = ()

    def __init__(self, m, L):
        self.m, self.L, self.N = m, L, m["pos"].shape[0]
        self.selected = np.ones(self.N, bool)

    def unshifted(self, got, want):
        raise NotImplementedError


class _NVE(_Setup):
    kicks = 1
    entries = ("azp_integrate_nve_step_one",)

    def __init__(self, m, L):
        super().__init__(m, L)
        self.minv = 1.0 / m["mass"]
        self.vel = m["disp"] / DT - self.kicks * ((0.5 * DT) * m["force"]) * self.minv[:, None]
        self.type_w = _type_w(m["typeid"])

    def launch(self, cbox, entries=None, with_image=True):
        m = self.m
        t = dict(pos=_dev(np.c_[m["pos"], self.type_w]), vel=_dev(np.c_[self.vel, m["mass"]]),
                 frc=_dev(np.c_[m["force"], np.arange(self.N, dtype=np.float64)]), image=_dev(np.array(m["image"])))
        a = _lib.NVEArgs()
        a.d_pos, a.d_vel, a.d_net_force = t["pos"].data_ptr(), t["vel"].data_ptr(), t["frc"].data_ptr()
        a.d_image = t["image"].data_ptr() if with_image else None
        a.box, a.dt, a.N = cbox, DT, self.N
        for e in (entries or self.entries):
            _call(e, a)
        return _host(t, ("pos", "vel", "image"))

    def reference(self, tilt, periodic):
        """v += ((dt / 2) f) (1 / m), once or twice; x += dt v; wrap (nve_kernel, csrc/external_forces.hip)."""
        m, v = self.m, self.vel
        for _ in range(self.kicks):
            v = v + ((0.5 * DT) * m["force"]) * self.minv[:, None]
        p, im = box_ref.wrap(m["pos"] + DT * v, m["image"], self.L, tilt, periodic)
        return dict(pos=p, vel=v, image=im, mass=m["mass"], type_w=self.type_w)

    def unshifted(self, got, want):
        assert np.abs(got - want).max() <= NVE_UNSHIFTED


class _NVETwoOne(_NVE):
    kicks = 2
    entries = ("azp_integrate_nve_step_two_one",)
    split = ("azp_integrate_nve_step_two", "azp_integrate_nve_step_one")


class _Thermostat(_Setup):
    exact = True
    entries = ("azp_thermostat_step_one",)
    ALPHA = 0.9

    def __init__(self, m, L):
        super().__init__(m, L)
        # masses, forces and types as the thermostat's own tests draw them; positions, velocities and images from the moves
        self.p = p = tthermo._Particles(self.N, seed=3000 + self.N % 97)
        p.pos, p.image = np.array(m["pos"]), np.array(m["image"])
        p.vel = (m["disp"] / DT - ((0.5 * DT) * p.force) * (1.0 / p.mass)[:, None]) / self.ALPHA

    def launch(self, cbox, entries=None, with_image=True):
        p = self.p
        p.d_pos, p.d_vel, p.d_image = tthermo._dev(np.c_[p.pos, p.type_w]), tthermo._dev(np.c_[p.vel, p.mass]), tthermo._dev(p.image)
        p.d_state[_lib.THERMOSTAT_ALPHA] = self.ALPHA  # (what azp_thermostat_advance would have left)
        a = p.args(dt=DT)
        a.box = cbox
        if not with_image:
            a.d_image = None
        for e in (entries or self.entries):
            tthermo._call(e, a)
        return _host(dict(pos=p.d_pos, vel=p.d_vel, image=p.d_image), ("pos", "vel", "image"))

    def reference(self, tilt, periodic):
        p = self.p
        pos, vel, im = thermostat_ref.step_one(p.pos, p.vel, p.mass, p.force, p.image, self.L, DT, self.ALPHA, tilt, periodic)
        return dict(pos=pos, vel=vel, image=im, mass=p.mass, type_w=p.type_w)

    def unshifted(self, got, want):
        np.testing.assert_array_equal(_bits(got), _bits(want))


class _Fire(_Setup):
    exact = True
    entries = ("azp_fire_step_one",)

    def __init__(self, m, L):
        super().__init__(m, L)
        self.state = s = dict(fire_ref.new_state(DT), keep=0.9, mix=0.03, dt=DT)
        self.p = p = tfire._Particles(self.N, seed=3000 + self.N % 97, L=L, pos=m["pos"])
        p.image = np.array(m["image"])
        p.vel = (m["disp"] / DT - ((0.5 * DT) * p.force) * (1.0 / p.mass)[:, None] - s["mix"] * p.force) / s["keep"]

    def launch(self, cbox, entries=None, with_image=True):
        p = self.p
        p.d_pos, p.d_vel, p.d_image = tfire._dev(np.c_[p.pos, p.type_w]), tfire._dev(np.c_[p.vel, p.mass]), tfire._dev(p.image)
        p.set_state(self.state)
        a = p.args()
        a.box = cbox
        if not with_image:
            a.d_image = None
        for e in (entries or self.entries):
            tfire._call(e, a)
        return _host(dict(pos=p.d_pos, vel=p.d_vel, image=p.d_image), ("pos", "vel", "image"))

    def reference(self, tilt, periodic):
        p = self.p
        pos, vel, im = fire_ref.step_one(p.pos, p.vel, p.mass, p.force, p.image, self.L, self.state, tilt, periodic)
        return dict(pos=pos, vel=vel, image=im, mass=p.mass, type_w=p.type_w)

    def unshifted(self, got, want):
        np.testing.assert_array_equal(_bits(got), _bits(want))


class _Flow(_Setup):
    """A constant flow without noise; types 0 and 1 are selected, type 2 is not."""

    U = (0.7, -0.3, 0.2)
    GAMMA = np.array([1.5, 0.7, 2.0])
    MASK = np.array([1, 1, 0], dtype=np.uint8)
    KT, SEED, TIMESTEP = 1.2, 5, 7

    def __init__(self, m, L):
        super().__init__(m, L)
        self.selected = self.MASK[m["typeid"]].astype(bool)
        self.gamma = self.GAMMA[m["typeid"]]
        self.type_w = _type_w(m["typeid"])
        self.tag = np.arange(self.N, dtype=np.uint32)
        self.accel = np.random.default_rng(self.N).normal(0.0, 5.0, (self.N, 3))
        self.force = np.array(m["force"])
        self.vel = self._velocities()

    def launch(self, cbox, entries=None, with_image=True):
        m = self.m
        t = dict(pos=_dev(np.c_[m["pos"], self.type_w]), vel=_dev(np.c_[self.vel, m["mass"]]),
                 accel=_dev(np.c_[self.accel, np.full(self.N, 9.0)]), frc=_dev(np.c_[self.force, np.arange(self.N, dtype=np.float64)]),
                 image=_dev(np.array(m["image"])), tag=_dev(self.tag.view(np.int32)), gamma=_dev(self.GAMMA), mask=_dev(self.MASK))
        a = _lib.FlowMethodArgs()
        a.d_pos, a.d_vel, a.d_accel, a.d_net_force = t["pos"].data_ptr(), t["vel"].data_ptr(), t["accel"].data_ptr(), t["frc"].data_ptr()
        a.d_image = t["image"].data_ptr() if with_image else None
        a.d_tag, a.d_gamma, a.d_type_mask = t["tag"].data_ptr(), t["gamma"].data_ptr(), t["mask"].data_ptr()
        a.box, a.dt, a.kT, a.timestep, a.seed, a.noiseless = cbox, DT, self.KT, self.TIMESTEP, self.SEED, 1
        a.N, a.ntypes = self.N, 3
        a.flow.kind = _lib.FLOW_CONSTANT
        for k in range(3):
            a.flow.p[k] = self.U[k]
        for e in (entries or self.entries):
            _call(e, a)
        return _host(t, ("pos", "vel", "image", "accel"))

    def unshifted(self, got, want):
        tflow._assert_close(got, want, "positions of the rows that were not shifted")


class _LangevinOne(_Flow):
    entries = ("azp_integrate_langevin_flow_step_one",)

    def _velocities(self):
        return self.m["disp"] / DT - (0.5 * DT) * self.accel

    def reference(self, tilt, periodic):
        m = self.m
        pos, vel, im = flow_ref.langevin_step_one(m["pos"], self.vel, self.accel, m["image"], self.L, DT, self.selected, tilt, periodic)
        return dict(pos=pos, vel=vel, image=im, accel=self.accel, mass=m["mass"], type_w=self.type_w)


class _LangevinTwoOne(_Flow):
    entries = ("azp_integrate_langevin_flow_step_two_one",)
    split = ("azp_integrate_langevin_flow_step_two", "azp_integrate_langevin_flow_step_one")

    def _velocities(self):
        # x - x0 = dt (v + dt a) with a = (f - gamma (v - U)) / m, solved for v
        m, g = self.m, self.gamma[:, None]
        minv = (1.0 / m["mass"])[:, None]
        return (m["disp"] / DT - DT * (self.force + g * np.array(self.U)) * minv) / (1.0 - DT * g * minv)

    def reference(self, tilt, periodic):
        m = self.m
        v1, a1 = flow_ref.langevin_step_two(m["pos"], self.vel, m["mass"], self.accel, self.force, self.tag, self.gamma, self.KT, DT,
                                            self.SEED, self.TIMESTEP, ("constant", self.U), True, self.selected)
        pos, vel, im = flow_ref.langevin_step_one(m["pos"], v1, a1, m["image"], self.L, DT, self.selected, tilt, periodic)
        return dict(pos=pos, vel=vel, image=im, accel=a1, mass=m["mass"], type_w=self.type_w)


class _Brownian(_Flow):
    entries = ("azp_integrate_brownian_flow_step",)

    def _velocities(self):
        # x - x0 = dt (U + f / gamma): the move is in the force; the velocities are not read
        self.force = self.gamma[:, None] * (self.m["disp"] / DT - np.array(self.U))
        return np.random.default_rng(self.N + 1).normal(0.0, 8.0, (self.N, 3))

    def reference(self, tilt, periodic):
        m = self.m
        pos, im = flow_ref.brownian_step(m["pos"], m["image"], self.force, self.tag, self.gamma, self.KT, DT, self.SEED, self.TIMESTEP,
                                         ("constant", self.U), True, self.L, self.selected, tilt, periodic)
        return dict(pos=pos, vel=self.vel, image=im, accel=self.accel, mass=m["mass"], type_w=self.type_w)


SETUPS = {"nve_step_one": _NVE, "nve_step_two_one": _NVETwoOne, "thermostat_step_one": _Thermostat, "fire_step_one": _Fire,
          "langevin_flow_step_one": _LangevinOne, "langevin_flow_step_two_one": _LangevinTwoOne, "brownian_flow_step": _Brownian}
CASES = [(k, b, box_cases.N_LARGE) for k in SETUPS for b in BOXES] + [(k, "tilt3", box_cases.N_SMALL) for k in SETUPS]


def _cbox(box_id):
    L, tilt, periodic = BOXES[box_id]
    return _lib.make_box(L, tilt, periodic)


@pytest.mark.parametrize("kernel,box_id,N", CASES)
def test_wrap_and_images(kernel, box_id, N):
    L, tilt, periodic = BOXES[box_id]
    m = box_cases.moves(box_id, N)
    s = SETUPS[kernel](m, L)
    sel = s.selected
    want = s.reference(tilt, periodic)
    pre = s.reference(tilt, (0, 0, 0))  # the same step without the wrap: the pre-wrap positions
    assert np.array_equal(pre["image"], m["image"])
    # the conditions the comparison rests on, from the reference alone
    margin = box_cases.face_distance(pre["pos"][sel], L, tilt, periodic)
    assert margin > box_cases.FACE_MARGIN, margin
    assert np.abs(pre["pos"]).max() < 16.0 and np.abs(box_ref.fractional(pre["pos"] - m["pos"], L, tilt)).max() < 0.5
    shift = want["image"] - m["image"]
    counts = box_cases.shift_counts(shift[sel], periodic)
    assert not shift[~sel].any()
    if N == box_cases.N_LARGE:
        assert min(counts.values()) >= box_cases.MIN_PER_COMBINATION, counts
    got = s.launch(_cbox(box_id))
    # 1. the counters, exactly
    np.testing.assert_array_equal(got["image"], want["image"])
    # 2. the rows that were not shifted: what the kernel's orthorhombic test pins
    moved = shift.any(axis=1)
    still = sel & ~moved
    assert still.sum() >= 3
    s.unshifted(got["pos"][still, :3], want["pos"][still])
    # 3. every row within BOUND
    dev = np.abs(got["pos"][:, :3] - want["pos"])
    bound = BOUND_OF[box_id]
    print("%s %s N=%d: %d rows shifted (every combination >= %d times), %d not; largest deviation of a shifted row %.3e, of any row "
          "%.3e (bound %.3e); nearest face %.2e" % (kernel, box_id, N, int(moved.sum()), min(counts.values()), int(still.sum()),
                                                    dev[moved].max(), dev.max(), bound, margin))
    assert dev.max() <= bound
    # 4. what the kernel must not touch, and the velocities
    np.testing.assert_array_equal(_bits(got["pos"][:, 3]), _bits(want["type_w"]))
    np.testing.assert_array_equal(_bits(got["vel"][:, 3]), _bits(want["mass"]))
    if s.exact or kernel == "brownian_flow_step":
        np.testing.assert_array_equal(_bits(got["vel"][:, :3]), _bits(want["vel"]))
    else:
        tflow._assert_close(got["vel"][:, :3], want["vel"], "velocities")
    if "accel" in got:
        np.testing.assert_array_equal(_bits(got["pos"][~sel, :3]), _bits(m["pos"][~sel]))
        np.testing.assert_array_equal(_bits(got["vel"][~sel, :3]), _bits(s.vel[~sel]))
        np.testing.assert_array_equal(_bits(got["accel"][~sel, :3]), _bits(s.accel[~sel]))
        assert (~sel).sum() > N // 5 and np.all(got["accel"][~sel, 3] == 9.0)
        tflow._assert_close(got["accel"][sel, :3], want["accel"][sel], "accelerations")
    # 5. without the reference's wrap: the shift the kernel applied is H times the change of its counters, and the
    # particle is back in the box. (The difference is taken of the shifts, which are of the size of the box, not of the
    # unwrapped positions, whose images of up to 4 would cost the comparison its last digits.)
    d_image = (got["image"] - m["image"]).astype(np.float64)
    unwrapped_change = (got["pos"][:, :3] - pre["pos"]) + d_image @ box_ref.box_matrix(L, tilt).T
    assert np.abs(unwrapped_change[sel]).max() <= bound, np.abs(unwrapped_change[sel]).max()
    f = box_ref.fractional(got["pos"][sel, :3], L, tilt)
    for d in range(3):
        if periodic[d]:
            assert f[:, d].min() >= -0.5 - 4 * ULP_HALF and f[:, d].max() < 0.5 + 4 * ULP_HALF, d
        else:
            assert not d_image[:, d].any()


def test_without_image_counters():
    """d_image = NULL: the same positions and velocities, bit for bit."""
    L, tilt, periodic = BOXES["tilt3"]
    s = _NVE(box_cases.moves("tilt3"), L)
    a, b = s.launch(_cbox("tilt3")), s.launch(_cbox("tilt3"), with_image=False)
    assert np.array_equal(_bits(a["pos"]), _bits(b["pos"])) and np.array_equal(_bits(a["vel"]), _bits(b["vel"]))
    assert np.array_equal(b["image"], s.m["image"]) and not np.array_equal(a["image"], s.m["image"])


@pytest.mark.parametrize("kernel", ["nve_step_two_one", "langevin_flow_step_two_one"])
def test_fused_entry_is_its_two_calls(kernel):
    """azp_*_step_two_one leaves the bits that step two followed by step one leave, image counters included."""
    L, tilt, periodic = BOXES["tilt3"]
    s = SETUPS[kernel](box_cases.moves("tilt3"), L)
    fused, two = s.launch(_cbox("tilt3")), s.launch(_cbox("tilt3"), entries=s.split)
    for k in fused:
        assert np.array_equal(fused[k].view(np.int32), two[k].view(np.int32)), k
    assert (fused["image"] != s.m["image"]).any(axis=1).sum() > box_cases.N_LARGE // 2


# ---------------------------------------------------------------------------------------------------------------------
# through Simulation.run: 512 particles in the tilt3 box, 400 steps
# ---------------------------------------------------------------------------------------------------------------------
RUN_N, RUN_STEPS = 512, 400
RUN_BOUND = RUN_STEPS * 2 * BOUND  # per step one rounding for the add and one per shift, eight at 8.9e-16 (see BOUND)


def _tilt3_box():
    import azplugins_amd as azp

    L, tilt, _ = BOXES["tilt3"]
    return azp.Box(L[0], L[1], L[2], *tilt)


def _free_flight(velocity, make_integrator):
    """RUN_STEPS steps without forces from uniform positions: (x0, unwrapped positions after the run, images)."""
    import azplugins_amd as azp

    L, tilt, _ = BOXES["tilt3"]
    rng = np.random.default_rng(404)
    x0 = rng.uniform(-0.5, 0.5, (RUN_N, 3)) @ box_ref.box_matrix(L, tilt).T
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.create_state_from_snapshot(azp.Snapshot.from_arrays(x0, _tilt3_box(), velocity=velocity(rng)))
    sim.operations.tuners.clear()  # rows are compared by index
    sim.operations.integrator = make_integrator(azp)
    sim.run(RUN_STEPS)
    st = sim.state
    pos, image = st.pos[:RUN_N, :3].cpu().numpy(), st.image[:RUN_N].cpu().numpy()
    f = box_ref.fractional(pos, L, tilt)
    assert f.min() >= -0.5 - 4 * ULP_HALF and f.max() < 0.5 + 4 * ULP_HALF
    # every particle crossed many faces, along every axis
    assert np.all((image != 0).sum(axis=0) > RUN_N // 2) and np.abs(image).max() > 10, np.abs(image).max(axis=0)
    return x0, box_ref.unwrapped(pos, image, L, tilt), image


def test_nve_free_flight_keeps_the_unwrapped_trajectory():
    """ConstantVolume without forces, dt |v| of 1 to 1.4 (0.2 of an edge): unwrapped(pos, image) = x0 + v t."""
    dt = 0.05
    vel = {}

    def velocity(rng):
        u = rng.normal(size=(RUN_N, 3))
        vel["v"] = u / np.linalg.norm(u, axis=1)[:, None] * rng.uniform(20.0, 28.0, (RUN_N, 1))
        return vel["v"]

    x0, got, image = _free_flight(velocity, lambda azp: azp.Integrator(dt=dt, forces=[], methods=[azp.ConstantVolume()]))
    dev = np.abs(got - (x0 + vel["v"] * (RUN_STEPS * dt))).max()
    print("NVE free flight: largest deviation of the unwrapped position %.3e (bound %.3e), largest image %d" % (dev, RUN_BOUND, np.abs(image).max()))
    assert dev <= RUN_BOUND


def test_brownian_constant_flow_keeps_the_unwrapped_trajectory():
    """flow.Brownian without noise and forces in a constant flow U: unwrapped(pos, image) = x0 + U t."""
    from azplugins_amd import flow

    dt, U = 0.05, (17.0, -14.0, 12.0)  # dt |U| = 1.25
    x0, got, image = _free_flight(lambda rng: rng.normal(size=(RUN_N, 3)), lambda azp: azp.Integrator(dt=dt, methods=[flow.Brownian(
        filter=azp.All(), kT=1.0, flow_field=flow.ConstantFlow(velocity=U), default_gamma=1.0, noiseless=True)]))
    dev = np.abs(got - (x0 + np.array(U) * (RUN_STEPS * dt))).max()
    print("Brownian constant flow: largest deviation of the unwrapped position %.3e (bound %.3e), largest image %d"
          % (dev, RUN_BOUND, np.abs(image).max()))
    assert dev <= RUN_BOUND


def test_bonded_chains_conserve_energy_to_second_order():
    """32 chains of 16 (tests/dihedral_cases.py's random chain, as in tests/test_gpu_bonded.py) with DoubleWell bonds in
    their well at r_0 -- the project has no harmonic bond; U_1 (1 - x^2)^2 is harmonic there with k = 8 U_1 / (r_1 -
    r_0)^2 = 640 -- in the tilt3 box, drifting through its faces, NVE over the same time with dt = 0.004 and 0.002. The
    largest |E(t) - E(0)| falls by 4 for a second-order integrator: the ratio is held to 4 within 20 % on either side.
    No bond ever exceeds half the smallest perpendicular width of the box (the minimum image of its two ends is the
    bond)."""
    import azplugins_amd as azp
    import dihedral_cases

    L, tilt, _ = BOXES["tilt3"]
    xy, xz, yz = tilt
    half_width = 0.5 * min(L[2], L[1] / np.sqrt(1.0 + yz * yz), L[0] / np.sqrt(1.0 + xy * xy + (xy * yz - xz) ** 2))
    h = box_ref.box_matrix(L, tilt)
    chains, length = 32, 16
    rng = np.random.default_rng(1604)
    xyz = np.concatenate([dihedral_cases.random_chain(rng, rng.uniform(-0.5, 0.5, 3) @ h.T, length) for _ in range(chains)])
    xyz = dihedral_cases.wrap(xyz, L, tilt)
    bonds = np.array([(c * length + i, c * length + i + 1) for c in range(chains) for i in range(length - 1)])
    vel = rng.normal(0.0, 0.5, (RUN_N, 3)) + np.repeat(rng.normal(0.0, 2.0, (chains, 3)), length, axis=0)  # chains drift
    assert xyz.shape == (RUN_N, 3)

    def longest_bond(pos):
        f = box_ref.fractional(pos[bonds[:, 1]] - pos[bonds[:, 0]], L, tilt)
        return float(np.linalg.norm((f - np.rint(f)) @ h.T, axis=1).max())

    drift, longest, crossed = {}, 0.0, 0
    for dt, every in ((0.004, 10), (0.002, 20)):
        sim = azp.Simulation(device="cuda:0", seed=1)
        sim.create_state_from_snapshot(azp.Snapshot.from_arrays(xyz, _tilt3_box(), velocity=vel, bonds=bonds))
        sim.operations.tuners.clear()
        dw = azp.bond.DoubleWell()
        dw.params["A-A"] = dict(r_0=1.0, r_1=1.5, U_1=20.0, U_tilt=0.0)
        sim.operations.integrator = azp.Integrator(dt=dt, forces=[dw], methods=[azp.ConstantVolume()])

        def total():
            v = sim.state.vel[:RUN_N].cpu().numpy()
            return dw.energy + 0.5 * float((v[:, 3] * (v[:, :3] ** 2).sum(axis=1)).sum())

        sim.run(0)
        E = [total()]
        for _ in range(20):  # 200 steps of 0.004, RUN_STEPS of 0.002
            sim.run(every)
            E.append(total())
            longest = max(longest, longest_bond(sim.state.pos[:RUN_N, :3].cpu().numpy()))
        assert sim.timestep * dt == pytest.approx(0.8)
        drift[dt] = float(np.abs(np.array(E) - E[0]).max())
        crossed = int((sim.state.image[:RUN_N].cpu().numpy() != 0).any(axis=1).sum())
        assert crossed > RUN_N // 8  # the chains did pass through the faces
    ratio = drift[0.004] / drift[0.002]
    print("bonded chains in tilt3: |dE| %.3e at dt = 0.004, %.3e at dt = 0.002, ratio %.3f; longest bond %.3f of %.3f; %d particles crossed"
          % (drift[0.004], drift[0.002], ratio, longest, half_width, crossed))
    assert longest <= half_width
    assert 4.0 / 1.2 < ratio < 4.8
