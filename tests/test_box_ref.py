"""tests/box_ref.py on the CPU: it reproduces the three restatements it replaced bit for bit on their own domains, leaves
every periodic fractional coordinate in [-0.5, 0.5), conserves the unwrapped position, never touches a non-periodic axis
-- and the seeded moves of tests/box_cases.py meet the conditions the GPU tests rely on."""

import numpy as np
import pytest

import box_cases
import box_ref
import fire_ref
import flow_ref
import thermostat_ref
import velocity_field_ref
import wall_ref

ULP_HALF = float(np.spacing(0.5))


# the restatements that tests/flow_ref.py, tests/wall_ref.py and tests/velocity_field_ref.py held before they became calls
# into box_ref, kept here as they were
def _former_flow_wrap(pos, image, L):
    pos, image = pos.copy(), image.copy()
    for d in range(3):
        hi = pos[:, d] >= 0.5 * L[d]
        lo = pos[:, d] < -0.5 * L[d]
        pos[hi, d] -= L[d]
        pos[lo, d] += L[d]
        image[:, d] += hi.astype(image.dtype) - lo.astype(image.dtype)
    return pos, image


def _former_wall_wrap(pos, L):
    x = np.array(pos, dtype=np.float64, copy=True)
    L = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,))
    for k in (2, 1, 0):
        h = 0.5 * L[k]
        hi = x[:, k] >= h
        lo = x[:, k] < -h
        x[hi, k] -= L[k]
        x[lo, k] += L[k]
    return x


def _former_velocity_field_wrap(xyz, L, tilt=(0.0, 0.0, 0.0), periodic=(True, True, True)):
    x, y, z = (np.array(xyz[:, k], dtype=np.float64) for k in range(3))
    Lx, Ly, Lz = (float(v) for v in L)
    xy, xz, yz = (float(v) for v in tilt)
    if periodic[2]:
        h = 0.5 * Lz
        up, dn = z >= h, z < -h
        z = np.where(up, z - Lz, np.where(dn, z + Lz, z))
        y = np.where(up, y - Lz * yz, np.where(dn, y + Lz * yz, y))
        x = np.where(up, x - Lz * xz, np.where(dn, x + Lz * xz, x))
    if periodic[1]:
        h, s = 0.5 * Ly, z * yz
        up, dn = y >= h + s, y < -h + s
        y = np.where(up, y - Ly, np.where(dn, y + Ly, y))
        x = np.where(up, x - Ly * xy, np.where(dn, x + Ly * xy, x))
    if periodic[0]:
        h, s = 0.5 * Lx, y * xy + z * (xz - xy * yz)
        x = np.where(x >= h + s, x - Lx, np.where(x < -h + s, x + Lx, x))
    return np.stack([x, y, z], axis=1)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def _cloud(rng, L, tilt, n, reach=0.95):
    """n positions up to ``reach`` box lengths from the centre along each lattice direction (one shift brings them back);
    in an untilted box six of them lie exactly on a face plane."""
    f = rng.uniform(-reach, reach, (n, 3))
    pos = f @ box_ref.box_matrix(L, tilt).T
    L = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,))
    if not any(tilt):
        for d in range(3):
            pos[d, d], pos[3 + d, d] = 0.5 * L[d], -0.5 * L[d]
    return pos


def test_matches_the_restatements_it_replaced():
    rng = np.random.default_rng(1)
    for L in ((6.0, 7.0, 8.0), (16.0, 16.0, 16.0), (12.0, 12.0, 12.0)):
        pos = _cloud(rng, L, (0, 0, 0), 20000)
        image = rng.integers(-3, 4, pos.shape).astype(np.int32)
        want_p, want_i = _former_flow_wrap(pos, image, L)
        for got_p, got_i in (box_ref.wrap(pos, image, L), flow_ref.wrap(pos, image, L)):
            assert np.array_equal(_bits(got_p), _bits(want_p)) and np.array_equal(got_i, want_i) and got_i.dtype == want_i.dtype
        assert (want_i != image).any(axis=1).sum() > 10000
        for Lw in (L, L[0]):  # (wall_ref takes one edge for a cube)
            want = _former_wall_wrap(pos, Lw)
            assert np.array_equal(_bits(wall_ref.wrap(pos, Lw)), _bits(want))
            assert np.array_equal(_bits(box_ref.wrap(pos, None, Lw)[0]), _bits(want))
    for tilt, periodic in (((0, 0, 0), (True, True, True)), ((0.2, -0.1, 0.15), (True, True, True)), ((0.5, 0.3, -0.4), (True, False, True)),
                           ((-0.35, 0.0, 0.0), (True, True, False)), ((0, 0, 0.45), (False, False, False))):
        L = (9.0, 8.0, 10.0)
        pos = _cloud(rng, L, tilt, 20000)
        want = _former_velocity_field_wrap(pos, L, tilt, periodic)
        assert np.array_equal(_bits(velocity_field_ref.wrap(pos, L, tilt, periodic)), _bits(want))
        assert np.array_equal(_bits(box_ref.wrap(pos, None, L, tilt, periodic)[0]), _bits(want))


def test_step_functions_default_to_the_orthorhombic_periodic_box():
    """The new ``tilt=`` and ``periodic=`` arguments of the per-kernel references default to what they computed before."""
    rng = np.random.default_rng(2)
    n, L, dt = 3000, (6.0, 7.0, 8.0), 0.05
    pos = rng.uniform(-0.5, 0.5, (n, 3)) * L
    vel, acc, force = rng.normal(0, 8, (n, 3)), rng.normal(0, 5, (n, 3)), rng.normal(0, 5, (n, 3))
    mass, image = rng.uniform(0.5, 2.0, n), rng.integers(-3, 4, (n, 3)).astype(np.int32)
    sel = np.ones(n, bool)
    hdt = 0.5 * dt
    p, v, im = thermostat_ref.step_one(pos, vel, mass, force, image, L, dt, 0.9)
    want = _former_flow_wrap(pos + dt * v, image, L)
    assert np.array_equal(_bits(p), _bits(want[0])) and np.array_equal(im, want[1]) and (im != image).any()
    s = dict(fire_ref.new_state(dt), keep=0.9, mix=0.03)
    p, v, im = fire_ref.step_one(pos, vel, mass, force, image, L, s)
    want = _former_flow_wrap(pos + dt * v, image, L)
    assert np.array_equal(_bits(p), _bits(want[0])) and np.array_equal(im, want[1])
    p, v, im = flow_ref.langevin_step_one(pos, vel, acc, image, L, dt, sel)
    want = _former_flow_wrap(pos + (vel + hdt * acc) * dt, image, L)
    assert np.array_equal(_bits(p), _bits(want[0])) and np.array_equal(im, want[1])
    gamma = np.full(n, 1.5)
    p, im = flow_ref.brownian_step(pos, image, force, np.arange(n), gamma, 1.0, dt, 1, 0, ("constant", (0.7, -0.3, 0.2)), True, L, sel)
    want = _former_flow_wrap(pos + (np.array([0.7, -0.3, 0.2]) + (force + 0.0) / gamma[:, None]) * dt, image, L)
    assert np.array_equal(_bits(p), _bits(want[0])) and np.array_equal(im, want[1])
    w = [dict(kind="plane", origin=(0.0, 0.0, -2.0), normal=(0.0, 0.0, 1.0))]
    prm = [dict(epsilon=1.0, sigma=1.0, r_cut=2.5, r_extrap=0.0)]
    far = pos * 1.3
    a = wall_ref.evaluate("lj93", w, prm, "shift", far, np.zeros(n, int), L)
    b = wall_ref.evaluate("lj93", w, prm, "shift", _former_wall_wrap(far, L), np.zeros(n, int), L)
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x), _bits(y))


def _random_boxes(rng, k):
    for _ in range(k):
        yield tuple(rng.uniform(4.0, 12.0, 3)), tuple(rng.uniform(-0.5, 0.5, 3))


def test_fractional_coordinates_after_a_wrap():
    """Every fractional coordinate of a periodic axis in [-0.5, 0.5) to 4 ulp(0.5), for random tilts in [-0.5, 0.5]^3."""
    rng = np.random.default_rng(3)
    boxes = [(L, t) for L, t, _ in box_cases.BOXES.values()] + list(_random_boxes(rng, 40))
    for L, tilt in boxes:
        for periodic in ((1, 1, 1), (1, 0, 1), (1, 1, 0), (0, 1, 1)):
            pos = _cloud(rng, L, tilt, 4000)
            f = box_ref.fractional(box_ref.wrap(pos, None, L, tilt, periodic)[0], L, tilt)
            for d in range(3):
                if periodic[d]:
                    assert f[:, d].min() >= -0.5 - 4 * ULP_HALF and f[:, d].max() < 0.5 + 4 * ULP_HALF, (L, tilt, periodic, d)


def test_unwrapped_position_is_conserved():
    """unwrapped(wrap(pos, image)) = unwrapped(pos, image) to 4 ulp(L_max) in every component."""
    rng = np.random.default_rng(4)
    worst = 0.0
    for L, tilt in _random_boxes(rng, 60):
        pos = _cloud(rng, L, tilt, 4000)
        image = rng.integers(-3, 4, pos.shape).astype(np.int32)
        p, im = box_ref.wrap(pos, image, L, tilt)
        assert (im != image).all(axis=1).sum() > 100  # corners are crossed
        # (pos - p) is the shift: compare it with H (im - image), both of the size of the box, not of the unwrapped position
        d = (p - pos) + (im - image).astype(np.float64) @ box_ref.box_matrix(L, tilt).T
        bound = 4 * float(np.spacing(max(L)))
        worst = max(worst, np.abs(d).max() / bound)
        assert np.abs(d).max() <= bound, (L, tilt)
        u0, u1 = box_ref.unwrapped(pos, image, L, tilt), box_ref.unwrapped(p, im, L, tilt)
        assert np.abs(u1 - u0).max() <= 4 * float(np.spacing(np.abs(u0).max()))
    print("largest change of the unwrapped position: %.2f of the bound" % worst)


def test_a_non_periodic_axis_is_never_shifted():
    rng = np.random.default_rng(5)
    L, tilt = (6.0, 7.0, 8.0), (0.5, 0.3, -0.4)
    pos = _cloud(rng, L, tilt, 20000)
    image = rng.integers(-3, 4, pos.shape).astype(np.int32)
    for periodic in ((1, 0, 1), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 0, 0)):
        p, im = box_ref.wrap(pos, image, L, tilt, periodic)
        for d in range(3):
            if not periodic[d]:
                assert np.array_equal(im[:, d], image[:, d])
        if not periodic[2]:
            assert np.array_equal(_bits(p[:, 2]), _bits(pos[:, 2]))
        if not periodic[2] and not periodic[1]:
            assert np.array_equal(_bits(p[:, 1]), _bits(pos[:, 1]))
        if not any(periodic):
            assert np.array_equal(_bits(p), _bits(pos))
    # periodic = (1, 0, 1): y is not wrapped and its counter stays, but a z shift still carries Lz yz into y
    p, im = box_ref.wrap(pos, image, L, tilt, (1, 0, 1))
    dz = im[:, 2] - image[:, 2]
    assert (dz != 0).sum() > 1000 and np.array_equal(im[:, 1], image[:, 1])
    want_y = np.where(dz > 0, pos[:, 1] - L[2] * tilt[2], np.where(dz < 0, pos[:, 1] + L[2] * tilt[2], pos[:, 1]))
    assert np.array_equal(_bits(p[:, 1]), _bits(want_y))
    assert np.abs(box_ref.fractional(p, L, tilt)[:, 1]).max() > 0.5  # (and some do stay outside in y)


@pytest.mark.parametrize("box_id", list(box_cases.BOXES))
@pytest.mark.parametrize("N", [box_cases.N_LARGE, box_cases.N_SMALL])
def test_seeded_moves(box_id, N):
    """What tests/test_gpu_box_wrap.py needs of its inputs, for the committed seed: starts inside the box, moves of at most
    0.45 of an edge per lattice direction, images in [-3, 3], no end point within 1e-9 (fractional) of a face and, at
    N = 5000, every shift combination of the box at least 20 times."""
    L, tilt, periodic = box_cases.BOXES[box_id]
    m = box_cases.moves(box_id, N)
    f0 = box_ref.fractional(m["pos"], L, tilt)
    assert np.abs(f0).max() < 0.5 and m["image"].min() == -3 and m["image"].max() == 3
    assert np.abs(box_ref.fractional(m["disp"], L, tilt)).max() <= box_cases.MAX_MOVE + 1e-12
    end = m["pos"] + m["disp"]
    assert box_cases.face_distance(end, L, tilt, periodic) > box_cases.FACE_MARGIN
    _, im = box_ref.wrap(end, m["image"], L, tilt, periodic)
    counts = box_cases.shift_counts(im - m["image"], periodic)
    assert len(counts) == 3 ** sum(periodic)
    if N == box_cases.N_LARGE:
        assert min(counts.values()) >= box_cases.MIN_PER_COMBINATION, counts
