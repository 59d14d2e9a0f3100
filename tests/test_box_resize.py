"""``update.BoxResize`` without a GPU: the scalar variants and the box variants against their closed forms, the host
matrix M = H_new H_old^-1, the numpy reference of the kernel (tests/box_resize_ref.py) and the conditions its seeded
cases have to meet, the C ABI's struct and argument checks, ``State.box`` and the refusals that need no device."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import azplugins_amd as azp
import box_ref
import box_resize_ref as ref
from azplugins_amd import _lib, update, variant
from azplugins_amd.state import Box

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -- scalar variants (hoomd.variant) ---------------------------------------------------------------------------------
def test_constant():
    v = variant.Constant(2.5)
    assert [v(t) for t in (0, 1, 10**12)] == [2.5] * 3 and v.min == v.max == 2.5
    assert v == variant.Constant(2.5) and v != variant.Constant(2.0) and "2.5" in repr(v)


def test_ramp_at_before_and_after_its_break_points():
    v = variant.Ramp(A=1.0, B=3.0, t_start=100, t_ramp=40)
    assert v(0) == v(99) == v(100) == 1.0          # A up to and at t_start
    assert v(101) == 1.0 * (1.0 - 1 / 40) + 3.0 * (1 / 40)
    assert v(120) == 2.0
    assert v(139) == 1.0 * (1.0 - 39 / 40) + 3.0 * (39 / 40)
    assert v(140) == v(141) == v(10**9) == 3.0     # B from t_start + t_ramp on
    assert (v.min, v.max) == (1.0, 3.0) and (variant.Ramp(3.0, 1.0, 0, 5).min, variant.Ramp(3.0, 1.0, 0, 5).max) == (1.0, 3.0)
    assert v == variant.Ramp(1.0, 3.0, 100, 40) and v != variant.Ramp(1.0, 3.0, 100, 41)
    assert repr(v) == "Ramp(A=1.0, B=3.0, t_start=100, t_ramp=40)"
    for bad in (dict(t_ramp=0), dict(t_ramp=-1), dict(t_ramp=2.5), dict(t_start=-1), dict(A=float("nan"))):
        with pytest.raises(azp.AzpError):
            variant.Ramp(**dict(dict(A=0.0, B=1.0, t_start=0, t_ramp=10), **bad))


def test_cycle_at_before_and_after_its_break_points():
    v = variant.Cycle(A=1.0, B=5.0, t_start=10, t_A=4, t_AB=8, t_B=2, t_BA=4)  # period 18
    for t0 in (10, 28, 10 + 18 * 1000):
        assert v(t0) == v(t0 + 3) == 1.0                       # A for t_A steps
        assert v(t0 + 4) == 1.0                                # the ramp starts at A
        assert v(t0 + 5) == 5.0 * (1 / 8) + 1.0 * (1.0 - 1 / 8)
        assert v(t0 + 8) == 3.0
        assert v(t0 + 11) == 5.0 * (7 / 8) + 1.0 * (1.0 - 7 / 8)
        assert v(t0 + 12) == v(t0 + 13) == 5.0                 # B for t_B steps
        assert v(t0 + 14) == 5.0                               # the ramp back starts at B
        assert v(t0 + 15) == 1.0 * (1 / 4) + 5.0 * (1.0 - 1 / 4)
        assert v(t0 + 17) == 1.0 * (3 / 4) + 5.0 * (1.0 - 3 / 4)
    assert v(0) == v(9) == 1.0
    assert (v.min, v.max) == (1.0, 5.0)
    assert v == variant.Cycle(1.0, 5.0, 10, 4, 8, 2, 4) and v != variant.Cycle(1.0, 5.0, 10, 4, 8, 2, 5)
    assert repr(v).startswith("Cycle(A=1.0, B=5.0, t_start=10")
    for bad in (dict(t_AB=0), dict(t_BA=0), dict(t_A=-1)):
        with pytest.raises(azp.AzpError):
            variant.Cycle(**dict(dict(A=0.0, B=1.0, t_start=0, t_A=1, t_AB=1, t_B=1, t_BA=1), **bad))


def test_power_at_before_and_after_its_break_points():
    v = variant.Power(A=2.0, B=8.0, power=3, t_start=50, t_ramp=10)
    assert v(0) == v(49) == v(50) == 2.0
    for t in (51, 55, 59):
        s = (t - 50) / 10
        assert v(t) == (8.0 ** (1 / 3) * s + 2.0 ** (1 / 3) * (1.0 - s)) ** 3.0
    assert v(55) == pytest.approx((0.5 * 2.0 + 0.5 * 2.0 ** (1 / 3)) ** 3, rel=1e-14)
    assert v(60) == v(61) == 8.0
    assert (v.min, v.max) == (2.0, 8.0) and v == variant.Power(2.0, 8.0, 3, 50, 10) and "power=3.0" in repr(v)
    for bad in (dict(power=0), dict(A=-1.0), dict(t_ramp=0)):
        with pytest.raises(azp.AzpError):
            variant.Power(**dict(dict(A=1.0, B=2.0, power=2, t_start=0, t_ramp=10), **bad))


def test_sphere_area_is_still_there():
    assert variant.SphereArea(10.0, 0.5)(0) == 10.0 and variant.box is azp.variant.box


# -- box variants (hoomd.variant.box) --------------------------------------------------------------------------------
def _six(b):
    return (b.Lx, b.Ly, b.Lz, b.xy, b.xz, b.yz)


def test_box_equality():
    a = Box(6.0, 7.0, 8.0, 0.1, 0.2, 0.3)
    assert a == Box(6.0, 7.0, 8.0, 0.1, 0.2, 0.3) and not a != Box(6.0, 7.0, 8.0, 0.1, 0.2, 0.3)
    for other in (Box(6.5, 7.0, 8.0, 0.1, 0.2, 0.3), Box(6.0, 7.0, 8.0, 0.1, 0.2, 0.31),
                  Box(6.0, 7.0, 8.0, 0.1, 0.2, 0.3, periodic=(1, 1, 0)), (6.0, 7.0, 8.0)):
        assert a != other
    assert a.volume == 6.0 * 7.0 * 8.0
    assert len({a, Box(6.0, 7.0, 8.0, 0.1, 0.2, 0.3)}) == 2  # (mutable: hashed by identity)


def test_box_constant():
    b = Box(6.0, 7.0, 8.0, 0.1, 0.0, 0.0)
    v = variant.box.Constant(b)
    assert v(0) == v(10**9) == b and v == variant.box.Constant(Box(6.0, 7.0, 8.0, 0.1, 0.0, 0.0))
    assert variant.box.Constant([6.0, 7.0, 8.0])(3) == Box(6.0, 7.0, 8.0)


def test_interpolate_at_s_0_at_s_1_and_in_between():
    a, b = Box(10.0, 11.0, 12.0, 0.0, 0.1, -0.2), Box(9.0, 11.0, 13.0, 0.4, 0.1, 0.3)
    v = variant.box.Interpolate(a, b, variant.Ramp(2.0, 6.0, 10, 20))  # (s from the variant's min and max, not 0 and 1)
    assert v.scale(0) == v.scale(10) == 0.0 and v.scale(30) == v.scale(31) == 1.0 and v.scale(15) == 0.25
    assert v(0) == a and v(10) == a and _six(v(10)) == _six(a)   # s = 0: the initial box, to the bit
    assert v(30) == b and v(1000) == b                            # s = 1: the final box, to the bit
    for t in (11, 15, 20, 29):
        s = (variant.Ramp(2.0, 6.0, 10, 20)(t) - 2.0) / 4.0
        assert _six(v(t)) == tuple(x * (1.0 - s) + y * s for x, y in zip(_six(a), _six(b)))
    assert _six(v(20)) == pytest.approx((9.5, 11.0, 12.5, 0.2, 0.1, 0.05), abs=1e-15)
    # a variant that never moves: s = 0
    assert variant.box.Interpolate(a, b, variant.Constant(3.0))(7) == a
    # a falling variant runs the interpolation backwards
    assert variant.box.Interpolate(a, b, variant.Ramp(1.0, 0.0, 0, 10))(0) == b
    assert v == variant.box.Interpolate(a, b, variant.Ramp(2.0, 6.0, 10, 20)) and v != variant.box.Interpolate(a, b, variant.Ramp(2.0, 6.0, 10, 21))
    assert v(15).periodic == a.periodic
    with pytest.raises(azp.AzpError, match="periodic"):
        variant.box.Interpolate(a, Box(9.0, periodic=(1, 1, 0)), variant.Ramp(0, 1, 0, 1))
    with pytest.raises(azp.AzpError, match="scalar variant"):
        variant.box.Interpolate(a, b, 0.5)


def test_inverse_volume_ramp_is_linear_in_the_inverse_volume_and_keeps_the_tilts():
    a = Box(10.0, 12.0, 14.0, 0.3, -0.1, 0.2, periodic=(1, 1, 0))
    v0, v1 = a.volume, 500.0
    v = variant.box.InverseVolumeRamp(a, v1, t_start=100, t_ramp=50)
    assert v(0) == a and v(100) == a
    for t in (0, 99, 100, 101, 110, 125, 149, 150, 151, 10**6):
        s = min(max((t - 100) / 50, 0.0), 1.0)
        b = v(t)
        assert 1.0 / b.volume == pytest.approx((1.0 - s) / v0 + s / v1, rel=1e-14)  # (a cube root, a cube and two divisions: a few eps)
        assert (b.xy, b.xz, b.yz) == (a.xy, a.xz, a.yz) and b.periodic == a.periodic
        f = (b.volume / v0) ** (1.0 / 3.0)
        assert (b.Lx / a.Lx, b.Ly / a.Ly, b.Lz / a.Lz) == pytest.approx((f, f, f), rel=1e-15)
    assert v(150).volume == pytest.approx(v1, rel=1e-15) and v(150) == v(10**6)
    assert v == variant.box.InverseVolumeRamp(a, 500.0, 100, 50) and v != variant.box.InverseVolumeRamp(a, 501.0, 100, 50)
    for bad in (dict(final_volume=0.0), dict(final_volume=float("inf")), dict(t_ramp=0), dict(initial_box=Box(10.0, 10.0, 0.0))):
        with pytest.raises(azp.AzpError):
            variant.box.InverseVolumeRamp(**dict(dict(initial_box=a, final_volume=500.0, t_start=0, t_ramp=10), **bad))


# -- M = H_new H_old^-1 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair_id", sorted(ref.ALL_PAIRS))
def test_matrix_is_upper_triangular_and_h_new_times_the_inverse_of_h_old(pair_id):
    """numpy inverts H_old by LU decomposition: a relative error of about cond(H_old) eps in the inverse, and another few eps
    for the product. cond(H) of these boxes is below 4 (edges within a factor 1.5, tilts of at most 0.5), the entries of M
    are at most 1.1: 64 eps = 1.4e-14 absolute is an order of magnitude of room, and six orders below what a wrong
    formula would give."""
    old, new = ref.ALL_PAIRS[pair_id]
    M = ref.matrix(old, new)
    assert M[1, 0] == M[2, 0] == M[2, 1] == 0.0
    h_old, h_new = box_ref.box_matrix(old[0], old[1]), box_ref.box_matrix(new[0], new[1])
    assert np.linalg.cond(h_old) < 4.0 and np.abs(M).max() <= 1.1
    assert np.abs(M - h_new @ np.linalg.inv(h_old)).max() <= 64 * np.finfo(np.float64).eps
    six = update.box_resize_matrix(ref.as_box(old), ref.as_box(new))
    assert six == (M[0, 0], M[0, 1], M[0, 2], M[1, 1], M[1, 2], M[2, 2])


def test_matrix_of_an_axis_that_does_not_change_is_exact():
    old, new = ref.PAIRS["ortho_to_xy"]
    assert update.box_resize_matrix(ref.as_box(old), ref.as_box(new)) == (1.0, 0.4, 0.0, 1.0, 0.0, 1.0)
    b = ref.as_box(ref.PAIRS["tilt3_to_tilt3"][0])
    m = update.box_resize_matrix(b, b)
    assert (m[0], m[3], m[5]) == (1.0, 1.0, 1.0) and max(abs(m[1]), abs(m[2]), abs(m[4])) <= 2 ** -52


# -- the reference and its cases -------------------------------------------------------------------------------------
CASES = [(p, 1037, False) for p in ref.PAIRS] + [(p, 1037, True) for p in ref.SHRUNK] + [("tilt3_to_tilt3", 1, False), ("tilt3_x0.3", 1, True)]


@pytest.mark.parametrize("pair_id,N,masked", CASES)
def test_reference_preserves_fractional_coordinates_and_cases_meet_their_conditions(pair_id, N, masked):
    old, new = ref.ALL_PAIRS[pair_id]
    c = ref.case(pair_id, N, masked)
    pos, image, sel = ref.resize(c["pos"], c["image"], c["typeid"], ref.MASK if masked else None, old, new)
    # what the GPU comparison rests on
    assert ref.face_distance(pos, new) > ref.FACE_MARGIN
    assert np.abs(c["pos"]).max() < 16.0 and np.abs(pos).max() < 16.0
    if N > 1:
        counts = ref.near_face_counts(pos, new)
        assert counts and min(counts.values()) >= ref.MIN_NEAR, counts
        assert sel.sum() > N // 5 and (masked and (~sel).sum() > N // 2 or not masked and sel.all())
    # a selected row keeps its fractional coordinates (up to whole images along the periodic axes)
    f0, f1 = box_ref.fractional(c["pos"], old[0], old[1]), box_ref.fractional(pos, new[0], new[1])
    d = (f1 - f0)[sel]
    for k in range(3):
        if new[2][k]:
            d[:, k] -= np.rint(d[:, k])
    assert np.abs(d).max() <= 1e-14 if sel.any() else True
    # every row: in the box, and unwrapped(pos, image) is the unwrapped position of the moved row
    for k in range(3):
        if new[2][k]:
            assert f1[:, k].min() >= -0.5 and f1[:, k].max() < 0.5
        else:
            assert np.array_equal(image[:, k], c["image"][:, k])
    moved = np.where(sel[:, None], ref.affine(c["pos"], ref.matrix(old, new)), c["pos"])
    shift = (image - c["image"]).astype(np.float64) @ box_ref.box_matrix(new[0], new[1]).T
    assert np.abs(pos + shift - moved).max() <= 8 * np.spacing(16.0)
    if masked and N > 1:
        assert np.abs(image - c["image"])[~sel].max() == 2  # rows that kept their position needed two shifts
        assert np.abs(image - c["image"])[sel].max() == 1


def test_multi_wrap_is_wrap_for_rows_less_than_one_image_outside():
    import box_cases

    for box_id in ("tilt3", "tilt_xy_slab", "tilt3_inexact"):
        L, tilt, periodic = box_cases.BOXES[box_id]
        m = box_cases.moves(box_id)
        want = box_ref.wrap(m["pos"] + m["disp"], m["image"], L, tilt, periodic)
        got = ref.multi_wrap(m["pos"] + m["disp"], m["image"], (L, tilt, periodic))
        assert np.array_equal(got[1], want[1]) and np.abs(got[0] - want[0]).max() <= 4 * np.spacing(16.0)


# -- C ABI -----------------------------------------------------------------------------------------------------------
def test_args_struct_matches_the_header(tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   'sizeof(azp_box_resize_args), offsetof(azp_box_resize_args, d_type_mask), offsetof(azp_box_resize_args, M), '
                   'offsetof(azp_box_resize_args, box)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    A = _lib.BoxResizeArgs
    assert got == [C.sizeof(A), A.d_type_mask.offset, A.M.offset, A.box.offset]
    assert "azp_box_resize" in _lib.SYMBOLS


def test_entry_point_refuses_bad_arguments_and_returns_at_once_for_no_particles():
    lib = _lib.lib()
    a = _lib.BoxResizeArgs()
    a.box = _lib.make_box((6.0, 7.0, 8.0))
    a.M[:] = (1.0, 0.0, 0.0, 1.0, 0.0, 1.0)
    assert lib.azp_box_resize(None, None) == -1
    assert lib.azp_box_resize(C.byref(a), None) == 0       # N = 0: success, no launch, no array needed
    a.N = 4
    assert lib.azp_box_resize(C.byref(a), None) == -1      # no positions
    a.d_pos = 256                                           # (never dereferenced: every call below is refused first)
    for bad_L in (0.0, -1.0, float("nan"), float("inf")):
        a.box = _lib.make_box((6.0, bad_L, 8.0))
        assert lib.azp_box_resize(C.byref(a), None) == -1
    a.box = _lib.make_box((6.0, 7.0, 8.0), (0.0, float("nan"), 0.0))
    assert lib.azp_box_resize(C.byref(a), None) == -1
    a.box = _lib.make_box((6.0, 7.0, 8.0))
    for bad_m in (float("nan"), float("inf")):
        a.M[2] = bad_m
        assert lib.azp_box_resize(C.byref(a), None) == -1
    a.M[2] = 0.0
    for bad_bs in (32, 100, 512):
        a.block_size = bad_bs
        assert lib.azp_box_resize(C.byref(a), None) == -1
    a.block_size = 0
    a.d_type_mask, a.ntypes = 256, 0
    assert lib.azp_box_resize(C.byref(a), None) == -1      # a mask of no types


# -- State.box -------------------------------------------------------------------------------------------------------
class _BareState(azp.State):
    """A ``State`` without its device arrays: what ``State.box`` touches."""

    def __init__(self, box):
        self._box = Box.from_box(box)
        self.position_generation = self.order_generation = self.type_generation = self.box_generation = 0
        self.types = ["A", "B", "C"]
        self.N, self.n_ghost = 0, 0
        self.device = "cuda:0"


def test_assigning_the_box_bumps_the_generations_and_an_equal_box_changes_nothing():
    st = _BareState(Box(10.0))
    b0 = st.box
    st.box = Box(10.0, 10.0, 10.0)          # equal in all six numbers and the flags
    st.set_box([10.0, 10.0, 10.0])
    assert st.box is b0 and (st.box_generation, st.position_generation) == (0, 0)
    st.box = Box(9.0)
    assert st.box == Box(9.0) and (st.box_generation, st.position_generation) == (1, 1)
    st.set_box(Box(9.0, xy=0.1))
    assert st.box.xy == 0.1 and (st.box_generation, st.position_generation) == (2, 2)
    st.set_box(Box(9.0, xy=0.1, periodic=(1, 1, 0)))  # the flags count
    assert st.box_generation == 3
    assert st.type_generation == st.order_generation == 0


def test_list_and_steppers_look_at_the_box_generation():
    import inspect

    from azplugins_amd import nlist, simulation, state

    assert "box_generation" in inspect.getsource(state.State.__init__)
    for fn in (nlist.Cell.compute, nlist.Cell.allows_speculative_launch, nlist.Cell._build, simulation._launch):
        assert "box_generation" in inspect.getsource(fn)


# -- the run loop ----------------------------------------------------------------------------------------------------
def test_only_updaters_that_change_types_bump_the_type_generation():
    from azplugins_amd.evaporate import ParticleEvaporator

    assert update._Updater._changes_types and update.TypeUpdater._changes_types and ParticleEvaporator._changes_types
    assert not update.BoxResize._changes_types
    calls = []

    class Quiet(update._Updater):
        _changes_types = False

        def _update(self, sim, timestep):
            calls.append(("quiet", timestep))

    class Loud(update._Updater):
        def _update(self, sim, timestep):
            calls.append(("loud", timestep))

    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.state = _BareState(Box(10.0))
    sim.timestep = 7
    sim._run_updaters([Quiet(1)])
    assert sim.state.type_generation == 0 and calls == [("quiet", 7)]
    sim._run_updaters([Quiet(1), Loud(1)])
    assert sim.state.type_generation == 1
    sim._run_updaters([])
    assert sim.state.type_generation == 1


# -- refusals that need no device ------------------------------------------------------------------------------------
def _resizer(**kw):
    args = dict(trigger=5, box=variant.box.Constant(Box(9.0)))
    args.update(kw)
    return update.BoxResize(**args)


def test_box_resize_properties():
    u = _resizer()
    assert u.trigger == azp.Periodic(5) and isinstance(u.filter, azp.All) and isinstance(u, update._Updater)
    assert _resizer(filter=azp.Type("B")).filter == azp.Type(["B"])
    with pytest.raises(azp.AzpError, match="filter"):
        _resizer(filter="B")
    with pytest.raises(azp.AzpError, match="variant.box"):
        _resizer(box=Box(9.0))
    sim = azp.Simulation(device="cuda:0", seed=1)
    sim.operations.add(u)
    assert sim.operations.updaters == [u]


class _Sim:
    def __init__(self, state, domain=None):
        self.state, self.domain, self.timestep = state, domain, 0


def test_refused_in_a_decomposed_run():
    with pytest.raises(azp.AzpError, match="decomposed"):
        _resizer()._update(_Sim(_BareState(Box(10.0)), domain=object()), 0)
    st = _BareState(Box(10.0))
    st.n_ghost = 3
    with pytest.raises(azp.AzpError, match="decomposed"):
        update.BoxResize.update(st, Box(9.0))


def test_refused_periodic_flags_that_differ():
    st = _BareState(Box(10.0))
    with pytest.raises(azp.AzpError, match="periodic flags"):
        update.BoxResize.update(st, Box(9.0, periodic=(1, 1, 0)))
    with pytest.raises(azp.AzpError, match="periodic flags"):
        _resizer(box=variant.box.Constant(Box(9.0, periodic=(0, 1, 1))))._update(_Sim(st), 0)
    assert st.box == Box(10.0) and st.box_generation == 0


@pytest.mark.parametrize("edge", [0.0, -3.0, float("nan"), float("inf")])
def test_refused_an_edge_that_is_not_positive_and_finite(edge):
    st = _BareState(Box(10.0))
    with pytest.raises(azp.AzpError, match="not positive and finite"):
        update.BoxResize.update(st, Box(9.0, edge, 9.0))
    with pytest.raises(azp.AzpError, match="not finite"):
        update.BoxResize.update(st, Box(9.0, xz=float("nan")))
    with pytest.raises(azp.AzpError, match="2-D"):
        update.BoxResize.update(_BareState(Box(10.0, 10.0, 0.0)), Box(9.0, 9.0, 1.0))
    assert st.box_generation == 0


def test_refused_a_type_the_state_lacks():
    st = _BareState(Box(10.0))
    with pytest.raises(azp.AzpError, match="does not have"):
        update.BoxResize.update(st, Box(9.0), filter=azp.Type("Z"))
    with pytest.raises(azp.AzpError, match="does not have"):
        _resizer(filter=azp.Type(["A", "Z"]))._update(_Sim(st), 0)
    assert st.box_generation == 0
