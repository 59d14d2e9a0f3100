"""angle.Table and dihedral.Table, host side (no GPU): what the parameter class refuses when a value is set, the
reference module (tests/bonded_table_ref.py) against itself, and the error returns of the two C entries."""

import ctypes as C
import math

import numpy as np
import pytest

import azplugins_amd as azp
import bonded_table_ref as R
from azplugins_amd import _lib
from azplugins_amd.force import BondedTableTypeParameter

CLASSES = (azp.angle.Table, azp.dihedral.Table)


@pytest.mark.parametrize("cls", CLASSES)
def test_parameter_class_refuses_at_assignment(cls):
    f = cls()
    assert isinstance(f.params, BondedTableTypeParameter)
    good = dict(U=[0.0, 1.0, 4.0], tau=[0.0, -2.0, -4.0])
    f.params["T"] = good
    back = f.params["T"]
    assert set(back) == {"U", "tau"} and np.array_equal(back["U"], good["U"]) and np.array_equal(back["tau"], good["tau"])
    back["U"][0] = 99.0                                   # a copy: the table is not edited in place
    assert f.params["T"]["U"][0] == 0.0
    for what, bad in (("unequal lengths", dict(U=[0.0, 1.0, 2.0], tau=[0.0, 1.0])),
                      ("fewer than 2 samples", dict(U=[0.0], tau=[0.0])),
                      ("no samples", dict(U=[], tau=[])),
                      ("a NaN in U", dict(U=[0.0, math.nan], tau=[0.0, 1.0])),
                      ("an infinity in tau", dict(U=[0.0, 1.0], tau=[0.0, math.inf])),
                      ("a missing key", dict(U=[0.0, 1.0])),
                      ("F in the place of tau", dict(U=[0.0, 1.0], F=[0.0, 1.0])),
                      ("a key too many", dict(U=[0.0, 1.0], tau=[0.0, 1.0], r_min=0.0)),
                      ("a two-dimensional array", dict(U=[[0.0, 1.0]], tau=[[0.0, 1.0]]))):
        with pytest.raises(ValueError):
            f.params["T"] = bad
        assert np.array_equal(f.params["T"]["U"], good["U"]), what   # the refused value left the old one in place
    with pytest.raises(KeyError):
        f.params["unset"]
    # width is per type: 2 samples next to 257
    f.params["S"] = dict(U=np.zeros(2), tau=np.zeros(2))
    f.params["L"] = dict(U=np.zeros(257), tau=np.zeros(257))
    assert len(f.params["S"]["U"]) == 2 and len(f.params["L"]["tau"]) == 257


def test_classes_and_docstrings():
    assert issubclass(azp.angle.Table, azp.angle.Angle) and issubclass(azp.dihedral.Table, azp.dihedral.Dihedral)
    assert azp.angle.Table._entry == "azp_angle_forces_table" and azp.dihedral.Table._entry == "azp_dihedral_forces_table"
    assert "Table" in azp.angle.__all__ and "Table" in azp.dihedral.__all__
    for module in (azp.angle, azp.dihedral):
        scope = module.__doc__[module.__doc__.index("Out of scope"):]
        assert "tabulated" not in scope.lower()
    with pytest.raises(azp.AzpError):
        azp.angle.Table().forces                       # not attached


def test_knots_and_end_points():
    U = np.array([3.0, 1.0, 4.0, 1.5, 9.0])
    tau = np.array([-1.0, 2.0, 0.5, -3.0, 7.0])
    table = dict(U=U, tau=tau)
    assert np.allclose(R.angle_knots(5), [0.0, math.pi / 4, math.pi / 2, 3 * math.pi / 4, math.pi], rtol=0, atol=1e-15)
    assert R.dihedral_knots(5)[0] == -math.pi and abs(R.dihedral_knots(5)[-1] - math.pi) < 1e-15
    for k, theta in enumerate(R.angle_knots(5)):
        got = R.angle_table(table, theta)
        assert abs(got[0] - U[k]) < 1e-14 and abs(got[1] - tau[k]) < 1e-14
    assert R.angle_table(table, math.pi) == (9.0, 7.0)          # theta == pi: the clamp gives the last knot
    assert R.dihedral_table(table, math.pi) == (9.0, 7.0)       # phi = +pi reads the last knot,
    assert R.dihedral_table(table, -math.pi) == (3.0, -1.0)     # phi = -pi the first
    assert R.dihedral_table(table, 0.0) == (4.0, 0.5)
    mid = R.angle_table(table, 0.5 * (R.angle_knots(5)[1] + R.angle_knots(5)[2]))
    assert abs(mid[0] - 2.5) < 1e-14 and abs(mid[1] - 1.25) < 1e-14


@pytest.mark.parametrize("kind", ["angle", "dihedral"])
def test_force_is_minus_the_slope_of_the_tabulated_energy(kind):
    """Inside an interval the tabulated energy is linear; a table whose tau is the slope of that very polygon
    (tau = -(U_{k+1} - U_k) / h on both knots of the interval) gives, in the reference, a force that is minus the
    centred finite difference of the tabulated energy. Checked through the whole reference path: one group, moved
    along each coordinate of each member, in the interior of an interval."""
    width = 9
    x = R.angle_knots(width) if kind == "angle" else R.dihedral_knots(width)
    h = x[1] - x[0]
    U = 2.0 * np.cos(1.3 * x) + 0.3 * x
    if kind == "angle":
        pos = np.array([[1.0, 0.1, 0.0], [0.0, 0.0, 0.0], [-0.2, 0.9, 0.3]])
        group, evaluate = [(0, 1, 2)], R.evaluate_angles
    else:
        pos = np.array([[1.0, 0.1, 0.0], [0.0, 0.0, 0.0], [0.1, 0.0, 1.0], [0.6, 0.7, 1.2]])
        group, evaluate = [(0, 1, 2, 3)], R.evaluate_dihedrals
    L = (20.0, 20.0, 20.0)
    x0 = evaluate([dict(U=U, tau=np.zeros(width))], pos, group, [0], L)["x"][0]
    k = int((x0 - x[0]) / h)
    assert min(x0 - x[k], x[k + 1] - x0) > 0.05 * h               # in the interior of interval k
    slope = (U[k + 1] - U[k]) / h
    tau = np.zeros(width)
    tau[k] = tau[k + 1] = -slope
    table = [dict(U=U, tau=tau)]
    out = evaluate(table, pos, group, [0], L)
    eps = 1e-6
    for i in range(pos.shape[0]):
        for c in range(3):
            plus, minus = pos.copy(), pos.copy()
            plus[i, c] += eps
            minus[i, c] -= eps
            fd = -(evaluate(table, plus, group, [0], L)["energy"] - evaluate(table, minus, group, [0], L)["energy"]) / (2.0 * eps)
            assert abs(out["force"][i, c] - fd) < 1e-8 * max(1.0, abs(slope)), (i, c, out["force"][i, c], fd)
    assert np.abs(out["force"]).max() > 0.1 and np.abs(out["force"].sum(axis=0)).max() < 1e-14


def test_reference_reproduces_the_analytic_harmonic_angle():
    """U = k/2 (theta - t0)^2 tabulated: tau = -k (theta - t0) is linear, so its interpolation is exact and the forces
    are angle_ref's Harmonic forces to rounding; the energy is off by at most k h^2 / 8 per angle."""
    import angle_cases
    import angle_ref

    k, t0, width = 10.0, 2.0, 65
    h = math.pi / (width - 1)
    table = R.sample("angle", width, lambda t: 0.5 * k * (t - t0) ** 2, lambda t: -k * (t - t0))
    xyz, angles, typeid, L, tilt = angle_cases.parity_system("triclinic")
    angles, typeid = angles[:60], np.zeros(60, dtype=np.int64)
    want = angle_ref.evaluate("Harmonic", [dict(k=k, t0=t0)], xyz, angles, typeid, L, tilt)
    got = R.evaluate_angles([table], xyz, angles, typeid, L, tilt)
    assert np.abs(got["force"] - want["force"]).max() < 1e-12 * np.abs(want["force"]).max()
    assert np.all(got["U"] >= want["U"] - 1e-13) and np.abs(got["U"] - want["U"]).max() <= k * h * h / 8.0 * (1.0 + 1e-12)


# ---------------------------------------------------------------------------
# the C entries, without a device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("entry,args", [("azp_angle_forces_table", _lib.AngleArgs), ("azp_dihedral_forces_table", _lib.DihedralArgs)])
def test_c_entries_refuse_null_and_accept_no_particles(entry, args):
    fn = getattr(_lib.lib(), entry)
    bad = -1  # AZP_ERROR_INVALID_ARGUMENT
    assert fn(None, None, None) == bad
    a = args()
    assert fn(C.byref(a), None, None) == 0      # N == 0: success before any array is looked at
    a.N = 4
    assert fn(C.byref(a), None, None) == bad    # NULL tables, NULL parameters
    params = np.zeros(4)
    assert fn(C.byref(a), params.ctypes.data, None) == bad   # still no table, no positions, no force array
