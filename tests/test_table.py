"""Tabulated potentials, host side (no GPU): azp_table_pack against the numpy restatement bit for bit, the restatement
against the analytic potential it tabulates within the linear-interpolation bound, the argument errors of pair.Table
and bond.Table, and the size of azp_table_params."""

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import azplugins_amd as azp
import helpers as H
import table_ref as R
from azplugins_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pack(r_min, r_end, U, F, closed):
    """azp_table_pack through the raw binding: (status, rows)."""
    U = np.ascontiguousarray(U, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.float64)
    rows = np.full((max(len(U) - (1 if closed else 0), 1), 4), np.nan)
    rc = _lib.lib().azp_table_pack(r_min, r_end, U.ctypes.data, F.ctypes.data, len(U), int(closed), rows.ctypes.data)
    return rc, rows


@pytest.mark.parametrize("width,closed", [(1, False), (2, False), (7, False), (2, True), (7, True)])
def test_table_pack_bits(width, closed):
    """The library's rows equal the restatement's bit for bit; the pair form folds the zero at the cutoff into its last
    row, the bond form stores both end points in width - 1 rows."""
    U = R.smooth_curve(11 + width, width, 3.0) + 0.1
    F = R.smooth_curve(12 + width, width, 50.0) - 0.3
    rc, rows = _pack(0.5, 2.5, U, F, closed)
    assert rc == 0
    ref = R.pack_rows(U, F, closed)
    assert ref.shape == (width - 1 if closed else width, 4)
    assert np.array_equal(rows.view(np.uint64), ref.view(np.uint64))
    if not closed:
        assert np.array_equal(rows[-1], [U[-1], 0.0 - U[-1], F[-1], 0.0 - F[-1]])
    else:
        assert np.array_equal(rows[-1], [U[-2], U[-1] - U[-2], F[-2], F[-1] - F[-2]])
    assert np.array_equal(_lib.table_pack(0.5, 2.5, U, F, closed).view(np.uint64), ref.view(np.uint64))


def test_table_pack_refuses_bad_input():
    U, F = np.arange(4.0), np.arange(4.0)
    nan = U.copy()
    nan[2] = np.nan
    inf = F.copy()
    inf[0] = np.inf
    for args in ((0.5, 0.5, U, F, False), (1.0, 0.5, U, F, False), (-0.1, 1.0, U, F, False), (0.0, np.inf, U, F, True),
                 (0.5, 1.0, nan, F, False), (0.5, 1.0, U, inf, True), (0.5, 1.0, U[:1], F[:1], True),
                 (0.5, 1.0, U[:0], F[:0], False)):
        rc, rows = _pack(*args)
        assert rc == -1 and np.all(np.isnan(rows)), args
    lib = _lib.lib()
    out = np.zeros((4, 4))
    assert lib.azp_table_pack(0.5, 1.0, None, F.ctypes.data, 4, 0, out.ctypes.data) == -1
    assert lib.azp_table_pack(0.5, 1.0, U.ctypes.data, F.ctypes.data, 4, 0, None) == -1
    assert _pack(0.0, 1.0, U, F, False)[0] == 0  # r_min = 0 is allowed


# ---------------------------------------------------------------------------
# the restatement against the potential it tabulates
# ---------------------------------------------------------------------------
PLJ = dict(epsilon=1.0, sigma=1.0, attraction_scale_factor=0.5)
R_MIN, R_CUT, WIDTH = 0.8, 3.0, 4096


def test_restatement_against_analytic_potential(oracle):
    """PerturbedLJ tabulated on [0.8, 3.0) at width 4096, summed by the restatement, against the oracle's analytic sum
    over the same list.

    Bound, per pair: linear interpolation of a function g with bounded second derivative on an interval of length dr
    is off by at most dr^2 / 8 max |g''|. With epsilon = sigma = 1, lambda <= 1 and U = 4 (r^-12 - r^-6) scaled by 1 in
    the WCA core and by lambda in the tail (U and U' are continuous at the joint, so the bound holds across it with
    the larger second derivative):
        |U''(r)|  <= 4 (156 r^-14 + 42 r^-8),   |F''(r)| = |U'''(r)| <= 4 (2184 r^-15 + 336 r^-9),
    both decreasing in r, so their values at the left knot r_k of a pair's interval bound the interval. A pair adds at
    most its |dF| to each force component (|d_c| / r <= 1) and half its |dU| to the particle's energy; the bounds are
    summed over each particle's neighbours. Rounding of the two float64 sums is allowed for with
    (neighbours + 8) * 2^-52 of the largest reference component. The listed pairs end at 2.8, short of the table's last
    interval, whose right knot is the implicit zero rather than U(r_cut)."""
    pos, L, _ = H.lattice_config(8, 1.0, 0.08, seed=5)
    box = oracle.make_box(L)
    nl = oracle.build_nlist(pos, box, 2.8)
    dr = (R_CUT - R_MIN) / WIDTH
    knots = R_MIN + dr * np.arange(WIDTH)
    ev = [oracle.eval_pair("PerturbedLennardJones", PLJ, float(r), R_CUT) for r in knots]
    assert all(e[0] for e in ev)
    U = np.array([e[2] for e in ev])
    F = np.array([e[1] for e in ev]) * knots  # F = -dU/dr = r * force_divr
    tab = R.pair_table(R_MIN, R_CUT, U, F)
    got, _ = R.pair_forces(pos, L, nl, [[tab]], R_CUT)
    ref = oracle.pair_forces("PerturbedLennardJones", pos, box, nl, oracle.pack_pair_params("PerturbedLennardJones", PLJ),
                             R_CUT, mode="none")
    i, j, d, r = R.pair_separations(pos, L, nl)
    assert r.min() >= R_MIN and r.max() < R_CUT - dr
    rk = R_MIN + dr * np.floor((r - R_MIN) / dr)
    n = pos.shape[0]
    dU = dr * dr / 8.0 * 4.0 * (156.0 * rk ** -14 + 42.0 * rk ** -8)
    dF = dr * dr / 8.0 * 4.0 * (2184.0 * rk ** -15 + 336.0 * rk ** -9)
    count = np.bincount(i, minlength=n)
    bound_e = 0.5 * np.bincount(i, weights=dU, minlength=n) + (count + 8) * 2.0 ** -52 * np.abs(ref[:, 3]).max()
    bound_f = np.bincount(i, weights=dF, minlength=n) + (count + 8) * 2.0 ** -52 * np.abs(ref[:, :3]).max()
    err_e = np.abs(got[:, 3] - ref[:, 3])
    err_f = np.abs(got[:, :3] - ref[:, :3]).max(axis=1)
    print("interpolation error / bound: energy %.3g, force %.3g; largest force error %.3g of the largest force"
          % ((err_e / bound_e).max(), (err_f / bound_f).max(), err_f.max() / np.abs(ref[:, :3]).max()))
    assert np.all(err_e <= bound_e)
    assert np.all(err_f <= bound_f)
    # the table is not the analytic potential in disguise: the interpolation error is there
    assert err_f.max() > 0.0 and err_e.max() > 0.0


# ---------------------------------------------------------------------------
# argument errors
# ---------------------------------------------------------------------------
def _pair(**kw):
    return azp.pair.Table(nlist=azp.nlist.Cell(buffer=0.3), default_r_cut=2.5, **kw)


def _good(width=8, r_min=0.5):
    return dict(r_min=r_min, U=R.smooth_curve(1, width), F=R.smooth_curve(2, width))


def test_pair_table_round_trip_and_exports():
    assert "Table" in azp.pair.__all__ and "Table" in azp.bond.__all__
    p = _pair()
    assert p._param_doubles == 4 and p._planned_entry == "azp_pair_forces_planned_table" and p.mode == "none"
    d = _good()
    p.params[("A", "B")] = d
    back = p.params[("B", "A")]
    assert back.keys() == d.keys() and back["r_min"] == 0.5
    assert np.array_equal(back["U"], d["U"]) and np.array_equal(back["F"], d["F"])
    back["U"][0] = 99.0  # a copy: the stored table is not edited through it
    assert p.params[("A", "B")]["U"][0] == d["U"][0]
    p.params[("B", "A")] = dict(d)  # the same table under the other order is no conflict
    b = azp.bond.Table()
    db = dict(_good(), r_max=1.5)
    b.params["A-A"] = db
    back = b.params["A-A"]
    assert back["r_min"] == 0.5 and back["r_max"] == 1.5 and np.array_equal(back["F"], db["F"])


def test_unequal_lengths_raise():
    d = _good()
    d["F"] = d["F"][:-1]
    with pytest.raises(ValueError, match="length"):
        _pair().params[("A", "A")] = d
    with pytest.raises(ValueError, match="length"):
        azp.bond.Table().params["A-A"] = dict(d, r_max=1.5)


def test_r_min_not_below_r_cut_raises():
    with pytest.raises(ValueError, match="r_cut"):
        _pair().params[("A", "A")] = _good(r_min=2.5)
    with pytest.raises(ValueError, match="r_cut"):
        _pair().params[("A", "A")] = _good(r_min=3.0)
    with pytest.raises(ValueError, match="r_min"):
        _pair().params[("A", "A")] = _good(r_min=-0.1)
    p = _pair()
    p.r_cut[("A", "A")] = 0.0  # never evaluated: any r_min goes
    p.params[("A", "A")] = _good(r_min=3.0)
    with pytest.raises(ValueError, match="r_max"):
        azp.bond.Table().params["A-A"] = dict(_good(r_min=1.5), r_max=1.5)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("column", ["U", "F"])
def test_non_finite_entries_raise(column, bad):
    d = _good()
    d[column][3] = bad
    with pytest.raises(ValueError, match="finite"):
        _pair().params[("A", "A")] = d
    with pytest.raises(ValueError, match="finite"):
        azp.bond.Table().params["A-A"] = dict(d, r_max=1.5)


def test_mode_shift_is_refused():
    with pytest.raises(ValueError, match="mode"):
        _pair(mode="shift")
    with pytest.raises(ValueError, match="mode"):
        _pair(mode="xplor")
    p = _pair()
    with pytest.raises(ValueError, match="mode"):
        p.mode = "shift"


def test_asymmetric_tables_raise():
    p = _pair()
    p.params[("A", "B")] = _good()
    other = _good()
    other["U"] = other["U"] + 1.0
    with pytest.raises(ValueError, match="same rows"):
        p.params[("B", "A")] = other
    assert np.array_equal(p.params[("A", "B")]["U"], _good()["U"])  # the refused table left no trace
    p.params[("A", "B")] = other  # replacing the table under the order it was set with is fine


def test_bond_width_below_two_raises():
    with pytest.raises(ValueError, match="at least 2"):
        azp.bond.Table().params["A-A"] = dict(_good(width=1), r_max=1.5)
    azp.bond.Table().params["A-A"] = dict(_good(width=2), r_max=1.5)
    _pair().params[("A", "A")] = _good(width=1)  # a pair table may have one sample
    with pytest.raises(ValueError, match="at least 1"):
        _pair().params[("A", "A")] = dict(r_min=0.5, U=[], F=[])


def test_table_params_size_matches_header():
    """sizeof(azp_table_params) == 32 (four float64 words per type pair), compiled against include/azp.h."""
    names = ["azp_table_params"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){' + "".join(
        'printf("%%zu\\n", sizeof(%s));' % n for n in names) + \
        'printf("%zu\\n%zu\\n", offsetof(azp_table_params, d_rows), offsetof(azp_table_params, n));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got == [32, 16, 24]
    assert C.sizeof(_lib.TableParams) == 32 and _lib.TableParams.d_rows.offset == 16 and _lib.TableParams.n.offset == 24
    assert azp.pair.Table._param_doubles * 8 == 32 and azp.bond.Table._param_doubles * 8 == 32
    rows = _lib.table_params_rows([(0.5, 2.5, 0x1000, 7), (0.0, 0.0, 0, 0)])
    assert rows.shape == (2, 4) and rows[0, 0] == 0.5 and rows[0, 1] == 2.5
    assert rows[0, 2:].view(np.uint64).tolist() == [0x1000, 7] and not rows[1].any()
