"""Host side of the cell list for tilted boxes: Box.nearest_plane_distance, nlist.cell_grid, and the geometry claim
behind fractional cells -- binned by the fractional coordinates along the lattice vectors, with
dim[k] = floor(w_k / r_list) cells over the perpendicular width w_k, the +-1 stencil holds every pair within r_list --
restated in NumPy (tests/nlist_tilted_cases.py) and compared row by row with the all-pairs reference. No GPU."""

import numpy as np
import pytest

import azplugins_amd as azp
import nlist_ref as R
import nlist_tilted_cases as T
from azplugins_amd import _lib, nlist


def test_nearest_plane_distance_is_volume_over_face_area():
    """50 random boxes with tilts in [-1, 1]: w_k = V / |cross product of the two other lattice vectors|."""
    rng = np.random.default_rng(20261019)
    for _ in range(50):
        L = rng.uniform(2.0, 12.0, 3)
        tilt = rng.uniform(-1.0, 1.0, 3)
        a, b, c = T.lattice(L, tilt)
        volume = abs(np.dot(a, np.cross(b, c)))
        brute = [volume / np.linalg.norm(np.cross(b, c)), volume / np.linalg.norm(np.cross(c, a)), volume / np.linalg.norm(np.cross(a, b))]
        got = azp.Box(*L, xy=tilt[0], xz=tilt[1], yz=tilt[2]).nearest_plane_distance
        assert len(got) == 3
        np.testing.assert_allclose(got, brute, rtol=1e-13)
    assert azp.Box(6.0, 7.0, 8.0).nearest_plane_distance == (6.0, 7.0, 8.0)


@pytest.mark.parametrize("L,tilt,dims", T.GRID_CASES, ids=lambda v: "x".join(str(x) for x in v) if isinstance(v, tuple) else None)
def test_cell_grid_dims(L, tilt, dims):
    box = azp.Box(*L, xy=tilt[0], xz=tilt[1], yz=tilt[2])
    got, lo, width, fractional = nlist.cell_grid(box, T.R_LIST)
    assert tuple(got) == dims and fractional is True
    assert tuple(lo) == (-0.5, -0.5, -0.5)
    assert tuple(width) == tuple(1.0 / d for d in dims)
    # a slab of cells is at least r_list thick, and one cell more along any axis would not be
    w = box.nearest_plane_distance
    for k in range(3):
        assert w[k] / dims[k] >= T.R_LIST > w[k] / (dims[k] + 1)


def test_cell_grid_of_an_untilted_box_is_cartesian():
    box = azp.Box(9.0, 8.0, 7.5, periodic=(True, False, True))
    dims, lo, width, fractional = nlist.cell_grid(box, T.R_LIST)
    assert fractional is False and tuple(dims) == (6, 5, 5)
    assert tuple(lo) == (-4.5, -4.0, -3.75) and tuple(width) == (9.0 / 6, 8.0 / 5, 7.5 / 5)
    assert tuple(nlist.cell_grid(box, T.R_LIST, sub=2)[0]) == (12, 10, 10)
    # an open axis may be narrower than two list radii (one cell)
    assert tuple(nlist.cell_grid(azp.Box(9.0, 1.0, 7.5, periodic=(True, False, True)), T.R_LIST)[0]) == (6, 1, 5)


def test_cell_grid_refuses_a_box_narrower_than_two_list_radii():
    """The 6.6 cube with tilt (0.5, 0.3, -0.4): L_x = 6.6 >= 5.6, but between its tilted faces the box is
    w_x = 5.39 < 2 r_list = 5.6 wide."""
    L, tilt, _ = T.GRID_CASES[0]
    box = azp.Box(*L, xy=tilt[0], xz=tilt[1], yz=tilt[2])
    assert box.nearest_plane_distance[0] == pytest.approx(5.39, abs=0.005)
    with pytest.raises(_lib.AzpError, match="box dimension 0"):
        nlist.cell_grid(box, 2.8)
    assert tuple(nlist.cell_grid(azp.Box(*L), 2.8)[0]) == (2, 2, 2)  # the untilted cube is wide enough
    open_x = azp.Box(*L, xy=tilt[0], xz=tilt[1], yz=tilt[2], periodic=(False, True, True))
    assert tuple(nlist.cell_grid(open_x, 2.8)[0]) == (1, 2, 2)  # and so is the tilted one when x is open


@pytest.mark.parametrize("L,tilt,dims", T.GRID_CASES, ids=lambda v: "x".join(str(x) for x in v) if isinstance(v, tuple) else None)
def test_fractional_cells_hold_every_pair(L, tilt, dims):
    """~600 particles per box, fully periodic: the rows of the restated scheme equal the all-pairs rows, every one,
    with the minimum image per pair; and with the image of every staged particle fixed once, relative to the home
    cell's centre, in the boxes of >= 3 cells per axis. (The kernels use that rule from 4 cells on. It still holds
    with 3: two staged images are at most 2/3 of a period apart, and where that is not the minimum image, the minimum
    image is a whole cell away, beyond r_list. On an axis of 2 cells, each visited once, it does not hold -- 534 of the
    601 rows of the third box come out wrong -- and no kernel uses it there.)"""
    n = 601
    cfg, ref = T.settled(lambda s: T.tilted_liquid(L, tilt, (1, 1, 1), n, s), 7)
    ref_n, ref_rows, borderline = ref
    assert borderline == 0 and ref_n.sum() > 5000
    box = azp.Box(*L, xy=tilt[0], xz=tilt[1], yz=tilt[2])
    assert tuple(nlist.cell_grid(box, T.R_LIST)[0]) == dims
    rules = ["pair"] + (["staged"] if min(dims) >= 3 else [])
    for rule in rules:
        rows = T.fractional_cell_rows(cfg, dims, rule)
        for i in range(n):
            assert np.array_equal(rows[i], ref_rows[i]), (rule, i)


def test_staged_images_with_open_axes():
    """The staged-image rule in partly periodic boxes of >= 4 cells per periodic axis, with particles beyond the
    open faces (no rows of their own)."""
    for tilt, periodic in ((T.TILT3, (1, 0, 1)), ((-0.35, 0.0, 0.0), (1, 1, 0))):
        cfg, ref = T.settled(lambda s: T.tilted_liquid((6.0, 7.0, 8.0), tilt, periodic, 900, s, rl=1.2, n_extra=200), 17)
        box = azp.Box(6.0, 7.0, 8.0, xy=tilt[0], xz=tilt[1], yz=tilt[2], periodic=periodic)
        dims = nlist.cell_grid(box, 1.2)[0]
        assert all(dims[k] >= 4 for k in range(3) if periodic[k])
        assert sum(int(np.count_nonzero(r >= 900)) for r in ref[1]) > 100  # listed particles beyond the faces
        for rule in ("pair", "staged"):
            rows = T.fractional_cell_rows(cfg, dims, rule)
            for i in range(cfg["N"]):
                assert np.array_equal(rows[i], ref[1][i]), (rule, i)
