"""The generators of the binning tests (binning_cases.py) produce what test_gpu_binning.py relies on -- checked here
with numpy alone, so the conditions hold whether or not a GPU is present."""

import numpy as np
import pytest

import binning_cases as B

RL3 = ((1.0, 0.8, 0.6), (0.8, 0.9, 0.0), (0.6, 0.0, 0.7))  # test_gpu_nlist_rows.RL3


def test_paths_of_the_table():
    """Every path of azp_nlist_bin is selected by some case of the table."""
    got = {B.paths_of(d, n) for d, n in B.TABLE}
    assert {("scan1x1", "small"), ("scan1x1", "wave"), ("scan1x2", "small"), ("scan1x2", "wave"), ("scan1x8", "small"),
            ("scan3x9", "small"), ("scan3x10", "wave"), ("scan3x10", "small"), ("scan1x17", "small"), ("scan3x17", "small"),
            ("scan3x64", "small")} == got
    assert B.paths_of((16, 16, 16), 6 * 4096) == ("scan1x1", "small") and B.paths_of((16, 16, 16), 6 * 4096 + 1)[1] == "wave"
    assert B.paths_of((41, 41, 41), 17)[0] == "scan1x17" and B.paths_of((41, 41, 41), 18)[0] == "scan3x17"


@pytest.mark.parametrize("case", B.TABLE, ids=B.case_id)
def test_occupancies_are_the_requested_ones(case):
    dims, n = case
    sys_ = B.occupancy_case(dims, n)
    ncell = int(np.prod(dims))
    counts = sys_["counts"]
    assert counts.shape == (ncell,) and counts.sum() == n and sys_["xyz"].shape == (n, 3)
    # the numpy cell rule puts every particle into the cell it was generated for, in both memory orders
    cell = B.cell_rule(sys_["xyz"], sys_["lo"], sys_["width"], dims, (1, 1, 1))
    assert np.array_equal(cell, sys_["cell"])
    assert np.array_equal(np.bincount(cell, minlength=ncell), counts)
    perm = B.shuffled(n)
    assert np.array_equal(np.sort(perm), np.arange(n))
    assert np.array_equal(np.bincount(cell[perm], minlength=ncell), counts)
    # nobody near a face
    frac = (sys_["xyz"] - sys_["lo"]) / sys_["width"]
    assert np.all(np.abs(frac - np.floor(frac) - 0.5) < 0.4 + 1e-9)
    occupancies = set(counts.tolist())
    marks = B.marked_cells(ncell)
    if n >= 100:
        wanted = B.SMALL_SET if B.paths_of(dims, n)[1] == "small" else B.WAVE_SET
        assert set(wanted) <= occupancies
        assert np.all(counts[marks] > 0)  # first cell, last cell, both sides of every block of 4,096 cells
    else:
        # 17 / 18 particles cannot hold the set: the first and the last cell and the leading block boundaries
        assert counts[0] > 0 and counts[-1] > 0 and np.count_nonzero(counts[marks]) == min(n, marks.size) and 0 in occupancies
    assert marks.size == 2 + 2 * ((ncell - 1) // B.SCAN_BLOCK) - (1 if ncell % B.SCAN_BLOCK == 1 and ncell > 1 else 0)


@pytest.mark.parametrize("dims", [(33, 33, 31), (41, 41, 41)], ids=lambda d: "x".join(str(x) for x in d))
def test_clumped_system_meets_its_conditions(dims):
    cfg, ref = B.clumped_system(dims, RL3)
    facts = B.clumped_facts(cfg, ref, dims)
    assert cfg["N"] == 280 * 16 + 240
    assert facts["borderline"] == 0
    assert facts["mean_row"] >= 8
    assert all(c > 0 for c in facts["crossing"])
    assert facts["occupied_above"][32768] > 0
    if np.prod(dims) > 65536:
        assert facts["occupied_above"][65536] > 0
    assert facts["top_cell"] < np.prod(dims)
