"""distance_check_kernel (csrc/nlist.hip) through its two entries, azp_nlist_displacements and azp_nlist_distance_check:
the kernel that decides every rebuild of a neighbor list. A check that misses a mover leaves a stale list behind.

n = 131,072 + 300: the launch is clamped to 512 workgroups of 256 threads, so 300 threads take a second trip of the
grid-stride loop. The reference is numpy FP64 with nlist_ref.min_image. Bars (those of
test_gpu_external_nve.test_sum_forces_and_displacements): |sqrt(max bits) - max| < 1e-12; every displacement is a
single-precision UPPER bound, exact (1 - 1e-15) <= disp <= exact (1 + 3e-7).
"""

import ctypes as C
import functools

import numpy as np
import pytest

import nlist_ref as R
from azplugins_amd import _lib
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = -1  # AZP_ERROR_INVALID_ARGUMENT (include/azp.h)
GRID_THREADS = 512 * 256
N = GRID_THREADS + 300
L = np.array([30.0, 20.0, 25.0])
LIMIT = 0.3
GUARD = 64


@functools.lru_cache(maxsize=1)
def _base():
    """(x0, d): positions in the box and displacements of at most 0.14 (nobody beyond LIMIT). Do not modify."""
    tag = np.arange(N, dtype=np.uint64)
    x0 = np.stack([(syn.u01(9, tag, c) - 0.5) * L[c] for c in range(3)], axis=1)
    d = 0.08 * np.stack([2.0 * syn.u01(10, tag, c) - 1.0 for c in range(3)], axis=1)
    return x0, d


def run(x0, x1, max_dist_sq, tilt=(0.0, 0.0, 0.0), periodic=(1, 1, 1), entry="displacements", bits=True, flag0=0):
    """(status, flag, max r^2, disp[n] as float64) of one call; the flag word pre-set to flag0, the maximum to 0, disp
    filled with -1 and followed by guard words."""
    import torch

    n = x0.shape[0]
    p0 = torch.zeros((max(n, 1), 4), dtype=torch.float64, device="cuda:0")  # (n = 0: still a buffer, not a null pointer)
    p1 = torch.zeros((max(n, 1), 4), dtype=torch.float64, device="cuda:0")
    p0[:n] = torch.from_numpy(syn.pos4(x0)).to("cuda:0")
    p1[:n] = torch.from_numpy(syn.pos4(x1)).to("cuda:0")
    box = _lib.make_box(L, tilt, periodic)
    row = torch.tensor([flag0, 0], dtype=torch.int64, device="cuda:0")
    disp = torch.full((n + GUARD,), -1.0, dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    bits_ptr = row.data_ptr() + 8 if bits else None
    lib = _lib.lib()
    if entry == "displacements":
        rc = lib.azp_nlist_displacements(n, p1.data_ptr(), p0.data_ptr(), C.byref(box), max_dist_sq, row.data_ptr(), bits_ptr,
                                         disp.data_ptr(), stream)
    else:
        rc = lib.azp_nlist_distance_check(n, p1.data_ptr(), p0.data_ptr(), C.byref(box), max_dist_sq, row.data_ptr(), bits_ptr, stream)
    torch.cuda.synchronize()
    flag, b = row.tolist()
    out = disp.cpu().numpy().astype(np.float64)
    assert np.all(out[n:] == -1.0)
    return rc, flag, float(np.array([b], dtype=np.int64).view(np.float64)[0]), out[:n]


def exact_displacements(x0, x1, tilt=(0.0, 0.0, 0.0), periodic=(1, 1, 1)):
    x, y, z = R.min_image(x1 - x0, L, tilt, periodic)
    return np.sqrt(x * x + y * y + z * z)


def assert_displacements(got, max_sq, exact):
    assert abs(np.sqrt(max_sq) - exact.max()) < 1e-12
    low = np.flatnonzero(got < exact * (1 - 1e-15))
    high = np.flatnonzero(got > exact * (1 + 3e-7))
    assert low.size == 0, "particle %d: %r below the exact %r (%d in all)" % (low[0], got[low[0]], exact[low[0]], low.size)
    assert high.size == 0, "particle %d: %r above the exact %r (%d in all)" % (high[0], got[high[0]], exact[high[0]], high.size)


def test_nobody_beyond_the_limit():
    x0, d = _base()
    x1 = syn.wrap(x0 + d, L)  # (some cross the periodic boundary: minimum image)
    assert np.count_nonzero(np.abs(x1 - x0).max(axis=1) > 1.0) > 100
    exact = exact_displacements(x0, x1)
    assert 0.1 < exact.max() < 0.15
    rc, flag, max_sq, got = run(x0, x1, LIMIT ** 2)
    assert rc == 0 and flag == 0
    assert_displacements(got, max_sq, exact)
    # the flag is OR-ed into: a word that was set stays set
    assert run(x0, x1, LIMIT ** 2, flag0=1)[1] == 1


@pytest.mark.parametrize("mover", [GRID_THREADS + 123, 0, GRID_THREADS - 1], ids=["second_trip", "first", "last_of_first_trip"])
def test_the_only_mover_is_seen(mover):
    x0, d = _base()
    d = d.copy()
    d[mover] = [0.31, 0.0, 0.0]
    x1 = syn.wrap(x0 + d, L)
    exact = exact_displacements(x0, x1)
    assert np.count_nonzero(exact > LIMIT) == 1 and np.argmax(exact) == mover
    rc, flag, max_sq, got = run(x0, x1, LIMIT ** 2)
    assert rc == 0 and flag == 1
    assert_displacements(got, max_sq, exact)
    # the check entry (disp = nullptr) on the same input: the same flag and maximum, with and without the maximum
    rc2, flag2, max_sq2, _ = run(x0, x1, LIMIT ** 2, entry="check")
    assert (rc2, flag2) == (0, 1) and max_sq2 == max_sq
    rc3, flag3, max_sq3, _ = run(x0, x1, LIMIT ** 2, entry="check", bits=False)
    assert (rc3, flag3, max_sq3) == (0, 1, 0.0)


def test_the_limit_is_strict():
    """One particle from x = 1.0 to x = 1.25, everybody else at rest: r^2 = 0.0625 exactly. Not beyond a limit of
    0.0625, beyond the next double below it."""
    x0 = _base()[0].copy()
    x0[GRID_THREADS + 7] = [1.0, 2.0, -3.0]
    x1 = x0.copy()
    x1[GRID_THREADS + 7, 0] = 1.25
    for entry in ("displacements", "check"):
        rc, flag, max_sq, got = run(x0, x1, 0.0625, entry=entry)
        assert (rc, flag, max_sq) == (0, 0, 0.0625)
        rc, flag, max_sq, got = run(x0, x1, float(np.nextafter(0.0625, 0.0)), entry=entry)
        assert (rc, flag, max_sq) == (0, 1, 0.0625)
    got = run(x0, x1, 0.0625)[3]
    assert np.count_nonzero(got) == 1 and 0.25 <= got[GRID_THREADS + 7] <= 0.25 * (1 + 3e-7)


def test_non_periodic_axis():
    """Periodic flags (1, 0, 1): 0.9 L along the open y is a displacement of 0.9 L, along the periodic x of 0.1 L."""
    periodic = (1, 0, 1)
    x0 = _base()[0].copy()
    iy, ix = 5, GRID_THREADS + 200
    x0[iy] = [1.0, -0.45 * L[1], 2.0]
    x0[ix] = [-0.45 * L[0], 1.0, 2.0]
    x1 = x0.copy()
    x1[iy, 1] = 0.45 * L[1]
    x1[ix, 0] = 0.45 * L[0]
    exact = exact_displacements(x0, x1, periodic=periodic)
    assert abs(exact[iy] - 0.9 * L[1]) < 1e-12 and abs(exact[ix] - 0.1 * L[0]) < 1e-12 and np.count_nonzero(exact) == 2
    rc, flag, max_sq, got = run(x0, x1, LIMIT ** 2, periodic=periodic)
    assert rc == 0 and flag == 1
    assert_displacements(got, max_sq, exact)
    assert abs(np.sqrt(max_sq) - 0.9 * L[1]) < 1e-12
    # the y mover alone decides with a limit between the two
    assert run(x0, x1, 10.0 ** 2, periodic=periodic)[1] == 1
    x1[iy] = x0[iy]
    assert run(x0, x1, 10.0 ** 2, periodic=periodic)[1] == 0


def test_tilted_box():
    """(xy, xz, yz) = (0.5, 0.3, -0.4): particles that cross the y, the z and the x face (the image across y is
    shifted by xy Ly in x, across z by xz Lz and yz Lz)."""
    tilt = (0.5, 0.3, -0.4)
    xy, xz, yz = tilt
    lattice = np.array([[L[0], 0.0, 0.0], [xy * L[1], L[1], 0.0], [xz * L[2], yz * L[2], L[2]]])
    tag = np.arange(N, dtype=np.uint64)
    x0 = np.stack([syn.u01(11, tag, c) - 0.5 for c in range(3)], axis=1) @ lattice
    d = _base()[1]
    x1 = x0 + d
    q = np.arange(N)
    x1[q % 5 == 0] -= lattice[1]  # four particles of five have crossed a face: stored as the image inside the box
    x1[q % 5 == 1] += lattice[2]
    x1[q % 5 == 2] -= lattice[0]
    x1[q % 5 == 3] += lattice[1]
    assert np.count_nonzero(np.linalg.norm(x1 - x0, axis=1) > 10.0) > 0.7 * N
    exact = exact_displacements(x0, x1, tilt=tilt)
    assert np.abs(exact - np.linalg.norm(d, axis=1)).max() < 1e-12  # (the reference finds the image)
    rc, flag, max_sq, got = run(x0, x1, LIMIT ** 2, tilt=tilt)
    assert rc == 0 and flag == 0
    assert_displacements(got, max_sq, exact)
    mover = GRID_THREADS + 11
    x1[mover] = x0[mover] + [0.0, 0.31, 0.0] + lattice[1]
    assert run(x0, x1, LIMIT ** 2, tilt=tilt)[1] == 1


def test_nan_position_gives_an_infinite_displacement():
    x0, d = _base()
    x1 = syn.wrap(x0 + d, L)
    x1[GRID_THREADS + 1, 1] = np.nan
    x1[77, 0] = np.nan
    rc, flag, max_sq, got = run(x0, x1, LIMIT ** 2)
    assert rc == 0
    assert got[GRID_THREADS + 1] == np.inf and got[77] == np.inf
    ok = np.ones(N, dtype=bool)
    ok[[77, GRID_THREADS + 1]] = False
    exact = exact_displacements(x0[ok], x1[ok])
    assert np.all(got[ok] >= exact * (1 - 1e-15)) and np.all(got[ok] <= exact * (1 + 3e-7))


def test_edge_arguments():
    import torch

    x0, d = _base()
    x0, x1 = x0[:1000], syn.wrap(x0[:1000] + d[:1000], L)
    rc, flag, max_sq, got = run(x0[:0], x1[:0], LIMIT ** 2)
    assert (rc, flag, max_sq) == (0, 0, 0.0)
    assert run(x0[:0], x1[:0], LIMIT ** 2, entry="check")[:2] == (0, 0)
    for bad in (-1.0, float("nan")):
        for entry in ("displacements", "check"):
            rc, flag, max_sq, got = run(x0, x1, bad, entry=entry)
            assert (rc, flag, max_sq) == (INVALID_ARGUMENT, 0, 0.0) and np.all(got == -1.0)
    lib = _lib.lib()
    p = torch.from_numpy(syn.pos4(x0)).to("cuda:0")
    row = torch.zeros(2, dtype=torch.int64, device="cuda:0")
    disp = torch.full((1000,), -1.0, dtype=torch.float32, device="cuda:0")
    box = _lib.make_box(L)
    good = [p.data_ptr(), p.data_ptr(), C.byref(box), LIMIT ** 2, row.data_ptr(), row.data_ptr() + 8, disp.data_ptr()]
    for k in (0, 1, 2, 4, 6):
        args = list(good)
        args[k] = None
        assert lib.azp_nlist_displacements(1000, *args, None) == INVALID_ARGUMENT, k
        if k != 6:
            assert lib.azp_nlist_distance_check(1000, *args[:6], None) == INVALID_ARGUMENT, k
    torch.cuda.synchronize()
    assert row.tolist() == [0, 0] and bool((disp == -1.0).all())
