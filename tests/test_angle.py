"""azplugins_amd.angle without a GPU: the NumPy reference (tests/angle_ref.py) against a hand-derived answer, against
its own energy (F = -dE/dr) and against the sum rules of a three-body force; the angle-table builder on CPU tensors
against a plain loop; ``localize_angles``; the C ABI (struct layout, exported symbols, argument errors, the two
parameter folds) and the validation of the Python classes."""

import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import angle_ref as ref
from azplugins_amd import _lib, angle
from azplugins_amd.state import Snapshot, build_angle_table, localize_angles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = (20.0, 20.0, 20.0)
POTENTIALS = ("Harmonic", "CosineSquared")


def test_hand_derived_known_answer():
    """k = 10, t0 = 2 pi / 3, a = (1, 0, 0), b = 0, c = (0, 2, 0): theta = pi / 2, U = 5 (pi / 6)^2,
    g = -k (theta - t0) = 10 pi / 6, F_a = -g dcb / (|dab||dcb|) = (0, -5 pi / 3, 0), F_c = -g dab / 2 = (-5 pi / 6, 0, 0)."""
    pos = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
    out = ref.evaluate("Harmonic", [dict(k=10.0, t0=2.0 * math.pi / 3.0)], pos, [(0, 1, 2)], [0], L)
    assert abs(out["energy"] - 1.3707783890) < 1e-9
    assert abs(out["energy"] - 5.0 * (math.pi / 6.0) ** 2) < 1e-14
    want = np.array([[0.0, -5.2359877560, 0.0], [2.6179938780, 5.2359877560, 0.0], [-2.6179938780, 0.0, 0.0]])
    assert np.abs(out["force"] - want).max() < 1e-9
    assert np.abs(out["energies"] - out["energy"] / 3.0).max() < 1e-15


def _random_angles(n, seed):
    """n separate angles (3 n particles) with theta in [0.2, pi - 0.2], arm lengths in [0.7, 1.6], random frames."""
    rng = np.random.default_rng(seed)
    pos = np.zeros((3 * n, 3))
    for j in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        theta = rng.uniform(0.2, math.pi - 0.2)
        ra, rc = rng.uniform(0.7, 1.6, size=2)
        b = rng.uniform(-3.0, 3.0, size=3)
        pos[3 * j] = b + ra * q[:, 0]
        pos[3 * j + 1] = b
        pos[3 * j + 2] = b + rc * (math.cos(theta) * q[:, 0] + math.sin(theta) * q[:, 1])
    angles = [(3 * j, 3 * j + 1, 3 * j + 2) for j in range(n)]
    return pos, angles, rng.integers(0, 2, size=n)


PARAMS = [dict(k=10.0, t0=2.0), dict(k=3.5, t0=2.6)]


@pytest.mark.parametrize("name", POTENTIALS)
def test_ref_force_is_minus_energy_gradient(name):
    """Central differences with h = 1e-6: truncation ~ h^2 = 1e-12, rounding ~ 1e-16 / h = 1e-10 of the energy."""
    pos, angles, typeid = _random_angles(50, 7)
    F = ref.evaluate(name, PARAMS, pos, angles, typeid, L)["force"]
    h = 1e-6
    num = np.zeros_like(F)
    for i in range(pos.shape[0]):
        mine = [j for j, g in enumerate(angles) if i in g]  # (the other angles' energy does not change)
        sub, st = [angles[j] for j in mine], [typeid[j] for j in mine]
        for k in range(3):
            p, m = pos.copy(), pos.copy()
            p[i, k] += h
            m[i, k] -= h
            num[i, k] = -(ref.energy_only(name, PARAMS, p, sub, st, L) - ref.energy_only(name, PARAMS, m, sub, st, L)) / (2.0 * h)
    err = np.abs(F - num).max() / np.abs(F).max()
    print("%s: force vs central difference %.3e of the largest force" % (name, err))
    assert err < 1e-7


@pytest.mark.parametrize("name", POTENTIALS)
def test_ref_sum_rules(name):
    pos, angles, typeid = _random_angles(50, 11)
    out = ref.evaluate(name, PARAMS, pos, angles, typeid, L)
    rows = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for j, (a, b, c) in enumerate(angles):
        Fa, Fb, Fc = out["F"][j]
        dab, dcb = out["d"][j]
        scale = max(np.abs(out["F"][j]).max(), 1.0)
        assert np.abs(Fa + Fb + Fc).max() < 1e-12 * scale
        assert np.abs(np.cross(dab, Fa) + np.cross(dcb, Fc)).max() < 1e-12 * scale   # net torque about b
        # the three members' virials add up to sum_k (r_k - r_b) (x) F_k (the k = b term vanishes)
        W = np.outer(dab, Fa) + np.outer(dcb, Fc)
        got = out["virial"][[a, b, c]].sum(axis=0)
        assert np.abs(got - np.array([W[r, s] for r, s in rows])).max() < 1e-12 * scale


def _table_topology():
    """A chain of 9 (0-8), a triangle (9-11), a 6-arm star (centre 12, arms 13-18), two particles without angles (19,
    20), and two angles that reach members beyond n_local = 21 (rows 21-23 stand for ghosts)."""
    angles = ref.chain_angles(0, 9) + ref.triangle_angles(9, 10, 11) + ref.star_angles(12, list(range(13, 19)))
    angles += [(8, 21, 22), (23, 22, 21)]  # one local end with two ghosts; ghosts only (no entry at all)
    typeid = [j % 3 for j in range(len(angles))]
    return angles, typeid, 21


def test_angle_table_matches_plain_loop():
    import torch

    angles, typeid, n_local = _table_topology()
    tab = build_angle_table(torch.tensor(angles, dtype=torch.int64), torch.tensor(typeid, dtype=torch.int64), n_local)
    want = ref.table_loop(angles, typeid, n_local)
    counts = [len(e) for e in want]
    assert counts[12] == 15 and counts[4] == 3 and counts[19] == counts[20] == 0 and counts[9] == 3
    assert tab["pitch"] == n_local and tab["width"] == 15
    assert tab["table"].shape == (15, n_local, 4) and tab["table"].dtype == torch.int32 and tab["table"].is_contiguous()
    assert tab["n_angles"].dtype == torch.int32 and tab["n_angles"].tolist() == counts
    table = tab["table"].numpy()
    for i in range(n_local):
        assert [tuple(int(x) for x in table[s, i]) for s in range(counts[i])] == want[i], i
        assert not table[counts[i]:, i].any()  # unused slots stay zero
    # no angles at all: one empty column per particle
    empty = build_angle_table(torch.zeros((0, 3), dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 5)
    assert empty["table"].shape == (1, 5, 4) and empty["n_angles"].tolist() == [0] * 5


def test_snapshot_angles():
    s = Snapshot()
    assert s.angles.N == 0 and s.angles.group.shape == (0, 3) and s.angles.types == []
    s = Snapshot.from_arrays(np.zeros((4, 3)), L)
    assert s.angles.N == 0
    s = Snapshot.from_arrays(np.zeros((4, 3)), L, angles=[(0, 1, 2), (1, 2, 3)], angle_typeid=[0, 1], angle_types=("X", "Y"))
    assert s.angles.N == 2 and s.angles.group.dtype == np.uint32 and s.angles.group.tolist() == [[0, 1, 2], [1, 2, 3]]
    assert s.angles.typeid.tolist() == [0, 1] and s.angles.types == ["X", "Y"] and s.bonds.N == 0
    assert Snapshot.from_arrays(np.zeros((3, 3)), L, angles=[(0, 1, 2)]).angles.types == ["A-A-A"]


def test_localize_angles():
    # rows 0-2 are local (tags 10, 11, 12), rows 3-5 ghosts (tags 13, 14 and tag 10 again: its own periodic image)
    tag = np.array([10, 11, 12, 13, 14, 10])
    angle_tags = np.array([[10, 11, 12], [11, 12, 13], [12, 13, 14], [13, 14, 10], [14, 13, 14]])
    typeid = np.array([0, 1, 2, 3, 4], dtype=np.uint32)
    group, tid = localize_angles(tag, 3, angle_tags[:4], typeid[:4])
    assert group.dtype == np.uint32
    # every angle with a local member; tag 10 resolves to row 0, the lowest, not to its ghost copy in row 5
    assert group.tolist() == [[0, 1, 2], [1, 2, 3], [2, 3, 4], [3, 4, 0]] and tid.tolist() == [0, 1, 2, 3]
    # an angle of ghosts only is dropped
    group, tid = localize_angles(tag, 3, angle_tags, typeid)
    assert group.shape == (4, 3) and tid.tolist() == [0, 1, 2, 3]
    group, tid = localize_angles(tag, 1, angle_tags, typeid)
    assert group.tolist() == [[0, 1, 2], [3, 4, 0]] and tid.tolist() == [0, 3]
    # a member that is not on the rank: the shell is too narrow
    with pytest.raises(_lib.AzpError, match="narrower than two bond lengths"):
        localize_angles(tag, 3, np.array([[11, 12, 15]]), np.array([0]))
    # ... but an angle without a local member may miss members
    group, _ = localize_angles(tag, 3, np.array([[13, 14, 15]]), np.array([0]))
    assert group.shape == (0, 3)


def test_abi_angle_struct_layout():
    fields = ["d_force", "d_virial", "virial_pitch", "N", "n_max", "d_pos", "box", "d_gpu_anglelist", "d_gpu_n_angles", "pitch",
              "n_angle_types", "compute_virial", "block_size"]
    efields = ["idx", "type", "pos"]
    names = ["azp_angle_entry", "azp_angle_args", "azp_angle_harmonic_params", "azp_angle_cossq_params"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){' + "".join(
        'printf("%%zu\\n", sizeof(%s));' % n for n in names) + "".join(
        'printf("%%zu\\n", offsetof(azp_angle_args, %s));' % f for f in fields) + "".join(
        'printf("%%zu\\n", offsetof(azp_angle_entry, %s));' % f for f in efields) + \
        'printf("%zu\\n%zu\\n", offsetof(azp_angle_harmonic_params, t0), offsetof(azp_angle_cossq_params, cos_t0));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == C.sizeof(_lib.AngleEntry) == 16
    assert got[1] == C.sizeof(_lib.AngleArgs)
    assert got[2] == got[3] == 16
    for k, f in enumerate(fields):
        assert got[4 + k] == getattr(_lib.AngleArgs, f).offset, f
    for k, f in enumerate(efields):
        assert got[4 + len(fields) + k] == getattr(_lib.AngleEntry, f).offset, f
    assert got[-2:] == [8, 8]


def test_abi_angle_symbols_and_argument_errors():
    lib = _lib.lib()
    for name in ("azp_angle_forces_harmonic", "azp_angle_forces_cosine_squared", "azp_angle_harmonic_params_make",
                 "azp_angle_harmonic_params_unpack", "azp_angle_cossq_params_make", "azp_angle_cossq_params_unpack"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    # Host memory stands in for the device arrays: every call below is refused (or has N = 0) before a launch.
    keep = (C.c_double * 64)()
    ptr = C.addressof(keep)

    def args(**kw):
        a = _lib.AngleArgs()
        a.N, a.n_max, a.pitch, a.virial_pitch, a.n_angle_types = 4, 4, 4, 4, 1
        a.d_force = a.d_virial = a.d_pos = a.d_gpu_anglelist = a.d_gpu_n_angles = ptr
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for name in ("azp_angle_forces_harmonic", "azp_angle_forces_cosine_squared"):
        fn = getattr(lib, name)
        assert fn(None, ptr, None) == -1
        assert fn(C.byref(_lib.AngleArgs()), None, None) == 0          # N = 0: nothing to do, nothing looked at
        assert fn(C.byref(args(N=0, block_size=96)), ptr, None) == 0
        assert fn(C.byref(args()), None, None) == -1                  # no parameters
        for missing in ("d_force", "d_pos", "d_gpu_anglelist", "d_gpu_n_angles"):
            assert fn(C.byref(args(**{missing: None})), ptr, None) == -1, missing
        assert fn(C.byref(args(compute_virial=1, d_virial=None)), ptr, None) == -1
        assert fn(C.byref(args(compute_virial=1, virial_pitch=3)), ptr, None) == -1
        assert fn(C.byref(args(pitch=3)), ptr, None) == -1
        assert fn(C.byref(args(n_angle_types=0)), ptr, None) == -1
        for bs in (1, 32, 96, 320, 512):
            assert fn(C.byref(args(block_size=bs)), ptr, None) == -1, bs
        assert fn(C.byref(args(n_angle_types=4097)), ptr, None) == _lib.ERROR_TOO_MANY_TYPES   # 16 B each: > 64 KiB


def test_parameter_folds():
    lib = _lib.lib()
    out = (C.c_double * 2)(7.0, 7.0)
    lib.azp_angle_harmonic_params_make(10.0, 2.0, C.addressof(out))
    assert list(out) == [10.0, 2.0]
    lib.azp_angle_cossq_params_make(3.5, 2.0, C.addressof(out))
    assert out[0] == 3.5 and abs(out[1] - math.cos(2.0)) <= math.ulp(1.0)
    k, t0 = C.c_double(), C.c_double()
    lib.azp_angle_cossq_params_unpack(C.addressof(out), C.byref(k), C.byref(t0))
    assert k.value == 3.5 and abs(t0.value - 2.0) < 1e-15
    for cls in (angle.Harmonic, angle.CosineSquared):
        f = cls()
        back = f._unpack(f._pack(dict(k=4.0, t0=1.25)))
        assert back["k"] == 4.0 and abs(back["t0"] - 1.25) < 1e-15


@pytest.mark.parametrize("cls", [angle.Harmonic, angle.CosineSquared])
def test_python_validation(cls):
    f = cls()
    assert isinstance(f, angle.Angle) and f.block_size == 0 and not f.compute_virial
    f.params["A-A-A"] = dict(k=10, t0=2)
    assert f.params["A-A-A"] == dict(k=10.0, t0=2.0)
    f.params["A-A-A"] = dict(k=0.0, t0=0.0)
    f.params["A-A-A"] = dict(k=-1.0, t0=math.pi)
    for bad in (dict(k=1.0, t0=-0.1), dict(k=1.0, t0=3.2), dict(k=1.0, t0=float("nan")), dict(k=float("inf"), t0=1.0),
                dict(k=float("nan"), t0=1.0)):
        with pytest.raises(ValueError):
            f.params["A-A-A"] = bad
    with pytest.raises(ValueError):
        f.params["A-A-A"] = dict(k=1.0)                    # t0 missing
    with pytest.raises(ValueError):
        f.params["A-A-A"] = dict(k=1.0, t0=1.0, r0=1.0)    # unknown key
    with pytest.raises(TypeError):
        f.params["A-A-A"] = dict(k="stiff", t0=1.0)
    assert f.params["A-A-A"] == dict(k=-1.0, t0=math.pi)   # a refused value changes nothing
    with pytest.raises(_lib.AzpError, match="not attached"):
        f.compute()


class _FakeState:
    angle_types = ["A-A-A", "B-B-B"]
    device = "cpu"


def test_unset_parameters_raise():
    f = angle.Harmonic()
    f.params["A-A-A"] = dict(k=1.0, t0=2.0)
    f._state = _FakeState()
    with pytest.raises(_lib.AzpError, match=r"Harmonic.params\['B-B-B'\] is not set"):
        f._build_tables()
    f.params["B-B-B"] = dict(k=2.0, t0=1.0)
    f._build_tables()
    assert f._tables.tolist() == [[1.0, 2.0], [2.0, 1.0]]
