"""azplugins_amd.dihedral without a GPU: the NumPy reference (tests/dihedral_ref.py) against a hand-derived answer,
against its own energy (F = -dE/dr) and against the sum rules of a four-body force; the dihedral-table builder on CPU
tensors against a plain loop; ``localize_dihedrals``; the C ABI (struct layout, exported symbols, argument errors, the
two parameter folds) and the validation of the Python classes."""

import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

import dihedral_cases as cases
import dihedral_ref as ref
from azplugins_amd import _lib, dihedral
from azplugins_amd.state import Snapshot, build_dihedral_table, localize_dihedrals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = (20.0, 20.0, 20.0)
POTENTIALS = ("Periodic", "OPLS")
PARAMS = cases.PARAMS


def test_hand_derived_known_answer():
    """a = (1, 0, 0), b = 0, c = (0, 0, 1), d = (0, 1, 1), Periodic k = 10, d = 1, n = 1, phi0 = 0: b1 = (-1, 0, 0),
    b2 = (0, 0, 1), b3 = (0, 1, 0), n1 = (0, 1, 0), n2 = (-1, 0, 0), phi = atan2(1, 0) = pi / 2, U = 5, U' = -5,
    F_a = U' n1 = (0, -5, 0), F_d = -U' n2 = (-5, 0, 0), s = t = 0, so F_b = -F_a and F_c = -F_d."""
    pos = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    out = ref.evaluate("Periodic", [dict(k=10.0, d=1, n=1, phi0=0.0)], pos, [(0, 1, 2, 3)], [0], L)
    assert abs(out["phi"][0] - math.pi / 2.0) < 1e-15
    assert abs(out["energy"] - 5.0) < 1e-14
    want = np.array([[0.0, -5.0, 0.0], [0.0, 5.0, 0.0], [5.0, 0.0, 0.0], [-5.0, 0.0, 0.0]])
    assert np.abs(out["force"] - want).max() < 1e-14
    assert np.abs(out["energies"] - 1.25).max() < 1e-15
    # the mirror image has the opposite sign, cis is 0 and trans is pi (IUPAC)
    assert abs(ref.angle_of(*ref.separations(pos[0], pos[1], pos[2], pos[3] * [1, -1, 1], L)) + math.pi / 2.0) < 1e-15
    assert ref.angle_of(*ref.separations(pos[0], pos[1], pos[2], [1.0, 0.0, 1.0], L)) == 0.0
    assert ref.angle_of(*ref.separations(pos[0], pos[1], pos[2], [-1.0, 0.0, 1.0], L)) == math.pi


def _random_dihedrals(n, seed):
    """n separate dihedrals (4 n particles): chains of 4 with bonds in [0.9, 1.1], bends in [0.5, pi - 0.5] and uniform
    torsions, in random frames."""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([cases.random_chain(rng, rng.uniform(-3.0, 3.0, size=3), 4) for _ in range(n)])
    return pos, [(4 * j, 4 * j + 1, 4 * j + 2, 4 * j + 3) for j in range(n)], rng.integers(0, 2, size=n)


@pytest.mark.parametrize("name", POTENTIALS)
def test_ref_force_is_minus_energy_gradient(name):
    """Central differences with h = 1e-6: truncation ~ h^2 = 1e-12, rounding ~ 1e-16 / h = 1e-10 of the energy."""
    pos, dihedrals, typeid = _random_dihedrals(40, 7)
    F = ref.evaluate(name, PARAMS[name], pos, dihedrals, typeid, L)["force"]
    h = 1e-6
    num = np.zeros_like(F)
    for i in range(pos.shape[0]):
        sub, st = [dihedrals[i // 4]], [typeid[i // 4]]  # (the other dihedrals' energy does not change)
        for k in range(3):
            p, m = pos.copy(), pos.copy()
            p[i, k] += h
            m[i, k] -= h
            num[i, k] = -(ref.energy_only(name, PARAMS[name], p, sub, st, L) - ref.energy_only(name, PARAMS[name], m, sub, st, L)) / (2.0 * h)
    err = np.abs(F - num).max() / np.abs(F).max()
    print("%s: force vs central difference %.3e of the largest force" % (name, err))
    assert np.abs(F).max() > 1.0 and err < 1e-6


@pytest.mark.parametrize("name", POTENTIALS)
def test_ref_sum_rules(name):
    pos, dihedrals, typeid = _random_dihedrals(40, 11)
    out = ref.evaluate(name, PARAMS[name], pos, dihedrals, typeid, L)
    for j, g in enumerate(dihedrals):
        Fa, Fb, Fc, Fd = out["F"][j]
        b1, b2, b3 = out["b"][j]
        scale = max(np.abs(out["F"][j]).max(), 1.0)
        assert np.abs(Fa + Fb + Fc + Fd).max() < 1e-12 * scale
        # net torque about b
        assert np.abs(np.cross(-b1, Fa) + np.cross(b2, Fc) + np.cross(b2 + b3, Fd)).max() < 1e-12 * scale
        # the four members' virials add up to the whole, and its trace is zero: U depends on directions only
        W = out["W"][j]
        assert np.abs(out["virial"][list(g)].sum(axis=0) - W).max() < 1e-12 * scale
        assert abs(W[0] + W[3] + W[5]) <= 1e-10 * np.abs(W).max() and np.abs(W).max() > 0.0


def _table_topology():
    """A chain of 9 (0-8), a 4-ring (9-12), a branched centre bond (13-14 with 15-17 and 18-20), two particles without
    dihedrals (21, 22), and two dihedrals that reach members beyond n_local = 23 (rows 23-26 stand for ghosts)."""
    d = ref.chain_dihedrals(0, 9) + ref.ring_dihedrals(9, 10, 11, 12) + ref.branched_dihedrals((15, 16, 17), 13, 14, (18, 19, 20))
    d += [(7, 8, 23, 24), (26, 25, 24, 23)]  # two local members with two ghosts; ghosts only (no entry at all)
    typeid = [j % 3 for j in range(len(d))]
    return d, typeid, 23


def test_dihedral_table_matches_plain_loop():
    import torch

    d, typeid, n_local = _table_topology()
    tab = build_dihedral_table(torch.tensor(d, dtype=torch.int64), torch.tensor(typeid, dtype=torch.int64), n_local)
    want = ref.table_loop(d, typeid, n_local)
    counts = [len(e) for e in want]
    assert counts[13] == counts[14] == 9 and counts[4] == 4 and counts[0] == 1 and counts[21] == counts[22] == 0 and counts[9] == 4
    assert counts[8] == 2 and counts[15] == 3
    assert tab["pitch"] == n_local and tab["width"] == 9
    assert tab["table"].shape == (9, n_local, 4) and tab["table"].dtype == torch.int32 and tab["table"].is_contiguous()
    assert tab["n_dihedrals"].dtype == torch.int32 and tab["n_dihedrals"].tolist() == counts
    table = tab["table"].numpy().view(np.uint32)
    for i in range(n_local):
        assert [tuple(int(x) for x in table[s, i]) for s in range(counts[i])] == want[i], i
        assert not table[counts[i]:, i].any()  # unused slots stay zero
    assert {int(w) >> 30 for w in table[:, :, 3].ravel()} == {0, 1, 2, 3}   # the top two bits do carry every position
    # no dihedrals at all: one empty column per particle
    empty = build_dihedral_table(torch.zeros((0, 4), dtype=torch.int64), torch.zeros(0, dtype=torch.int64), 5)
    assert empty["table"].shape == (1, 5, 4) and empty["n_dihedrals"].tolist() == [0] * 5


def test_snapshot_dihedrals():
    s = Snapshot()
    assert s.dihedrals.N == 0 and s.dihedrals.group.shape == (0, 4) and s.dihedrals.types == []
    s = Snapshot.from_arrays(np.zeros((5, 3)), L)
    assert s.dihedrals.N == 0
    s = Snapshot.from_arrays(np.zeros((5, 3)), L, dihedrals=[(0, 1, 2, 3), (1, 2, 3, 4)], dihedral_typeid=[0, 1], dihedral_types=("X", "Y"))
    assert s.dihedrals.N == 2 and s.dihedrals.group.dtype == np.uint32 and s.dihedrals.group.tolist() == [[0, 1, 2, 3], [1, 2, 3, 4]]
    assert s.dihedrals.typeid.tolist() == [0, 1] and s.dihedrals.types == ["X", "Y"] and s.bonds.N == 0 and s.angles.N == 0
    assert Snapshot.from_arrays(np.zeros((4, 3)), L, dihedrals=[(0, 1, 2, 3)]).dihedrals.types == ["A-A-A-A"]
    s.dihedrals.N = 3
    assert s.dihedrals.group.shape == (3, 4) and s.dihedrals.typeid.shape == (3,)


def test_localize_dihedrals():
    # rows 0-2 are local (tags 10, 11, 12), rows 3-6 ghosts (tags 13, 14, 15 and tag 10 again: its own periodic image)
    tag = np.array([10, 11, 12, 13, 14, 15, 10])
    dtags = np.array([[10, 11, 12, 13], [11, 12, 13, 14], [12, 13, 14, 15], [13, 14, 15, 10], [15, 14, 13, 14]])
    typeid = np.array([0, 1, 2, 3, 4], dtype=np.uint32)
    group, tid = localize_dihedrals(tag, 3, dtags[:4], typeid[:4])
    assert group.dtype == np.uint32
    # every dihedral with a local member; tag 10 resolves to row 0, the lowest, not to its ghost copy in row 6
    assert group.tolist() == [[0, 1, 2, 3], [1, 2, 3, 4], [2, 3, 4, 5], [3, 4, 5, 0]] and tid.tolist() == [0, 1, 2, 3]
    # a dihedral of ghosts only is dropped
    group, tid = localize_dihedrals(tag, 3, dtags, typeid)
    assert group.shape == (4, 4) and tid.tolist() == [0, 1, 2, 3]
    group, tid = localize_dihedrals(tag, 1, dtags, typeid)
    assert group.tolist() == [[0, 1, 2, 3], [3, 4, 5, 0]] and tid.tolist() == [0, 3]
    # a member that is not on the rank: the shell is too narrow
    with pytest.raises(_lib.AzpError, match="narrower than three bond lengths"):
        localize_dihedrals(tag, 3, np.array([[11, 12, 13, 16]]), np.array([0]))
    # ... but a dihedral without a local member may miss members
    group, _ = localize_dihedrals(tag, 3, np.array([[13, 14, 15, 16]]), np.array([0]))
    assert group.shape == (0, 4)


def test_abi_dihedral_struct_layout():
    fields = ["d_force", "d_virial", "virial_pitch", "N", "n_max", "d_pos", "box", "d_gpu_dihedrallist", "d_gpu_n_dihedrals", "pitch",
              "n_dihedral_types", "compute_virial", "block_size"]
    efields = ["idx", "type_pos"]
    pfields = ["k", "cos_phi0", "sin_phi0", "d", "n"]
    names = ["azp_dihedral_entry", "azp_dihedral_args", "azp_dihedral_periodic_params", "azp_dihedral_opls_params"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){' + "".join(
        'printf("%%zu\\n", sizeof(%s));' % n for n in names) + "".join(
        'printf("%%zu\\n", offsetof(azp_dihedral_args, %s));' % f for f in fields) + "".join(
        'printf("%%zu\\n", offsetof(azp_dihedral_entry, %s));' % f for f in efields) + "".join(
        'printf("%%zu\\n", offsetof(azp_dihedral_periodic_params, %s));' % f for f in pfields) + \
        'printf("%zu\\n", offsetof(azp_dihedral_opls_params, k4));return 0;}'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]
    assert got[0] == C.sizeof(_lib.DihedralEntry) == 16
    assert got[1] == C.sizeof(_lib.DihedralArgs)
    assert got[2] == got[3] == 32 == C.sizeof(_lib.DihedralPeriodicParams)
    for k, f in enumerate(fields):
        assert got[4 + k] == getattr(_lib.DihedralArgs, f).offset, f
    at = 4 + len(fields)
    for k, f in enumerate(efields):
        assert got[at + k] == getattr(_lib.DihedralEntry, f).offset, f
    at += len(efields)
    for k, f in enumerate(pfields):
        assert got[at + k] == getattr(_lib.DihedralPeriodicParams, f).offset, f
    assert got[-1] == 24
    # the fields of azp_angle_args, with the dihedral names
    assert [(n.replace("dihedral", "angle"), t) for n, t, *_ in _lib.DihedralArgs._fields_] == [f[:2] for f in _lib.AngleArgs._fields_]


def test_abi_dihedral_symbols_and_argument_errors():
    lib = _lib.lib()
    for name in ("azp_dihedral_forces_periodic", "azp_dihedral_forces_opls", "azp_dihedral_periodic_params_make",
                 "azp_dihedral_periodic_params_unpack", "azp_dihedral_opls_params_make", "azp_dihedral_opls_params_unpack"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert lib.azp_version() == 2
    # Host memory stands in for the device arrays: every call below is refused (or has N = 0) before a launch.
    keep = (C.c_double * 64)()
    ptr = C.addressof(keep)

    def args(**kw):
        a = _lib.DihedralArgs()
        a.N, a.n_max, a.pitch, a.virial_pitch, a.n_dihedral_types = 4, 4, 4, 4, 1
        a.d_force = a.d_virial = a.d_pos = a.d_gpu_dihedrallist = a.d_gpu_n_dihedrals = ptr
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for name in ("azp_dihedral_forces_periodic", "azp_dihedral_forces_opls"):
        fn = getattr(lib, name)
        assert fn(None, ptr, None) == -1
        assert fn(C.byref(_lib.DihedralArgs()), None, None) == 0          # N = 0: nothing to do, nothing looked at
        assert fn(C.byref(args(N=0, block_size=96)), ptr, None) == 0
        assert fn(C.byref(args()), None, None) == -1                     # no parameters
        for missing in ("d_force", "d_pos", "d_gpu_dihedrallist", "d_gpu_n_dihedrals"):
            assert fn(C.byref(args(**{missing: None})), ptr, None) == -1, missing
        assert fn(C.byref(args(compute_virial=1, d_virial=None)), ptr, None) == -1
        assert fn(C.byref(args(compute_virial=1, virial_pitch=3)), ptr, None) == -1
        assert fn(C.byref(args(pitch=3)), ptr, None) == -1
        assert fn(C.byref(args(n_dihedral_types=0)), ptr, None) == -1
        for bs in (1, 32, 96, 192, 320, 512):
            assert fn(C.byref(args(block_size=bs)), ptr, None) == -1, bs
        assert fn(C.byref(args(n_dihedral_types=2049)), ptr, None) == _lib.ERROR_TOO_MANY_TYPES   # 32 B each: > 64 KiB


def test_parameter_folds():
    lib = _lib.lib()
    p = _lib.DihedralPeriodicParams()
    lib.azp_dihedral_periodic_params_make(10.0, -1, 3, 0.6, C.addressof(p))
    assert p.k == 10.0 and p.d == -1 and p.n == 3
    assert abs(p.cos_phi0 - math.cos(0.6)) <= math.ulp(1.0) and abs(p.sin_phi0 - math.sin(0.6)) <= math.ulp(1.0)
    k, phi0, d, n = C.c_double(), C.c_double(), C.c_int(), C.c_uint()
    lib.azp_dihedral_periodic_params_unpack(C.addressof(p), C.byref(k), C.byref(d), C.byref(n), C.byref(phi0))
    assert k.value == 10.0 and d.value == -1 and n.value == 3 and abs(phi0.value - 0.6) < 1e-15
    out = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    lib.azp_dihedral_opls_params_make(1.5, -2.5, 3.5, 4.5, C.addressof(out))
    assert list(out) == [1.5, -2.5, 3.5, 4.5]
    f = dihedral.Periodic()
    back = f._unpack(f._pack(dict(k=4.0, d=1, n=2, phi0=-1.25)))
    assert back["k"] == 4.0 and back["d"] == 1 and back["n"] == 2 and abs(back["phi0"] + 1.25) < 1e-15
    f = dihedral.OPLS()
    assert f._unpack(f._pack(dict(k1=0.1, k2=-0.2, k3=0.3, k4=-0.4))) == dict(k1=0.1, k2=-0.2, k3=0.3, k4=-0.4)


def test_python_validation_periodic():
    f = dihedral.Periodic()
    assert isinstance(f, dihedral.Dihedral) and f.block_size == 0 and not f.compute_virial
    assert not hasattr(dihedral.Dihedral, "_cpp_class_name") or dihedral.Dihedral._cpp_class_name is None
    f.params["A-A-A-A"] = dict(k=10, d=1, n=2, phi0=0)
    assert f.params["A-A-A-A"] == dict(k=10.0, d=1, n=2, phi0=0.0)
    f.params["A-A-A-A"] = dict(k=-1.0, d=-1.0, n=3.0, phi0=-4.0)
    for bad in (dict(k=1.0, d=0, n=1, phi0=0.0), dict(k=1.0, d=2, n=1, phi0=0.0), dict(k=1.0, d=1, n=0, phi0=0.0),
                dict(k=1.0, d=1, n=1.5, phi0=0.0), dict(k=1.0, d=1, n=-2, phi0=0.0), dict(k=float("inf"), d=1, n=1, phi0=0.0),
                dict(k=float("nan"), d=1, n=1, phi0=0.0), dict(k=1.0, d=1, n=1, phi0=float("nan")),
                dict(k=1.0, d=1, n=float("nan"), phi0=0.0)):
        with pytest.raises(ValueError):
            f.params["A-A-A-A"] = bad
    with pytest.raises(ValueError):
        f.params["A-A-A-A"] = dict(k=1.0, d=1, n=1)                       # phi0 missing
    with pytest.raises(ValueError):
        f.params["A-A-A-A"] = dict(k=1.0, d=1, n=1, phi0=0.0, t0=1.0)     # unknown key
    with pytest.raises(TypeError):
        f.params["A-A-A-A"] = dict(k="stiff", d=1, n=1, phi0=0.0)
    assert f.params["A-A-A-A"] == dict(k=-1.0, d=-1, n=3, phi0=-4.0)     # a refused value changes nothing
    with pytest.raises(_lib.AzpError, match="not attached"):
        f.compute()


def test_python_validation_opls():
    f = dihedral.OPLS()
    assert isinstance(f, dihedral.Dihedral) and f.block_size == 0
    f.params["A-A-A-A"] = dict(k1=1, k2=-2, k3=0, k4=4.5)
    assert f.params["A-A-A-A"] == dict(k1=1.0, k2=-2.0, k3=0.0, k4=4.5)
    for bad in (dict(k1=float("nan"), k2=0.0, k3=0.0, k4=0.0), dict(k1=0.0, k2=0.0, k3=0.0, k4=float("inf"))):
        with pytest.raises(ValueError):
            f.params["A-A-A-A"] = bad
    with pytest.raises(ValueError):
        f.params["A-A-A-A"] = dict(k1=1.0, k2=1.0, k3=1.0)               # k4 missing
    with pytest.raises(ValueError):
        f.params["A-A-A-A"] = dict(k1=1.0, k2=1.0, k3=1.0, k4=1.0, k5=1.0)
    assert f.params["A-A-A-A"] == dict(k1=1.0, k2=-2.0, k3=0.0, k4=4.5)
    with pytest.raises(_lib.AzpError, match="not attached"):
        f.compute()


class _FakeState:
    dihedral_types = ["A-A-A-A", "B-B-B-B"]
    device = "cpu"


def test_unset_parameters_raise():
    f = dihedral.OPLS()
    f.params["A-A-A-A"] = dict(k1=1.0, k2=2.0, k3=3.0, k4=4.0)
    f._state = _FakeState()
    with pytest.raises(_lib.AzpError, match=r"OPLS.params\['B-B-B-B'\] is not set"):
        f._build_tables()
    f.params["B-B-B-B"] = dict(k1=-1.0, k2=0.0, k3=0.5, k4=0.0)
    f._build_tables()
    assert f._tables.tolist() == [[1.0, 2.0, 3.0, 4.0], [-1.0, 0.0, 0.5, 0.0]]
    p = dihedral.Periodic()
    p._state = _FakeState()
    with pytest.raises(_lib.AzpError, match=r"Periodic.params\['A-A-A-A'\] is not set"):
        p._build_tables()
