"""azplugins_amd.special_pair and azp_rdf_subtract_excluded without a GPU: the ABI of their argument structs, the
calls the library refuses before it launches anything, the parameter fold and what ``params`` / ``r_cut`` accept."""

import ctypes as C
import math
import os
import subprocess
import tempfile

import pytest

from azplugins_amd import _lib, special_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_numbers(body):
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "azp.h"\nint main(){' + body + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        return [int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split()]


def test_abi_struct_layouts():
    fields = ["d_force", "d_virial", "virial_pitch", "N", "n_max", "d_pos", "box", "d_gpu_pairlist", "d_gpu_pair_pos", "d_gpu_n_pairs",
              "pitch", "n_pair_types", "compute_virial", "block_size"]
    xfields = ["rdf", "d_n_excl", "d_excl", "excl_pitch"]
    got = _c_numbers('printf("%zu\\n%zu\\n%zu\\n%zu\\n", sizeof(azp_special_pair_args), sizeof(azp_special_pair_lj_params), '
                     'sizeof(azp_rdf_exclusion_args), sizeof(azp_bond_args));'
                     + "".join('printf("%%zu\\n", offsetof(azp_special_pair_args, %s));' % f for f in fields)
                     + "".join('printf("%%zu\\n", offsetof(azp_rdf_exclusion_args, %s));' % f for f in xfields))
    assert got[0] == C.sizeof(_lib.PairGroupArgs) and got[1] == 32
    assert got[2] == C.sizeof(_lib.RdfExclusionArgs) == C.sizeof(_lib.RdfArgs) + 24
    assert got[3] == C.sizeof(_lib.BondArgs)      # azp_bond_args is as it was
    for k, f in enumerate(fields):
        assert got[4 + k] == getattr(_lib.PairGroupArgs, f).offset, f
    for k, f in enumerate(xfields):
        assert got[4 + len(fields) + k] == getattr(_lib.RdfExclusionArgs, f).offset, f


def test_special_pair_argument_errors():
    lib = _lib.lib()
    for name in ("azp_special_pair_forces_lj", "azp_special_pair_lj_params_make", "azp_special_pair_lj_params_unpack"):
        assert name in _lib.SYMBOLS and getattr(lib, name) is not None
    # Host memory stands in for the device arrays: every call below is refused (or has N = 0) before a launch.
    keep = (C.c_double * 64)()
    ptr = C.addressof(keep)

    def args(**kw):
        a = _lib.PairGroupArgs()
        a.N, a.n_max, a.pitch, a.virial_pitch, a.n_pair_types = 4, 4, 4, 4, 1
        a.d_force = a.d_virial = a.d_pos = a.d_gpu_pairlist = a.d_gpu_pair_pos = a.d_gpu_n_pairs = ptr
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    fn = lib.azp_special_pair_forces_lj
    assert fn(None, ptr, None) == -1
    assert fn(C.byref(_lib.PairGroupArgs()), None, None) == 0          # N = 0: nothing to do, nothing looked at
    assert fn(C.byref(args(N=0, block_size=96)), ptr, None) == 0
    assert fn(C.byref(args()), None, None) == -1                       # no parameters
    for missing in ("d_force", "d_pos", "d_gpu_pairlist", "d_gpu_pair_pos", "d_gpu_n_pairs"):
        assert fn(C.byref(args(**{missing: None})), ptr, None) == -1, missing
    assert fn(C.byref(args(compute_virial=1, d_virial=None)), ptr, None) == -1
    assert fn(C.byref(args(compute_virial=1, virial_pitch=3)), ptr, None) == -1
    assert fn(C.byref(args(pitch=3)), ptr, None) == -1
    assert fn(C.byref(args(n_pair_types=0)), ptr, None) == -1
    for bs in (1, 32, 96, 320, 512):
        assert fn(C.byref(args(block_size=bs)), ptr, None) == -1, bs
    assert fn(C.byref(args(n_pair_types=2049)), ptr, None) == _lib.ERROR_TOO_MANY_TYPES   # 32 B each: > 64 KiB


def test_rdf_subtract_argument_errors():
    lib = _lib.lib()
    assert "azp_rdf_subtract_excluded" in _lib.SYMBOLS
    keep = (C.c_double * 64)()
    ptr = C.addressof(keep)

    def args(**kw):
        x = _lib.RdfExclusionArgs()
        x.rdf.N, x.rdf.n_total, x.rdf.num_bins, x.rdf.r_max, x.rdf.scale = 4, 4, 8, 2.0, 4.0
        x.rdf.box = _lib.make_box((10.0, 10.0, 10.0), (0.0, 0.0, 0.0), [1, 1, 1])
        x.rdf.d_pos = x.rdf.d_out = x.d_n_excl = x.d_excl = ptr
        x.excl_pitch = 4
        for k, v in kw.items():
            obj, _, name = k.rpartition("__")
            setattr(getattr(x, obj) if obj else x, name, v)
        return x

    fn = lib.azp_rdf_subtract_excluded
    assert fn(None, None) == -1
    assert fn(C.byref(args(rdf__N=0, rdf__n_total=0)), None) == 0      # nothing to do
    for bad in (dict(rdf__r_max=0.0), dict(rdf__r_max=6.0), dict(rdf__num_bins=0), dict(rdf__num_bins=_lib.RDF_MAX_BINS + 1),
                dict(rdf__scale=0.0), dict(rdf__n_total=3), dict(rdf__d_out=None), dict(rdf__d_pos=None), dict(d_n_excl=None),
                dict(d_excl=None), dict(excl_pitch=3)):
        assert fn(C.byref(args(**bad)), None) == -1, bad


def test_parameter_fold_and_validation():
    lib = _lib.lib()
    out = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    lib.azp_special_pair_lj_params_make(0.5, 2.0, 3.0, C.addressof(out))
    assert list(out) == [4.0 * 0.5 * 2.0 ** 12, 4.0 * 0.5 * 2.0 ** 6, 9.0, 0.0]      # (powers of two: exact)
    f = special_pair.LJ()
    back = f._unpack(f._pack(dict(epsilon=1.3, sigma=0.9, r_cut=2.5)))
    assert abs(back["epsilon"] - 1.3) < 1e-14 and abs(back["sigma"] - 0.9) < 1e-15 and abs(back["r_cut"] - 2.5) < 1e-15
    assert f._unpack(f._pack(dict(epsilon=0.0, sigma=1.0, r_cut=1.0))) == dict(epsilon=0.0, sigma=0.0, r_cut=1.0)
    f.params["A-A"] = dict(epsilon=1, sigma=2)
    assert f.params["A-A"] == dict(epsilon=1.0, sigma=2.0)
    f.r_cut["A-A"] = 3
    assert f.r_cut["A-A"] == 3.0 and isinstance(f.r_cut["A-A"], float)
    with pytest.raises(KeyError):
        f.r_cut["B-B"]
    for bad in (dict(epsilon=1.0), dict(epsilon=1.0, sigma=1.0, r_cut=2.0), dict(epsilon=math.inf, sigma=1.0),
                dict(epsilon=1.0, sigma=-0.5), dict(epsilon=1.0, sigma=math.nan)):
        with pytest.raises((ValueError, TypeError)):
            f.params["A-A"] = bad
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError):
            f.r_cut["A-A"] = bad
    assert f._kind == "pair" and special_pair.LJ._entry == "azp_special_pair_forces_lj"
