"""azp_halo_pack_fields / azp_halo_unpack_fields (csrc/external_forces.hip: halo_fields_kernel, one lane per 4-byte word
of a packed row, every field on an 8-byte boundary, padding zeroed) through the C ABI against numpy byte slicing, and
DeviceDomain.pack / transfer on the device against their CPU branch. Everything is compared bit for bit: the arrays
hold random BITS (NaN payloads and denormals among the doubles).
"""


import numpy as np
import pytest

from azplugins_amd import _lib
from azplugins_amd import synthetic as syn

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = -1  # AZP_ERROR_INVALID_ARGUMENT (include/azp.h)
ROWS = 5000            # rows of every source array
GUARD_ROWS = 64
FILL, DST_FILL = 0xA5, 0x5A
SHAPE = {"pos": ((4,), np.float64), "vel": ((4,), np.float64), "orientation": ((4,), np.float64), "angmom": ((4,), np.float64),
         "inertia": ((3,), np.float64), "tag": ((), np.int32), "image": ((3,), np.int32)}
ROW_BYTES = {"pos": 32, "vel": 32, "orientation": 32, "angmom": 32, "inertia": 24, "tag": 4, "image": 12}


def source(name, rows=ROWS, seed=1):
    """``rows`` rows of random bits in the layout of the per-particle array ``name``."""
    shape, dtype = SHAPE[name]
    count = rows * int(np.prod(shape, dtype=np.int64))
    salt = sorted(SHAPE).index(name)
    bits = syn.hash64(seed + salt, np.arange(count, dtype=np.uint64), salt)
    if dtype == np.int32:
        bits = (bits >> np.uint64(32)).astype(np.uint32)
    return bits.view(dtype).reshape((rows,) + shape).copy()


def indices(n, seed=3):
    """int64, unsorted, with repeats."""
    idx = (syn.hash64(seed, np.arange(n, dtype=np.uint64), 2) % np.uint64(ROWS)).astype(np.int64)
    assert n < 1000 or (np.unique(idx).size < n and np.any(np.diff(idx) < 0))
    return idx


def packed_width(names):
    return sum((ROW_BYTES[f] + 7) // 8 * 8 for f in names)


def pack_ref(src, names, idx):
    """uint8 [n, packed row]: field after field, each on an 8-byte boundary, zeros between."""
    out = np.zeros((idx.size, packed_width(names)), dtype=np.uint8)
    off = 0
    for f in names:
        rb = ROW_BYTES[f]
        out[:, off: off + rb] = np.ascontiguousarray(src[f][idx]).view(np.uint8).reshape(idx.size, rb)
        off += (rb + 7) // 8 * 8
    return out


def field_table(ptrs, row_bytes, length=None):
    fields = (_lib.HaloField * (length or len(ptrs)))()
    for c, (p, rb) in enumerate(zip(ptrs, row_bytes)):
        fields[c].d_data = p
        fields[c].row_bytes = rb
    return fields


def bytes_of(t):
    import torch

    return t.view(torch.uint8).cpu().numpy().reshape(-1)


LAYOUTS = [(("pos", "tag", "image", "inertia"), 3333), (("tag",), 3333), (("pos", "vel"), 3333),
           (("pos", "vel", "orientation", "tag"), 3333), (("pos", "tag", "image", "inertia"), 1)]


@pytest.mark.parametrize("names,n", LAYOUTS, ids=lambda v: "+".join(v) if isinstance(v, tuple) else "n%d" % v)
def test_pack_and_unpack_are_byte_slicing(names, n):
    """Pack n rows picked by d_idx into a buffer pre-filled with 0xA5 (64 guard rows behind it), unpack them into
    sentinel-filled arrays at an offset of N rows, as DeviceDomain.transfer does."""
    import torch

    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    wbytes = packed_width(names)
    assert wbytes == {("pos", "tag", "image", "inertia"): 80, ("tag",): 8, ("pos", "vel"): 64, ("pos", "vel", "orientation", "tag"): 104}[names]
    assert n == 1 or (n * (wbytes // 4)) % 256 != 0  # (the last workgroup is ragged)
    src = {f: source(f) for f in names}
    dev = {f: torch.from_numpy(src[f]).to("cuda:0") for f in names}
    idx = indices(n)
    d_idx = torch.from_numpy(idx).to("cuda:0")
    packed = torch.full(((n + GUARD_ROWS) * wbytes,), FILL, dtype=torch.uint8, device="cuda:0")
    fields = field_table([dev[f].data_ptr() for f in names], [ROW_BYTES[f] for f in names])
    assert lib.azp_halo_pack_fields(n, len(names), fields, d_idx.data_ptr(), packed.data_ptr(), wbytes, stream) == 0
    torch.cuda.synchronize()
    got = bytes_of(packed)
    want = pack_ref(src, names, idx)
    assert np.all(got[n * wbytes:] == FILL)
    assert np.array_equal(got[: n * wbytes].reshape(n, wbytes), want)  # (fields, and zeros in every padding word)
    for f in names:
        assert np.array_equal(bytes_of(dev[f]), src[f].view(np.uint8).reshape(-1))

    N = 777
    dst = {f: torch.full(((N + n + GUARD_ROWS) * ROW_BYTES[f],), DST_FILL, dtype=torch.uint8, device="cuda:0") for f in names}
    fields = field_table([dst[f].data_ptr() + N * ROW_BYTES[f] for f in names], [ROW_BYTES[f] for f in names])
    assert lib.azp_halo_unpack_fields(n, len(names), fields, packed.data_ptr(), wbytes, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bytes_of(packed), got)
    for f in names:
        rb = ROW_BYTES[f]
        b = bytes_of(dst[f])
        assert np.all(b[: N * rb] == DST_FILL) and np.all(b[(N + n) * rb:] == DST_FILL), f
        assert np.array_equal(b[N * rb: (N + n) * rb], np.ascontiguousarray(src[f][idx]).view(np.uint8).reshape(-1)), f


def test_nothing_to_pack_is_a_success():
    lib = _lib.lib()
    assert lib.azp_halo_pack_fields(0, 0, None, None, None, 0, None) == 0
    assert lib.azp_halo_unpack_fields(0, 0, None, None, 0, None) == 0


def test_bad_arguments_are_refused_and_nothing_is_written():
    import torch

    lib = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    n = 100
    names = ("pos", "tag")
    src = {f: torch.from_numpy(source(f)).to("cuda:0") for f in names}
    before = {f: bytes_of(src[f]).copy() for f in names}
    d_idx = torch.from_numpy(indices(n)).to("cuda:0")
    packed = torch.full((n * 64,), FILL, dtype=torch.uint8, device="cuda:0")
    ptrs = [src[f].data_ptr() for f in names]
    good = dict(n_fields=2, ptrs=ptrs, rb=[32, 4], idx=d_idx.data_ptr(), packed=packed.data_ptr(), width=40)
    cases = {
        "no fields": dict(n_fields=0),
        "five fields": dict(n_fields=5, ptrs=ptrs + ptrs + ptrs[:1], rb=[32, 4, 32, 4, 32], width=120),
        "row_bytes 0": dict(rb=[32, 0], width=32),
        "row_bytes 6": dict(rb=[32, 6], width=40),
        "width is not the rounded sum": dict(width=48),
        "width is the unrounded sum": dict(width=36),
        "null d_packed": dict(packed=None),
        "null d_idx": dict(idx=None),
        "null field pointer": dict(ptrs=[ptrs[0], None]),
    }
    for what, change in cases.items():
        k = dict(good, **change)
        fields = field_table(k["ptrs"], k["rb"], length=5)
        rc = lib.azp_halo_pack_fields(n, k["n_fields"], fields, k["idx"], k["packed"], k["width"], stream)
        assert rc == INVALID_ARGUMENT, "pack: " + what
        if what != "null d_idx":  # (unpack takes no indices)
            rc = lib.azp_halo_unpack_fields(n, k["n_fields"], fields, k["packed"], k["width"], stream)
            assert rc == INVALID_ARGUMENT, "unpack: " + what
    assert lib.azp_halo_pack_fields(n, 2, None, d_idx.data_ptr(), packed.data_ptr(), 40, stream) == INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert np.all(bytes_of(packed) == FILL)
    for f in names:
        assert np.array_equal(bytes_of(src[f]), before[f])
    # (the good arguments are good)
    fields = field_table(good["ptrs"], good["rb"], length=5)
    assert lib.azp_halo_pack_fields(n, 2, fields, good["idx"], good["packed"], 40, stream) == 0
    torch.cuda.synchronize()
    assert np.all(bytes_of(packed)[: n * 40].reshape(n, 40)[:, 36:] == 0)


# ---------------------------------------------------------------------------
# DeviceDomain.pack / transfer: the device branch equals the CPU branch
# ---------------------------------------------------------------------------
EXCHANGES = [["pos"], ["pos", "vel"], ["pos", "orientation"], ["pos", "vel", "orientation", "tag"], ["pos", "image", "inertia"]]


@pytest.mark.parametrize("names", EXCHANGES, ids=lambda v: "+".join(v))
def test_domain_exchange_on_the_device_equals_the_cpu_branch(names):
    """One process, no process group: the all-to-all is a copy from the send to the receive buffer, so an exchange
    writes local row send_idx[k] into ghost row k. ["pos"] alone is received straight into the ghost region; every
    other list goes through the pack and unpack kernels on the device and through torch byte slicing on the CPU."""
    import torch

    from azplugins_amd.decomposition import Decomposition
    from azplugins_amd.domain import DeviceDomain

    N, n_ghost = 1201, 333
    all_names = ("pos", "vel", "orientation", "tag", "image", "inertia")
    host = {f: source(f, rows=N + n_ghost, seed=11) for f in all_names}
    send_idx = (syn.hash64(12, np.arange(n_ghost, dtype=np.uint64), 1) % np.uint64(N)).astype(np.int64)
    results = {}
    for device in ("cuda:0", "cpu"):
        arrays = {f: torch.from_numpy(host[f].copy()).to(device) for f in all_names}
        dom = DeviceDomain(Decomposition(np.array([20.0, 12.0, 12.0]), 2, 1.5), 0, arrays)
        dom.N_local, dom.n_ghost = N, n_ghost
        dom.send_idx = torch.from_numpy(send_idx).to(device)
        dom.send_splits, dom.recv_splits = [0, n_ghost], [0, n_ghost]
        dom.exchange(names)
        if device != "cpu":
            torch.cuda.synchronize()
        results[device] = {f: arrays[f].cpu().numpy() for f in all_names}
    for f in all_names:
        rb = ROW_BYTES[f]
        raw = {d: np.ascontiguousarray(results[d][f]).view(np.uint8).reshape(N + n_ghost, rb) for d in results}
        src = np.ascontiguousarray(host[f]).view(np.uint8).reshape(N + n_ghost, rb)
        assert np.array_equal(raw["cuda:0"], raw["cpu"]), f
        assert np.array_equal(raw["cuda:0"][:N], src[:N]), f
        assert np.array_equal(raw["cuda:0"][N:], src[send_idx] if f in names else src[N:]), f
