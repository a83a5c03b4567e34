"""GPU tier of the device XTC writer (csrc/xtc_encode.h, ``xtc.encode_xtc_dev`` / ``write_xtc_dev``): the reference writer's file,
byte for byte, from the committed inputs (tests/golden/xtc_encode_inputs.npz -> tests/golden/xtc_reference/<name>.xtc); more than one
wave of walk lanes; chunks; refusal; and, when oracle/_ref/libxtcref.so is there, a large file and the random sweep written by the
reference at test time."""
import os
import struct

import numpy as np
import pytest

from moleculekit_amd import xtc
from tests import xtc_cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIX = os.path.join(GOLDEN, "xtc_reference")
REF_LIB = os.path.join(os.path.dirname(GOLDEN), "..", "oracle", "_ref", "libxtcref.so")
WHOLE = ["water", "water_one_frame", "chain_001", "chain_005_neg", "close_far", "flag_free", "precisions", "per_axis_x", "triple64",
         "atoms1", "atoms2", "atoms3", "atoms9", "atoms10", "atoms11"]
STATUS = {"triple65": [2, 2], "zigzag": [2, 2], "smallidx_ends": [0, 0, 0, 0, 2]}
_INPUTS = {}


def inputs(name):
    if not _INPUTS:
        with np.load(os.path.join(GOLDEN, "xtc_encode_inputs.npz")) as z:
            _INPUTS.update({k: z[k] for k in z.files})
    return _INPUTS[name + "__coords"], _INPUTS[name + "__box"], _INPUTS[name + "__precision"]


def fixture_bytes(name):
    with open(os.path.join(FIX, name + ".xtc"), "rb") as f:
        return f.read()


def record_ends(buf):
    ends, p = [0], 0
    while p < len(buf):
        n, = struct.unpack(">i", buf[p + 4:p + 8])
        p += 56 + 12 * n if n <= 9 else 92 + (struct.unpack(">i", buf[p + 88:p + 92])[0] + 3) // 4 * 4
        ends.append(p)
    return ends


def dev_args(coords, box, ctx):
    """``(xyz CUDA tensor [F, N, 3], box [3, 3, F], time, step)`` with the times and steps the fixtures were written with (0..F-1)."""
    import torch
    F = coords.shape[0]
    xyz = torch.as_tensor(np.ascontiguousarray(coords, np.float32)).to(torch.device("cuda", ctx.device))
    return xyz, np.ascontiguousarray(np.transpose(box, (1, 2, 0))), np.arange(F, dtype=np.float32), np.arange(F, dtype=np.int32)


def encode(coords, box, precision, ctx):
    image, offsets, status = xtc.encode_xtc_dev(*dev_args(coords, box, ctx), precision=precision, ctx=ctx)
    assert image.dtype.itemsize == 1 and image.is_cuda and offsets.dtype == np.int64 and status.dtype == np.int32
    assert image.numel() == offsets[-1]
    return image.cpu().numpy().tobytes(), offsets, status


@pytest.mark.parametrize("name", WHOLE)
def test_fixture_inputs_give_the_reference_writers_file(name, hip_ctx, tmp_path):
    coords, box, prec = inputs(name)
    want = fixture_bytes(name)
    got, offsets, status = encode(coords, box, prec, hip_ctx)
    assert status.tolist() == [0] * coords.shape[0]
    assert got == want and offsets.tolist() == record_ends(want)
    fn = tmp_path / (name + ".xtc")
    xtc.write_xtc_dev(fn, *dev_args(coords, box, hip_ctx), precision=prec, ctx=hip_ctx)
    assert fn.read_bytes() == want and os.listdir(tmp_path) == [name + ".xtc"]
    xtc.write_xtc_dev(fn, *dev_args(coords, box, hip_ctx), precision=prec, append=True, ctx=hip_ctx)
    assert fn.read_bytes() == want + want and os.listdir(tmp_path) == [name + ".xtc"]
    # what the device reader makes of the written file: the reference reader's coordinates, bit for bit
    fn.write_bytes(want)
    xtc.write_xtc_dev(fn, *dev_args(coords, box, hip_ctx), precision=prec, ctx=hip_ctx)
    with np.load(os.path.join(FIX, name + "_decoded.npz")) as z:
        ref = z["coords"]
    back = xtc.read_xtc_frames_dev(str(fn), ctx=hip_ctx)[0].cpu().numpy()
    assert back.dtype == np.float32 and back.tobytes() == ref.tobytes()


@pytest.mark.parametrize("name", sorted(STATUS))
def test_fixture_inputs_outside_the_device_path_get_status_2(name, hip_ctx):
    coords, box, prec = inputs(name)
    want = fixture_bytes(name)
    ends = record_ends(want)
    got, offsets, status = encode(coords, box, prec, hip_ctx)
    assert status.tolist() == STATUS[name]
    keep = [k for k, s in enumerate(STATUS[name]) if s == 0]
    assert got == b"".join(want[ends[k]:ends[k + 1]] for k in keep) and want.startswith(got)
    sizes = [ends[k + 1] - ends[k] if s == 0 else 0 for k, s in enumerate(STATUS[name])]
    assert offsets.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()


def tiled_water(F=70):
    coords, box, _ = inputs("water_one_frame")
    shift = (np.arange(F, dtype=np.float32)[:, None, None] * np.array([0.37, -0.21, 0.13], np.float32)).astype(np.float32)
    x = (np.repeat(coords, F, axis=0) + shift).astype(np.float32)
    return x, np.repeat(box, F, axis=0)


def test_more_than_one_wave_of_walk_lanes_with_a_partial_last_wave(hip_ctx, tmp_path):
    """70 frames of 1 002 atoms: two waves of walk lanes, six live lanes in the second.  Every frame's record equals the record of the
    same frame encoded alone (the header's time and step aside, which are the frame's own) -- and the reference's, when its codec is
    there."""
    x, box = tiled_water()
    F = x.shape[0]
    xyz, b, t, s = dev_args(x, box, hip_ctx)
    image, offsets, status = xtc.encode_xtc_dev(xyz, b, t, s, ctx=hip_ctx)
    assert status.tolist() == [0] * F
    got = image.cpu().numpy().tobytes()
    assert len({got[offsets[f] + 16:offsets[f + 1]] for f in range(F)}) == F          # (the shifts make every frame's record its own)
    for f in range(F):
        one, o1, s1 = xtc.encode_xtc_dev(xyz[f:f + 1], b[:, :, f:f + 1], t[f:f + 1], s[f:f + 1], ctx=hip_ctx)
        assert s1.tolist() == [0] and got[offsets[f]:offsets[f + 1]] == one.cpu().numpy().tobytes(), f
    if os.path.exists(REF_LIB):
        from oracle.xtcref import ref_write_xtc
        ref_write_xtc(tmp_path / "ref.xtc", x, box)
        assert got == (tmp_path / "ref.xtc").read_bytes()


def test_chunks_that_do_and_do_not_divide_the_frame_count_give_the_same_file(hip_ctx, tmp_path):
    x, box = tiled_water(12)
    args = dev_args(x, box, hip_ctx)
    xtc.write_xtc_dev(tmp_path / "whole.xtc", *args, ctx=hip_ctx)
    want = (tmp_path / "whole.xtc").read_bytes()
    assert len(record_ends(want)) == 13
    for chunk in (1, 4, 5, 12, 100):
        xtc.write_xtc_dev(tmp_path / "c.xtc", *args, chunk=chunk, ctx=hip_ctx)
        assert (tmp_path / "c.xtc").read_bytes() == want, chunk


def test_refusal_leaves_the_target_alone_and_the_context_usable(hip_ctx, tmp_path):
    coords, box, prec = inputs("zigzag")
    with pytest.raises(RuntimeError, match="outside what the device"):
        xtc.write_xtc_dev(tmp_path / "new.xtc", *dev_args(coords, box, hip_ctx), precision=prec, ctx=hip_ctx)
    assert os.listdir(tmp_path) == []
    (tmp_path / "old.xtc").write_bytes(b"what was there")
    for append in (False, True):
        with pytest.raises(RuntimeError, match="frame 0 .*outside what the device"):
            xtc.write_xtc_dev(tmp_path / "old.xtc", *dev_args(coords, box, hip_ctx), precision=prec, append=append, ctx=hip_ctx)
        assert os.listdir(tmp_path) == ["old.xtc"] and (tmp_path / "old.xtc").read_bytes() == b"what was there"
    coords, box, prec = inputs("water")
    assert encode(coords, box, prec, hip_ctx)[0] == fixture_bytes("water")


def test_hostile_values_on_the_device(hip_ctx):
    coords, box, _ = inputs("water_one_frame")
    x = np.repeat(coords, 4, axis=0)
    x[1, 5, 1], x[2, 17, 2] = np.nan, -np.inf
    x[3, 3, 0], x[3, 7, 0] = 2.1e6, -2.1e6
    got, offsets, status = encode(x, np.repeat(box, 4, axis=0), 1000.0, hip_ctx)
    assert status.tolist() == [0, 2, 2, 2]
    assert got == fixture_bytes("water_one_frame") and offsets.tolist() == [0] + [len(got)] * 4


def test_xtcwrite_of_a_molecule(hip_ctx, tmp_path):
    """``XTCwrite`` on a duck-typed molecule (Angstrom, fs): the bytes of the same arrays given to ``encode_xtc_dev`` in nm with the
    float32 0.1 as the scale, and the header fields of the reference's rules."""
    import types
    import torch
    coords, box, _ = inputs("water_one_frame")
    ang = np.ascontiguousarray(np.repeat(coords, 2, axis=0).transpose(1, 2, 0) * np.float32(10.0))      # [N, 3, F]
    bv = (np.repeat(box, 2, axis=0).transpose(1, 2, 0) * np.float32(10.0)).astype(np.float32)
    mol = types.SimpleNamespace(coords=ang, numFrames=2, box=np.zeros((3, 2)), boxvectors=bv, step=np.array([500, 1000]),
                                time=np.array([1000.0, 2000.0]), fstep=0.002)
    fn = tmp_path / "mol.xtc"
    fn.write_bytes(b"stale")
    xtc.XTCwrite(mol, str(fn), ctx=hip_ctx)
    xyz = torch.as_tensor(np.ascontiguousarray(ang.transpose(2, 0, 1))).to(torch.device("cuda", hip_ctx.device))
    image, offsets, status = xtc.encode_xtc_dev(xyz, (bv * 0.1).astype(np.float32), np.array([1.0, 2.0], np.float32), np.array([500, 1000]),
                                                scale=float(np.float32(0.1)), ctx=hip_ctx)
    got = fn.read_bytes()
    assert status.tolist() == [0, 0] and got == image.cpu().numpy().tobytes()
    assert struct.unpack(">iiif", got[:16]) == (1995, 1002, 500, 1.0) and struct.unpack(">f", got[56:60]) == (1000.0,)
    back = xtc.read_xtc_frames_dev(str(fn), ctx=hip_ctx)[0].cpu().numpy()
    assert np.abs(back - ang.transpose(2, 0, 1) * 0.1).max() <= 0.5e-3 + 1e-5


needs_ref = pytest.mark.skipif(not os.path.exists(REF_LIB), reason="oracle/_ref/libxtcref.so is not there")


@needs_ref
def test_large_water_against_the_reference_writer(hip_ctx, tmp_path):
    from oracle.xtcref import ref_write_xtc
    c = xtc_cases.water(np.random.default_rng(31), nmol=10000, F=8)
    ref_write_xtc(tmp_path / "ref.xtc", c.coords, c.box)
    got, offsets, status = encode(c.coords, c.box, 1000.0, hip_ctx)
    assert status.tolist() == [0] * 8 and got == (tmp_path / "ref.xtc").read_bytes()


@needs_ref
def test_random_sweep_against_the_reference_writer(hip_ctx, tmp_path):
    from tests.test_xtc_encode_cpu import split_records
    rng = np.random.default_rng(2024)
    whole = 0
    for i in range(200):
        c = xtc_cases.random_case(rng, i)
        fn = xtc_cases.write(c, tmp_path / "sweep.xtc")
        with open(fn, "rb") as f:
            recs = split_records(f.read())
        F = c.coords.shape[0]
        got, offsets, status = encode(c.coords, c.box, np.broadcast_to(np.asarray(c.precision, np.float32), (F,)), hip_ctx)
        assert status.tolist() == [2 if refused else 0 for _, refused in recs], c.name
        assert got == b"".join(r for r, refused in recs if not refused), c.name
        whole += not any(refused for _, refused in recs)
    assert whole >= 170
