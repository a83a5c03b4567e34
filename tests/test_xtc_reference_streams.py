"""Both XTC decoders -- the host one (csrc/xtc_reader.h) and the device one (csrc/xtc_gpu.h: k_xtc_scan walks a frame per lane,
k_xtc_expand decodes a group per thread) -- on streams the REFERENCE's writer compresses (oracle/xtcref.py): runs of small
atoms, the swap, changes of run length, steps of ``smallidx`` to both ends of its table, precisions 10 to 1e5, per-axis bit
fields, 64- and 65-bit mixed-radix numbers, 1 to 11 atoms.  The bar is what the reference's reader decodes from the same file,
bit for bit: coordinates, boxes, times, steps.

CPU tier: the seeded cases of tests/xtc_cases.py and a random sweep of small files, written and read by the reference codec
(built on demand from the reference tree), through the host decoder and the device kernels run by the host emulation (tests/emu).
GPU tier (-m gpu): the committed fixtures (tests/golden/xtc_reference, tests/golden/make_golden_xtc_reference.py) through
``read_xtc_frames_dev`` and ``iterVoxelizeXTC``, plus a large file and the sweep when oracle/_ref/libxtcref.so is there."""
import os
import struct

import numpy as np
import pytest

from moleculekit_amd import xtc
from tests import xtc_cases

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "xtc_reference")
FIX_NAMES = sorted(f[:-4] for f in os.listdir(FIX) if f.endswith(".xtc")) if os.path.isdir(FIX) else []
NAMED = [c.name for c in xtc_cases.named_cases()]
_REACH = {}


def _ref():
    from oracle import xtcref
    if not xtcref.available():
        pytest.skip("neither the reference tree nor oracle/_ref/libxtcref.so is there")
    return xtcref


def _fm(c):                          # [N, 3, F] (the host decoder's layout) -> [F, N, 3]
    return np.ascontiguousarray(np.transpose(c, (2, 0, 1)))


def _headers(fn):
    """The record headers, parsed here from the file's bytes: per frame (step, time, box, raw, precision, lo, hi, smallidx, nbytes)."""
    buf = open(fn, "rb").read()
    out, p = [], 0
    while p < len(buf):
        magic, n, step = struct.unpack(">iii", buf[p:p + 12])
        assert magic == 1995
        t, = struct.unpack(">f", buf[p + 12:p + 16])
        box = np.frombuffer(buf[p + 16:p + 52], ">f4").astype(np.float32).reshape(3, 3)
        p += 56
        if n <= 9:
            out.append(dict(step=step, time=t, box=box, raw=1))
            p += 12 * n
            continue
        prec, = struct.unpack(">f", buf[p:p + 4])
        lo = np.array(struct.unpack(">iii", buf[p + 4:p + 16]), np.int64)
        hi = np.array(struct.unpack(">iii", buf[p + 16:p + 28]), np.int64)
        smallidx, nbytes = struct.unpack(">ii", buf[p + 28:p + 36])
        out.append(dict(step=step, time=t, box=box, raw=0, precision=prec, lo=lo, hi=hi, smallidx=smallidx, nbytes=nbytes))
        p += 36 + (nbytes + 3) // 4 * 4
    return out


def _check_desc(fn, desc):
    """chunk_desc's fields against the record headers: smallidx, the mixed-radix width (or per-axis fields), raw, ranges."""
    d = np.ascontiguousarray(desc).view(xtc.DESC_DTYPE).reshape(-1)
    for f, h in enumerate(_headers(fn)):
        assert int(d["raw"][f]) == h["raw"]
        if h["raw"]:
            continue
        rng = h["hi"] - h["lo"] + 1
        assert int(d["smallidx"][f]) == h["smallidx"] and int(d["nbytes"][f]) == h["nbytes"]
        assert np.array_equal(d["lo"][f], h["lo"]) and np.array_equal(d["range"][f], rng)
        if (rng > 0xffffff).any():
            assert int(d["triple_bits"][f]) == 0
            assert [int(v) for v in d["field_bits"][f]] == [int(v).bit_length() for v in rng]
        else:
            assert int(d["triple_bits"][f]) == (int(rng[0]) * int(rng[1]) * int(rng[2])).bit_length()
        assert d["inv_precision"][f] == np.float32(1.0 / float(np.float32(h["precision"])))


def _check_device(fn, ref_coords, N, sel=None):
    """The emulated device decoder against the reference's coordinates: status 0 and the same bits for every frame the headers
    say the device takes; a refused frame is either decoded exactly the same (status 0) or refused (status 2) -- 2 where its
    numbers exceed 64 bits -- and never anything else.  Returns the walk's reach."""
    got, st, desc, grp, ng = xtc_cases.device_decode_emulated(fn, sel, scale=1.0, groups=True)
    d = desc.view(xtc.DESC_DTYPE).reshape(-1)
    for f in range(len(st)):
        ok = xtc.device_decodable(desc[f:f + 1], N)
        if ok or st[f] == 0:
            assert st[f] == 0, (os.path.basename(fn), f, int(st[f]))
            assert np.array_equal(got[f].view(np.uint32), ref_coords[f].view(np.uint32)), (os.path.basename(fn), f)
        else:
            assert st[f] == 2, (os.path.basename(fn), f, int(st[f]))
        if d["triple_bits"][f] > 64:
            assert st[f] == 2 and not ok
    if xtc.device_decodable(desc, N):
        assert not st.any()
    return xtc_cases.reach(grp, ng, st, desc), st, desc


def _check_file(fn, N, rng):
    """One reference-written file through everything on the CPU tier; -> the walk's reach."""
    xtcref = _ref()
    rc, rb, rt, rs, _ = xtcref.ref_read_xtc(fn, N)
    F = rc.shape[0]
    assert xtc.get_xtc_natoms(fn) == N and xtc.get_xtc_nframes(fn) == F
    for nt in (1, 0):
        c, b, t, s = xtc.read_xtc(fn, nthreads=nt)
        assert np.array_equal(_fm(c).view(np.uint32), rc.view(np.uint32)), (os.path.basename(fn), nt)
        assert np.array_equal(_fm(b), rb) and np.array_equal(t, rt) and np.array_equal(s, rs)
    sel = rng.choice(F, size=int(rng.integers(1, F + 2)), replace=True)
    for nt in (1, 0):
        c, b, t, s = xtc.read_xtc_frames(fn, sel, nthreads=nt)
        assert np.array_equal(_fm(c).view(np.uint32), rc[sel].view(np.uint32)) and np.array_equal(_fm(b), rb[sel])
        assert np.array_equal(t, rt[sel]) and np.array_equal(s, rs[sel])
    desc, lo, hi, b, t, s = xtc.chunk_desc(fn, np.arange(F), N)
    assert np.array_equal(_fm(b), rb) and np.array_equal(t, rt) and np.array_equal(s, rs)
    _check_desc(fn, desc)
    r, st, _ = _check_device(fn, rc, N)
    _check_device(fn, rc[sel], N, sel)
    return r


@pytest.mark.parametrize("name", NAMED)
def test_reference_written_case_bit_exact_in_both_decoders(name, tmp_path):
    """Every seeded case of tests/xtc_cases.py: written by the reference, decoded by the host decoder (all frames, a random
    selection with repeats, 1 and all threads) and by the device kernels (emulated) exactly as the reference reads it."""
    case = {c.name: c for c in xtc_cases.named_cases()}[name]
    _ref()
    fn = xtc_cases.write(case, tmp_path / (name + ".xtc"))
    r = _check_file(fn, case.coords.shape[1], np.random.default_rng(len(name)))
    _REACH[name] = r
    print(f"\n[reach] {name:16s} max small/group {r['max_small']}  smallidx {r['idx_lo']}..{r['idx_hi']}  flagged groups "
          f"{r['flagged']}  runs across a refill {r['run_across_refill']}")


def test_cases_together_reach_every_state_of_the_walk(tmp_path):
    """The named cases together drive the walk through: smallidx 9 (the table's first usable entry) and >= 65, groups of 8 small
    atoms (the writer's maximum), a run whose bits cross a window refill, flagged groups -- checked on the group records of
    the emulated k_xtc_scan, so a generator that stops reaching its state fails here rather than testing less unnoticed."""
    _ref()
    for c in xtc_cases.named_cases():
        if c.name not in _REACH:
            fn = xtc_cases.write(c, tmp_path / (c.name + ".xtc"))
            xtcref = _ref()
            _REACH[c.name] = _check_device(fn, xtcref.ref_read_xtc(fn, c.coords.shape[1])[0], c.coords.shape[1])[0]
    rs = list(_REACH.values())
    lo = min(r["idx_lo"] for r in rs if r["idx_lo"] is not None)
    hi = max(r["idx_hi"] for r in rs if r["idx_hi"] is not None)
    assert lo == 9 and hi >= 65
    assert max(r["max_small"] for r in rs) == 8
    assert sum(r["run_across_refill"] for r in rs) > 0 and sum(r["flagged"] for r in rs) > 0


def test_random_sweep_of_reference_written_files(tmp_path):
    """~200 small files drawn at random from the generators and their knobs (atom counts 1 to ~240, 1-4 frames, precisions 10
    to 1e5 per file or per frame, frames of different generators mixed in one file)."""
    _ref()
    rng = np.random.default_rng(2024)
    for i in range(200):
        c = xtc_cases.random_case(rng, i)
        fn = xtc_cases.write(c, tmp_path / f"s{i}.xtc")
        _check_file(fn, c.coords.shape[1], rng)
        os.remove(fn)


@pytest.mark.parametrize("N", [1, 2])
def test_chunk_desc_of_one_and_two_atom_files(N, tmp_path):
    """A raw record of n <= 9 atoms is 56 + 12 n bytes: with 1 or 2 atoms the file's last frame ends before the 92 bytes a
    compressed header takes -- chunk_desc (the probe of iterVoxelizeXTC(decode="auto") and the host half of the device decoder)
    must take every frame, the last one included, and the emulated device decoder read them as the reference does."""
    xtcref = _ref()
    c = xtc_cases.few_atoms(np.random.default_rng(N), N, F=3)
    fn = xtc_cases.write(c, tmp_path / "few.xtc")
    rc = xtcref.ref_read_xtc(fn, N)[0]
    for sel in (np.arange(3), np.array([2]), np.array([2, 0])):
        desc, lo, hi, b, t, s = xtc.chunk_desc(fn, sel, N)
        if 2 in sel:
            assert hi == os.path.getsize(fn)
        assert (desc.view(xtc.DESC_DTYPE)["raw"] == 1).all()
        got, st, _ = xtc_cases.device_decode_emulated(fn, sel)
        assert not st.any() and np.array_equal(got, rc[sel])
    assert xtc.device_decodable(xtc.chunk_desc(fn, np.arange(3), N)[0], N)


def test_zigzag_file_is_refused_by_the_headers_and_by_the_device(tmp_path):
    """40 atoms alternating between two points 1 000 nm apart per axis: ranges of ~1e6 quanta (a 60-bit triple, which the device
    takes) but a header smallidx of 65 -- its runs are coded in 65 bits, which it does not.  device_decodable must say so (the
    choice of iterVoxelizeXTC(decode="auto")), the emulated walk must refuse every frame (status 2) and the host decoder read it."""
    xtcref = _ref()
    c = xtc_cases.zigzag()
    fn = xtc_cases.write(c, tmp_path / "zigzag.xtc")
    rc = xtcref.ref_read_xtc(fn, 40)[0]
    assert np.array_equal(_fm(xtc.read_xtc(fn)[0]), rc)
    got, st, desc = xtc_cases.device_decode_emulated(fn)
    d = desc.view(xtc.DESC_DTYPE)
    assert (d["smallidx"] == 65).all() and (d["triple_bits"] == 60).all()
    assert list(st) == [2, 2] and np.isnan(got).all()
    assert not xtc.device_decodable(desc, 40)


@pytest.mark.parametrize("name", FIX_NAMES)
def test_committed_fixtures_decode_like_the_reference(name):
    """The committed fixtures (what the GPU tier reads) still decode, on the CPU tier, to what the reference read from them."""
    fn = os.path.join(FIX, name + ".xtc")
    g = np.load(os.path.join(FIX, name + "_decoded.npz"))
    N = g["coords"].shape[1]
    c, b, t, s = xtc.read_xtc(fn)
    assert np.array_equal(_fm(c).view(np.uint32), g["coords"].view(np.uint32))
    assert np.array_equal(_fm(b), g["box"]) and np.array_equal(t, g["time"]) and np.array_equal(s, g["step"])
    _check_device(fn, g["coords"], N)


# ------------------------------------------------------------------------------------------------
# GPU tier
# ------------------------------------------------------------------------------------------------
def _dev_check(fn, ref_coords, rb, rt, rs, N, hip_ctx, sel=None):
    """read_xtc_frames_dev against the reference and the host decoder; a file the headers refuse may instead raise."""
    F = ref_coords.shape[0]
    sel = np.arange(F) if sel is None else sel
    desc = xtc.chunk_desc(fn, sel, N)[0]
    try:
        xyz, b, t, s = xtc.read_xtc_frames_dev(fn, sel, scale=1.0, ctx=hip_ctx)
    except RuntimeError as e:
        assert not xtc.device_decodable(desc, N) and "outside what the device decoder takes" in str(e), (os.path.basename(fn), str(e))
        return False
    host = _fm(xtc.read_xtc_frames(fn, sel)[0])
    got = xyz.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), ref_coords[sel].view(np.uint32)), os.path.basename(fn)
    assert np.array_equal(got.view(np.uint32), host.view(np.uint32))
    assert np.array_equal(_fm(b), rb[sel]) and np.array_equal(t, rt[sel]) and np.array_equal(s, rs[sel])
    return True


@pytest.mark.gpu
def test_gpu_device_decoder_on_reference_fixtures(hip_ctx):
    """read_xtc_frames_dev on every committed fixture: the reference's bits and the host decoder's, for all frames and a reversed
    selection; every file the headers accept is decoded (the 1- and 2-atom files among them), the zig-zag and 65-bit files raise."""
    decoded = set()
    for name in FIX_NAMES:
        fn = os.path.join(FIX, name + ".xtc")
        g = np.load(os.path.join(FIX, name + "_decoded.npz"))
        N, F = g["coords"].shape[1], g["coords"].shape[0]
        ok = _dev_check(fn, g["coords"], g["box"], g["time"], g["step"], N, hip_ctx)
        if ok:
            decoded.add(name)
            _dev_check(fn, g["coords"], g["box"], g["time"], g["step"], N, hip_ctx, np.arange(F)[::-1])
        if xtc.device_decodable(xtc.chunk_desc(fn, np.arange(F), N)[0], N):
            assert ok, name
    assert {"atoms1", "atoms2", "water", "chain_001", "flag_free", "triple64", "per_axis_x"} <= decoded
    assert "zigzag" not in decoded and "triple65" not in decoded


def _voxelize(fn, decode, pbc=False, frames=None, chunk=2):
    import torch
    from moleculekit_amd import batch
    N = xtc.get_xtc_natoms(fn)
    rng = np.random.default_rng(N)
    sig = np.where(rng.random((N, 4)) < 0.5, rng.choice([1.1, 1.52, 1.7], size=(N, 1)), 0.0)
    sig[0] = 1.6
    center = xtc.read_xtc_frames(fn, np.array([0]))[0][:, :, 0].mean(0).astype(np.float64) * 10.0
    out = [f for _, f in batch.iterVoxelizeXTC(fn, sig, center, [12, 12, 12], 1.0, pbc=pbc, frames=frames, chunk=chunk, decode=decode)]
    torch.cuda.synchronize()
    return torch.cat(out).cpu().numpy()


@pytest.mark.gpu
def test_gpu_iter_voxelize_xtc_on_reference_streams(hip_ctx):
    """iterVoxelizeXTC: on the water box with runs and the swap, decode="gpu" and "auto" give the feature bits of decode="host";
    on the 1- and 2-atom files "gpu" and "auto" too; on the zig-zag file "auto" picks the host (the same bits) and "gpu" raises
    instead of yielding features."""
    water = os.path.join(FIX, "water.xtc")
    for pbc in (False, True):
        want = _voxelize(water, "host", pbc=pbc)
        assert want.any()
        for decode in ("gpu", "auto"):
            assert np.array_equal(_voxelize(water, decode, pbc=pbc), want), (pbc, decode)
    for name in ("atoms1", "atoms2"):
        fn = os.path.join(FIX, name + ".xtc")
        want = _voxelize(fn, "host")
        for decode in ("gpu", "auto"):
            assert np.array_equal(_voxelize(fn, decode), want), (name, decode)
    zz = os.path.join(FIX, "zigzag.xtc")
    assert np.array_equal(_voxelize(zz, "auto"), _voxelize(zz, "host"))
    with pytest.raises(RuntimeError, match="outside what the device"):
        _voxelize(zz, "gpu")


@pytest.mark.gpu
def test_gpu_zigzag_file_raises_from_read_xtc_frames_dev(hip_ctx):
    """The device decoder has no auto mode: for the zig-zag file (65-bit runs) it raises a clear error and returns nothing."""
    with pytest.raises(RuntimeError, match="outside what the device decoder takes"):
        xtc.read_xtc_frames_dev(os.path.join(FIX, "zigzag.xtc"), ctx=hip_ctx)


@pytest.mark.gpu
def test_gpu_large_reference_written_water_file(hip_ctx, tmp_path):
    """30 000 water-like atoms x 64 frames written by the reference at test time (~8 MB: not committed): many waves of the walk,
    many LDS windows per frame, every frame bit-exact with the reference reader and the host decoder."""
    from oracle import xtcref
    if not os.path.exists(xtcref.oracle.XTCREF_PATH):
        pytest.skip("oracle/_ref/libxtcref.so was not built")
    c = xtc_cases.water(np.random.default_rng(77), nmol=10000, F=64)
    fn = xtc_cases.write(c, tmp_path / "water30k.xtc")
    rc, rb, rt, rs, _ = xtcref.ref_read_xtc(fn, 30000)
    assert _dev_check(fn, rc, rb, rt, rs, 30000, hip_ctx)
    assert _dev_check(fn, rc, rb, rt, rs, 30000, hip_ctx, np.arange(5, 64, 3))


@pytest.mark.gpu
def test_gpu_random_sweep_of_reference_written_files(hip_ctx, tmp_path):
    """The CPU tier's random sweep through the real device decoder (when oracle/_ref/libxtcref.so is there)."""
    from oracle import xtcref
    if not os.path.exists(xtcref.oracle.XTCREF_PATH):
        pytest.skip("oracle/_ref/libxtcref.so was not built")
    rng = np.random.default_rng(2024)
    n_dev = 0
    for i in range(200):
        c = xtc_cases.random_case(rng, i)
        fn = xtc_cases.write(c, tmp_path / f"s{i}.xtc")
        N = c.coords.shape[1]
        rc, rb, rt, rs, _ = xtcref.ref_read_xtc(fn, N)
        n_dev += _dev_check(fn, rc, rb, rt, rs, N, hip_ctx)
        os.remove(fn)
    assert n_dev >= 150
