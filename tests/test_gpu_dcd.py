"""GPU tier of the DCD path (csrc/dcd_kernels.h; ``dcd.read_dcd_frames_dev`` / ``encode_dcd_dev`` / ``write_dcd_dev``,
``batch.iterVoxelizeDCD``): the reference reader's float32 bits for every case, selection and frame list of
tests/golden/dcd_cases.npz, the reference writer's file bytes, the round trip, the streamed voxelizer feed and the decoder's guard."""
import os

import numpy as np
import pytest

from moleculekit_amd import _lib, batch, dcd

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = np.load(os.path.join(GOLDEN, "dcd_cases.npz"))
NAMES = [str(n) for n in G["names"]]
WRITTEN = [n for n in NAMES if n.startswith("w_")]
OBLIQUE = {"cell_cos_oblique", "w_n63_f5"}            # angles through asin / sin of something other than 0: within one ulp (libm)
REMARK = slice(180, 260)                              # the creation-time remark of the writer's header
POISON = 0xCD


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulp_close(a, b, dtype):
    a, b = np.asarray(a, dtype), np.asarray(b, dtype)
    return bool(np.all(np.abs(a - b) <= np.spacing(np.abs(b))))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("dcd_gpu")
    out = {}
    for n in NAMES:
        out[n] = str(d / (n + ".dcd"))
        with open(out[n], "wb") as fh:
            fh.write(G[n + "/bytes"].tobytes())
    return out


def selections(N):
    return [None, np.arange(N, dtype=np.int32)[::-1].copy(), np.arange(0, N, 3, dtype=np.int32), np.array([N // 2], np.int32)]


def frame_lists(F):
    return [None, np.arange(F)[::-1].copy(), np.arange(0, F, 3), np.arange(0, F, 7)] + ([np.array([3, 0, 3, 1])] if F >= 4 else [])


@pytest.mark.parametrize("name", NAMES)
def test_device_read_equals_the_reference(files, name, hip_ctx):
    full = G[name + "/a0/xyz"]
    F, N = full.shape[:2]
    for atoms in selections(N):
        for fr in frame_lists(F):
            idx = np.arange(F) if fr is None else fr
            want = full[idx] if atoms is None else full[idx][:, atoms]
            xyz, lengths, angles = dcd.read_dcd_frames_dev(files[name], frames=fr, atom_indices=atoms, ctx=hip_ctx)
            assert xyz.is_cuda and tuple(xyz.shape) == want.shape
            assert np.array_equal(bits(xyz.cpu().numpy()), bits(want))
            if name + "/a0/lengths" not in G:
                assert lengths is None and angles is None
            else:
                assert np.array_equal(bits(lengths), bits(G[name + "/a0/lengths"][idx]))
                if name in OBLIQUE:
                    assert ulp_close(angles, G[name + "/a0/angles"][idx], np.float32)
                else:
                    assert np.array_equal(bits(angles), bits(G[name + "/a0/angles"][idx]))


def test_scale_is_one_float32_multiplication(files, hip_ctx):
    full = G["w_n1000_f5/a0/xyz"]
    got = dcd.read_dcd_frames_dev(files["w_n1000_f5"], scale=10.0, ctx=hip_ctx)[0].cpu().numpy()
    with np.errstate(invalid="ignore"):
        want = full * np.float32(10)
    finite = np.isfinite(full)
    assert np.array_equal(bits(got)[finite], bits(want)[finite]) and np.array_equal(np.isnan(got), np.isnan(want))


def to_dev(a, ctx):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to(torch.device("cuda", ctx.device))


def written_inputs(name):
    L = G[name + "/in_lengths"] if name + "/in_lengths" in G else None
    A = G[name + "/in_angles"] if name + "/in_angles" in G else None
    istart, nsavc, delta = G[name + "/in_header"]
    return G[name + "/in_xyz"], L, A, int(istart), int(nsavc), float(delta)


def same_file(name, ours, theirs, F):
    """Every byte but the header's creation-time remark; the cosines of an oblique cell within one float64 ulp."""
    ours, theirs = np.frombuffer(ours, np.uint8), np.asarray(theirs)
    assert len(ours) == len(theirs)
    keep = np.ones(dcd.HEADER_BYTES, bool)
    keep[REMARK] = False
    assert np.array_equal(ours[:dcd.HEADER_BYTES][keep], theirs[:dcd.HEADER_BYTES][keep])
    assert ours[REMARK].tobytes().startswith(b"REMARKS Created ")
    a, b = ours[dcd.HEADER_BYTES:].reshape(F, -1), theirs[dcd.HEADER_BYTES:].reshape(F, -1)
    if name in OBLIQUE:
        assert np.array_equal(a[:, 52:], b[:, 52:]) and np.array_equal(a[:, :4], b[:, :4])
        assert ulp_close(a[:, 4:52].copy().view(np.float64), b[:, 4:52].copy().view(np.float64), np.float64)
    else:
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", WRITTEN)
def test_device_writer_equals_the_reference_written_file(name, hip_ctx, tmp_path):
    xyz, L, A, istart, nsavc, delta = written_inputs(name)
    F, N = xyz.shape[:2]
    d_xyz = to_dev(xyz, hip_ctx)
    image = dcd.encode_dcd_dev(d_xyz, L, A, ctx=hip_ctx)
    assert image.is_cuda and image.numel() == len(G[name + "/bytes"]) - dcd.HEADER_BYTES
    head = dcd.file_header(N, F, istart, nsavc, delta, L is not None)
    same_file(name, head + image.cpu().numpy().tobytes(), G[name + "/bytes"], F)
    for chunk in (None, 2):                                              # one call; chunks of 2 with a short last one
        p = str(tmp_path / ("%s_%s.dcd" % (name, chunk)))
        dcd.write_dcd_dev(p, d_xyz, L, A, istart=istart, nsavc=nsavc, delta=delta, chunk=chunk, ctx=hip_ctx)
        same_file(name, open(p, "rb").read(), G[name + "/bytes"], F)
        assert not [f for f in os.listdir(tmp_path) if ".tmp." in f]
        back = dcd.read_dcd_frames_dev(p, ctx=hip_ctx)[0]                # read back: the input tensor's bits
        assert np.array_equal(bits(back.cpu().numpy()), bits(xyz))
        assert dcd.read_header(p) == tuple(G[name + "/header"].tolist())


class Mol:
    pass


def test_dcdwrite_of_a_duck_typed_molecule(hip_ctx, tmp_path):
    xyz, L, A, istart, nsavc, delta = written_inputs("w_n9_f4")
    m = Mol()
    m.coords, m.box, m.boxangles = np.transpose(xyz, (1, 2, 0)), L.T, A.T
    m.step, m.fstep = np.arange(4) * 250 + 1000, 250 * 0.04888821 * 0.0409 / 1000
    p = str(tmp_path / "mol.dcd")
    dcd.DCDwrite(m, p, ctx=hip_ctx)
    got = np.fromfile(p, np.uint8)
    theirs = G["w_n9_f4/bytes"]
    assert np.array_equal(got[dcd.HEADER_BYTES:], theirs[dcd.HEADER_BYTES:]) and np.array_equal(got[:44], theirs[:44])
    assert abs(dcd.read_header(p)[2] - 0.0409) < 1e-6                     # (DELTA through fstep: float arithmetic, not the bits)


def test_guard_descriptor_past_the_uploaded_bytes(files, hip_ctx):
    """The decoder is told it has fewer bytes than the buffer really holds, so the last frames' descriptors point past that count (the
    buffer itself holds them safely): status 1, and the output's poison stays."""
    import torch
    p = files["w_n257_f5"]
    dev = torch.device("cuda", hip_ctx.device)
    desc, lo, hi, _ = dcd.chunk_desc(p, np.arange(5))
    sel, src = dcd.source_table(p, None, 257)
    d = desc.view(dcd.DESC_DTYPE).reshape(-1)
    limit = int(d["z_off"][3]) + 4 * 257 - 4                              # frame 3's z plane ends 4 bytes behind it; frame 4 lies beyond
    raw = to_dev(np.fromfile(p, np.uint8)[lo:hi], hip_ctx)
    out = torch.full((5 * 257 * 3 * 4,), POISON, dtype=torch.uint8, device=dev).view(torch.float32).view(5, 257, 3)
    st = torch.full((5,), -7, dtype=torch.int32, device=dev)
    d_desc, d_sel, d_src = to_dev(desc, hip_ctx), to_dev(sel, hip_ctx), to_dev(src, hip_ctx)
    _lib._check(_lib.load().mkamd_dcd_decode_dev(hip_ctx._h, torch.cuda.current_stream(dev).cuda_stream or None, raw.data_ptr(), limit,
                                                 d_desc.data_ptr(), 5, d_sel.data_ptr(), d_src.data_ptr(), 257, None, 257, 1.0, out.data_ptr(),
                                                 st.data_ptr()))
    torch.cuda.synchronize(dev)
    assert st.cpu().tolist() == [0, 0, 0, 1, 1]
    host = out.cpu().numpy()
    assert np.array_equal(bits(host[:3]), bits(G["w_n257_f5/a0/xyz"][:3]))
    assert (host[3:].view(np.uint8) == POISON).all()


@pytest.mark.parametrize("name,pbc", [("w_n257_f5", True), ("fixed_third", True), ("fixed_third_big", False), ("w_n64_f4_nocell", False)])
def test_streamed_voxelizer_feed_equals_the_host_arrays(files, name, pbc, hip_ctx):
    """Chunks of 2 (a short last one for 5 frames) into an 8^3 grid: bit-equal to iterVoxelizeTrajectory on the host-read arrays."""
    import torch
    xyz, lengths, _ = dcd.load_dcd(files[name])
    F, N = xyz.shape[:2]
    rng = np.random.default_rng(3)
    channels = np.where(rng.random((N, 3)) < 0.6, rng.choice([1.2, 1.7, 2.0], (N, 3)), 0.0).astype(np.float32)
    center, boxsize = xyz[0, N // 2].astype(np.float64), [8, 8, 8]          # (on an atom: the grid is not empty)
    coords = np.ascontiguousarray(np.transpose(xyz, (1, 2, 0)))
    box = np.ascontiguousarray(lengths.T) if pbc else None
    want = torch.cat([f for _, f in batch.iterVoxelizeTrajectory(coords, channels, center, boxsize, box=box, chunk=2, ctx=hip_ctx)]).cpu().numpy()
    assert want.shape[0] == F and want.any()
    for decode in ("gpu", "host"):
        for pipelined in (True, False):
            got_idx, got = [], []
            for idx, f in batch.iterVoxelizeDCD(files[name], channels, center, boxsize, pbc=pbc, chunk=2, ctx=hip_ctx, decode=decode,
                                                pipelined=pipelined):
                got_idx.append(np.asarray(idx))
                got.append(f)
            assert np.concatenate(got_idx).tolist() == list(range(F))
            assert np.array_equal(torch.cat(got).cpu().numpy().view(np.uint32), want.view(np.uint32)), (decode, pipelined)
    # a selection of frames and atoms through the device path
    atoms, fr = np.arange(0, N, 3), np.arange(F)[::-1].copy()
    sub = np.ascontiguousarray(coords[atoms][:, :, fr])
    want = torch.cat([f for _, f in batch.iterVoxelizeTrajectory(sub, channels[atoms], center, boxsize, box=None if box is None else box[:, fr],
                                                                 chunk=2, ctx=hip_ctx)]).cpu().numpy()
    got = torch.cat([f for _, f in batch.iterVoxelizeDCD(files[name], channels[atoms], center, boxsize, pbc=pbc, frames=fr, atom_indices=atoms,
                                                         chunk=2, ctx=hip_ctx)]).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
