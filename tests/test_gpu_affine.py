"""GPU tier: the fused per-item affine of the voxelizer on the paths production takes (tests/test_affine_paths.py is the CPU tier and
pins, on the launch recorder, WHICH kernels the shapes below select -- all paths give the same bits, so no value seen here can).

Two references, on the device: ``align.apply_transforms`` writes float32(M x + t) and the same call with ``affine=None`` voxelizes
it -- the fused call must give those bits; the oracle on a sample of items gives the values, within cases.TOL.  The aligned
streams (``align=`` of iterVoxelizeTrajectory / iterVoxelizeXTC) run with a real-shaped channel matrix -- 8 channels, a handful of
distinct sigmas -- so that they take the topology handle, and with ions the split exact fix-up, as production does.
"""
import os

import numpy as np
import pytest

from tests.cases import TOL
from tests.synth import synth_sigmas
from tests.test_affine_paths import move_back, random_affines

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "align_cases.npz")
XTC = os.path.join(HERE, "golden", "xtc", "metricdistance_traj.xtc")


def _oracle_gap(feats, coords, sig, origin, nv):
    """feats [V, C] of one item against the oracle on its float32 coordinates"""
    from oracle import oracle
    centers = oracle.grid_centers(np.asarray(origin, np.float64), np.asarray(nv), 1.0)
    exp = oracle.calculate_occupancy(centers, np.ascontiguousarray(coords, np.float32), np.asarray(sig, np.float64))
    return float(np.abs(np.asarray(feats, np.float64) - exp).max())


def _molecule_sigmas(rng, n, n_ions):
    """a getChannels-shaped matrix: 8 channels, the atom's radius where a property holds -- five radii, plus 2.27 A (Na) and 2.75 A (K)
    on `n_ions` atoms spread over the molecule: 5 or 7 distinct sigmas"""
    sig = synth_sigmas(rng, n)
    if n_ions:
        ions = np.linspace(0, n - 1, n_ions).astype(int)
        sig[ions] = 0.0
        sig[ions, 7] = 2.27
        sig[ions[::2], 5] = 2.75
        sig[ions[::2], 7] = 2.75
    assert len(np.unique(sig[sig != 0])) <= 15
    return sig


# ---- the plain entry: shapes chosen by the rules of choose_lattice_path ------------------------------------------------------
GPU_SHAPES = {
    "one_molecule_24": dict(B=1, n=3000, nv=24),             # k_bin_solo, a team of waves per tile
    "ligands_64": dict(B=64, n=60, nv=24),                   # k_prepass_items, the workgroup-per-item kernel
    "items_8x2000_48": dict(B=8, n=2000, nv=48),             # k_prepass_items, a wave per tile
    "big_in_order": dict(B=40, n=6000, nv=24),               # k_bin_direct in front of the chain
    "big_promised": dict(B=40, n=6000, nv=24, promise=True),  # the chain beside the previous call's tile kernel, the lean tiles
}


@pytest.mark.parametrize("shape", list(GPU_SHAPES))
def test_plain_entry_with_affine_on_the_device(hip_ctx, shape):
    import torch
    from moleculekit_amd import align, batch
    s = GPU_SHAPES[shape]
    B, n, nvx, promise = s["B"], s["n"], s["nv"], s.get("promise", False)
    rng = np.random.default_rng(100 + B + n)
    dev = torch.device("cuda", hip_ctx.device)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
    spread = 3.0 if n <= 100 else None
    target = (rng.normal(nvx / 2, spread, size=(B * n, 3)) if spread else rng.uniform(-4.0, nvx + 4.0, size=(B * n, 3))).astype(np.float32)
    sig = np.concatenate([synth_sigmas(rng, n) for _ in range(B)]).astype(np.float32)
    sig[::211] = 0.0                                                                 # some wide atoms (one sigma each, so that the
    sig[::211, 3] = sig[::211, 7] = 2.27                                             # direct binning takes them): the exact fix-up runs
    offs = np.arange(B + 1, dtype=np.int64) * n
    A = random_affines(rng, B, identity_at=1 if B > 1 else -1)
    src = move_back(target, offs, A)
    origins = np.zeros((B, 3))
    nv = [nvx] * 3
    d_src, d_aff = t(src, np.float32), t(A, np.float64)
    applied = align.apply_transforms(d_src.view(B, n, 3), d_aff, ctx=hip_ctx).view(B * n, 3)
    d_offs, d_sig, d_org = t(offs, np.int64), t(sig, np.float32), t(origins, np.float64)
    torch.cuda.synchronize()
    hip_ctx.set_pipelining(False)
    n0 = hip_ctx.pipelined_calls()

    def run(coords, affine, **kw):
        outs = []
        for _ in range(2):                       # (twice on the context: the second big call in order is binned by k_bin_direct)
            if promise:
                hip_ctx.promise_inputs(None)
            outs.append(batch.voxelize_lattice_torch(coords, d_offs, d_sig, d_org, nv, 1.0, ctx=hip_ctx, affine=affine, **kw))
        return outs

    fused = run(d_src, d_aff)
    ref = run(applied, None)
    fused_cf = run(d_src, d_aff, channel_first=True)
    bare = batch.voxelize_lattice_torch(d_src, d_offs, d_sig, d_org, nv, 1.0, ctx=hip_ctx)
    torch.cuda.synchronize(); hip_ctx.synchronize()
    if promise:
        assert hip_ctx.pipelined_calls() - n0 == 6
    for f in fused + ref[1:]:
        assert torch.equal(f, ref[0])
    V = nvx ** 3
    for f in fused_cf:
        assert tuple(f.shape) == (B, 8, nvx, nvx, nvx)
        assert torch.equal(f.permute(0, 2, 3, 4, 1).reshape(B, V, 8), ref[0])
    assert float((fused[0] - bare).abs().max()) > 0.1                               # (a call that ignored the affine gives `bare`)
    a = applied.view(B, n, 3).cpu().numpy()
    got = fused[0].cpu().numpy()
    worst = max(_oracle_gap(got[b], a[b], sig[b * n:(b + 1) * n], origins[b], nv) for b in sorted({0, min(1, B - 1), B - 1}))
    print(f"{shape}: worst gap to the oracle {worst:.2e}")
    assert worst <= TOL


# ---- the topology entry ------------------------------------------------------------------------------------------------------
def _trajectory(rng, n, F, n_ions, nvx=24):
    """target frames [F, n, 3] of one molecule inside an nvx^3 grid at the origin; the ions on voxel centres (many voxels next to
    their cut-off shells)"""
    sig = _molecule_sigmas(rng, n, n_ions)
    base = rng.uniform(-3.0, nvx + 3.0, size=(n, 3))
    ion = (sig == 2.27).any(axis=1) | (sig == 2.75).any(axis=1)
    base[ion] = rng.integers(2, nvx - 2, size=(int(ion.sum()), 3))
    frames = base[None] + rng.normal(0, 0.3, size=(F, n, 3)) * (~ion)[None, :, None]
    return frames.astype(np.float32), sig


@pytest.mark.parametrize("F", [16, 300])
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("channel_first", [False, True])
def test_topology_entry_with_affine_on_the_device(hip_ctx, wide, F, channel_first):
    import torch
    from moleculekit_amd import _lib, align, batch
    n, nvx = 3000, 24
    rng = np.random.default_rng(7 + F + int(wide))
    dev = torch.device("cuda", hip_ctx.device)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
    target, sig = _trajectory(rng, n, F, 6 if wide else 0)
    offs = np.arange(F + 1, dtype=np.int64) * n
    A = random_affines(rng, F)
    src = move_back(target.reshape(F * n, 3), offs, A)
    topo = _lib.Topology(hip_ctx, sig, 1.0)
    assert topo.has_wide_sigmas == wide
    d_src, d_aff, d_offs, d_org = t(src, np.float32), t(A, np.float64), t(offs, np.int64), t(np.zeros((F, 3)), np.float64)
    applied = align.apply_transforms(d_src.view(F, n, 3), d_aff, ctx=hip_ctx).view(F * n, 3)
    torch.cuda.synchronize()
    hip_ctx.set_pipelining(False)
    nv = [nvx] * 3
    kw = dict(ctx=hip_ctx, channel_first=channel_first)
    fused = batch.voxelize_lattice_torch(d_src, d_offs, None, d_org, nv, 1.0, topology=topo, affine=d_aff, **kw)
    again = batch.voxelize_lattice_torch(d_src, d_offs, None, d_org, nv, 1.0, topology=topo, affine=d_aff, **kw)
    ref = batch.voxelize_lattice_torch(applied, d_offs, None, d_org, nv, 1.0, topology=topo, **kw)
    d_sig = t(sig, np.float64).repeat(F, 1).contiguous()
    plain = batch.voxelize_lattice_torch(d_src, d_offs, d_sig, d_org, nv, 1.0, affine=d_aff, **kw)
    bare = batch.voxelize_lattice_torch(d_src, d_offs, None, d_org, nv, 1.0, topology=topo, **kw)
    torch.cuda.synchronize(); hip_ctx.synchronize()
    assert torch.equal(fused, ref) and torch.equal(again, ref) and torch.equal(plain, ref)
    assert float((fused - bare).abs().max()) > 0.1
    got = fused.permute(0, 2, 3, 4, 1).reshape(F, nvx ** 3, 8) if channel_first else fused
    a = applied.view(F, n, 3).cpu().numpy()
    worst = max(_oracle_gap(got[f].cpu().numpy(), a[f], sig, np.zeros(3), nv) for f in (0, 1, F - 1))
    print(f"topology wide={wide} F={F} channel_first={channel_first}: worst gap to the oracle {worst:.2e}")
    assert worst <= TOL


# ---- iterVoxelizeTrajectory(align=...) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True])
def test_aligned_trajectory_stream_equals_aligned_then_voxelized(hip_ctx, wide):
    """host and device source, pipelined and in order, an unsorted ``frames=`` list, a chunk that does not divide it: each chunk's
    affine slice has to follow its frames, the short last chunk included"""
    import torch
    from moleculekit_amd import _lib, align, batch
    from tests.test_affine_paths import quat_rotation
    rng = np.random.default_rng(31 + int(wide))
    N, F, chunk = 3000, 37, 8
    dev = torch.device("cuda", hip_ctx.device)
    sig = _molecule_sigmas(rng, N, 6 if wide else 0).astype(np.float32)
    assert sig.shape[1] == 8 and len(np.unique(sig[sig != 0])) <= 15
    topo = _lib.Topology(hip_ctx, sig, 1.0)                          # what _stream_voxelize builds: it succeeds, so the streams below
    assert topo.has_wide_sigmas == wide                               # take the handle (and with ions the split fix-up)
    topo.close()
    base = rng.uniform(-14.0, 14.0, size=(N, 3))
    ion = (sig > 2.0).any(axis=1)
    base[ion] = rng.integers(-9, 10, size=(int(ion.sum()), 3))
    xyz = np.empty((F, N, 3), np.float32)
    for f in range(F):                                                # every frame somewhere else, turned some other way
        R = quat_rotation(rng.normal(size=4))
        xyz[f] = (base + rng.normal(0, 0.2, size=(N, 3)) * (~ion)[:, None]) @ R.T + rng.uniform(-80, 80, 3)
    sel = np.sort(rng.choice(N, 150, replace=False))
    ref = base[sel].astype(np.float32)
    frames = rng.permutation(F)[:29]
    assert len(frames) % chunk and not np.array_equal(frames, np.sort(frames))
    center, box = np.zeros(3), [24, 24, 24]
    coords = np.ascontiguousarray(xyz.transpose(1, 2, 0))             # [N, 3, F], Molecule.coords
    d_coords = torch.as_tensor(coords, device=dev)
    d_xyz = torch.as_tensor(xyz, device=dev)
    aligned = align.align_trajectory(d_xyz, torch.as_tensor(ref, device=dev), sel, np.arange(len(sel)), ctx=hip_ctx)
    a_coords = aligned.permute(1, 2, 0).contiguous()
    torch.cuda.synchronize()
    want_idx, want = [], []
    for idx, f in batch.iterVoxelizeTrajectory(a_coords, sig, center, box, 1.0, frames=frames, chunk=chunk, ctx=hip_ctx):
        want_idx.append(np.asarray(idx)); want.append(f)
    want = torch.cat(want)
    assert np.array_equal(np.concatenate(want_idx), frames)
    for name, src in (("host", coords), ("device", d_coords)):
        for piped in (True, False):
            got_idx, got = [], []
            for idx, f in batch.iterVoxelizeTrajectory(src, sig, center, box, 1.0, frames=frames, chunk=chunk, ctx=hip_ctx, pipelined=piped,
                                                       align=(ref, sel)):
                got_idx.append(np.asarray(idx)); got.append(f)
            torch.cuda.synchronize()
            assert [len(i) for i in got_idx] == [8, 8, 8, 5]
            assert np.array_equal(np.concatenate(got_idx), frames)
            assert torch.equal(torch.cat(got), want), (name, piped)
    plain = torch.cat([f for _, f in batch.iterVoxelizeTrajectory(coords, sig, center, box, 1.0, frames=frames[:8], chunk=chunk, ctx=hip_ctx)])
    assert float((plain - want[:8]).abs().max()) > 0.1               # (the alignment did something)
    a = aligned.cpu().numpy()
    worst = max(_oracle_gap(want[k].cpu().numpy(), a[frames[k]], sig, center - 12.0, box) for k in (0, 13, 28))
    print(f"aligned trajectory stream wide={wide}: worst gap to the oracle {worst:.2e}")
    assert worst <= TOL


# ---- iterVoxelizeXTC(align=...) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ramp", [0, 4])
@pytest.mark.parametrize("decode", ["gpu", "host"])
def test_aligned_xtc_stream_with_a_channel_matrix(hip_ctx, decode, ramp):
    import torch
    from moleculekit_amd import _lib, align, batch, xtc
    g = np.load(GOLDEN)
    ca = g["rmsd_ca_idx"]
    dev = torch.device("cuda", hip_ctx.device)
    frames = np.arange(3, 50)
    xyz, _, _, _ = xtc.read_xtc_frames_dev(XTC, frames, scale=10.0, ctx=hip_ctx)
    N = int(xyz.shape[1])
    sig = _molecule_sigmas(np.random.default_rng(5), N, 6).astype(np.float32)
    topo = _lib.Topology(hip_ctx, sig, 1.0)
    assert topo.has_wide_sigmas
    topo.close()
    ref = xyz[0, ca].cpu().numpy()
    center = ref.astype(np.float64).mean(0)
    box = [16, 16, 16]
    sizes, streamed = [], []
    for idx, f in batch.iterVoxelizeXTC(XTC, sig, center, box, 1.0, pbc=False, frames=frames, chunk=16, ctx=hip_ctx, align=(ref, ca),
                                        decode=decode, ramp=ramp):
        sizes.append(len(idx)); streamed.append(f)
    streamed = torch.cat(streamed)
    assert sizes == ([4, 8, 16, 16, 3] if ramp else [16, 16, 15])
    aligned = align.align_trajectory(xyz, torch.as_tensor(ref, device=dev), ca, np.arange(len(ca)), ctx=hip_ctx)
    coords = aligned.permute(1, 2, 0).contiguous()
    direct = torch.cat([f for _, f in batch.iterVoxelizeTrajectory(coords, sig, center, box, 1.0, chunk=16, ctx=hip_ctx)])
    torch.cuda.synchronize()
    assert torch.equal(streamed, direct)
    plain = torch.cat([f for _, f in batch.iterVoxelizeXTC(XTC, sig, center, box, 1.0, pbc=False, frames=frames[:16], chunk=16, ctx=hip_ctx)])
    assert not torch.equal(plain, streamed[:16])
    a = aligned.cpu().numpy()
    worst = max(_oracle_gap(streamed[k].cpu().numpy(), a[k], sig, center - 8.0, box) for k in (0, 21, 46))
    print(f"aligned XTC stream decode={decode} ramp={ramp}: worst gap to the oracle {worst:.2e}")
    assert worst <= TOL
