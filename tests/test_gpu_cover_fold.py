"""GPU tier: the cover fold (round 8; include/mkamd_voxel.h mkamd_ctx_set_cover_fold) -- a call that bins through
a topology handle tests an atom once where channel 7 of its group holds it with the sigma of another channel.  Every case compares,
bit for bit (``torch.equal``), the handle call with the fold on against the plain call (no handle) on the same inputs and against the
same handle with the knob off, on the shapes of tests/test_gpu_batch_topology.py: a ragged batch of five items (one empty, one absent
from every channel) on 16^3 and 24x16x8 grids, steered to the kernel chain and the one-wave tile kernels."""
import numpy as np
import pytest

from tests.test_gpu_batch_topology import GRIDS, SIZES, make_batch, tens

pytestmark = pytest.mark.gpu


@pytest.fixture
def chain(hip_ctx):
    hip_ctx.set_prepass_mode(0); hip_ctx.set_tile_team(0); hip_ctx.set_tile_items(0); hip_ctx.set_direct_binning(0)
    try:
        yield hip_ctx
    finally:
        hip_ctx.set_prepass_mode(-1); hip_ctx.set_tile_team(-1); hip_ctx.set_tile_items(-1); hip_ctx.set_direct_binning(-1)
        hip_ctx.set_tile_k(0); hip_ctx.set_lds_tier(-1); hip_ctx.set_cover_fold(0)
        hip_ctx.synchronize()


def three(ctx, xyz, offs, sig, nv, origin, sdt=np.float32, box=None, max_images=1, lo=None, hi=None, origins=None):
    """(plain call, handle call with the fold, handle call with the knob off, the handle's cover masks) on items [lo, hi)"""
    from moleculekit_amd import _lib, batch
    t = tens(ctx)
    B = len(offs) - 1
    lo, hi = (0, B) if lo is None else (lo, hi)
    a0, a1 = int(offs[lo]), int(offs[hi])
    topo = _lib.Topology(ctx, t(sig, sdt), 1.0, atom_offsets=offs)
    G = (sig.shape[1] + 7) // 8
    masks = [topo.cover_mask(g) for g in range(G)]
    d_xyz, d_offs, d_sig = t(xyz[a0:a1], np.float32), t(offs[lo:hi + 1] - a0, np.int64), t(sig[a0:a1], sdt)
    org = np.tile(np.asarray(origin, dtype=np.float64), (hi - lo, 1)) + np.arange(lo, hi)[:, None] * 0.25 if origins is None else origins[lo:hi]
    d_org = t(org, np.float64)
    d_box = None if box is None else t(np.tile(box, (hi - lo, 1)), np.float32)
    kw = dict(box=d_box, max_images=max_images, ctx=ctx)
    plain = batch.voxelize_lattice_torch(d_xyz, d_offs, d_sig, d_org, nv, 1.0, **kw)
    assert topo.used_for(lo, hi - lo, nv, periodic=box is not None, max_images=max_images)
    on = batch.voxelize_lattice_torch(d_xyz, d_offs, None, d_org, nv, 1.0, topology=topo, topology_first_item=lo, **kw)
    ctx.set_cover_fold(-1)
    off = batch.voxelize_lattice_torch(d_xyz, d_offs, None, d_org, nv, 1.0, topology=topo, topology_first_item=lo, **kw)
    ctx.set_cover_fold(0)
    ctx.synchronize()
    topo.close()
    return plain, on, off, masks


def clear_bits(mask):
    return bin(~mask & 0xfffe).count("1")


@pytest.mark.parametrize("sdt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_synthetic_rows_fold_the_heavy_classes(chain, grid, K, sdt):
    """tests/synth.py rows: channel 7 = every heavy atom at its radius, hydrogens (1.1 A) in channels 0..6 only -- the four heavy
    classes are covered, the hydrogens' class is not (the one clear bit; without it the fold would be dead and this test blind)"""
    import torch
    nv, origin = GRIDS[grid]
    chain.set_tile_k(K)
    xyz, offs, sig = make_batch()
    plain, on, off, masks = three(chain, xyz, offs, sig, nv, origin, sdt=sdt)
    assert clear_bits(masks[0]) == 1 and not masks[0] & 1
    nohyd = sig.copy(); nohyd[nohyd == 1.1] = 0.0                      # ... and the clear bit is the hydrogens': without them nothing is violated
    assert three(chain, xyz, offs, nohyd, nv, origin, sdt=sdt)[3][0] == 0xfffe
    assert torch.equal(plain, on) and torch.equal(plain, off) and float(plain.max()) > 0.5
    assert float(plain[1].abs().max()) == 0.0 and float(plain[3].abs().max()) == 0.0      # the empty item, the absent one


def test_a_violator_takes_its_class_out_of_the_mask(chain):
    """one heavy atom in a channel c < 7 but not in channel 7; one atom with different sigmas in channels 3 and 7: each clears one
    more bit, values unchanged"""
    import torch
    nv, origin = GRIDS["16"]
    xyz, offs, sig = make_batch()
    a = int(np.nonzero(sig[:, 7] == 1.7)[0][3])
    one = sig.copy(); one[a, 2] = 1.7; one[a, 7] = 0.0
    plain, on, off, masks = three(chain, xyz, offs, one, nv, origin)
    assert clear_bits(masks[0]) == 2 and torch.equal(plain, on) and torch.equal(plain, off)
    two = sig.copy(); two[a, 3] = 1.55
    plain, on, off, masks = three(chain, xyz, offs, two, nv, origin)
    assert clear_bits(masks[0]) == 2 and torch.equal(plain, on) and torch.equal(plain, off)


def test_atoms_only_in_channel_7(chain):
    import torch
    xyz, offs, sig = make_batch()
    sig[:, :7] = 0.0
    plain, on, off, masks = three(chain, xyz, offs, sig, *GRIDS["24x16x8"])
    assert masks[0] == 0xfffe and torch.equal(plain, on) and torch.equal(plain, off) and float(plain[..., 7].max()) > 0.5


def test_an_atom_on_a_voxel_centre_in_channels_3_and_7(chain):
    """the negative-d2 corner: rounding of the expanded distance may leave -1e-7 for the pair (atom, its voxel), where |d2| is not
    monotone -- every value there gives occupancy exactly 1.0f"""
    import torch
    nv, origin = GRIDS["16"]
    xyz, offs, sig = make_batch()
    rows = np.nonzero(sig[: offs[1], 7] == 1.7)[0][:40]
    sig[rows, 3] = 1.7
    xyz[rows] = np.round(xyz[rows] * 0.6)                               # whole numbers inside the grid; item 0's origin is whole
    for K in (4, 8):
        chain.set_tile_k(K)
        plain, on, off, masks = three(chain, xyz, offs, sig, nv, origin)
        assert torch.equal(plain, on) and torch.equal(plain, off)
        g = plain[0].reshape(16, 16, 16, 8)
        i = (xyz[rows] + 8).astype(int)
        assert bool((g[i[:, 0], i[:, 1], i[:, 2], 3] == 1.0).all()) and bool((g[i[:, 0], i[:, 1], i[:, 2], 7] == 1.0).all())


def test_two_channel_groups_with_a_short_one(chain):
    import torch
    xyz, offs, sig = make_batch(C=11)
    for grid in sorted(GRIDS):
        plain, on, off, masks = three(chain, xyz, offs, sig, *GRIDS[grid])
        assert clear_bits(masks[0]) >= 1 and clear_bits(masks[1]) >= 1      # the short group has no channel 7: all it carries is violated
        assert torch.equal(plain, on) and torch.equal(plain, off) and float(plain[..., 8:].max()) > 0.1, grid


def test_periodic_box_with_two_images(chain):
    import torch
    xyz, offs, sig = make_batch()
    nv, origin = GRIDS["24x16x8"]
    plain, on, off, _ = three(chain, xyz, offs, sig, nv, origin, box=np.array([23.0, 24.0, 25.0]), max_images=2)
    assert torch.equal(plain, on) and torch.equal(plain, off) and float(plain.max()) > 0.5


@pytest.mark.parametrize("n", [2700, 3400], ids=["over_640_only_before_the_fold", "over_640_either_way"])
def test_tiles_around_the_640_entry_tier(chain, n):
    """the 640-entry tier forced: at 2 700 atoms every tile of the 16 x 16 x 8 grid holds more than 640 entries with the full lists and
    fewer without the duplicates, at 3 400 most hold more either way and go to the DENSE instance, which keeps the full lists (the
    counts are asserted on the emulated tier, tests/test_emu_cover_fold.py, where the tier statistics can be read)"""
    import torch
    from tests.synth import synth_sigmas
    rng = np.random.default_rng(7)
    sig = np.ascontiguousarray(synth_sigmas(rng, n))
    xyz = rng.uniform([-13, -13, -9], [13, 13, 9], size=(n, 3)).astype(np.float32)
    offs = np.array([0, n], np.int64)
    chain.set_lds_tier(0)
    plain, on, off, _ = three(chain, xyz, offs, sig, [16, 16, 8], [-8.0, -8.0, -4.0])
    assert torch.equal(plain, on) and torch.equal(plain, off) and float(plain.max()) > 0.5


def test_a_range_of_a_batch_handle(chain):
    import torch
    xyz, offs, sig = make_batch()
    plain, on, off, _ = three(chain, xyz, offs, sig, *GRIDS["24x16x8"], lo=2, hi=4)
    assert torch.equal(plain, on) and torch.equal(plain, off) and plain.shape[0] == 2 and float(plain[0].max()) > 0.5


def test_two_promised_calls_back_to_back(chain):
    """pipelined (>= 200 000 atoms per call: 8 items of 26 000 around a 16^3 grid)"""
    import torch
    from moleculekit_amd import _lib, batch
    t = tens(chain)
    xyz, offs, sig = make_batch(sizes=[26000] * 7 + [26003], seed=2)
    xyz = xyz * np.float32(3.0)                                       # 0.09 atoms per A^3: tiles of the 640-entry tier, not dense ones
    nv, origin = GRIDS["16"]
    B = len(offs) - 1
    d_offs, d_sig, d_org = t(offs, np.int64), t(sig, np.float32), t(np.tile(origin, (B, 1)), np.float64)
    xa = t(xyz, np.float32)
    xb = (xa + 0.37).contiguous()
    ref = [batch.voxelize_lattice_torch(x, d_offs, d_sig, d_org, nv, 1.0, ctx=chain) for x in (xa, xb)]
    topo = _lib.Topology(chain, d_sig, 1.0, atom_offsets=offs)
    chain.synchronize()
    assert clear_bits(topo.cover_mask(0)) == 1
    before = chain.pipelined_calls()
    outs = []
    for x in (xa, xb):
        chain.promise_inputs(None)
        outs.append(batch.voxelize_lattice_torch(x, d_offs, None, d_org, nv, 1.0, ctx=chain, topology=topo))
    chain.synchronize()
    assert chain.pipelined_calls() >= before + 2
    assert torch.equal(outs[0], ref[0]) and torch.equal(outs[1], ref[1]) and not torch.equal(ref[0], ref[1])
    topo.close()


def test_a_frame_handle_call_of_one_item_folds_inside_the_team_kernel(hip_ctx):
    """one 24^3 grid of a frame handle, the library left to itself: a frame handle always bins through the handle (the TOPO binning
    kernels; the launch sequence is pinned on the emulated tier, tests/test_emu_cover_fold.py) and 27 tiles are the team regime"""
    import torch
    from moleculekit_amd import _lib, batch
    from tests.synth import synth_sigmas
    t = tens(hip_ctx)
    rng = np.random.default_rng(9)
    n = 3000
    sig = np.ascontiguousarray(synth_sigmas(rng, n), np.float32)
    xyz = rng.uniform(-15, 15, size=(n, 3)).astype(np.float32)
    d_xyz, d_offs, d_sig, d_org = t(xyz, np.float32), t([0, n], np.int64), t(sig, np.float32), t([[-12.0, -12.0, -12.0]], np.float64)
    nv = [24, 24, 24]
    plain = batch.voxelize_lattice_torch(d_xyz, d_offs, d_sig, d_org, nv, 1.0, ctx=hip_ctx)
    topo = _lib.Topology(hip_ctx, d_sig, 1.0)
    assert clear_bits(topo.cover_mask(0)) == 1
    try:
        on = batch.voxelize_lattice_torch(d_xyz, d_offs, None, d_org, nv, 1.0, ctx=hip_ctx, topology=topo)
        hip_ctx.synchronize()
        assert "k_voxelize_tiles_team" in hip_ctx.last_tile_kernel()
        hip_ctx.set_cover_fold(-1)
        off = batch.voxelize_lattice_torch(d_xyz, d_offs, None, d_org, nv, 1.0, ctx=hip_ctx, topology=topo)
        hip_ctx.synchronize()
    finally:
        hip_ctx.set_cover_fold(0)
    assert torch.equal(plain, on) and torch.equal(plain, off) and float(plain.max()) > 0.5
    topo.close()
