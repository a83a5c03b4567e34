"""GPU tier: the BATCH topology handle (include/mkamd_voxel.h (3c), round 7) -- what the pre-pass derives from the sigmas, built once
over all atoms of a resident, ragged batch of different molecules -- against the plain call on the same inputs, bit for bit
(``torch.equal``), on the smallest shapes that still take the count / scan / fill chain in front of the tile kernels
(``set_prepass_mode(0)``, ``set_tile_team(0)``, ``set_direct_binning(0)``; pipelining on and off)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# a ragged batch of five items: 300 ... 2 000 atoms, item 1 EMPTY, item 3 absent from every channel (all sigmas zero)
SIZES = [1300, 0, 2000, 300, 777]
GRIDS = {"16": ([16, 16, 16], [-8.0, -8.0, -8.0]), "24x16x8": ([24, 16, 8], [-12.0, -8.0, -4.0])}


def make_batch(C=8, sizes=SIZES, seed=5, wide_items=(), multi=False, lattice=False):
    """coords / offsets / sigmas / origins (one origin per item, slightly shifted) of a ragged batch; `wide_items`: items that get
    atoms with sigma 2.27 A (> 1.81 A: the exact cut-off fix-up), `lattice`: those atoms on voxel centres, where the 5 A shell meets
    other voxel centres exactly; `multi`: atoms with several distinct sigmas in one row (ATOM_MULTI_SIGMA)."""
    from tests.synth import synth_sigmas
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    sig = synth_sigmas(rng, n)                                            # [n, 8]
    if C > 8:
        sig = np.concatenate([sig, sig[:, :C - 8] * 0.8], axis=1)         # (the same radius class x 0.8: still few classes)
    elif C < 8:
        sig = sig[:, :C]
    sig = np.ascontiguousarray(sig)
    xyz = rng.uniform(-11.0, 11.0, size=(n, 3)).astype(np.float32)
    if len(sizes) > 3 and sizes[3]:
        sig[offs[3]:offs[4]] = 0.0                                        # present in no channel at all
    for b in wide_items:
        rows = np.arange(offs[b], offs[b + 1])[::41]
        sig[rows, min(6, C - 1)] = 2.27
        if lattice:
            xyz[rows] = np.round(xyz[rows])                               # (origins below are whole numbers)
    if multi:
        rows = np.arange(n)[::7]
        sig[rows, 0] = 1.1
        sig[rows, 1] = 1.9
    return xyz, offs, sig


def dev_of(hip_ctx):
    import torch
    return torch.device("cuda", hip_ctx.device)


def tens(hip_ctx):
    import torch
    dev = dev_of(hip_ctx)
    return lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)


@pytest.fixture
def chain(hip_ctx):
    """The context steered to the kernel chain + the one-wave tile kernels, and put back afterwards."""
    hip_ctx.set_prepass_mode(0); hip_ctx.set_tile_team(0); hip_ctx.set_tile_items(0); hip_ctx.set_direct_binning(0)
    try:
        yield hip_ctx
    finally:
        hip_ctx.set_prepass_mode(-1); hip_ctx.set_tile_team(-1); hip_ctx.set_tile_items(-1); hip_ctx.set_direct_binning(-1)
        hip_ctx.set_tile_k(0); hip_ctx.set_exact_redo(0)
        hip_ctx.synchronize()


def both(ctx, xyz, offs, sig, nv, origin, sdt=np.float32, box=None, max_images=1, affine=None, first=0, lo=None, hi=None, topo=None):
    """(plain call, batch-handle call) on items [lo, hi) of the batch (default: all of it)."""
    import torch
    from moleculekit_amd import _lib, batch
    t = tens(ctx)
    B = len(offs) - 1
    lo, hi = (0, B) if lo is None else (lo, hi)
    a0, a1 = int(offs[lo]), int(offs[hi])
    own = topo is None
    if own:
        topo = _lib.Topology(ctx, t(sig, sdt), 1.0, atom_offsets=offs)
    d_xyz, d_offs, d_sig = t(xyz[a0:a1], np.float32), t(offs[lo:hi + 1] - a0, np.int64), t(sig[a0:a1], sdt)
    d_org = t(np.tile(np.asarray(origin, dtype=np.float64), (hi - lo, 1)) + np.arange(lo, hi)[:, None] * 0.25, np.float64)
    d_box = None if box is None else t(np.tile(box, (hi - lo, 1)), np.float32)
    d_aff = None if affine is None else t(affine[lo:hi], np.float64)
    kw = dict(box=d_box, max_images=max_images, ctx=ctx, affine=d_aff)
    plain = batch.voxelize_lattice_torch(d_xyz, d_offs, d_sig, d_org, nv, 1.0, **kw)
    got = batch.voxelize_lattice_torch(d_xyz, d_offs, None, d_org, nv, 1.0, topology=topo, topology_first_item=lo, **kw)
    ctx.synchronize()
    assert topo.used_for(lo, hi - lo, nv, periodic=box is not None, max_images=max_images) or a1 == a0
    if own:
        topo.close()
    return plain, got


@pytest.mark.parametrize("sdt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_ragged_batch_is_bitwise_the_plain_call(chain, grid, K, sdt):
    import torch
    nv, origin = GRIDS[grid]
    chain.set_tile_k(K)
    xyz, offs, sig = make_batch()
    plain, got = both(chain, xyz, offs, sig, nv, origin, sdt=sdt)
    assert torch.equal(plain, got) and float(plain.max()) > 0.5
    assert float(plain[1].abs().max()) == 0.0 and float(plain[3].abs().max()) == 0.0      # the empty item, the absent one


def test_two_channel_groups_with_a_partial_one(chain):
    import torch
    xyz, offs, sig = make_batch(C=11)
    for grid in sorted(GRIDS):
        plain, got = both(chain, xyz, offs, sig, *GRIDS[grid])
        assert torch.equal(plain, got) and float(plain[..., 8:].max()) > 0.1, grid


def test_per_item_affines(chain):
    import torch
    from moleculekit_amd import batch
    xyz, offs, sig = make_batch()
    rng = np.random.default_rng(3)
    q, _ = np.linalg.qr(rng.normal(size=(len(SIZES), 3, 3)))
    aff = np.concatenate([q.reshape(len(SIZES), 9), rng.uniform(-1, 1, size=(len(SIZES), 3))], axis=1)
    plain, got = both(chain, xyz, offs, sig, *GRIDS["16"], affine=aff)
    bare, _ = both(chain, xyz, offs, sig, *GRIDS["16"])
    assert torch.equal(plain, got) and not torch.equal(plain, bare)


def test_periodic_box_with_two_images(chain):
    import torch
    xyz, offs, sig = make_batch()
    nv, origin = GRIDS["24x16x8"]
    plain, got = both(chain, xyz, offs, sig, nv, origin, box=np.array([23.0, 24.0, 25.0]), max_images=2)
    assert torch.equal(plain, got) and float(plain.max()) > 0.5


def test_atoms_with_several_sigmas_in_one_row(chain):
    import torch
    xyz, offs, sig = make_batch(multi=True)
    for sdt in (np.float32, np.float64):
        plain, got = both(chain, xyz, offs, sig, *GRIDS["16"], sdt=sdt)
        assert torch.equal(plain, got)


@pytest.mark.parametrize("redo", [0, -1], ids=["redo_list", "in_k_tail"])
def test_wide_sigmas_in_two_items(chain, redo):
    """sigma 2.27 A (> 1.81 A) in items 0 and 4, the atoms on voxel centres: their 5 A shells pass through other voxel centres, which
    the exact cut-off fix-up re-decides in double -- through the handle's batch-wide wide list and its own sigma copy."""
    import torch
    from moleculekit_amd import _lib
    chain.set_exact_redo(redo)
    xyz, offs, sig = make_batch(wide_items=(0, 4), lattice=True)
    t = tens(chain)
    topo = _lib.Topology(chain, t(sig, np.float32), 1.0, atom_offsets=offs)
    assert topo.has_wide_sigmas and topo.n_items == len(SIZES) and topo.n_atoms == int(offs[-1])
    for grid in sorted(GRIDS):
        nv, origin = GRIDS[grid]
        plain, got = both(chain, xyz, offs, sig, nv, [float(round(o)) for o in origin], topo=topo)
        assert torch.equal(plain, got), grid
    # a chunk that starts behind the first wide item: only item 4's wide atoms are its jobs
    plain, got = both(chain, xyz, offs, sig, *GRIDS["16"], lo=2, hi=5, topo=topo)
    assert torch.equal(plain, got)
    topo.close()


def test_wide_sigmas_in_an_item_of_more_than_one_slice(chain):
    """an item of more than 2 048 atoms: k_exact_redo walks it in slices -- of the item's OWN length, beside shorter items"""
    import torch
    xyz, offs, sig = make_batch(sizes=[500, 4300, 0, 900], wide_items=(0, 1), lattice=True, seed=8)
    plain, got = both(chain, xyz, offs, sig, [16, 16, 16], [-8.0, -8.0, -8.0])
    assert torch.equal(plain, got) and float(plain.max()) > 0.5


def test_a_chunk_of_the_batch(chain):
    """items [2, 4) through the whole batch's handle against the plain call on those items alone"""
    import torch
    xyz, offs, sig = make_batch(C=11, multi=True)
    plain, got = both(chain, xyz, offs, sig, *GRIDS["24x16x8"], lo=2, hi=4)
    assert torch.equal(plain, got) and plain.shape[0] == 2 and float(plain[0].max()) > 0.5
    plain, got = both(chain, xyz, offs, sig, *GRIDS["24x16x8"], lo=1, hi=2)            # the empty item alone
    assert torch.equal(plain, got) and float(plain.abs().max()) == 0.0


def test_promised_calls_back_to_back_are_pipelined_and_bitwise(chain):
    """two promised calls with changed coordinates in between: pipelined (a call of >= 200 000 atoms: the library's threshold, so
    this one case is that big -- 8 items of 26 000 atoms on a 16^3 grid), both bitwise the in-order plain calls"""
    import torch
    from moleculekit_amd import _lib, batch
    t = tens(chain)
    xyz, offs, sig = make_batch(sizes=[26000] * 7 + [26003], seed=2)
    nv, origin = GRIDS["16"]
    B = len(offs) - 1
    d_offs, d_sig, d_org = t(offs, np.int64), t(sig, np.float32), t(np.tile(origin, (B, 1)), np.float64)
    xa = t(xyz, np.float32)
    xb = (xa + 0.37).contiguous()
    ref = [batch.voxelize_lattice_torch(x, d_offs, d_sig, d_org, nv, 1.0, ctx=chain) for x in (xa, xb)]
    topo = _lib.Topology(chain, d_sig, 1.0, atom_offsets=offs)
    chain.synchronize()
    before = chain.pipelined_calls()
    outs = []
    for x in (xa, xb):
        chain.promise_inputs(None)
        outs.append(batch.voxelize_lattice_torch(x, d_offs, None, d_org, nv, 1.0, ctx=chain, topology=topo))
    chain.synchronize()
    assert chain.pipelined_calls() >= before + 2
    assert torch.equal(outs[0], ref[0]) and torch.equal(outs[1], ref[1]) and not torch.equal(ref[0], ref[1])
    topo.close()


def test_refusals(chain):
    import torch
    from moleculekit_amd import _lib, batch
    t = tens(chain)
    xyz, offs, sig = make_batch()
    nv, origin = GRIDS["16"]
    B = len(offs) - 1
    d_xyz, d_sig, d_org = t(xyz, np.float32), t(sig, np.float32), t(np.tile(origin, (B, 1)), np.float64)
    topo = _lib.Topology(chain, d_sig, 1.0, atom_offsets=offs)
    call = lambda o, **kw: batch.voxelize_lattice_torch(d_xyz, t(o, np.int64), None, d_org, nv, 1.0, ctx=chain, topology=topo, **kw)
    plain = batch.voxelize_lattice_torch(d_xyz, t(offs, np.int64), d_sig, d_org, nv, 1.0, ctx=chain)
    # the right total split differently: flagged on the device, reported at the next synchronize (the output is not looked at)
    bad = offs.copy()
    bad[3] -= 5
    call(bad)
    with pytest.raises(ValueError, match="topology"):
        chain.synchronize()
    assert torch.equal(call(offs), plain)                                   # ... and the context carries on
    chain.synchronize()
    with pytest.raises(ValueError, match="range of the batch topology"):   # not a range of its items: refused at once
        call(offs, topology_first_item=1)
    with pytest.raises(ValueError, match="range of the batch topology"):
        batch.voxelize_lattice_torch(d_xyz[:-3], t(offs, np.int64), None, d_org, nv, 1.0, ctx=chain, topology=topo)
    for setter, on, off in ((chain.set_force_general, True, False), (chain.set_value_tolerance, 1e-6, 0.0)):
        setter(on)
        try:
            with pytest.raises(ValueError, match="class-sorted path only"):
                call(offs)
        finally:
            setter(off)
    assert torch.equal(call(offs), plain)
    topo.close()
    # 16 distinct sigmas in the batch: no class ids to reuse, creation fails
    sig16 = sig.copy()
    sig16[:16, 0] = np.linspace(1.0, 1.75, 16)
    with pytest.raises(ValueError, match="15 distinct"):
        _lib.Topology(chain, t(sig16, np.float32), 1.0, atom_offsets=offs)
    with pytest.raises(ValueError, match="atom offsets"):
        _lib.Topology(chain, d_sig, 1.0, atom_offsets=offs[:-1])


def test_calls_the_chain_does_not_serve_fall_back_to_the_sigma_copy(hip_ctx):
    """left to itself the library gives five small items the one-launch per-item pre-pass: the handle says so (used_for) and the call
    is the plain call on the handle's own sigma copy -- the caller's may be gone"""
    import torch
    from moleculekit_amd import _lib, batch
    t = tens(hip_ctx)
    xyz, offs, sig = make_batch()
    nv, origin = GRIDS["16"]
    B = len(offs) - 1
    d_xyz, d_offs, d_sig, d_org = t(xyz, np.float32), t(offs, np.int64), t(sig, np.float32), t(np.tile(origin, (B, 1)), np.float64)
    plain = batch.voxelize_lattice_torch(d_xyz, d_offs, d_sig, d_org, nv, 1.0, ctx=hip_ctx)
    topo = _lib.Topology(hip_ctx, d_sig, 1.0, atom_offsets=offs)
    assert not topo.used_for(0, B, nv)
    d_sig.zero_()
    assert torch.equal(batch.voxelize_lattice_torch(d_xyz, d_offs, None, d_org, nv, 1.0, ctx=hip_ctx, topology=topo), plain)
    a0 = int(offs[2])
    got = batch.voxelize_lattice_torch(d_xyz[a0:], t(offs[2:] - a0, np.int64), None, d_org[2:], nv, 1.0, ctx=hip_ctx, topology=topo,
                                       topology_first_item=2)
    assert torch.equal(got, plain[2:])
    hip_ctx.synchronize()
    topo.close()


def sharded(hip_ctx, sig, sizes, env):
    from moleculekit_amd.distributed import ShardedVoxelizer
    rng = np.random.default_rng(4)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    xyz = rng.uniform(-19, 19, size=(int(offs[-1]), 3)).astype(np.float32)
    origins = np.tile([-16.0, -16.0, -16.0], (len(sizes), 1))
    old = os.environ.get("MKAMD_BATCH_TOPOLOGY")
    if env is None:
        os.environ.pop("MKAMD_BATCH_TOPOLOGY", None)
    else:
        os.environ["MKAMD_BATCH_TOPOLOGY"] = env
    try:
        return ShardedVoxelizer.from_host(xyz, offs, sig, origins, [32, 32, 32], 1.0, device=dev_of(hip_ctx), ctx=hip_ctx)
    finally:
        os.environ.pop("MKAMD_BATCH_TOPOLOGY", None)
        if old is not None:
            os.environ["MKAMD_BATCH_TOPOLOGY"] = old


def test_sharded_voxelizer_builds_the_handle_by_default_and_stays_bitwise(hip_ctx):
    """nine items of 5 000 ... 6 000 atoms on 32^3 grids (more than 4 096 atoms per item and more than 1 024 tile waves: the library
    takes the chain and the one-wave tile kernels by itself; eight such items are still the small-call regime): a handle by default,
    none with MKAMD_BATCH_TOPOLOGY=0 (read at construction), none for 16 distinct sigmas; voxelize() and the chunked gather agree
    bit for bit in both settings."""
    import torch
    import torch.distributed as dist
    from tests.synth import synth_sigmas
    sizes = [5000, 5300, 6000, 5100, 5017, 5999, 5500, 5001, 5250]
    sig = synth_sigmas(np.random.default_rng(6), int(sum(sizes))).astype(np.float32)
    on, off = sharded(hip_ctx, sig, sizes, None), sharded(hip_ctx, sig, sizes, "0")
    assert on._topo is not None and on._topo.n_items == len(sizes) and off._topo is None
    assert tuple(on._d["sigmas"].shape) == tuple(off._d["sigmas"].shape) == (int(sum(sizes)), 8)      # stays resident
    a, b = on.voxelize(), off.voxelize()
    assert torch.equal(a, b) and float(a.max()) > 0.5
    sig16 = sig.copy()
    sig16[:16, 0] = np.linspace(1.0, 1.75, 16)
    assert sharded(hip_ctx, sig16, sizes, None)._topo is None
    own_group = not dist.is_initialized()
    if own_group:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29653")
        torch.cuda.set_device(dev_of(hip_ctx))
        dist.init_process_group("nccl", rank=0, world_size=1)
    try:
        ga = on.voxelize_gather(nchunks=4, loopback=True)
        gb = off.voxelize_gather(nchunks=4, loopback=True)
        torch.cuda.synchronize()
        assert torch.equal(ga, a) and torch.equal(gb, a)
    finally:
        if own_group:
            dist.destroy_process_group()
