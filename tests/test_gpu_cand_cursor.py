"""GPU tier: the run cursor of the tile kernels' candidate traversal and the cover fold once per channel (round 9; DESIGN.md
section 1) on the smallest shapes at which the traversal can still go wrong: 16 x 16 x 8 and 24 x 16 x 8 grids at K = 4 and K = 8.

Every case is held two ways: against the oracle at the tolerance of tests/test_gpu_parity.py (tests/cases.py: TOL), and ``torch.equal``
between the COLUMN layout and the DIRECT layout of the same inputs (``set_direct_binning(0 / 1)``, in order) -- the two have different
run tables (9 cell columns against up to 27 cells plus the item's spill run), so a slip of the cursor in one shows as a difference from
the other.  Where a topology handle applies, the handle call runs with the cover fold on and off (``set_cover_fold(0 / -1)``, what
MKAMD_COVER_FOLD=1 / 0 select): both ``torch.equal`` to the plain call."""
import numpy as np
import pytest

from tests.cases import TOL, oracle_lattice
from tests.test_gpu_batch_topology import GRIDS, make_batch, tens

pytestmark = pytest.mark.gpu

GRIDS8 = {"16x16x8": ([16, 16, 8], [-8.0, -8.0, -4.0]), "24x16x8": GRIDS["24x16x8"]}


@pytest.fixture
def chain(hip_ctx):
    hip_ctx.set_prepass_mode(0); hip_ctx.set_tile_team(0); hip_ctx.set_tile_items(0); hip_ctx.set_direct_binning(0)
    try:
        yield hip_ctx
    finally:
        hip_ctx.set_prepass_mode(-1); hip_ctx.set_tile_team(-1); hip_ctx.set_tile_items(-1); hip_ctx.set_direct_binning(-1)
        hip_ctx.set_tile_k(0); hip_ctx.set_lds_tier(-1); hip_ctx.set_cover_fold(0); hip_ctx.set_force_general(False)
        hip_ctx.synchronize()


def held_two_ways(ctx, xyz, offs, sig, nv, origins, box=None, max_images=1, handle=True, frame_handle=False):
    """-> the column layout's features (torch, [B, V, C]) after: column layout == direct layout (three calls: the first builds the class
    table through the chain), == the handle call with the fold on and with it off, and |column - oracle| <= TOL"""
    import torch
    from moleculekit_amd import _lib, batch
    t = tens(ctx)
    B = len(offs) - 1
    origins = np.asarray(origins, np.float64).reshape(B, 3)
    d_xyz, d_offs, d_sig, d_org = t(xyz, np.float32), t(offs, np.int64), t(sig, np.float32), t(origins, np.float64)
    bx = None if box is None else np.tile(np.asarray(box, np.float32), (B, 1))
    kw = dict(box=None if bx is None else t(bx, np.float32), max_images=max_images, ctx=ctx)
    ctx.set_direct_binning(0)
    col = batch.voxelize_lattice_torch(d_xyz, d_offs, d_sig, d_org, nv, 1.0, **kw)
    ctx.set_direct_binning(1)
    direct = [batch.voxelize_lattice_torch(d_xyz, d_offs, d_sig, d_org, nv, 1.0, **kw) for _ in range(3)]
    ctx.set_direct_binning(0)
    ctx.synchronize()
    for d in direct:
        assert torch.equal(col, d)
    if handle:
        topo = _lib.Topology(ctx, d_sig, 1.0) if frame_handle else _lib.Topology(ctx, d_sig, 1.0, atom_offsets=offs)
        try:
            on = batch.voxelize_lattice_torch(d_xyz, d_offs, None, d_org, nv, 1.0, topology=topo, **kw)
            ctx.set_cover_fold(-1)
            off = batch.voxelize_lattice_torch(d_xyz, d_offs, None, d_org, nv, 1.0, topology=topo, **kw)
            ctx.synchronize()
        finally:
            ctx.set_cover_fold(0)
            topo.close()
        assert torch.equal(col, on) and torch.equal(col, off)
    exp = oracle_lattice(np.asarray(xyz, np.float32), offs, np.asarray(sig, np.float64), origins, nv, 1.0, box=bx)
    err = np.abs(col.cpu().numpy().astype(np.float64) - exp).max() if B else 0.0
    print("max-abs-err against the oracle: %.3e" % err)
    assert err <= TOL
    return col


ITEM_SIZES = [0, 1, 63, 64, 65, 256, 257, 300]          # candidates of a tile on both sides of N > 4 * 64 (the survivor-list switch)


@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("grid", sorted(GRIDS8))
def test_items_around_the_survivor_list_switch(chain, grid, K):
    """eight items of 0 ... 300 atoms packed around the corner the middle tiles share: a tile there has the whole item as candidates"""
    from tests.synth import synth_sigmas
    nv, origin = GRIDS8[grid]
    rng = np.random.default_rng(21)
    n = sum(ITEM_SIZES)
    offs = np.concatenate([[0], np.cumsum(ITEM_SIZES)]).astype(np.int64)
    sig = np.ascontiguousarray(synth_sigmas(rng, n))
    xyz = rng.uniform(-2.4, 2.4, size=(n, 3)).astype(np.float32)
    chain.set_tile_k(K)
    out = held_two_ways(chain, xyz, offs, sig, nv, np.tile(origin, (len(ITEM_SIZES), 1)))
    assert float(out[0].abs().max()) == 0.0 and float(out[5].max()) > 0.5 and float(out[7].max()) > 0.5


@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("grid", sorted(GRIDS8))
def test_ragged_batch_with_an_empty_item(chain, grid, K):
    nv, origin = GRIDS8[grid]
    xyz, offs, sig = make_batch()
    B = len(offs) - 1
    chain.set_tile_k(K)
    out = held_two_ways(chain, xyz, offs, sig, nv, np.tile(origin, (B, 1)) + np.arange(B)[:, None] * 0.25)
    assert float(out[1].abs().max()) == 0.0 and float(out[3].abs().max()) == 0.0 and float(out[0].max()) > 0.5


@pytest.mark.parametrize("n", [2700, 3400], ids=["hot_instance", "dense_instance_too"])
def test_tier_0_forced(chain, n):
    """the 640-entry tier forced on one 16 x 16 x 8 grid: at 2 700 atoms the tiles stay in the hot instance (with the fold), at 3 400
    most go to the DENSE instance as well (tests/test_emu_cover_fold.py reads the counts on the emulated tier)"""
    from tests.synth import synth_sigmas
    rng = np.random.default_rng(7)
    sig = np.ascontiguousarray(synth_sigmas(rng, n))
    xyz = rng.uniform([-13, -13, -9], [13, 13, 9], size=(n, 3)).astype(np.float32)
    chain.set_lds_tier(0)
    out = held_two_ways(chain, xyz, np.array([0, n], np.int64), sig, [16, 16, 8], [[-8.0, -8.0, -4.0]])
    assert float(out.max()) > 0.5


@pytest.mark.parametrize("K", [4, 8])
def test_two_channel_groups(chain, K):
    xyz, offs, sig = make_batch(C=11)
    nv, origin = GRIDS8["24x16x8"]
    chain.set_tile_k(K)
    out = held_two_ways(chain, xyz, offs, sig, nv, np.tile(origin, (len(offs) - 1, 1)))
    assert float(out[..., 8:].max()) > 0.1


@pytest.mark.parametrize("K", [4, 8])
def test_periodic_box_with_two_images(chain, K):
    xyz, offs, sig = make_batch()
    nv, origin = GRIDS8["24x16x8"]
    chain.set_tile_k(K)
    out = held_two_ways(chain, xyz, offs, sig, nv, np.tile(origin, (len(offs) - 1, 1)), box=[23.0, 24.0, 25.0], max_images=2)
    assert float(out.max()) > 0.5


@pytest.mark.parametrize("grid", sorted(GRIDS8))
def test_one_grid_per_call_takes_the_team_kernel(chain, grid):
    """a team's wave takes every fourth (K = 4: every eighth) chunk and keeps the per-chunk search of the runs (the cursor serves the
    traversals that visit every chunk; a strided cursor is walked on the emulated tier only, tests/test_emu_cand_cursor.py): the team
    kernel against the same oracle and layouts as the rest"""
    from tests.synth import synth_sigmas
    nv, origin = GRIDS8[grid]
    rng = np.random.default_rng(9)
    n = 1500
    sig = np.ascontiguousarray(synth_sigmas(rng, n))
    xyz = rng.uniform(-13, 13, size=(n, 3)).astype(np.float32) * np.array([1.0, 0.8, 0.6], np.float32)
    chain.set_tile_team(1)
    out = held_two_ways(chain, xyz, np.array([0, n], np.int64), sig, nv, [origin], frame_handle=True)
    assert "k_voxelize_tiles_team" in chain.last_tile_kernel() and float(out.max()) > 0.5


@pytest.mark.parametrize("K", [4, 8])
def test_force_general(chain, K):
    import torch
    from moleculekit_amd import batch
    xyz, offs, sig = make_batch()
    nv, origin = GRIDS8["16x16x8"]
    B = len(offs) - 1
    chain.set_tile_k(K)
    sorted_path = held_two_ways(chain, xyz, offs, sig, nv, np.tile(origin, (B, 1)), handle=False)
    chain.set_force_general(True)
    general = held_two_ways(chain, xyz, offs, sig, nv, np.tile(origin, (B, 1)), handle=False)
    assert torch.equal(sorted_path, general)


def test_a_pipelined_pair_of_promised_calls(chain):
    """>= 200 000 atoms per call (8 items of 26 000 around a 16 x 16 x 8 grid): the second call's pre-pass runs beside the first call's
    tile kernel"""
    import torch
    from moleculekit_amd import _lib, batch
    t = tens(chain)
    xyz, offs, sig = make_batch(sizes=[26000] * 7 + [26003], seed=2)
    xyz = xyz * np.float32(3.0)                                       # 0.09 atoms per A^3: tiles of the 640-entry tier, not dense ones
    nv, origin = GRIDS8["16x16x8"]
    B = len(offs) - 1
    d_offs, d_sig, d_org = t(offs, np.int64), t(sig, np.float32), t(np.tile(origin, (B, 1)), np.float64)
    xa = t(xyz, np.float32)
    xb = (xa + 0.37).contiguous()
    ref = [batch.voxelize_lattice_torch(x, d_offs, d_sig, d_org, nv, 1.0, ctx=chain) for x in (xa, xb)]
    chain.set_direct_binning(1)
    direct = [batch.voxelize_lattice_torch(x, d_offs, d_sig, d_org, nv, 1.0, ctx=chain) for x in (xa, xb, xa, xb)]
    chain.set_direct_binning(0)
    topo = _lib.Topology(chain, d_sig, 1.0, atom_offsets=offs)
    chain.synchronize()
    outs = {}
    for fold in (0, -1):
        chain.set_cover_fold(fold)
        before = chain.pipelined_calls()
        outs[fold] = []
        for x in (xa, xb):
            chain.promise_inputs(None)
            outs[fold].append(batch.voxelize_lattice_torch(x, d_offs, None, d_org, nv, 1.0, ctx=chain, topology=topo))
        chain.synchronize()
        assert chain.pipelined_calls() >= before + 2
    chain.set_cover_fold(0)
    topo.close()
    for i in range(2):
        assert torch.equal(outs[0][i], ref[i]) and torch.equal(outs[-1][i], ref[i]) and torch.equal(direct[2 + i], ref[i])
    assert not torch.equal(ref[0], ref[1])
    a0, a1 = int(offs[2]), int(offs[3])                               # one item against the oracle
    exp = oracle_lattice(xyz[a0:a1], np.array([0, a1 - a0]), sig[a0:a1].astype(np.float64), np.asarray([origin], np.float64), nv, 1.0)
    err = np.abs(ref[0][2].cpu().numpy().astype(np.float64) - exp[0]).max()
    print("max-abs-err against the oracle: %.3e" % err)
    assert err <= TOL
