"""CPU tier: the survivors a tile keeps in registers between its histogram pass and its placement pass (round 10)
on the host emulation of the product's kernels.  The batches of tests/survivor_cases.py through the emulated tile kernels at both
depths: the counts every target tile reports from inside the kernel (MK_SURV_PROBE: candidates, survivors, the path taken, the x-reach
values per survivor register) are the ones the cases were built for, and the handle call with the fold on and off is bit for bit the
plain call.  The mutation check: with the placement reading register 1's x-reach for register 0 (-DMK_DIAG=256) the comparison must fail."""
import numpy as np
import pytest

from tests import emu_build as E
from tests import emu_survivor_regs_build as ES
from tests import survivor_cases as SC

ALL_XR = 0xFFFFFF                                            # bit 3 j + xr: every x-reach value in every one of the eight registers

_plain = {}


def plain(grid, K):
    """the plain call's features of a batch, computed once"""
    if (grid, K) not in _plain:
        xyz, offs, sig, org, nv = SC.batch(grid, K)
        out, err = E.voxelize_lattice(xyz, offs, sig, org, nv, 1.0, prepass_mode=0, tile_team=0, tile_items=0, direct=0, tile_k=K)
        assert err == 0
        out.setflags(write=False)
        _plain[(grid, K)] = out
    return _plain[(grid, K)]


def target_rows(r, n_items):
    """the probe's row of every item's target tile: x tile X0 / K, y and z tile 0 (tiles are numbered x-major)"""
    tiles = r["tiles"]
    per_item = len(tiles) // n_items
    assert per_item * n_items == len(tiles) and per_item > 0
    return tiles.reshape(n_items, per_item, 6)


@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("grid", sorted(SC.GRIDS))
def test_chunk_boundaries_and_both_sides_of_the_list_condition(grid, K):
    xyz, offs, sig, org, nv = SC.batch(grid, K)
    B = len(offs) - 1
    ref = plain(grid, K)
    on = ES.voxelize(xyz, offs, sig, org, nv, tile_k=K)
    off = ES.voxelize(xyz, offs, sig, org, nv, tile_k=K, cover_fold=-1)
    assert on["err"] == 0 and off["err"] == 0
    assert np.array_equal(on["out"], ref) and np.array_equal(off["out"], ref)
    assert ref.max() > 0.5 and not ref[8].any() and not ref[9].any()          # the empty item, the item absent from every channel
    # the fold is on in `on`: the covered classes 1.7 and 1.52 (tests/survivor_cases.py), not the hydrogens' 1.1
    m = int(on["masks"][0])
    assert m & ES.EC.class_bit(on["table"], np.float32(1.7)) and m & ES.EC.class_bit(on["table"], np.float32(1.52))
    assert not m & ES.EC.class_bit(on["table"], np.float32(1.1))
    # what the kernel itself counted in every item's target tile
    rows = target_rows(on, B)
    tny, tnz = nv[1] // 8, nv[2] // 8
    t = (SC.X0 // K) * tny * tnz
    for b, item in enumerate(SC.ITEMS):
        if item[4] is not None:
            got = tuple(int(v) for v in rows[b, t, 2:5])
            print("item", b, "target tile: candidates, survivors, list =", got, "x-reach seen %06x" % rows[b, t, 5])
            assert got == item[4], (b, got)
    assert np.array_equal(rows[..., 2:], target_rows(off, B)[..., 2:])
    # the hot instance placed the long lists: ALL atoms of such an item hold fewer entries (fold off) than the smallest tier's 640,
    # with every sub-bucket (15 channel-class groups x 3 x-reach values) padded by one
    for b, item in enumerate(SC.ITEMS):
        if item[2] is SC.LEAN:
            assert int((sig[offs[b]:offs[b + 1]] > 0).sum()) + 45 <= 640, b
    # every x-reach value in every survivor register, over the tiles of the call.  In the mixed item's tile the list runs through the
    # bands in the order of the cells (low x first): its first register mixes xr 1 with xr 0, its last one xr 0 with xr 2 -- a lane's
    # registers hold different values, which is what the packed word has to keep apart
    assert int(np.bitwise_or.reduce(rows[..., 5].ravel())) == ALL_XR
    seen = int(rows[SC.MIXED_479, t, 5])
    assert seen & 7 == 0b011 and (seen >> 21) & 7 == 0b101, "%06x" % seen


@pytest.mark.parametrize("K", [4, 8])
def test_the_mutant_that_reads_the_wrong_x_reach_is_caught(K):
    grid = "16x16x8"
    xyz, offs, sig, org, nv = SC.batch(grid, K)
    ref = plain(grid, K)
    mut = ES.voxelize(xyz, offs, sig, org, nv, tile_k=K, mutant=True)
    assert mut["err"] == 0 and not np.array_equal(mut["out"], ref)
    # only tiles that placed from the kept survivors can differ: the items below 257 candidates, the one over 480 survivors, the empty
    # and the absent one keep the plain call's bits
    for b in (1, 8, 9):
        assert np.array_equal(mut["out"][b], ref[b]), b


def test_force_general_is_bitwise_the_sorted_path():
    grid, K = "16x16x8", 8
    xyz, offs, sig, org, nv = SC.batch(grid, K)
    gen, err = E.voxelize_lattice(xyz, offs, sig, org, nv, 1.0, prepass_mode=0, tile_team=0, tile_items=0, direct=0, tile_k=K, force_general=True)
    assert err == 0 and np.array_equal(gen, plain(grid, K))
