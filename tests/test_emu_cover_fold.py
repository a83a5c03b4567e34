"""CPU tier: the cover fold (round 8; GridDesc::cover_violated) on the host emulation of the product's kernels --
the cover masks k_topology_ids leaves in a handle, the ragged batch of tests/test_emu_batch_topology.py through the emulated tile
kernels at both depths with the fold on and off against the plain call (bit for bit), the dense tiers, and the mutation check: with
the fold compiled out while channel 7 still leaves the covered atoms out (-DMK_DIAG=128) the comparison must fail."""
import numpy as np
import pytest

from tests import emu_build as E
from tests import emu_cover_fold_build as EC
from tests.synth import synth_sigmas

SIZES = [700, 0, 1100, 300, 450]          # item 1 empty, item 3 absent from every channel
NV = [16, 16, 8]
HEAVY = (1.7, 1.55, 1.52, 1.8)


def ragged(C=8, sdt=np.float32, seed=12):
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(offs[-1])
    sig = synth_sigmas(rng, n)
    if C > 8:
        sig = np.concatenate([sig, sig[:, :C - 8] * 0.8], axis=1)
    sig = np.ascontiguousarray(sig, sdt)
    sig[offs[3]:offs[4]] = 0.0
    xyz = rng.uniform(-10, 10, size=(n, 3)).astype(np.float32)
    origins = np.tile([-8.0, -8.0, -4.0], (len(SIZES), 1)) + np.arange(len(SIZES))[:, None] * 1.0
    return xyz, offs, sig, origins


def bits(h, sigmas, dt):
    return [EC.class_bit(h["table"], dt(s)) for s in sigmas]


@pytest.mark.parametrize("sdt", [np.float32, np.float64], ids=["f32", "f64"])
def test_cover_masks_of_a_handle(sdt):
    xyz, offs, sig, origins = ragged(sdt=sdt)
    h = EC.voxelize(xyz, offs, sig, origins, NV, run=False)
    m = int(h["masks"][0])
    heavy, hyd = bits(h, HEAVY, sdt), bits(h, [1.1], sdt)[0]
    assert all(m & b for b in heavy) and not m & hyd and not m & 1          # hydrogens sit in channels 0..6 and never in channel 7
    # one heavy atom in a channel c < 7 that is NOT in channel 7: its class leaves the mask, the others stay
    a = int(np.nonzero(sig[:, 7] == sdt(1.7))[0][5])
    one = sig.copy(); one[a, 2] = one[a, 7]; one[a, 7] = 0.0
    m1 = int(EC.voxelize(xyz, offs, one, origins, NV, run=False)["masks"][0])
    assert m1 == m & ~bits(h, [1.7], sdt)[0]
    # an atom with different sigmas in channel 3 and channel 7: channel 3's class is violated, channel 7's is not
    two = sig.copy(); two[a, 3] = sdt(1.55)
    m2 = int(EC.voxelize(xyz, offs, two, origins, NV, run=False)["masks"][0])
    assert m2 == m & ~bits(h, [1.55], sdt)[0]
    # atoms only in channel 7: nothing to violate -- every class of the table is covered
    only7 = sig.copy(); only7[:, :7] = 0.0
    h7 = EC.voxelize(xyz, offs, only7, origins, NV, run=False)
    assert int(h7["masks"][0]) == 0xfffe and (h7["table"][:4] != 0xffffffff).all()
    # C = 11: the second, short group has no channel 7 at all -- every class its channels carry is violated
    x11, o11, s11, g11 = ragged(C=11, sdt=sdt)
    h11 = EC.voxelize(x11, o11, s11, g11, NV, run=False)
    scaled = [EC.class_bit(h11["table"], sdt(np.float64(s) * 0.8)) for s in (1.1, 1.7)]
    assert int(h11["masks"][0]) & 0xfffe == int(h11["masks"][0]) and all(int(h11["masks"][0]) & b for b in bits(h11, HEAVY, sdt))
    assert not any(int(h11["masks"][1]) & b for b in scaled)


@pytest.mark.parametrize("K", [4, 8])
def test_ragged_batch_with_and_without_the_fold_is_bitwise_the_plain_call(K):
    xyz, offs, sig, origins = ragged()
    a = int(np.nonzero(sig[: offs[1], 7] == np.float32(1.7))[0][0])
    sig[a, 3] = 1.7
    xyz[a] = [-3.0, 2.0, 1.0]                                # on a voxel centre of item 0, in channels 3 and 7: the negative-d2 corner
    plain, e0 = E.voxelize_lattice(xyz, offs, sig, origins, NV, 1.0, prepass_mode=0, tile_team=0, tile_items=0, direct=0, tile_k=K)
    on = EC.voxelize(xyz, offs, sig, origins, NV, tile_k=K)
    off = EC.voxelize(xyz, offs, sig, origins, NV, tile_k=K, cover_fold=-1)
    assert e0 == 0 and on["err"] == 0 and off["err"] == 0 and int(on["masks"][0]) & EC.class_bit(on["table"], np.float32(1.7))
    assert np.array_equal(plain, off["out"]) and np.array_equal(plain, on["out"])
    assert plain.max() > 0.5 and not plain[1].any() and not plain[3].any()
    v = ((-3 + 8) * 16 + (2 + 8)) * 8 + (1 + 4)              # the voxel the atom sits on
    assert plain[0, v, 3] == 1.0 and plain[0, v, 7] == 1.0
    chunk = EC.voxelize(xyz, offs, sig, origins, NV, lo=2, hi=4, tile_k=K)
    assert chunk["err"] == 0 and np.array_equal(chunk["out"], plain[2:4])
    # the mutation: channel 7 leaves the covered atoms out and nothing folds them back in -- this comparison must notice
    mut = EC.voxelize(xyz, offs, sig, origins, NV, tile_k=K, mutant=True)
    assert mut["err"] == 0 and not np.array_equal(mut["out"], plain)
    assert np.array_equal(mut["out"][..., :7], plain[..., :7]) and (mut["out"][..., 7] <= plain[..., 7]).all()
    assert np.array_equal(EC.voxelize(xyz, offs, sig, origins, NV, tile_k=K, mutant=True, cover_fold=-1)["out"], plain)


def test_a_team_of_waves_folds_its_partial_flushes():
    xyz, offs, sig, origins = ragged()
    plain, _ = E.voxelize_lattice(xyz, offs, sig, origins, NV, 1.0, prepass_mode=0, tile_team=0, tile_items=0, direct=0)
    team = EC.voxelize(xyz, offs, sig, origins, NV, tile_team=1)
    assert team["err"] == 0 and np.array_equal(team["out"], plain)
    assert not np.array_equal(EC.voxelize(xyz, offs, sig, origins, NV, tile_team=1, mutant=True)["out"], plain)


def test_frame_handle_two_groups_and_a_periodic_box():
    rng = np.random.default_rng(3)
    n, F = 900, 2
    sig = synth_sigmas(rng, n)
    sig = np.ascontiguousarray(np.concatenate([sig, sig[:, :3] * 0.8], axis=1), np.float32)       # C = 11
    xyz = rng.uniform(0, 23, size=(F * n, 3)).astype(np.float32)
    offs = np.arange(F + 1, dtype=np.int64) * n
    origins = np.tile([-0.5, 3.5, 7.5], (F, 1))
    box = np.tile([23.0, 24.0, 25.0], (F, 1))
    nv = [24, 16, 8]
    plain, e0 = E.voxelize_lattice(xyz, offs, np.tile(sig, (F, 1)), origins, nv, 1.0, box=box, max_images=4, prepass_mode=0, tile_team=0, tile_items=0,
                                   direct=0)
    on = EC.voxelize(xyz, offs, sig, origins, nv, frame_atoms=n, box=box, max_images=4)
    off = EC.voxelize(xyz, offs, sig, origins, nv, frame_atoms=n, box=box, max_images=4, cover_fold=-1)
    assert e0 == 0 and on["err"] == 0 and np.array_equal(on["out"], plain) and np.array_equal(off["out"], plain) and plain[..., 8:].max() > 0.1
    assert not np.array_equal(EC.voxelize(xyz, offs, sig, origins, nv, frame_atoms=n, box=box, max_images=4, mutant=True)["out"], plain)


def dense_item(n, seed=7):
    rng = np.random.default_rng(seed)
    sig = np.ascontiguousarray(synth_sigmas(rng, n), np.float32)
    xyz = rng.uniform([-13, -13, -9], [13, 13, 9], size=(n, 3)).astype(np.float32)
    return xyz, np.array([0, n], np.int64), sig, np.array([[-8.0, -8.0, -4.0]])


@pytest.mark.parametrize("n,over_off,over_on", [(2700, True, False), (3400, True, True)], ids=["dense_only_before_the_fold", "dense_either_way"])
def test_tiles_around_the_640_entry_tier(n, over_off, over_on):
    """tier 0 forced (640 entries per tile): tiles whose entries exceed it go to the DENSE instance, which keeps the full lists; a tile
    goes there by its deduplicated total.  feedback[0] = tiles of the call over tier 0."""
    xyz, offs, sig, origins = dense_item(n)
    plain, _ = E.voxelize_lattice(xyz, offs, sig, origins, NV, 1.0, prepass_mode=0, tile_team=0, tile_items=0, direct=0, lds_tier=0)
    on = EC.voxelize(xyz, offs, sig, origins, NV, lds_tier=0)
    off = EC.voxelize(xyz, offs, sig, origins, NV, lds_tier=0, cover_fold=-1)
    print("tiles over tier 0: fold off", off["feedback"][0], "on", on["feedback"][0], "of", on["feedback"][3])
    assert (off["feedback"][0] > 0) == over_off and (on["feedback"][0] > 0) == over_on
    assert np.array_equal(on["out"], plain) and np.array_equal(off["out"], plain)


def test_a_frame_handle_call_of_one_item_bins_through_the_handle_and_runs_the_team_kernel():
    """the launch sequence of run_lattice for one 24^3 grid of a frame handle: the handle's own binning (the TOPO instances -- a frame
    handle never falls back to the plain call) in front of the team kernel, so the fold runs inside a team"""
    st, text = E.trace_lattice(topo=1, B=1, total_atoms=3000, nx=24, ny=24, nz=24)
    assert st == 0 and "k_bin_count<float, 0, false, true>" in text and "k_voxelize_tiles_team<" in text
    assert "k_bin_solo" not in text and "k_prepass_items" not in text
