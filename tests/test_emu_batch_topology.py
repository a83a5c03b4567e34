"""CPU tier: the BATCH topology handle (round 7) on the host emulation of the product's kernels -- one ragged case bit for bit against
the plain call, the device-side check of the call's items, and the launch sequences run_lattice issues for such a call (in the style
of tests/test_lattice_paths.py: chain, periodic, wide; the calls the chain does not serve)."""
import re

import numpy as np
import pytest

from tests import emu_batch_topo_build as EB
from tests import emu_build as E
from tests.synth import synth_sigmas

SIZES = [700, 0, 1100, 300, 450]          # item 1 empty, item 3 absent from every channel
NV = [16, 16, 8]


def ragged(C=8, wide=False):
    rng = np.random.default_rng(12)
    offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(offs[-1])
    sig = synth_sigmas(rng, n)
    if C > 8:
        sig = np.concatenate([sig, sig[:, :C - 8] * 0.8], axis=1)
    sig = np.ascontiguousarray(sig, np.float32)
    sig[::7, 0] = 1.1; sig[::7, 1] = 1.9                     # atoms with several distinct sigmas in one row
    sig[offs[3]:offs[4]] = 0.0
    xyz = rng.uniform(-10, 10, size=(n, 3)).astype(np.float32)
    if wide:
        for b in (0, 4):
            rows = np.arange(offs[b], offs[b + 1])[::37]
            sig[rows, 6] = 2.27
            xyz[rows] = np.round(xyz[rows])
    origins = np.tile([-8.0, -8.0, -4.0], (len(SIZES), 1)) + np.arange(len(SIZES))[:, None] * 1.0
    return xyz, offs, sig, origins


@pytest.mark.parametrize("C,wide", [(8, False), (11, True)], ids=["C8", "C11_wide"])
def test_ragged_batch_and_a_chunk_are_bitwise_the_plain_call(C, wide):
    xyz, offs, sig, origins = ragged(C, wide)
    plain, e0 = E.voxelize_lattice(xyz, offs, sig, origins, NV, 1.0, prepass_mode=0, tile_team=0, tile_items=0, direct=0)
    got, e1, nwide = EB.voxelize_range(xyz, offs, sig, origins, NV)
    assert e0 == 0 and e1 == 0 and nwide > 0                 # (the synthetic radii include wide ones: the fix-up runs in every case)
    assert np.array_equal(plain, got) and plain.max() > 0.5 and not plain[1].any() and not plain[3].any()
    chunk, e2, _ = EB.voxelize_range(xyz, offs, sig, origins, NV, lo=2, hi=5)
    assert e2 == 0 and np.array_equal(chunk, plain[2:5])
    if wide:
        inplace, e3, _ = EB.voxelize_range(xyz, offs, sig, origins, NV, exact_redo=-1)
        assert e3 == 0 and np.array_equal(inplace, plain)


def test_items_that_are_not_the_handles_are_flagged_on_the_device():
    xyz, offs, sig, origins = ragged(8, True)
    bad = offs.copy()
    bad[3] -= 5                                               # the right total, split differently
    _, err, _ = EB.voxelize_range(xyz, offs, sig, origins, NV, call_offsets=bad)
    assert err & 8                                            # MK_ERR_TOPOLOGY
    with pytest.raises(RuntimeError, match="range of the batch topology"):
        EB.voxelize_range(xyz, offs, sig, origins, NV, lo=1, hi=5, call_offsets=offs)      # another atom count than the range's


def test_calls_the_chain_does_not_serve_are_the_plain_call_on_the_handles_sigmas():
    xyz, offs, sig, origins = ragged()
    plain, _ = E.voxelize_lattice(xyz, offs, sig, origins, NV, 1.0)
    for knobs in (dict(prepass_mode=-1, tile_team=-1, tile_items=-1, direct=-1), dict(prepass_mode=1), dict(direct=1), dict(direct=2)):
        got, err, _ = EB.voxelize_range(xyz, offs, sig, origins, NV, **knobs)
        assert err == 0 and np.array_equal(got, plain), knobs
        chunk, err, _ = EB.voxelize_range(xyz, offs, sig, origins, NV, lo=2, hi=4, **knobs)
        assert err == 0 and np.array_equal(chunk, plain[2:4]), knobs


def kernels(text):
    return [l.split()[1].replace("mkamd::", "") for l in text.splitlines() if l.lstrip().startswith("launch ")]


def line_of(text, kernel):
    return [l for l in text.splitlines() if l.lstrip().startswith("launch ") and kernel in l][0]


def test_launch_sequences_of_a_batch_handle_call():
    # 30 items of 5 000 atoms on 24^3 grids, in order: the chain with the TOPO binning kernels, nothing that reads a sigma row in front
    # of the tile kernel, the handle's table to the tile kernels
    st, text = EB.trace()
    k = kernels(text)
    assert st == 0 and k[0] == "k_bin_count<float," and "0, false, true>" in line_of(text, "k_bin_count")
    assert "k_bin_fill<float, false, true>" in text
    assert not any(x.startswith(("k_bin_solo", "k_prepass_items", "k_bin_direct")) for x in k)
    assert "topo.ids " in line_of(text, "k_bin_count") and "topo.table" in line_of(text, "k_voxelize_tiles") and "topo.sigmas" in line_of(text, "k_tail")
    assert "topo.sigmas" not in text.split("k_tail")[0]
    # a chunk: every sigma-side array handed over at the range's first atom (item 10 of 5 000 atoms: ids 4 bytes per atom, 8 x 4 per sigma row)
    st, text = EB.trace(first_item=10, B=10, tile_team=0)
    assert st == 0 and "topo.ids+%d " % (10 * 5000 * 4) in line_of(text, "k_bin_count") and "topo.sigmas+%d " % (10 * 5000 * 32) in line_of(text, "k_tail")
    # periodic
    st, text = EB.trace(pbc=1, max_images=2)
    assert st == 0 and "k_bin_count<float, 1, false, true>" in text
    # wide atoms: k_tail + the shells + the redo list, jobs = the wide atoms of the RANGE; inside k_tail alone with exact_redo -1
    st, text = EB.trace(wide_every=1000)
    assert st == 0 and "k_exact_redo<float>" in text and "grid 150 " in line_of(text, "k_exact_shells<float, false>")
    st, half = EB.trace(wide_every=1000, first_item=15, tile_team=0)
    assert st == 0 and "grid 75 " in line_of(half, "k_exact_shells<float, false>") and "topo.wide_list+%d " % (75 * 4) in line_of(half, "k_exact_shells<float, false>")
    st, text = EB.trace(wide_every=1000, exact_redo=-1)
    assert st == 0 and "k_exact_shells" not in text and "topo.wide_list" in line_of(text, "k_tail")
    # big calls: pipelined they keep the handle; in order the same call takes the direct pass -- the plain call on the handle's sigma copy
    st, text = EB.trace(n_items=80, pipelining=1, calls=2)
    assert st == 0 and text.count("k_bin_count<float, 0, false, true>") == 2 and "k_bin_direct" not in text
    st, text = EB.trace(n_items=80)
    assert st == 0 and kernels(text)[0].startswith("k_bin_direct<float>") and "topo.sigmas" in line_of(text, "k_bin_direct") and "topo.ids" not in text
    # ligand-sized items (the one-launch per-item pre-pass) and a small call (the one-launch pre-pass of the team regime): plain as well
    st, text = EB.trace(n_items=64, item_atoms=60)
    assert st == 0 and kernels(text)[0].startswith("k_prepass_items<float") and "topo.sigmas" in text and "topo.ids" not in text
    st, text = EB.trace(first_item=10, B=10)
    assert st == 0 and kernels(text)[0].startswith("k_bin_solo<float>") and "topo.sigmas+%d " % (10 * 5000 * 32) in line_of(text, "k_bin_solo")
