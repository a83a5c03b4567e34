"""GPU tier: the class flush of the tile kernels (round 11) -- one scalar branch on `fast` per class, the cutoff
applied to the class minimum as a masked minimum (mk_min_bits_where, csrc/kernels.h: on the device one asm statement that narrows EXEC
with v_cmpx, takes the minimum and restores EXEC).  This is the only tier that runs the device form.

The inputs are the batches of tests/class_flush_cases.py, one item per case, on 16 x 16 x 8 at K = 8 and 8 x 16 x 16 at K = 4: atoms at
exactly 5 A and 1e-3 A nearer, an atom on a voxel centre in channels 3 and 7, a fast and an exact class in one channel, a one-entry
group, a group that reaches half of the planes only, an empty channel, an item absent from every channel.  Every batch is held as
tests/test_gpu_cand_cursor.py holds its cases (`held_two_ways`: the column and the direct layout, the handle call with the cover fold
on and off, all ``torch.equal``; the oracle at tests/cases.py: TOL); ``force_general`` and the one-item calls (the team kernel) are
``torch.equal`` to them."""
import numpy as np
import pytest

from tests import class_flush_cases as CF
from tests.test_gpu_batch_topology import tens
from tests.test_gpu_cand_cursor import chain, held_two_ways          # noqa: F401  (chain: the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", [4, 8])
def test_every_path_flushes_the_same_bits(chain, K):
    import torch
    from moleculekit_amd import batch
    xyz, offs, sig, origins, nv = CF.batch(K)
    chain.set_tile_k(K)
    out = held_two_ways(chain, xyz, offs, sig, nv, origins)
    CF.check_values(out.cpu().numpy(), K)
    chain.set_force_general(True)
    general = held_two_ways(chain, xyz, offs, sig, nv, origins, handle=False)
    chain.set_force_general(False)
    assert torch.equal(out, general)
    # one item per call: four waves per tile, every wave flushes its own partial minima
    t = tens(chain)
    chain.set_tile_team(1)
    for b in range(len(offs) - 1):
        a0, a1 = int(offs[b]), int(offs[b + 1])
        one = batch.voxelize_lattice_torch(t(xyz[a0:a1], np.float32), t([0, a1 - a0], np.int64), t(sig[a0:a1], np.float32), t(origins[b:b + 1], np.float64),
                                           nv, 1.0, ctx=chain)
        chain.synchronize()
        if sig[a0:a1].any():
            assert "k_voxelize_tiles_team" in chain.last_tile_kernel()
        assert torch.equal(one[0], out[b]), CF.ITEMS[b]
