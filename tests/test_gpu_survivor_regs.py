"""GPU tier: the survivors a tile keeps in registers between its histogram pass and its placement pass (round 10)
on the shapes of tests/test_gpu_cand_cursor.py: 16 x 16 x 8 and 24 x 16 x 8 grids at K = 4 and K = 8.

The inputs are the batches of tests/survivor_cases.py, one item per case, each aimed at one tile: survivor counts of 63, 64, 65, 128, 129
and 479 (the chunk boundaries of the eight survivor registers of a lane), 490 (over the list's 480: the two traversals), 256 and 257
candidates (the two sides of the list condition), a survivor in all eight channels beside survivors in one, survivors whose channel-7
entry the cover fold takes away beside ones whose channel 7 stays, every x-reach value in every survivor register, an empty item and
an item absent from every channel.  The counts are not guessed: tests/test_emu_survivor_regs.py reads them out of the emulated kernel
for these very inputs and asserts them.

Every batch is held as tests/test_gpu_cand_cursor.py holds its cases (`held_two_ways`): against the oracle at tests/cases.py: TOL,
``torch.equal`` between the column layout and the direct layout, and ``torch.equal`` to the handle call with the cover fold on and off;
``force_general`` is ``torch.equal`` to the sorted path."""
import pytest

from tests import survivor_cases as SC
from tests.test_gpu_cand_cursor import chain, held_two_ways          # noqa: F401  (chain: the fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("K", [4, 8])
@pytest.mark.parametrize("grid", sorted(SC.GRIDS))
def test_survivor_counts_at_the_chunk_boundaries(chain, grid, K):
    xyz, offs, sig, origins, nv = SC.batch(grid, K)
    chain.set_tile_k(K)
    out = held_two_ways(chain, xyz, offs, sig, nv, origins)
    assert float(out[8].abs().max()) == 0.0 and float(out[9].abs().max()) == 0.0          # the empty item, the absent one
    for b, item in enumerate(SC.ITEMS):
        if item[4] is not None:
            assert float(out[b].max()) > 0.5, b
    # the atoms in all eight channels reach every one of them
    assert float(out[0].amax(dim=0).min()) > 0.5


@pytest.mark.parametrize("K", [4, 8])
def test_force_general(chain, K):
    import torch
    grid = "16x16x8"
    xyz, offs, sig, origins, nv = SC.batch(grid, K)
    chain.set_tile_k(K)
    sorted_path = held_two_ways(chain, xyz, offs, sig, nv, origins, handle=False)
    chain.set_force_general(True)
    general = held_two_ways(chain, xyz, offs, sig, nv, origins, handle=False)
    assert torch.equal(sorted_path, general)
