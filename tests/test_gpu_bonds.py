"""GPU tier of the bond guesser (moleculekit_amd/bonds.py): the device's lists held against what the compiled reference returned on
the golden cases (tests/golden/bond_cases.npz) -- through ``guess_bonds_tensor``, ``bond_grid_search`` and ``guess_bonds``, with a
thread per owner, with a wave per owner and with the plan's own choice.  Reads nothing of the reference: tests/golden only.

Pass criterion (tests/test_bonds_cpu.py states it): equal arrays, rows in order; no tolerance.
"""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bonds_cases as C  # noqa: E402
import bonds_restatement as R  # noqa: E402
from test_bonds_cpu import GOLDEN, PLANS, same_list  # noqa: E402

pytestmark = pytest.mark.gpu
THREAD_KERNEL, WAVE_KERNEL = "mkamd::k_bond_pairs_thread", "mkamd::k_bond_pairs_wave"


@pytest.fixture(scope="module")
def B():
    from moleculekit_amd import bonds
    return bonds


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from moleculekit_amd import _lib
    c = _lib.default_context(0)
    yield c
    c.set_bond_plan(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def device_list(B, torch, ctx, c, plan="unforced", cutoff=True):
    ctx.set_bond_plan(PLANS[plan])
    try:
        pairs = B.guess_bonds_tensor(torch.as_tensor(c["coords"], device="cuda"), torch.as_tensor(c["radii"], device="cuda"),
                                     torch.as_tensor(c["is_h"].astype(np.int32), device="cuda"), c["grid_cutoff"] if cutoff else None, ctx=ctx)
        torch.cuda.synchronize()
        kernel = ctx.last_dist_kernel()
    finally:
        ctx.set_bond_plan(0)
    assert pairs.dtype == torch.int32 and pairs.is_cuda and pairs.dim() == 2 and pairs.shape[1] == 2
    return pairs.cpu().numpy(), kernel


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", C.GOLDEN)
def test_device_list_is_the_references(B, torch, ctx, golden, name, plan):
    c = C.case(name)
    pairs, kernel = device_list(B, torch, ctx, c, plan)
    same_list(pairs, golden[f"{name}/pairs"], f"{name} / {plan}")
    crowded = name == "crowded"
    assert kernel == {"unforced": WAVE_KERNEL if crowded else THREAD_KERNEL, "wave": WAVE_KERNEL, "thread": THREAD_KERNEL}[plan]


@pytest.mark.parametrize("name", C.GOLDEN)
def test_the_references_functions_match_the_reference(B, ctx, golden, name):
    c = C.case(name)
    pairs = B.bond_grid_search(c["coords"], c["grid_cutoff"], c["is_h"], c["radii"], ctx=ctx)
    assert pairs.dtype == np.uint32
    same_list(pairs, golden[f"{name}/pairs"], name + " through bond_grid_search")
    if "element" in c:
        pairs = B.guess_bonds(C.as_mol(c, frame=1, frames=3), ctx=ctx)
        assert pairs.dtype == np.uint32
        same_list(pairs, golden[f"{name}/pairs"], name + " through guess_bonds")


def test_the_default_cutoff_is_the_references(B, torch, ctx, golden):
    pairs, _ = device_list(B, torch, ctx, C.case("3ptb"), cutoff=False)
    same_list(pairs, golden["3ptb/pairs"], "3ptb with the default grid_cutoff")


@pytest.mark.parametrize("name", ["3ptb_shuffled", "water", "crowded"])
def test_two_consecutive_calls_give_identical_bits(B, torch, ctx, name):
    c = C.case(name)
    first, _ = device_list(B, torch, ctx, c)
    second, _ = device_list(B, torch, ctx, c)
    assert first.tobytes() == second.tobytes() and len(first)


def test_over_cap_raises_and_the_context_serves_the_next_call(B, torch, ctx, golden):
    over = C.over_cap()
    for plan in PLANS:
        with pytest.raises(ValueError, match=r"crowded box: box 0 .* holds 4097 atoms, more than the 4096"):
            device_list(B, torch, ctx, over, plan)
    with pytest.raises(ValueError, match="holds 4097 atoms"):
        B.bond_grid_search(over["coords"], over["grid_cutoff"], over["is_h"], over["radii"], ctx=ctx)
    pairs, _ = device_list(B, torch, ctx, C.case("3ptb"))
    same_list(pairs, golden["3ptb/pairs"], "3ptb after the refused call")
    inside = {k: (v[:-1] if isinstance(v, np.ndarray) else v) for k, v in over.items()}           # 4 096 coincident atoms: inside the cap, no bond
    pairs, kernel = device_list(B, torch, ctx, inside)
    assert pairs.shape == (0, 2) and kernel == WAVE_KERNEL


def test_errors_and_empty_results_on_the_device(B, torch, ctx):
    c = C.case("one_box")
    bad = dict(c, coords=c["coords"].copy())
    bad["coords"][5, 2] = np.nan
    with pytest.raises(ValueError, match="finite"):
        device_list(B, torch, ctx, bad)
    with pytest.raises(ValueError, match="grid_cutoff"):
        device_list(B, torch, ctx, dict(c, grid_cutoff=0.0))
    one = {k: (v[:1] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    none = {k: (v[:0] if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    assert device_list(B, torch, ctx, one)[0].shape == (0, 2) and device_list(B, torch, ctx, none)[0].shape == (0, 2)
    same_list(device_list(B, torch, ctx, c)[0], C.restated("one_box")[0], "one_box after the refused calls")


def test_wrap_with_guessed_bonds_end_to_end(B, ctx):
    """the water case through wrap_molecule(guessBonds=True, guess_on_device=True) against wrap() on the restatement's groups"""
    import moleculekit_amd.wrap as W

    c = C.case("water")
    rng = np.random.default_rng(11)
    frames, box = 3, 31.0
    shift = rng.uniform(-40.0, 40.0, size=(1, 3, frames)).astype(np.float32)
    coords = (c["coords"][:, :, None] + shift).astype(np.float32)
    mol = types.SimpleNamespace(coords=coords.copy(), box=np.full((3, frames), box, np.float32), boxangles=np.full((3, frames), 90.0, np.float32),
                                bonds=np.zeros((0, 2), np.uint32), numAtoms=len(coords), frame=2, numFrames=frames, element=c["element"], name=c["name"])
    groups = W.bonded_groups(R.guess(coords[:, :, 2], c["element"], c["name"]), len(coords))
    assert len(groups) == 1001                                          # the waters
    corner = np.arange(30, dtype=np.uint32)                             # ten waters at a corner of the lattice: most of the others move
    want = W.wrap(coords.copy(), mol.box, groups, centersel=corner, ctx=ctx)
    W.wrap_molecule(mol, corner, guessBonds=True, guess_on_device=True, ctx=ctx)
    assert np.array_equal(mol.coords, want) and not np.array_equal(want, coords)
