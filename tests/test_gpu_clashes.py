"""GPU tier of the steric-clash search (moleculekit_amd/clashes.py, moleculekit_amd/distance.py: find_clashes): the device's arrays held
against what the compiled reference returned on the golden cases (tests/golden/clash_cases.npz) -- through ``find_clashes_tensor``,
``find_clashes`` (host arrays) and the C host entry, with a thread per owner, with a wave per owner and with the plan's own choice.
Reads nothing of the reference: tests/golden only.

Pass criterion (tests/test_clashes_cpu.py states it): equal arrays, rows in order; no tolerance.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clashes_cases as C  # noqa: E402
from test_clashes_cpu import GOLDEN, PLANS, golden_inputs, golden_result, library_inputs, same_result  # noqa: E402

pytestmark = pytest.mark.gpu
THREAD_KERNEL, WAVE_KERNEL = "mkamd::k_clash_pairs_thread", "mkamd::k_clash_pairs_wave"
EXPECTED = {"unforced": WAVE_KERNEL, "wave": WAVE_KERNEL, "thread": THREAD_KERNEL}       # (every golden case has at most 8 192 owners)
NO_PAIR_KERNEL = ("empty_sel1",)                                                          # ... and a call without owners never reaches the pair kernels


@pytest.fixture(scope="module")
def CL():
    from moleculekit_amd import clashes
    return clashes


@pytest.fixture(scope="module")
def D():
    from moleculekit_amd import distance
    return distance


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from moleculekit_amd import _lib
    c = _lib.default_context(0)
    yield c
    c.set_clash_plan(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def device_arrays(CL, torch, ctx, c, plan="unforced", index_selections=False):
    """through find_clashes_tensor -> (pairs, distances, overlaps) as numpy, the kernel the call noted"""
    n = len(c["coords"])
    radii, mask1, mask2, ex, _ = library_inputs(c)
    sel = lambda m: None if m is None else torch.as_tensor(np.flatnonzero(m) if index_selections else m, device="cuda")   # noqa: E731
    ctx.set_clash_plan(PLANS[plan])
    try:
        out = CL.find_clashes_tensor(torch.as_tensor(c["coords"], device="cuda").reshape(n, 3), torch.as_tensor(radii, device="cuda"), sel(mask1),
                                     sel(mask2), c["overlap"], ex, ctx=ctx)
        torch.cuda.synchronize()
        kernel = ctx.last_dist_kernel()
    finally:
        ctx.set_clash_plan(0)
    p, d, o = out
    assert p.is_cuda and p.dtype == torch.int64 and p.dim() == 2 and p.shape[1] == 2 and d.dtype == torch.float32 and o.dtype == torch.float32
    return (p.cpu().numpy(), d.cpu().numpy(), o.cpu().numpy()), kernel


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", C.GOLDEN)
def test_device_arrays_are_the_references(CL, torch, ctx, golden, name, plan):
    got, kernel = device_arrays(CL, torch, ctx, golden_inputs(golden, name), plan)
    same_result(got, golden_result(golden, name), f"{name} / {plan}")
    if name not in NO_PAIR_KERNEL:
        assert kernel == EXPECTED[plan]


@pytest.mark.parametrize("name", ["cross_overlap", "cross_equal", "3ptb_cross_mask", "lanes65"])
def test_index_tensors_select_like_masks(CL, torch, ctx, golden, name):
    got, _ = device_arrays(CL, torch, ctx, golden_inputs(golden, name), index_selections=True)
    same_result(got, golden_result(golden, name), name + " with index tensors")


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", C.GOLDEN)
def test_find_clashes_matches_the_reference(D, ctx, golden, name, plan):
    c = C.case(name)
    ctx.set_clash_plan(PLANS[plan])
    try:
        got = D.find_clashes(C.as_mol(c, frame=1, frames=3), ctx=ctx, **C.kwargs(c))
    finally:
        ctx.set_clash_plan(0)
    same_result(got, golden_result(golden, name), f"{name} through find_clashes / {plan}")


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", C.GOLDEN)
def test_the_c_host_entry_matches_the_reference(ctx, golden, name, plan):
    c = golden_inputs(golden, name)
    radii, mask1, mask2, ex, cutoff = library_inputs(c)
    ctx.set_clash_plan(PLANS[plan])
    try:
        p, d, o, info = ctx.find_clashes_host(c["coords"], radii, np.ascontiguousarray(mask1, np.uint32),
                                              None if mask2 is None else np.ascontiguousarray(mask2, np.uint32), None if ex is None else ex.start,
                                              None if ex is None else ex.partner, c["overlap"], cutoff)
        kernel = ctx.last_dist_kernel()
    finally:
        ctx.set_clash_plan(0)
    assert p.dtype == np.int32
    same_result((p.astype(np.int64), d, o), golden_result(golden, name), f"{name} through the C host entry / {plan}")
    if info[5] > 0:
        assert kernel == EXPECTED[plan]


def test_many_owners_in_sparse_boxes_take_the_thread_kernels_unforced(CL, torch, ctx):
    c = dict(C.lattice(), bonds_used=C.NO_BONDS, exclude_bonded=False, exclude_14=False)
    thread, kernel = device_arrays(CL, torch, ctx, c)
    assert kernel == THREAD_KERNEL and len(thread[0]) > 1000
    wave, kernel = device_arrays(CL, torch, ctx, c, "wave")
    assert kernel == WAVE_KERNEL and all(x.tobytes() == y.tobytes() for x, y in zip(thread, wave))


@pytest.mark.parametrize("name", ["overlap_m15", "3ptb_cross_mask", "crowded"])
def test_two_consecutive_calls_give_identical_bits(CL, torch, ctx, golden, name):
    c = golden_inputs(golden, name)
    first, _ = device_arrays(CL, torch, ctx, c)
    second, _ = device_arrays(CL, torch, ctx, c)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, second)) and len(first[0])


def test_over_cap_raises_and_the_context_serves_the_next_call(CL, D, torch, ctx, golden):
    over = dict(C.over_cap(), bonds_used=C.NO_BONDS)
    for plan in PLANS:
        with pytest.raises(ValueError, match=r"crowded box: box 0 .* holds 4097 atoms, more than the 4096"):
            device_arrays(CL, torch, ctx, over, plan)
    with pytest.raises(ValueError, match="holds 4097 atoms"):
        D.find_clashes(C.as_mol(over), guess_bonds=False, ctx=ctx)
    got, _ = device_arrays(CL, torch, ctx, golden_inputs(golden, "overlap_06"))
    same_result(got, golden_result(golden, "overlap_06"), "overlap_06 after the refused calls")


def test_errors_on_the_device(CL, D, torch, ctx, golden):
    c = golden_inputs(golden, "overlap_06")
    bad = dict(c, coords=c["coords"].copy())
    bad["coords"][5, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        device_arrays(CL, torch, ctx, bad)
    with pytest.raises(ValueError, match="non-finite"):
        D.find_clashes(C.as_mol(bad), guess_bonds=False, ctx=ctx)
    unselected = dict(bad, sel1=np.delete(np.arange(60), 5))                            # the bad atom in no selection: not looked at
    got, _ = device_arrays(CL, torch, ctx, unselected)
    assert len(got[0]) and not (got[0] == 5).any()
    coords, radii = torch.as_tensor(c["coords"], device="cuda"), torch.as_tensor(CL.clash_radii(c["element"]), device="cuda")
    with pytest.raises(ValueError, match="out of range"):
        CL.find_clashes_tensor(coords, radii, torch.tensor([0, 60], device="cuda"), ctx=ctx)
    with pytest.raises(ValueError, match="shape"):
        CL.find_clashes_tensor(coords, radii, torch.ones(59, dtype=torch.bool, device="cuda"), ctx=ctx)
    with pytest.raises(ValueError, match="exclusions were built for"):
        CL.find_clashes_tensor(coords, radii, torch.ones(60, dtype=torch.bool, device="cuda"), exclusions=CL.clash_exclusions([(0, 1)], 59), ctx=ctx)
    with pytest.raises(ValueError, match="ascend"):
        ctx.find_clashes_host(c["coords"], CL.clash_radii(c["element"]), np.ones(60, np.uint32), None, np.array([0, 2] + [2] * 59, np.uint32),
                              np.array([7, 3], np.uint32), 0.6, 2.8)
    got, _ = device_arrays(CL, torch, ctx, c)
    same_result(got, golden_result(golden, "overlap_06"), "overlap_06 after the refused calls")
