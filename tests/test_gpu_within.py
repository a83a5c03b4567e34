"""GPU tier of the proximity selection (moleculekit_amd/within.py): the device's booleans held against what the compiled reference left
in its results array on the golden cases (tests/golden/within_cases.npz) -- through ``within_trajectory`` (masks and index tensors),
``within`` and ``within_distance`` (host arrays) and the C host entry, with the all-pairs kernel forced, the cell list forced and the
plan's own choice.  Reads nothing of the reference: tests/golden only.

Pass criterion (tests/test_within_cpu.py states it): equal arrays; no tolerance.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import within_cases as C  # noqa: E402
from test_within_cpu import GOLDEN, PLANS, expected_kernel, golden_inputs, golden_result  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def W():
    from moleculekit_amd import within
    return within


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from moleculekit_amd import _lib
    c = _lib.default_context(0)
    yield c
    c.set_within_plan(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def device_result(W, torch, ctx, c, plan="unforced", masks=False, **kw):
    """through within_trajectory with the case's gate -> (bool [F, n1] as numpy with the preset ORed in, the kernel the call noted)"""
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")   # noqa: E731
    N = c["coords"].shape[1]
    if masks:
        sel = lambda idx: dev(np.isin(np.arange(N), idx))   # noqa: E731
    else:
        sel = lambda idx: dev(idx.astype(np.int64))   # noqa: E731
    ctx.set_within_plan(PLANS[plan])
    try:
        out = W.within_trajectory(dev(c["coords"]), sel(c["sel1"]), sel(c["sel2"]), c["cutoff"], bounds=(dev(c["mn"]), dev(c["mx"])), ctx=ctx, **kw)
        torch.cuda.synchronize()
        kernel = ctx.last_dist_kernel()
    finally:
        ctx.set_within_plan(0)
    assert out.is_cuda and out.dim() == 2
    got = out.cpu().numpy().astype(bool)
    return (got if c["preset"] is None else got | c["preset"]), kernel


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", C.GOLDEN)
def test_device_booleans_are_the_references(W, torch, ctx, golden, name, plan):
    c = golden_inputs(golden, name)
    got, kernel = device_result(W, torch, ctx, c, plan)
    assert got.dtype == bool and np.array_equal(got, golden_result(golden, name)), f"{name} / {plan}"
    assert kernel == expected_kernel(name, plan, c["coords"].shape[0])


MASKABLE = [n for n in C.GOLDEN if n not in ("unsorted_duplicates",)]     # (a mask has neither order nor duplicates)


@pytest.mark.parametrize("name", MASKABLE)
def test_masks_select_like_index_tensors(W, torch, ctx, golden, name):
    c = golden_inputs(golden, name)
    assert np.array_equal(np.sort(c["sel1"]), c["sel1"]) and len(np.unique(c["sel1"])) == len(c["sel1"])
    got, _ = device_result(W, torch, ctx, c, masks=True)
    assert np.array_equal(got, golden_result(golden, name))


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", C.GOLDEN)
def test_host_arrays_match_the_reference(W, ctx, golden, name, plan):
    c = golden_inputs(golden, name)
    F = c["coords"].shape[0]
    mol = C.Mol(c)
    ctx.set_within_plan(PLANS[plan])
    try:
        # within_distance: the reference's signature, a frame a call, ORing into the preset
        for f in range(F):
            results = np.zeros(len(c["sel1"]), bool) if c["preset"] is None else c["preset"][f].copy()
            W.within_distance(np.ascontiguousarray(mol.coords[:, :, f]), c["cutoff"], c["sel1"], c["sel2"], c["mn"][f], c["mx"][f], results, ctx=ctx)
            assert np.array_equal(results, golden_result(golden, name)[f]), f"{name} frame {f} through within_distance / {plan}"
            assert F > 1 or ctx.last_dist_kernel() == expected_kernel(name, plan)     # (a frame of traj3 alone may take either path)
        # within: all frames in one call, no gate
        got = W.within(mol.coords, c["sel1"], c["sel2"], c["cutoff"], ctx=ctx)
        assert got.shape == (len(c["sel1"]), F) and np.array_equal(got.T, C.ungated(name)), f"{name} through within / {plan}"
        # the C host entry, with the gate
        out = ctx.within_distance_host(mol.coords, c["sel1"], c["sel2"], c["cutoff"], np.ascontiguousarray(np.stack([c["mn"], c["mx"]], axis=1)))
        kernel = ctx.last_dist_kernel()
    finally:
        ctx.set_within_plan(0)
    assert out.dtype == np.uint8 and out.shape == (F, len(c["sel1"]))
    got = out.astype(bool) if c["preset"] is None else out.astype(bool) | c["preset"]
    assert np.array_equal(got, golden_result(golden, name)), f"{name} through the C host entry / {plan}"
    assert kernel == expected_kernel(name, plan, F)


def test_traj3_is_one_call_with_a_different_answer_per_frame(W, torch, ctx, golden):
    c = golden_inputs(golden, "traj3")
    got, kernel = device_result(W, torch, ctx, c)
    want = golden_result(golden, "traj3")
    assert kernel == "mkamd::k_within_pairs" and got.shape == (3, 300) and np.array_equal(got, want)
    assert (want[0] != want[1]).any() and (want[1] != want[2]).any()


def test_out_and_a_stream_of_the_callers(W, torch, ctx, golden):
    c = golden_inputs(golden, "queries_outside_grid")
    want = golden_result(golden, "queries_outside_grid")
    for dtype in (torch.bool, torch.uint8):
        out = torch.full((1, len(c["sel1"])), 1 if dtype == torch.uint8 else True, dtype=dtype, device="cuda")     # every element is written
        got, _ = device_result(W, torch, ctx, c, out=out)
        assert np.array_equal(got, want) and np.array_equal(out.cpu().numpy().astype(bool), want)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        got, _ = device_result(W, torch, ctx, c, stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(got, want)
    one = W.within_trajectory(torch.as_tensor(c["coords"][0], device="cuda"), torch.as_tensor(c["sel1"].astype(np.int64), device="cuda"),
                              torch.as_tensor(c["sel2"].astype(np.int64), device="cuda"), c["cutoff"], ctx=ctx)           # [N, 3] -> [n1]
    assert tuple(one.shape) == (len(c["sel1"]),) and one.dtype == torch.bool and np.array_equal(one.cpu().numpy(), want[0])


def test_two_consecutive_calls_give_identical_bytes(W, torch, ctx, golden):
    for name, plan in (("box_edges", "cells"), ("3ptb_protein_of_ligand", "pairs"), ("crowded_box", "cells")):
        c = golden_inputs(golden, name)
        first, _ = device_result(W, torch, ctx, c, plan)
        second, _ = device_result(W, torch, ctx, c, plan)
        assert first.tobytes() == second.tobytes() and first.any()


def test_errors_on_the_device(W, torch, ctx, golden):
    c = golden_inputs(golden, "self_in_source")
    xyz = torch.as_tensor(c["coords"], device="cuda")
    ok = torch.as_tensor(c["sel2"].astype(np.int64), device="cuda")
    with pytest.raises(ValueError, match="out of range"):
        W.within_trajectory(xyz, torch.tensor([0, 90], device="cuda"), ok, 3.0, ctx=ctx)
    with pytest.raises(ValueError, match="mask must have shape"):
        W.within_trajectory(xyz, torch.ones(89, dtype=torch.bool, device="cuda"), ok, 3.0, ctx=ctx)
    with pytest.raises(ValueError, match="float32"):
        W.within_trajectory(xyz.double(), ok, ok, 3.0, ctx=ctx)
    with pytest.raises(ValueError, match="integer index"):
        W.within_trajectory(xyz, ok.float(), ok, 3.0, ctx=ctx)
    with pytest.raises(ValueError, match="bounds"):
        W.within_trajectory(xyz, ok, ok, 3.0, bounds=(torch.zeros((2, 3), device="cuda"), torch.zeros((2, 3), device="cuda")), ctx=ctx)
    with pytest.raises(ValueError, match="out:"):
        W.within_trajectory(xyz, ok, ok, 3.0, out=torch.zeros((1, 5), dtype=torch.bool, device="cuda"), ctx=ctx)
    with pytest.raises(ValueError, match="out of range"):
        ctx.within_distance_host(np.zeros((4, 3, 1), np.float32), np.array([4], np.uint32), np.array([0], np.uint32), 3.0)
    got, _ = device_result(W, torch, ctx, c)
    assert np.array_equal(got, golden_result(golden, "self_in_source"))
