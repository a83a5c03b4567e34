"""GPU tier of the ring interactions (moleculekit_amd/interactions.py): the device's lists held against what the compiled reference
returned on the golden cases (tests/golden/ring_cases.npz) and against the numpy restatement of its loops on every case
(tests/rings_restatement.py) -- through the device entry, the host entry and the three ``*_calculate`` functions, under both lane
assignments, in one chunk and in many, on the current and on a non-default stream.  Reads nothing of the reference: tests/golden only.

Pass criteria (tests/test_rings_cpu.py states them): frame offsets, pairs and the bits of the float32 distances equal; every float32
angle within one float32 unit in the last place; the stacked-copy case drops the pair in exactly the reference's frames.  The number of
angles that are not bit-equal is printed (it is not a criterion).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rings_cases as RC  # noqa: E402
from test_rings_cpu import GOLDEN, _Mol, _nested, assert_same_lists  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = [c["name"] for c in RC.cases()]
KIND = {RC.PIPI: "pipi", RC.CATIONPI: "cationpi", RC.SIGMAHOLE: "sigmahole"}


@pytest.fixture(scope="module")
def I():
    from moleculekit_amd import interactions
    return interactions


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from moleculekit_amd import _lib
    c = _lib.default_context(0)
    yield c
    c.set_ring_plan(0, 0)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def device_lists(I, torch, ctx, c, avoid=0, chunk=0, stream=None, box=True):
    atoms, s1, second = RC.flatten(c)
    ctx.set_ring_plan(avoid, chunk)
    try:
        offs, pairs, da = I.ring_interactions_trajectory(KIND[c["kind"]], torch.as_tensor(c["coords"], device="cuda"),
                                                         torch.as_tensor(c["box"], device="cuda") if box else None, atoms, s1, second, c["thr"],
                                                         ctx=ctx, stream=stream)
        torch.cuda.synchronize()
        name = ctx.last_dist_kernel()
    finally:
        ctx.set_ring_plan(0, 0)
    if avoid:
        assert name.endswith("k_ring_count_frames" if avoid == 2 else "k_ring_count_pairs"), name
    assert pairs.dtype == torch.int32 and da.dtype == torch.float32 and pairs.is_cuda and da.is_cuda
    assert tuple(pairs.shape) == tuple(da.shape) == (int(offs[-1]), 2)
    return offs, pairs.cpu().numpy().view(np.uint32), da.cpu().numpy()


def host_lists(I, ctx, c, avoid=0, chunk=0):
    atoms, s1, second = RC.flatten(c)
    ctx.set_ring_plan(avoid, chunk)
    try:
        return I._host_call(c["kind"], c["coords"], c["box"], atoms, s1, second, c["thr"], ctx=ctx)
    finally:
        ctx.set_ring_plan(0, 0)


@pytest.mark.parametrize("name", RC.GOLDEN)
def test_device_entry_matches_the_reference(I, torch, ctx, golden, name):
    c = RC.case(name)
    want = (golden[f"{name}/offsets"], golden[f"{name}/pairs"], golden[f"{name}/distang"])
    off = 0
    for avoid in (0, 1, 2):
        off = max(off, assert_same_lists(device_lists(I, torch, ctx, c, avoid=avoid), want, f"{name} [avoid {avoid}]"))
    print(f"{name}: {len(want[1])} pairs, {off} angles not bit-equal to the reference's")


@pytest.mark.parametrize("name", NAMES)
def test_every_case_through_every_entry_and_plan(I, torch, ctx, name):
    c = RC.case(name)
    want = RC.expected(c)
    F = c["coords"].shape[2]
    off = 0
    for avoid, chunk in ((0, 0), (2, 0), (1, 0), (2, 64), (1, 7), (2, 5) if F <= 70 else (2, 128)):
        off = max(off, assert_same_lists(device_lists(I, torch, ctx, c, avoid=avoid, chunk=chunk), want, f"{name} device [avoid {avoid}, chunk {chunk}]"))
    for avoid, chunk in ((0, 0), (1, 64), (2, 3) if F <= 70 else (2, 64)):
        off = max(off, assert_same_lists(host_lists(I, ctx, c, avoid=avoid, chunk=chunk), want, f"{name} host [avoid {avoid}, chunk {chunk}]"))
    print(f"{name}: {len(want[1])} pairs, {off} angles not bit-equal to the restatement's")


def test_stacked_copy_drops_exactly_the_reference_frames(I, torch, ctx, golden):
    c = RC.case("pp_stacked_copy")
    per_frame = np.diff(golden["pp_stacked_copy/offsets"])
    assert 0 < per_frame.sum() < per_frame.size
    for avoid in (1, 2):
        offs, _, _ = device_lists(I, torch, ctx, c, avoid=avoid)
        assert np.array_equal(np.diff(offs), per_frame)
    assert np.array_equal(np.diff(host_lists(I, ctx, c)[0]), per_frame)


def test_non_default_stream_and_null_box(I, torch, ctx):
    c = RC.case("cp_65x64_f200")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        coords = torch.as_tensor(c["coords"], device="cuda")
    s.synchronize()
    atoms, s1, second = RC.flatten(c)
    offs, pairs, da = I.ring_interactions_trajectory("cationpi", coords, None, atoms, s1, second, c["thr"], ctx=ctx, stream=s.cuda_stream)
    assert_same_lists((offs, pairs.cpu().numpy().view(np.uint32), da.cpu().numpy()), RC.expected(c), "foreign stream, box None")
    c = RC.case("pp_9x7_f65_box")
    assert_same_lists(device_lists(I, torch, ctx, c, stream=s.cuda_stream), RC.expected(c), "foreign stream, periodic")


@pytest.mark.parametrize("name", ["pp_shared_rings_fused", "pp_9x7_f65_box", "cp_fused_5x9_f2", "cp_7x9_f65_box", "sh_63x130_f3", "sh_6x8_f64_box"])
def test_calculate_functions_on_the_device(I, name):
    c = RC.case(name)
    fn = {RC.PIPI: I.pipi_calculate, RC.CATIONPI: I.cationpi_calculate, RC.SIGMAHOLE: I.sigmahole_calculate}[c["kind"]]
    idx, da = fn(_Mol(c), c["rings1"], c["second"], *c["thr"])
    offs, pairs, distang = RC.expected(c)
    want_idx, want_da = _nested(offs, pairs, distang)
    assert idx == want_idx
    got = np.array([v for f in da for v in f], np.float64).astype(np.float32).reshape(-1, 2)
    assert_same_lists((offs, pairs, got), (offs, pairs, distang), name)
    assert [len(f) for f in da] == [len(f) for f in want_da]
    ridx, _ = fn(_Mol(c), c["rings1"], c["second"], *c["thr"], return_rings=True)
    f = next(f for f in range(len(idx)) if idx[f])
    assert ridx[f][0][0] is c["rings1"][idx[f][0][0]]


def test_host_entry_refuses_bad_lists(I, ctx):
    c = RC.case("cp_3x63_f3")
    atoms, s1, cations = RC.flatten(c)
    from moleculekit_amd import _lib
    N = c["coords"].shape[0]
    thr = np.array([5, 60, 0, 0], np.float32)
    bad = cations.copy()
    bad[5] = N
    with pytest.raises(Exception, match="partner atom index out of range"):
        ctx.ring_interactions_host(RC.CATIONPI, c["coords"], c["box"], atoms, s1, None, bad, len(bad), thr)
    short = s1.copy()
    short[1] = short[0] + 2
    with pytest.raises(Exception, match="fewer than 3 atoms"):
        ctx.ring_interactions_host(RC.CATIONPI, c["coords"], c["box"], atoms, short, None, cations, len(cations), thr)
    with pytest.raises(Exception, match="kind must be"):
        ctx.ring_interactions_host(5, c["coords"], c["box"], atoms, s1, None, cations, len(cations), thr)
    with pytest.raises(Exception, match="ring plan"):
        ctx.set_ring_plan(3, 0)
    assert _lib is not None
