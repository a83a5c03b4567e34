"""GPU tier of the secondary structure (moleculekit_amd/dssp.py): the conditions of tests/test_dssp_cpu.py on
the device.  The device's bytes equal the numpy restatement's on every case of tests/dssp_cases.py and on 3PTB with seeded noise --
tensor route, host route and MetricSecondaryStructure.project; each energy plan forced through Context.set_dssp_plan (1: not the
frame-lane kernel, 2: not the acceptor-lane kernel, + 4: chunks of 64 frames), the kernel taken asserted through
last_dist_kernel(); 1, 2, 63, 64, 65 and 130 frames; two runs the same bytes; the reference's three known answers.  The call takes
no box, so there is no box on a wrong device to refuse; a non-contiguous coordinate tensor is.  Reads tests/golden only."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dssp_cases as C  # noqa: E402
import dssp_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
KERNELS = {1: "k_dssp_energy_atoms", 2: "k_dssp_energy_frames"}


@pytest.fixture(scope="module")
def ctx():
    from moleculekit_amd import _lib
    c = _lib.default_context()
    yield c
    c.set_dssp_plan(0)


@pytest.fixture(scope="module")
def cases():
    return C.cases()


@pytest.fixture(scope="module")
def noisy():
    """3PTB x 130 noisy frames and the restatement's full codes: computed once, never modified"""
    case = C.noisy_3ptb(130)
    return case, R.dssp(*case)[2]


def both_routes(ctx, case, simplified, avoid):
    """the host route's result, after asserting that the tensor route gives the same bytes and that the forced kernel ran"""
    import torch
    from moleculekit_amd.dssp import dssp, dssp_trajectory
    coords, rest = case[0], case[1:]
    ctx.set_dssp_plan(avoid)
    try:
        host = dssp(coords, *rest, simplified=simplified, ctx=ctx)
        k_host = ctx.last_dist_kernel()
        dev = dssp_trajectory(torch.as_tensor(coords).cuda(), *rest, simplified=simplified, ctx=ctx)
        torch.cuda.synchronize()
        k_dev = ctx.last_dist_kernel()
    finally:
        ctx.set_dssp_plan(0)
    if avoid & 3:
        assert KERNELS[avoid & 3] in k_host and KERNELS[avoid & 3] in k_dev, (k_host, k_dev)
    assert dev.dtype == torch.uint8 and np.array_equal(dev.cpu().numpy(), host), "tensor route and host route differ"
    return host


@pytest.mark.parametrize("avoid", [1, 2, 1 | 4, 2 | 4])
def test_every_case_equals_the_restatement(ctx, cases, avoid):
    for name, case in cases.items():
        want = R.dssp(*case)[2]
        got = both_routes(ctx, case, False, avoid)
        assert got.shape == want.shape and np.array_equal(got, want), f"{name} (avoid {avoid}): {int((got != want).sum())} codes differ"
        assert np.array_equal(both_routes(ctx, case, True, avoid), R.simplify(want)), name


@pytest.mark.parametrize("frames", [1, 2, 63, 64, 65, 130])
def test_noisy_3ptb_frame_counts_under_each_plan(ctx, noisy, frames):
    case, want = noisy
    sub = (np.ascontiguousarray(case[0][:, :, :frames]),) + case[1:]
    for avoid in (0, 1, 2, 2 | 4):
        got = both_routes(ctx, sub, False, avoid)
        assert np.array_equal(got, want[:frames]), f"{frames} frames (avoid {avoid}): {int((got != want[:frames]).sum())} codes differ"
        if avoid == 0:
            assert "k_dssp_energy_atoms" in ctx.last_dist_kernel()                       # (223 x 130 < 32 768)


def test_plan_switches_at_the_measured_product(ctx, cases):
    """frames x residues < 32 768: lanes along acceptors; from there on lanes along frames -- the same bytes on both sides"""
    coords, *rest = cases["hairpin"]                                                  # 16 residues
    want = R.dssp(coords, *rest)[2][0]
    for frames, name in ((2047, "k_dssp_energy_atoms"), (2048, "k_dssp_energy_frames")):
        got = both_routes(ctx, (np.ascontiguousarray(np.repeat(coords, frames, axis=2)),) + tuple(rest), False, 0)
        assert name in ctx.last_dist_kernel(), (frames, ctx.last_dist_kernel())
        assert got.shape == (frames, 16) and np.all(got == want[None])


def test_host_route_packed_and_whole_array_uploads(ctx, noisy):
    """The host route uploads only the rows of the 4 R backbone atoms when those are at most a quarter of a > 1-MB array
    (csrc/host_pack.h): the 892 backbone atoms of 3PTB scattered, unsorted, over 6 000 atoms x 130 frames (9.4 MB) -- packed
    (mask 0) and with the whole array uploaded (Context.set_dist_kernels(32)), the restatement's bytes both times."""
    from moleculekit_amd.dssp import dssp
    (coords, ca, nco, pro, chain), want = noisy
    rng = np.random.default_rng(41)
    where = rng.permutation(6000)[:coords.shape[0]]
    big = rng.normal(0, 20, (6000, 3, coords.shape[2])).astype(np.float32)
    big[where] = coords
    assert coords.shape[0] * 4 <= 6000 and big.nbytes > (1 << 20) and np.any(np.diff(where[ca]) < 0)
    for mask in (0, 32):
        ctx.set_dist_kernels(mask)
        try:
            got = dssp(big, where[ca], where[nco], pro, chain, simplified=False, ctx=ctx)
        finally:
            ctx.set_dist_kernels(0)
        assert np.array_equal(got, want), (mask, int((got != want).sum()))


def test_two_runs_give_identical_bytes(ctx, noisy):
    import torch
    from moleculekit_amd.dssp import dssp_trajectory
    case, want = noisy
    d = torch.as_tensor(case[0]).cuda()
    for avoid in (1, 2):
        ctx.set_dssp_plan(avoid)
        try:
            a = dssp_trajectory(d, *case[1:], simplified=False, ctx=ctx)
            b = dssp_trajectory(d, *case[1:], simplified=False, ctx=ctx)
        finally:
            ctx.set_dssp_plan(0)
        assert torch.equal(a, b) and np.array_equal(a.cpu().numpy(), want)


def test_known_answers_through_the_projection(ctx):
    from moleculekit_amd.dssp import MetricSecondaryStructure
    g = np.load(C.GOLDEN)
    for structure, key, sel in (("2hbb", "expected_2hbb", "all"), ("2hbb", "expected_2hbb_5_49", (5, 49)), ("3ptb", "expected_3ptb", "all")):
        (coords, *_), f = C.golden_case(structure)
        mol = types.SimpleNamespace(coords=coords, numFrames=1, **f)
        if sel != "all":
            sel = (f["resid"] >= sel[0]) & (f["resid"] <= sel[1])
        got = MetricSecondaryStructure(sel).project(mol, ctx=ctx)
        assert got.dtype == np.int32 and np.array_equal(got, g[key]), f"{key}: {int((got != g[key]).sum())} labels differ"
    full = MetricSecondaryStructure(simplified=False).project(mol, ctx=ctx)
    text = MetricSecondaryStructure(simplified=False, integer=False).project(mol, ctx=ctx)
    assert np.array_equal(R.simplify(full), g["expected_3ptb"]) and np.array_equal(text == "E", full == R.E)
    assert MetricSecondaryStructure().getMapping(mol)["type"].__len__() == 223


def test_non_contiguous_and_empty_tensors(ctx, cases):
    import torch
    from moleculekit_amd.dssp import dssp_trajectory
    coords, *rest = cases["helix_noise_frames"]
    want = R.dssp(coords, *rest)[2]
    t = torch.as_tensor(np.ascontiguousarray(coords.transpose(2, 1, 0))).cuda().permute(2, 1, 0)      # [N, 3, F], frame-major in memory
    assert not t.is_contiguous()
    assert np.array_equal(dssp_trajectory(t, *rest, simplified=False, ctx=ctx).cpu().numpy(), want)
    assert np.array_equal(dssp_trajectory(t[:, :, 0], *rest, simplified=False, ctx=ctx).cpu().numpy(), want[:1])
    assert dssp_trajectory(t[:, :, :0], *rest, ctx=ctx).shape == (0, 16)
    assert dssp_trajectory(t, rest[0][:0], rest[1][:0], rest[2][:0], rest[3][:0], ctx=ctx).shape == (66, 0)
    with pytest.raises(ValueError, match="float32"):
        dssp_trajectory(t.double(), *rest, ctx=ctx)


def test_library_refusals(ctx, cases):
    from moleculekit_amd import _lib
    L = _lib.load()
    coords, ca, nco, pro, chain = cases["alpha_7"]
    ca, nco = ca.astype(np.uint32), nco.astype(np.uint32)
    out = np.zeros((1, 7), np.uint8)
    p = _lib._ptr

    def call(coords_p=p(coords), N=28, F=1, ca_p=p(ca), R_=7, out_p=p(out)):
        return L.mkamd_dssp_host(ctx._h, coords_p, N, F, ca_p, p(nco), p(pro), p(chain), R_, 0, out_p)

    assert call() == 0
    for kw, msg in ((dict(N=5), "out of range"), (dict(coords_p=None), "NULL"), (dict(out_p=None), "NULL"), (dict(F=-1), "negative"),
                    (dict(R_=(1 << 18) + 1), "too many residues"), (dict(F=1 << 30), "too many frames")):
        assert call(**kw) != 0
        with pytest.raises(Exception, match=msg):
            _lib._check(call(**kw))
    with pytest.raises(Exception, match="dssp plan"):
        ctx.set_dssp_plan(3)
    assert call() == 0                                                                # the context stays usable
