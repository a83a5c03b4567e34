"""GPU tier of the shell densities (moleculekit_amd/shell.py): the device's counts EQUAL to the numpy restatement of the reference's
histogram (tests/shell_restatement.py), MetricShell EQUAL to the array the reference holds for its own test (the reference asserts
allclose; counts are integers and the nearest of the 498 600 distances is 1.6e-4 Angstrom from a shell edge), the reference's small
three-atom test at its literals.  Reads nothing of the reference: tests/golden only."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shell_cases as C  # noqa: E402
import shell_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
EDGES = R.edges_and_volumes(4, 3)[0]


@pytest.fixture(scope="module")
def S():
    from moleculekit_amd import shell
    return shell


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx():
    from moleculekit_amd import _lib
    c = _lib.default_context(0)
    yield c
    c.set_dist_kernels(0)


def device_counts(S, torch, ctx, coords, box, sel1, sel2, chains, edges, force=0, **kw):
    """the tensor route; force: 256 not the frame-lane kernel, 512 not the atom-lane kernel"""
    ctx.set_dist_kernels(force)
    try:
        got = S.shell_counts_trajectory(torch.as_tensor(coords, device="cuda"), torch.as_tensor(box, device="cuda"), sel1, sel2, chains, edges,
                                        ctx=ctx, **kw)
        torch.cuda.synchronize()
        name = ctx.last_dist_kernel()
    finally:
        ctx.set_dist_kernels(0)
    if force:
        assert ("k_shell_atoms" if force == 256 else "k_shell_frames") in name, name
    return got.cpu().numpy()


def check(S, torch, ctx, coords, box, sel1, sel2, chains, edges, dist=R.oracle_dist, **kw):
    want = R.counts(dist, coords, box, sel1, sel2, chains, edges, **kw)
    for force in (0, 256, 512):
        got = device_counts(S, torch, ctx, coords, box, sel1, sel2, chains, edges, force=force, **kw)
        assert got.dtype == np.int32 and np.array_equal(got, want), f"force {force}: {int((got != want).sum())} of {want.size} counts differ"
    return want


@pytest.fixture(scope="module")
def real():
    mol, g = C.fixture()
    chains = C.selection_chains(4507, g["mol_heavy"])
    return mol, g, chains, R.counts(R.oracle_dist, mol.coords, mol.box, g["ca"], g["mol_heavy"], chains, EDGES)


def test_real_trajectory_counts_equal_the_restatement(S, torch, ctx, real):
    mol, g, chains, counts = real
    assert np.array_equal(check(S, torch, ctx, mol.coords, mol.box, g["ca"], g["mol_heavy"], chains, EDGES), counts)
    # the restatement on the device's own distances: the same counts
    assert np.array_equal(R.counts(R.gpu_dist, mol.coords, mol.box, g["ca"], g["mol_heavy"], chains, EDGES), counts)


def test_metricshell_equals_the_reference_held_array(S, real):
    mol, g, _, _ = real
    ca = np.zeros(4507, bool)
    ca[g["ca"]] = True
    got = S.MetricShell(ca, g["mol_heavy"], periodic="selections").project(mol)
    assert got.dtype == np.float64 and got.shape == (200, 1108)
    assert np.array_equal(got, g["refdata"])


def test_metricshell_simple(S):
    """the reference's test_metricshell_simple: three atoms, both parameter sets, allclose to its literals"""
    coords = np.zeros((3, 3, 1), F32)
    coords[1, :, 0] = [0.5, 0, 0]
    coords[2, :, 0] = [0, 1.5, 0]
    mol = types.SimpleNamespace(coords=coords, box=None, name=np.array(["CL"] * 3), resname=np.array(["CL"] * 3), resid=np.arange(3))
    got = S.MetricShell("all", "all", periodic=None).project(mol)
    assert np.allclose(got, [[0.01768388256576615, 0, 0, 0, 0.01768388256576615, 0, 0, 0, 0.01768388256576615, 0, 0, 0]])
    got = S.MetricShell("all", "all", numshells=2, shellwidth=1, periodic=None).project(mol)
    assert np.allclose(got, [[0.23873241, 0.03410463, 0.23873241, 0.03410463, 0.0, 0.06820926]])


@pytest.mark.parametrize("F", [1, 3, 70])
@pytest.mark.parametrize("n2", [1, 63, 1000])
@pytest.mark.parametrize("n1", [1, 7, 64, 300])
def test_random_periodic_boxes(S, torch, ctx, n1, n2, F):
    coords, box, sel1, sel2, chains = C.random_case(n1, n2, F, seed=1000 * n1 + 10 * n2 + F)
    check(S, torch, ctx, coords, box, sel1, sel2, chains, EDGES)


@pytest.mark.parametrize("n1,n2,F", [(300, 5000, 200), (1, 20000, 1)])
def test_large_shapes(S, torch, ctx, n1, n2, F):
    coords, box, sel1, sel2, chains = C.random_case(n1, n2, F, seed=n1 + n2 + F, box_len=60.0)
    want = R.counts(R.gpu_dist, coords, box, sel1, sel2, chains, EDGES)
    assert want.sum() > 0
    for force in ((0,) if n1 * n2 * F > 10 ** 8 else (0, 256, 512)):
        assert np.array_equal(device_counts(S, torch, ctx, coords, box, sel1, sel2, chains, EDGES, force=force), want)
    if F == 1:
        assert np.array_equal(R.counts(R.oracle_dist, coords, box, sel1, sel2, chains, EDGES), want)


@pytest.mark.parametrize("mode", ["selections", "chains"])
def test_symmetric(S, torch, ctx, mode):
    coords, box = C.random_system(90, 5, seed=11, box_len=20.0)
    sel = np.sort(np.random.default_rng(3).permutation(90)[:70]).astype(U32)
    chains = C.selection_chains(90, sel) if mode == "selections" else np.random.default_rng(4).integers(0, 3, 90).astype(U32)
    want = check(S, torch, ctx, coords, box, sel, sel, chains, EDGES, symmetric=True)
    assert want.sum() > 0 and np.array_equal(check(S, torch, ctx, coords, box, sel, sel, chains, EDGES), want)


def test_three_chains(S, torch, ctx):
    coords, box, sel1, sel2, _ = C.random_case(40, 200, 6, seed=21, box_len=18.0)
    chains = np.random.default_rng(22).integers(0, 3, coords.shape[0]).astype(U32)
    check(S, torch, ctx, coords, box, sel1, sel2, chains, EDGES)
    check(S, torch, ctx, coords, box, sel1, sel2, chains, EDGES, pbc=False)


@pytest.mark.parametrize("truncate", [7.5, 7.3, 6, 100.0])
def test_truncate(S, torch, ctx, truncate):
    coords, box, sel1, sel2, chains = C.random_case(20, 150, 4, seed=31, box_len=40.0)
    check(S, torch, ctx, coords, box, sel1, sel2, chains, EDGES, truncate=truncate)


@pytest.mark.parametrize("numshells,shellwidth", [(4, 0.7), (1, 3), (32, 1), (32, 0.7), (9, 2), (17, 1.1)])
def test_shell_numbers_and_float_widths(S, torch, ctx, numshells, shellwidth):
    coords, box, sel1, sel2, chains = C.random_case(9, 400, 3, seed=41, box_len=14.0)
    check(S, torch, ctx, coords, box, sel1, sel2, chains, R.edges_and_volumes(numshells, shellwidth)[0])
    coords, box, sel1, sel2, chains = C.random_case(9, 400, 70, seed=42, box_len=14.0)
    check(S, torch, ctx, coords, box, sel1, sel2, chains, R.edges_and_volumes(numshells, shellwidth)[0])


def test_overlapping_duplicate_nan_and_zero_box(S, torch, ctx):
    coords, box = C.random_system(120, 4, seed=51, box_len=16.0)
    sel1, sel2 = np.arange(0, 80, dtype=U32), np.arange(40, 120, dtype=U32)
    check(S, torch, ctx, coords, box, sel1, sel2, C.selection_chains(120, sel2), EDGES)
    dup1, dup2 = np.array([5, 5, 7, 5, 90], U32), np.array([3, 3, 3, 50, 51, 50, 5], U32)
    check(S, torch, ctx, coords, box, dup1, dup2, C.selection_chains(120, dup2), EDGES)
    bad = coords.copy()
    bad[sel2[3], 1, 1] = np.nan
    bad[sel1[2], 0, 2] = np.nan
    check(S, torch, ctx, bad, box, sel1, sel2, C.selection_chains(120, sel2), EDGES)
    check(S, torch, ctx, bad, box, sel1, sel2, C.selection_chains(120, sel2), EDGES, truncate=7.5)
    assert check(S, torch, ctx, coords, np.zeros_like(box), np.arange(0, 40, dtype=U32), sel2, C.selection_chains(120, sel2), EDGES).sum() == 0


def test_exact_edges_and_one_ulp_either_side(S, torch, ctx):
    coords, box, sel1, sel2, chains = C.edge_case()
    for pbc in (False, True):
        want = check(S, torch, ctx, coords, box, sel1, sel2, chains, EDGES, pbc=pbc)
        assert want.sum() > 0


def test_tensor_host_and_projection_routes_agree(S, torch, ctx, real):
    mol, g, chains, counts = real
    host = S.shell_counts(mol.coords, mol.box, g["ca"], g["mol_heavy"], chains, EDGES)
    dev = device_counts(S, torch, ctx, mol.coords, mol.box, g["ca"], g["mol_heavy"], chains, EDGES)
    proj = S.MetricShell(g["ca"], g["mol_heavy"], periodic="selections").project(mol)
    assert np.array_equal(host, counts) and np.array_equal(dev, counts)
    assert np.array_equal(proj, R.density(counts, R.edges_and_volumes(4, 3)[1]))
    # the host call without packing the selected rows: the same
    ctx.set_dist_kernels(32)
    try:
        assert np.array_equal(S.shell_counts(mol.coords, mol.box, g["ca"], g["mol_heavy"], chains, EDGES, ctx=ctx), counts)
    finally:
        ctx.set_dist_kernels(0)


def test_two_runs_are_equal_and_a_batch_equals_frame_by_frame(S, torch, ctx):
    coords, box, sel1, sel2, chains = C.random_case(64, 1000, 70, seed=91)
    a = device_counts(S, torch, ctx, coords, box, sel1, sel2, chains, EDGES)
    b = device_counts(S, torch, ctx, coords, box, sel1, sel2, chains, EDGES)
    assert np.array_equal(a, b)
    for f in (0, 1, 33, 69):
        one = device_counts(S, torch, ctx, np.ascontiguousarray(coords[:, :, f:f + 1]), np.ascontiguousarray(box[:, f:f + 1]), sel1, sel2, chains, EDGES)
        assert np.array_equal(one[0], a[f])


def test_out_and_a_non_default_stream(S, torch, ctx):
    coords, box, sel1, sel2, chains = C.random_case(7, 300, 5, seed=92)
    want = R.counts(R.oracle_dist, coords, box, sel1, sel2, chains, EDGES)
    dc, db = torch.as_tensor(coords, device="cuda"), torch.as_tensor(box, device="cuda")
    out = torch.full((5, 7, 4), -3, dtype=torch.int32, device="cuda")
    assert S.shell_counts_trajectory(dc, db, sel1, sel2, chains, EDGES, out=out, ctx=ctx) is out
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    with pytest.raises(ValueError, match="out must be"):
        S.shell_counts_trajectory(dc, db, sel1, sel2, chains, EDGES, out=out[:, :, :3], ctx=ctx)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    got = S.shell_counts_trajectory(dc, db, sel1, sel2, chains, EDGES, stream=stream.cuda_stream, ctx=ctx)
    stream.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


def test_context_is_usable_after_einval(S, torch, ctx):
    from moleculekit_amd import _lib
    coords, box, sel1, sel2, chains = C.random_case(7, 300, 5, seed=93)
    d = [torch.as_tensor(a.view(np.int32) if a.dtype == U32 else a, device="cuda") for a in (coords, box, sel1, sel2, chains)]
    out = torch.zeros((5, 7, 33), dtype=torch.int32, device="cuda")
    thr, down, good = np.zeros(35, F32), np.array([0, 4, 1], F32), S.shell_thresholds(EDGES)       # (named: alive during the calls)
    with pytest.raises(ValueError, match="numshells"):
        _lib._check(_lib.load().mkamd_shell_counts_dev(ctx._h, d[0].data_ptr(), coords.shape[0], 5, d[1].data_ptr(), d[2].data_ptr(), 7, d[3].data_ptr(),
                                                       300, d[4].data_ptr(), 0, 1, _lib._ptr(thr), 34, out.data_ptr()))
    with pytest.raises(ValueError, match="non-decreasing"):
        _lib._check(_lib.load().mkamd_shell_counts_dev(ctx._h, d[0].data_ptr(), coords.shape[0], 5, d[1].data_ptr(), d[2].data_ptr(), 7, d[3].data_ptr(),
                                                       300, d[4].data_ptr(), 0, 1, _lib._ptr(down), 3, out.data_ptr()))
    with pytest.raises(ValueError, match="out of range"):
        far, res = np.array([9999], U32), np.zeros((5, 1, 4), np.int32)
        _lib._check(_lib.load().mkamd_shell_counts_host(ctx._h, _lib._ptr(coords), coords.shape[0], 5, _lib._ptr(box), _lib._ptr(far), 1, _lib._ptr(sel2),
                                                        300, _lib._ptr(chains), 0, 1, _lib._ptr(good), 5, _lib._ptr(res)))
    want = R.counts(R.oracle_dist, coords, box, sel1, sel2, chains, EDGES)
    assert np.array_equal(device_counts(S, torch, ctx, coords, box, sel1, sel2, chains, EDGES), want)
