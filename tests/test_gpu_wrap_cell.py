"""GPU tier of the periodic wrap of triclinic boxes (moleculekit_amd/wrap.py, csrc/wrap_cell_kernels.h).  Reads
tests/golden only.

The cases of tests/wrap_cell_cases.py -- without those on which the reference's own loops would not end within a few steps: the cap is
exercised on the host -- run through ``wrap_cell_trajectory`` in all three unit cells under every launch plan the pipeline can be
steered to (``ctx.set_dist_kernels``: 16384 no lane-per-group kernel, 32768 no wave-per-group kernel), in place and out of place, and
through the host entry ``wrap_cell`` with and without ``rows``.  Everything is bit-equal to the restatement of the reference
(tests/wrap_cell_restatement.py, itself pinned to the compiled reference by tests/test_wrap_cell_cpu.py; NaNs by position)."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wrap_cell_cases as C  # noqa: E402
import wrap_cell_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

PLANS = {"default": (0, "k_wrap_cell_lanes + mkamd::k_wrap_cell_waves"), "waves_only": (16384, "k_wrap_cell_prep + mkamd::k_wrap_cell_waves"),
         "lanes_only": (32768, "k_wrap_cell_lanes")}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from moleculekit_amd import _lib, wrap

    ctx = _lib.Context(0)
    yield type("G", (), dict(torch=torch, ctx=ctx, W=wrap, lib=_lib, dev=torch.device("cuda", 0)))
    ctx.set_dist_kernels(0)
    ctx.close()


def _bits(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("name", C.device_cases())
def test_cases_under_every_launch_plan(gpu, name, plan):
    avoid, kernels = PLANS[plan]
    c = C.cases()[name]
    gpu.ctx.set_dist_kernels(avoid)
    d = gpu.torch.as_tensor(c.xyz.copy(), device=gpu.dev)
    d_bv = gpu.torch.as_tensor(c.boxvectors.copy(), device=gpu.dev)
    for mode in R.MODES:
        want, want_status = C.expected(name, mode)
        assert not want_status.any()
        got = gpu.W.wrap_cell_trajectory(d, c.boxvectors, c.starts, mode, centersel=c.centersel, center=c.center, ctx=gpu.ctx)
        launched = gpu.ctx.last_dist_kernel()
        if plan != "default" or np.diff(c.starts.astype(np.int64)).max() > C.SMALL_MAX:
            assert kernels in launched, launched
        assert "k_wrap_cell_prep" in launched
        assert ("k_wrap_centre" in launched) == (c.centersel is not None and len(c.centersel) > 0)
        assert got.data_ptr() != d.data_ptr()
        assert np.array_equal(_bits(d).view(np.uint32), c.xyz.view(np.uint32)), "out of place leaves the input untouched"
        C.assert_same_bits(_bits(got), want, f"{name} / {mode} / {plan}, out of place")
        given = gpu.torch.full_like(d, -7.0)
        assert gpu.W.wrap_cell_trajectory(d, d_bv, c.starts, mode, centersel=c.centersel, center=c.center, out=given, ctx=gpu.ctx) is given
        C.assert_same_bits(_bits(given), want, f"{name} / {mode} / {plan}, into a given tensor, box vectors on the device")
        work = d.clone()
        assert gpu.W.wrap_cell_trajectory(work, c.boxvectors, c.starts, mode, centersel=c.centersel, center=c.center, out=work, ctx=gpu.ctx) is work
        C.assert_same_bits(_bits(work), want, f"{name} / {mode} / {plan}, in place")
    gpu.ctx.set_dist_kernels(0)


def test_unchecked_calls_return_a_zero_status_on_clean_input(gpu):
    c = C.cases()["octa_frames_65"]
    d = gpu.torch.as_tensor(c.xyz.copy(), device=gpu.dev)
    stream = gpu.torch.cuda.Stream(device=gpu.dev)
    gpu.torch.cuda.synchronize()
    for mode in R.MODES:
        got, status = gpu.W.wrap_cell_trajectory(d, c.boxvectors, c.starts, mode, centersel=c.centersel, ctx=gpu.ctx, check=False)
        assert status.dtype == gpu.torch.int32 and tuple(status.shape) == (3,) and status.is_cuda
        gpu.ctx.synchronize()
        assert _bits(status).tolist() == [0, 0, 0] and gpu.W.status_error(_bits(status)) is None
        C.assert_same_bits(_bits(got), C.expected("octa_frames_65", mode)[0], f"{mode}, unchecked")
    got, status = gpu.W.wrap_cell_trajectory(d, c.boxvectors, c.starts, "compact", centersel=c.centersel, stream=stream.cuda_stream, ctx=gpu.ctx,
                                             check=False)
    stream.synchronize()
    assert _bits(status).tolist() == [0, 0, 0]
    C.assert_same_bits(_bits(got), C.expected("octa_frames_65", "compact")[0], "on a foreign stream")


@pytest.mark.parametrize("name", ["dodeca_sel_inside_moving", "octa_frames_64", "ortho_center", "nan"])
def test_host_entry_with_and_without_rows(gpu, name):
    c = C.cases()[name]
    gpu.ctx.set_dist_kernels(0)
    coords = R.from_frame_major(c.xyz)
    before = coords.copy()
    starts = c.starts.astype(np.int64)
    rng = np.random.default_rng(3)
    named = rng.permutation(np.unique(np.r_[starts[:-1][::2], starts[1:][::3] - 1, rng.integers(0, starts[-1], 5)]))
    mask = np.zeros(coords.shape[0], bool)
    mask[named] = True
    for mode in R.MODES:
        want = R.from_frame_major(C.expected(name, mode)[0])
        got = gpu.W.wrap_cell(coords, c.boxvectors, c.starts, mode, centersel=c.centersel, center=c.center, ctx=gpu.ctx)
        assert np.array_equal(coords.view(np.uint32), before.view(np.uint32))
        C.assert_same_bits(got, want, f"{name} / {mode}: host entry, every row")
        # rows: a few atoms out of groups of every kind; what comes back is their rows, in the order given
        sub = gpu.W.wrap_cell(coords, c.boxvectors, c.starts, mode, centersel=c.centersel, center=c.center, rows=named, ctx=gpu.ctx)
        assert sub.shape == (named.size, 3, coords.shape[2])
        C.assert_same_bits(sub, np.ascontiguousarray(want[named]), f"{name} / {mode}: host entry, rows")
        C.assert_same_bits(gpu.W.wrap_cell(coords, c.boxvectors, c.starts, mode, centersel=c.centersel, center=c.center, rows=mask, ctx=gpu.ctx),
                           np.ascontiguousarray(want[mask]), f"{name} / {mode}: host entry, a mask of rows")


def test_bonds_instead_of_starts(gpu):
    c = C.cases()["octa_frames_2"]
    s = c.starts.astype(np.int64)
    bonds = np.concatenate([np.stack([np.arange(a, b - 1), np.arange(a + 1, b)], axis=1) for a, b in zip(s[:-1], s[1:])])
    got = gpu.W.wrap_cell(R.from_frame_major(c.xyz), c.boxvectors, bonds, "compact", centersel=c.centersel, ctx=gpu.ctx)
    C.assert_same_bits(got, R.from_frame_major(C.expected("octa_frames_2", "compact")[0]), "groups from bonds")


@pytest.mark.parametrize("unitcell", R.MODES)
def test_wrap_molecule_on_a_triclinic_box(gpu, unitcell):
    """Molecule.wrap's semantics on a molecule-like object: lengths and angles -> box vectors, bonds -> groups, in place on mol.coords"""
    lengths, angles = C.BOXES["skew"]
    sizes = (1, 2, 3, 17, 65, 300)
    s = C.starts_of(sizes).astype(np.int64)
    N, F = int(s[-1]), 3
    rng = np.random.default_rng(21)
    box = (np.array(lengths)[:, None] * (1 + 0.01 * rng.uniform(-1, 1, F))[None]).astype(np.float32)
    boxangles = np.repeat(np.array(angles, np.float32)[:, None], F, axis=1)
    boxangles[:, 1] = 90                                                                    # a frame of 90 degrees among the others
    coords = rng.normal(0, 120, (N, 3, F)).astype(np.float32)
    left = np.setdiff1d(np.arange(N - 1), s[1:-1] - 1)                                      # a chain of bonds along every group
    mol = types.SimpleNamespace(coords=coords.copy(), box=box, boxangles=boxangles, bonds=np.stack([left, left + 1], axis=1).astype(np.uint32))
    sel = np.arange(int(s[5]), int(s[5]) + 40)
    bv = gpu.W.box_vectors(box, boxangles)
    assert bv[1, 0, 1] == 0 and bv[1, 0, 0] != 0
    want, status = R.wrap_cell(coords, bv, s, unitcell, sel, None)
    assert not status.any()
    held = mol.coords
    with pytest.raises(NotImplementedError):
        gpu.W.wrap_molecule(mol, sel, unitcell=unitcell, ctx=gpu.ctx)
    gpu.W.wrap_molecule(mol, sel, unitcell=unitcell, ctx=gpu.ctx, triclinic_on_device=True)
    assert mol.coords is held
    C.assert_same_bits(mol.coords, want, f"wrap_molecule / {unitcell}")


def test_the_library_refuses_bad_calls(gpu):
    c = C.cases()["octa_frames_2"]
    coords = R.from_frame_major(c.xyz)
    N, _, F = coords.shape
    out = np.zeros_like(coords)
    L, p = gpu.lib.load(), gpu.lib._ptr
    sel = np.array([1, 2], np.uint32)
    cen = np.zeros(3, np.float32)
    assert int(L.mkamd_wrap_cell_max_steps()) == gpu.W.WRAP_CELL_MAX_STEPS

    def host(coords_=coords, bv=c.boxvectors, rows=None, starts=c.starts, sel_=sel, n_c=2, cen_=None, mode=1, out_=out, n=N):
        bv = None if bv is None else np.ascontiguousarray(bv)
        gpu.lib._check(L.mkamd_wrap_cell_host(gpu.ctx._h, p(coords_), n, F, p(bv), p(rows), 0 if rows is None else rows.size, p(starts),
                                              starts.size - 1, p(sel_), n_c, p(cen_), mode, p(out_)))

    host()
    C.assert_same_bits(out, R.wrap_cell(coords, c.boxvectors, c.starts, "compact", sel, None)[0], "the raw host entry")
    for mode in (3, -1):
        with pytest.raises(ValueError, match="mode must be 0"):
            host(mode=mode)
    for (i, j), value, text in (((2, 2), 0.0, "must be positive"), ((1, 1), -5.0, "must be positive"), ((2, 1), np.nan, "not finite"),
                                ((0, 0), np.inf, "not finite"), ((1, 2), 1.0, "not lower triangular")):
        bad = c.boxvectors.copy()
        bad[i, j, 1] = value
        with pytest.raises(ValueError, match=text):                                         # refused before anything is launched
            host(bv=bad)
    with pytest.raises(ValueError, match="NULL pointer"):
        host(bv=None)
    with pytest.raises(ValueError, match="NULL pointer"):
        host(sel_=None, n_c=0, cen_=None)
    with pytest.raises(ValueError, match="NULL pointer"):
        host(out_=None)
    with pytest.raises(ValueError, match="must increase"):
        host(starts=np.r_[c.starts[:3], c.starts[2:]].astype(np.uint32))
    with pytest.raises(ValueError, match="centersel: atom index out of range"):
        host(sel_=np.array([1, N], np.uint32))
    with pytest.raises(ValueError, match="not among the rows"):
        host(rows=np.array([0, 5, 6], np.uint32), starts=np.array([0, 1, 3], np.uint32), out_=np.zeros((3, 3, F), np.float32))
    d = gpu.torch.as_tensor(c.xyz.copy(), device=gpu.dev)
    d_bv = gpu.torch.as_tensor(c.boxvectors.copy(), device=gpu.dev)
    status = gpu.torch.zeros(3, dtype=gpu.torch.int32, device=gpu.dev)
    with pytest.raises(ValueError, match="mode must be 0"):                                 # the device form, past the wrapper
        gpu.lib._check(L.mkamd_wrap_cell_dev(gpu.ctx._h, d.data_ptr(), N, F, d_bv.data_ptr(), None, 1, None, 0, None, 0, p(cen), 3, d.data_ptr(),
                                             status.data_ptr()))
    with pytest.raises(ValueError, match="NULL pointer"):
        gpu.lib._check(L.mkamd_wrap_cell_dev(gpu.ctx._h, d.data_ptr(), N, F, None, None, 1, None, 0, None, 0, p(cen), 2, d.data_ptr(), None))
    with pytest.raises(ValueError, match="neither a centre selection nor a centre"):
        gpu.lib._check(L.mkamd_wrap_cell_dev(gpu.ctx._h, d.data_ptr(), N, F, d_bv.data_ptr(), None, 1, None, 0, None, 0, None, 2, d.data_ptr(), None))
    with pytest.raises(ValueError, match="boxvectors must be float64"):
        gpu.W.wrap_cell_trajectory(d, d_bv.float(), c.starts, "compact", center=[0, 0, 0], ctx=gpu.ctx)
    with pytest.raises(ValueError, match="must be positive"):
        bad = c.boxvectors.copy()
        bad[2, 2, 0] = 0.0
        gpu.W.wrap_cell_trajectory(d, gpu.torch.as_tensor(bad, device=gpu.dev), c.starts, "compact", center=[0, 0, 0], ctx=gpu.ctx)
    with pytest.raises(ValueError, match="shares xyz's memory"):
        gpu.W.wrap_cell_trajectory(d, c.boxvectors, c.starts, "compact", center=[0, 0, 0], out=d.view(d.shape), ctx=gpu.ctx)
    gpu.ctx.synchronize()
    assert np.array_equal(_bits(d).view(np.uint32), c.xyz.view(np.uint32)) and _bits(status).tolist() == [0, 0, 0]
