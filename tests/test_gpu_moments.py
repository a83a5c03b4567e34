"""GPU tier of the group moments (moleculekit_amd/moments.py).  Reads tests/golden only.

Every kernel form is forced through the avoid bits of ``ctx.set_dist_kernels`` (4096: not the form in which a lane group owns a
(frame, group); 8192: not the segmented form) and asserted through ``ctx.last_dist_kernel()``; both routes run (CUDA tensors, host
arrays) and must give the same bits.  The conditions are derived, not measured (tests/moments_cases.py): ``center``, ``gyration`` and
``spherical`` at most one float32 ulp from float32(restatement) -- the restatement fed the bits of ``align.apply_transforms`` where an
affine is involved --, ``fluct`` within (F + group size + 8) 2^-52 max|x|^2, NaN exactly where the restatement has NaN, two runs of
the same call bit-equal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import moments_cases as C  # noqa: E402
import moments_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

FORMS = {"owned": (8192, "false>"), "segmented": (4096, "k_mom_fold")}


@pytest.fixture(scope="module")
def gpu():
    import torch
    from moleculekit_amd import _lib, align, moments

    ctx = _lib.Context(0)
    yield type("G", (), dict(torch=torch, ctx=ctx, M=moments, align=align, dev=torch.device("cuda", 0)))
    ctx.set_dist_kernels(0)
    ctx.close()


@pytest.fixture(scope="module")
def cases(gpu):
    out = {}
    for name in C.CASES:
        c = C.case(name)
        c.d_xyz = gpu.torch.as_tensor(c.xyz, device=gpu.dev)
        c.coords = np.ascontiguousarray(c.xyz.transpose(1, 2, 0))                       # Molecule.coords [N, 3, F]
        c.d_affine = gpu.torch.as_tensor(c.affine, device=gpu.dev) if c.affine is not None else None
        # what the restatement is fed: the bits align.apply_transforms stores
        c.moved = gpu.align.apply_transforms(c.d_xyz, c.d_affine, ctx=gpu.ctx).cpu().numpy() if c.affine is not None else c.xyz
        out[name] = c
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", C.CASES)
def test_center_and_gyration(gpu, cases, name, form):
    c = cases[name]
    avoid, tag = FORMS[form]
    gpu.ctx.set_dist_kernels(avoid)
    for out, restate in (("center", R.center), ("gyration", R.gyration)):
        got = gpu.M.group_moments_trajectory(c.d_xyz, c.groups, weights=c.weights, affine=c.d_affine, out=out, ctx=gpu.ctx).cpu().numpy()
        assert tag in gpu.ctx.last_dist_kernel() and f"k_mom_sums<{gpu.M.MODES[out]}," in gpu.ctx.last_dist_kernel()
        C.assert_one_ulp(got, restate(c.moved, c.groups, c.weights), f"{name} {out} {form}")
        again = gpu.M.group_moments_trajectory(c.d_xyz, c.groups, weights=c.weights, affine=c.d_affine, out=out, ctx=gpu.ctx).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(again)), f"{name} {out} {form}: two runs differ"
        if c.affine is None:                                   # the host route takes no ready-made affine: see test_routes_with_alignment
            host = gpu.M.group_moments(c.coords, c.groups, weights=c.weights, out=out, ctx=gpu.ctx)
            assert tag in gpu.ctx.last_dist_kernel()
            assert np.array_equal(_bits(got), _bits(host)), f"{name} {out} {form}: the tensor and the host route differ"


def test_the_large_group_is_segmented_by_the_plan(gpu, cases):
    c = cases["large"]
    gpu.ctx.set_dist_kernels(0)
    got = gpu.M.group_moments_trajectory(c.d_xyz, c.groups, weights=c.weights, out="gyration", ctx=gpu.ctx).cpu().numpy()
    assert "k_mom_fold" in gpu.ctx.last_dist_kernel()
    C.assert_one_ulp(got, R.gyration(c.xyz, c.groups, c.weights), "large gyration")


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name,pair", [("mixed", (5, 8)), ("mixed", (0, 1)), ("three", (0, 1)), ("residues", (3, 200))])
def test_spherical(gpu, cases, name, pair, form):
    c = cases[name]
    avoid, tag = FORMS[form]
    gpu.ctx.set_dist_kernels(avoid)
    groups = [c.groups[pair[0]], c.groups[pair[1]]]
    got = gpu.M.group_moments_trajectory(c.d_xyz, groups, affine=c.d_affine, out="spherical", ctx=gpu.ctx).cpu().numpy()
    assert tag in gpu.ctx.last_dist_kernel() and "k_mom_sums<2," in gpu.ctx.last_dist_kernel()
    C.assert_one_ulp(got, R.spherical(c.moved, *groups), f"{name} spherical {form}")
    if c.affine is None:
        host = gpu.M.group_moments(c.coords, groups, out="spherical", ctx=gpu.ctx)
        assert np.array_equal(_bits(got), _bits(host))


def test_spherical_of_coincident_centroids(gpu, cases):
    c = cases["three"]
    gpu.ctx.set_dist_kernels(0)
    got = gpu.M.group_moments_trajectory(c.d_xyz, [c.groups[1], c.groups[1]], out="spherical", ctx=gpu.ctx).cpu().numpy()
    assert np.all(got[:, 0] == 0) and np.all(np.isnan(got[:, 1]))
    C.assert_one_ulp(got, R.spherical(c.xyz, c.groups[1], c.groups[1]), "coincident spherical")


@pytest.mark.parametrize("given_ref", [False, True])
@pytest.mark.parametrize("name", ["mixed", "one", "three", "residues"])
def test_fluctuation(gpu, cases, name, given_ref):
    c = cases[name]
    atoms = np.concatenate(c.groups)
    offsets = np.r_[0, np.cumsum([g.size for g in c.groups])]
    ref = np.random.default_rng(7).normal(size=(atoms.size, 3)) * 3 + c.moved[0, atoms] if given_ref else None
    xmax = np.abs(c.moved).max()
    gpu.ctx.set_dist_kernels(0)
    got = gpu.M.fluctuation_trajectory(c.d_xyz, atoms, ref=ref, affine=c.d_affine, ctx=gpu.ctx).cpu().numpy()
    assert gpu.ctx.last_dist_kernel() == ("" if given_ref else "mkamd::k_mom_mean + ") + "mkamd::k_mom_fluct_atoms"
    C.assert_fluct(got, R.fluctuation(c.moved, atoms, ref), c.F, 1, xmax, f"{name} fluct atoms")
    if c.affine is None:
        assert np.array_equal(_bits(got), _bits(gpu.M.fluctuation(c.coords, atoms, ref=ref, ctx=gpu.ctx)))
    for form, (avoid, tag) in FORMS.items():
        gpu.ctx.set_dist_kernels(avoid)
        got = gpu.M.fluctuation_trajectory(c.d_xyz, atoms, ref=ref, groups=offsets, affine=c.d_affine, ctx=gpu.ctx).cpu().numpy()
        assert tag in gpu.ctx.last_dist_kernel() and "k_mom_sums<3," in gpu.ctx.last_dist_kernel()
        C.assert_fluct(got, R.fluctuation(c.moved, atoms, ref, offsets), c.F, int(np.diff(offsets).max()), xmax, f"{name} fluct groups {form}")
        again = gpu.M.fluctuation_trajectory(c.d_xyz, atoms, ref=ref, groups=offsets, affine=c.d_affine, ctx=gpu.ctx).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(again))
        if c.affine is None:
            assert np.array_equal(_bits(got), _bits(gpu.M.fluctuation(c.coords, atoms, ref=ref, groups=offsets, ctx=gpu.ctx)))


def test_routes_with_alignment(gpu, cases):
    """the alignment inside the host route (mkamd_align_transforms_dev on the packed rows) and kabsch_transforms + the tensor route give
    the same bits, and both are the restatement of the trajectory align_trajectory writes"""
    c = cases["three"]
    gpu.ctx.set_dist_kernels(0)
    rng = np.random.default_rng(11)
    sel = np.sort(rng.choice(c.N, size=40, replace=False))
    ref = (c.xyz[0, sel] + rng.normal(size=(40, 3))).astype(np.float32)
    d_ref = gpu.torch.as_tensor(ref, device=gpu.dev)
    aff, _ = gpu.align.kabsch_transforms(c.d_xyz, d_ref, sel, np.arange(40), ctx=gpu.ctx)
    moved = gpu.align.apply_transforms(c.d_xyz, aff, ctx=gpu.ctx).cpu().numpy()
    atoms = np.concatenate(c.groups)
    offsets = np.r_[0, np.cumsum([g.size for g in c.groups])]
    for out, restate in (("center", R.center), ("gyration", R.gyration)):
        got = gpu.M.group_moments_trajectory(c.d_xyz, c.groups, weights=c.weights, affine=aff, out=out, ctx=gpu.ctx).cpu().numpy()
        host = gpu.M.group_moments(c.coords, c.groups, weights=c.weights, align=(sel, ref), out=out, ctx=gpu.ctx)
        assert np.array_equal(_bits(got), _bits(host)), out
        C.assert_one_ulp(got, restate(moved, c.groups, c.weights), f"aligned {out}")
    got = gpu.M.fluctuation_trajectory(c.d_xyz, atoms, groups=offsets, affine=aff, ctx=gpu.ctx).cpu().numpy()
    host = gpu.M.fluctuation(c.coords, atoms, groups=offsets, align=(sel, ref), ctx=gpu.ctx)
    assert np.array_equal(_bits(got), _bits(host))
    C.assert_fluct(got, R.fluctuation(moved, atoms, None, offsets), c.F, 64, np.abs(moved).max(), "aligned fluct")


def test_nan_stays_in_its_group(gpu, cases):
    c = cases["three"]
    gpu.ctx.set_dist_kernels(0)
    xyz = c.xyz.copy()
    only = np.setdiff1d(c.groups[0], np.concatenate(c.groups[1:]))[0]
    xyz[5, only, 1] = np.nan
    d = gpu.torch.as_tensor(xyz, device=gpu.dev)
    for out, restate in (("center", R.center), ("gyration", R.gyration)):
        got = gpu.M.group_moments_trajectory(d, c.groups, weights=c.weights, out=out, ctx=gpu.ctx).cpu().numpy()
        with np.errstate(invalid="ignore"):
            C.assert_one_ulp(got, restate(xyz, c.groups, c.weights), f"nan {out}")


def test_the_library_refuses_bad_calls(gpu, cases):
    c = cases["three"]
    with pytest.raises(IndexError, match="out of range"):
        gpu.M.group_moments(c.coords, [[c.N]], ctx=gpu.ctx)
    atoms, offs = np.array([c.N], np.uint32), np.array([0, 1], np.uint32)             # past the wrapper: the library's own check
    out = np.zeros((c.F, 3), np.float32)
    from moleculekit_amd import _lib
    with pytest.raises(ValueError, match="atoms: atom index out of range"):
        _lib._check(_lib.load().mkamd_group_moments_host(gpu.ctx._h, _lib._ptr(c.coords), c.N, c.F, None, None, 0, _lib._ptr(atoms),
                                                         _lib._ptr(offs), None, 1, 0, _lib._ptr(out)))
    with pytest.raises(ValueError, match="exactly two unweighted groups"):
        gpu.M.group_moments_trajectory(c.d_xyz, c.groups, out="spherical", ctx=gpu.ctx)
    with pytest.raises(ValueError, match="affine must be a float64 CUDA tensor"):
        gpu.M.group_moments_trajectory(c.d_xyz, c.groups, affine=gpu.torch.zeros((2, 12), dtype=gpu.torch.float64, device=gpu.dev), ctx=gpu.ctx)


# ------------------------------------------------------------------------------------------------
# the four projection classes on the carried trajectory, against the reference-held arrays and literals (tests/golden/moments_cases.npz)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def held():
    """tests/moments_cases.py::reference_case: the last 20 frames and frame 0 of the trajectory, as decoded and wrapped with the wrap_box
    restatement about the reference's centersel (the classes then run with pbc=False)"""
    return C.reference_case()


def test_projections_raise_with_pbc_and_the_fixtures_box(gpu, held):
    mol, sel = held.raw20, held.sel
    assert np.any(mol.box != 0)
    for metric in (gpu.M.MetricCoordinate(sel["ca"]), gpu.M.MetricGyration(sel["protein"]),
                   gpu.M.MetricFluctuation(sel["ca"], trajalnsel=sel["ca"]),
                   gpu.M.MetricSphericalCoordinate(held.pdb, sel["mol"], sel["within8"], trajalnsel=sel["ca"])):
        with pytest.raises(NotImplementedError, match="pbc=False"):
            metric.project(mol)


def test_metric_gyration_against_the_reference_literals(gpu, held):
    got = gpu.M.MetricGyration(held.sel["protein"], pbc=False).project(held.mol20, ctx=gpu.ctx)
    assert got.dtype == np.float32 and got.shape == (20, 4)
    print("gyration: max |got - literal|", np.abs(got[:, 0] - held.g["gyration_last20"]).max())
    assert np.all(np.abs(got[:, 0] - held.g["gyration_last20"]) < 1e-3)


def test_metric_coordinate_against_the_reference_literals(gpu, held):
    got = gpu.M.MetricCoordinate(held.sel["ca"], pbc=False).project(held.mol20, ctx=gpu.ctx)
    assert got.dtype == np.float32 and got.shape == (20, 3 * 277)
    print("coordinate: max |got - literal|", np.abs(got[-1, -20:] - held.g["coord_last20"]).max())
    assert np.all(np.abs(got[-1, -20:] - held.g["coord_last20"]) < 1e-3)
    # test_project_align: the refmol is frame 0 as read (not wrapped), the alignment over the C-alpha atoms of both
    got = gpu.M.MetricCoordinate(held.sel["ca"], refmol=held.raw0, trajalnsel=held.sel["ca"], pbc=False).project(held.mol20, ctx=gpu.ctx)
    print("coordinate, aligned: max |got - literal|", np.abs(got[-1, -20:] - held.g["coord_align_last20"]).max())
    assert np.all(np.abs(got[-1, -20:] - held.g["coord_align_last20"]) < 1e-3)


@pytest.mark.parametrize("mode,atomsel", [("atom", "ca"), ("residue", "noh")])
def test_metric_fluctuation_against_the_reference_arrays(gpu, held, mode, atomsel):
    """the reference wraps its refmol too (ref0 is frame 0 wrapped) and projects it through MetricCoordinate aligned onto itself"""
    for name, refmol in (("ref", held.ref0), ("mean", None)):
        got = gpu.M.MetricFluctuation(held.sel[atomsel], refmol=refmol, trajalnsel=held.sel["ca"], mode=mode, pbc=False).project(held.mol20, ctx=gpu.ctx)
        want = held.g[f"fluct_{mode}_{name}"]
        assert got.dtype == np.float64 and got.shape == want.shape == (20, 277)
        print(f"fluctuation {mode} {name}: max |got - held|", np.abs(got - want).max())
        assert np.allclose(got, want, atol=1e-3)


def test_metric_spherical_coordinate_on_the_trajectory(gpu, held):
    """The reference-held array of this projection (fixture key `spherical`) is NOT compared with: the reference's test wraps with
    GUESSED bonds, which the fixture cannot carry (its files list none), and the restatement with the stored bonds misses the array by up
    to 29.8 Angstrom / 0.83 rad / 5.6 rad against a bound of 1e-4 (tests/test_moments_cpu.py).  What is checked
    here, at that bound, is the class on the wrapped frames against the float64 restatement fed a float64 Kabsch alignment on the PDB's
    own coordinates -- the reference's refmol -- besides the synthetic checks of the mode above."""
    sel = held.sel
    got = gpu.M.MetricSphericalCoordinate(held.pdb, sel["mol"], sel["within8"], trajalnsel=sel["ca"], pbc=False).project(held.mol20, ctx=gpu.ctx)
    ca = np.flatnonzero(sel["ca"])
    moved = R.kabsch_align(np.ascontiguousarray(held.mol20.coords.transpose(2, 0, 1)), ca, held.pdb.coords[ca, :, 0])
    want = R.spherical(moved, np.flatnonzero(sel["mol"]), np.flatnonzero(sel["within8"]))
    assert got.dtype == np.float32 and got.shape == (20, 3)
    assert np.allclose(got, want, rtol=0, atol=1e-4)


def test_install_hooks(gpu):
    pytest.importorskip("moleculekit")
    import moleculekit.projections.metriccoordinate as mc

    from moleculekit_amd import moments

    original = mc.MetricCoordinate.project
    try:
        saved = moments.install()
        assert saved[0] is original and mc.MetricCoordinate.project is moments._reference_coordinate
        assert moments.install() == saved                                     # idempotent
    finally:
        moments.uninstall()
    assert mc.MetricCoordinate.project is original
    moments.uninstall()
