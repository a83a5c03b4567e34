"""GPU tier of the alignment row (moleculekit_amd/align.py): the reference's own alignment and MetricRmsd answers on its trajectory
(tests/golden/align_cases.npz, tests/golden/make_golden_align.py), a large trajectory against a float64 restatement, the
aligned voxel streams against aligned-then-voxelized frames, and every launch plan and apply path of the kernels on the cases of
tests/align_cases.py (shared with the emulator tier), the plan taken asserted through ``ctx.last_dist_kernel()``."""
import os

import numpy as np
import pytest

from tests import align_cases as C
from tests.cases import TOL

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "align_cases.npz")
XTC = os.path.join(HERE, "golden", "xtc", "metricdistance_traj.xtc")


def _traj():
    """the committed trajectory through the project's own reader, in Angstrom like the reference's (x 10 in float32)"""
    from moleculekit_amd import xtc
    n = xtc.get_xtc_nframes(XTC)
    c = xtc.read_xtc_frames(XTC, np.arange(n))[0]
    return np.ascontiguousarray(c * np.float32(10.0))


def kabsch64(P, Q):
    P = np.asarray(P, np.float64)
    Q = np.asarray(Q, np.float64)
    cP, cQ = P.mean(0), Q.mean(0)
    V, S, Wt = np.linalg.svd((P - cP).T @ (Q - cQ))
    Z = np.eye(3)
    Z[2, 2] = np.sign(np.linalg.det(Wt.T) * np.linalg.det(V))
    R = Wt.T @ Z @ V.T
    return R, cQ - R @ cP


@pytest.mark.parametrize("case", ["selfalign", "refmol", "matching", "selected"])
def test_molecule_align_cases_match_reference(hip_ctx, case):
    from moleculekit_amd import align
    g = np.load(GOLDEN)
    coords = _traj()
    lig = np.ascontiguousarray(coords[g["lig_idx"]])
    assert np.abs(lig - g["lig_coords"]).max() <= 1e-5
    lig = g["lig_coords"].copy()
    sel, refsel, frames = g[f"{case}_sel"], g[f"{case}_refsel"], g[f"{case}_frames"]
    if case == "selfalign":
        refc = lig
    elif case == "matching":
        refc = np.ascontiguousarray(np.roll(lig, 3, axis=2))
    else:
        refc = np.ascontiguousarray(lig[sel][:, :, 3:4])
    before = lig.copy()
    align._pp_align(lig, refc, sel, refsel, frames, int(g[f"{case}_refframe"]), bool(g[f"{case}_matching"]), inplace=True, ctx=hip_ctx)
    held = np.abs(lig - g[f"{case}_held"]).max()
    real = np.abs(lig - g[f"{case}_real"]).max()
    print(f"{case}: worst gap vs the reference-held array {held:.2e}, vs the real _pp_align {real:.2e}")
    assert held < 1e-3 and real < 1e-3
    others = np.setdiff1d(np.arange(lig.shape[2]), frames)
    assert np.array_equal(lig[:, :, others], before[:, :, others])


@pytest.mark.parametrize("name", ["reflected", "coplanar", "oneatom"])
def test_extra_cases_match_real_pp_align(hip_ctx, name):
    from moleculekit_amd import align
    g = np.load(GOLDEN)
    k = f"extra_{name}_"
    out = align._pp_align(g[k + "coords"], g[k + "ref"], g[k + "sel"], g[k + "refsel"], g[k + "frames"], 0, False, ctx=hip_ctx)
    assert np.abs(out - g[k + "out"]).max() < 1e-3


def test_rmsd_trajectory_reproduces_metricrmsd(hip_ctx):
    import torch
    from moleculekit_amd import align
    g = np.load(GOLDEN)
    coords = _traj()
    dev = torch.device("cuda", hip_ctx.device)
    xyz = torch.as_tensor(np.ascontiguousarray(coords.transpose(2, 0, 1)), device=dev)
    ca = g["rmsd_ca_idx"]
    got = align.rmsd_trajectory(xyz, xyz[0], ca, ca, ctx=hip_ctx).cpu().numpy()
    torch.cuda.synchronize()
    print(f"MetricRmsd: worst gap vs known {np.abs(got[-20:] - g['rmsd_known']).max():.2e}, vs the reference's values "
          f"{np.abs(got - g['rmsd_nopbc']).max():.2e}")
    assert np.all(np.abs(got[-20:] - g["rmsd_known"]) < 1e-3)
    assert np.abs(got - g["rmsd_nopbc"]).max() < 1e-4
    assert np.abs(got - g["rmsd_pbc"]).max() < 1e-4
    sub = align.rmsd_trajectory(xyz, xyz[0], ca, ca, frames=np.arange(180, 200), ctx=hip_ctx).cpu().numpy()
    assert np.array_equal(sub, got[180:])


def test_large_trajectory_within_one_ulp_and_deterministic(hip_ctx):
    import torch
    from moleculekit_amd import align
    rng = np.random.default_rng(12)
    N, F, nsel = 30000, 256, 3000
    ref = (rng.normal(size=(N, 3)) * 20).astype(np.float32)
    xyz = np.empty((F, N, 3), np.float32)
    for f in range(F):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
        xyz[f] = ref @ R.T + rng.uniform(-1000, 1000, 3) + rng.normal(scale=0.5, size=(N, 3))
    sel = np.sort(rng.choice(N, nsel, replace=False))
    dev = torch.device("cuda", hip_ctx.device)
    d_xyz = torch.as_tensor(xyz, device=dev)
    d_ref = torch.as_tensor(ref, device=dev)
    aff, fit = align.kabsch_transforms(d_xyz, d_ref, sel, ctx=hip_ctx)
    out = align.apply_transforms(d_xyz, aff, ctx=hip_ctx)
    aff2, fit2 = align.kabsch_transforms(d_xyz, d_ref, sel, ctx=hip_ctx)
    out2 = align.apply_transforms(d_xyz, aff2, ctx=hip_ctx)
    got, a = out.cpu().numpy(), aff.cpu().numpy()
    assert torch.equal(aff, aff2) and torch.equal(fit, fit2) and torch.equal(out, out2)
    worst = 0.0
    for f in range(0, F, 16):
        R, t = kabsch64(xyz[f][sel], ref[sel])
        exp = (xyz[f].astype(np.float64) @ R.T + t).astype(np.float32)
        ulps = np.abs(got[f].astype(np.float64) - exp) / np.spacing(np.abs(exp)).astype(np.float64)
        worst = max(worst, float(ulps.max()))
        assert np.abs(a[f, :9] - R.ravel()).max() < 1e-9
    print(f"30 000 atoms x 256 frames: worst {worst:.2f} ulp vs the float64 restatement")
    assert worst <= 1.0
    # frames outside the list are bitwise untouched (in place)
    frames = np.array([7, 3, 200])
    inplace = d_xyz.clone()
    aff3, _ = align.kabsch_transforms(inplace, d_ref, sel, frames=frames, ctx=hip_ctx)
    align.apply_transforms(inplace, aff3, frames=frames, out=inplace, ctx=hip_ctx)
    keep = np.setdiff1d(np.arange(F), frames)
    assert torch.equal(inplace[keep], d_xyz[keep])
    assert torch.equal(inplace[frames], out[frames])


def test_large_selection_one_frame(hip_ctx):
    import torch
    from moleculekit_amd import align
    rng = np.random.default_rng(13)
    N = 100000
    ref = (rng.normal(size=(N, 3)) * 30).astype(np.float32)
    xyz = (ref[::-1] + 5.0).astype(np.float32)[None]
    dev = torch.device("cuda", hip_ctx.device)
    aff, fit = align.kabsch_transforms(torch.as_tensor(xyz, device=dev), torch.as_tensor(ref, device=dev), np.arange(N), ctx=hip_ctx)
    R, t = kabsch64(xyz[0], ref)
    assert np.abs(aff.cpu().numpy()[0, :9] - R.ravel()).max() < 1e-9


def test_aligned_xtc_stream_equals_aligned_then_voxelized(hip_ctx):
    import torch
    from moleculekit_amd import align, batch, xtc
    from oracle import oracle
    g = np.load(GOLDEN)
    ca = g["rmsd_ca_idx"]
    dev = torch.device("cuda", hip_ctx.device)
    frames = np.arange(40)
    xyz, _, _, _ = xtc.read_xtc_frames_dev(XTC, frames, scale=10.0, ctx=hip_ctx)
    N = int(xyz.shape[1])
    ref = xyz[0, ca].cpu().numpy()
    center = ref.astype(np.float64).mean(0)
    rng = np.random.default_rng(0)
    sig = rng.uniform(1.0, 2.0, size=(N, 2)).astype(np.float32)
    box = [16, 16, 16]
    streamed = torch.cat([f for _, f in batch.iterVoxelizeXTC(XTC, sig, center, box, 1.0, pbc=False, frames=frames, chunk=16,
                                                               ctx=hip_ctx, align=(ref, ca))])
    aff, _ = align.kabsch_transforms(xyz, torch.as_tensor(ref, device=dev), ca, np.arange(len(ca)), ctx=hip_ctx)
    aligned = align.apply_transforms(xyz, aff, ctx=hip_ctx)
    coords = aligned.permute(1, 2, 0).contiguous()                                  # [N, 3, F] on the device
    direct = torch.cat([f for _, f in batch.iterVoxelizeTrajectory(coords, sig, center, box, 1.0, chunk=16, ctx=hip_ctx)])
    torch.cuda.synchronize()
    assert torch.equal(streamed, direct)
    plain = torch.cat([f for _, f in batch.iterVoxelizeXTC(XTC, sig, center, box, 1.0, pbc=False, frames=frames[:16], chunk=16, ctx=hip_ctx)])
    assert not torch.equal(plain, streamed[:16])                                    # (the alignment did something)
    a = aligned.cpu().numpy()
    nv = np.ceil(np.array(box, np.float64)).astype(int)
    centers = oracle.grid_centers(center - np.array(box, np.float64) / 2, nv, 1.0)
    worst = 0.0
    for f in (0, 17, 39):
        exp = oracle.calculate_occupancy(centers, a[f], sig)
        worst = max(worst, float(np.abs(streamed[f].cpu().numpy() - exp).max()))
    print(f"aligned stream vs oracle: {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("ions", [0, 5])
def test_aligned_xtc_stream_with_getchannels_shaped_sigmas(hip_ctx, ions):
    """The case above draws thousands of distinct sigmas, which no topology handle takes (at most 15): its streams fall back to the
    repeated sigma matrix.  A getChannels-shaped matrix -- 8 channels, the atom's radius where a property holds, a handful of
    distinct values, with and without ions -- is what production passes: the handle is built (checked here directly), so the
    aligned stream runs the topology binning and, with ions, the split exact fix-up."""
    import torch
    from moleculekit_amd import _lib, align, batch, xtc
    from oracle import oracle
    from tests.synth import synth_sigmas
    g = np.load(GOLDEN)
    ca = g["rmsd_ca_idx"]
    dev = torch.device("cuda", hip_ctx.device)
    frames = np.arange(40)
    xyz, _, _, _ = xtc.read_xtc_frames_dev(XTC, frames, scale=10.0, ctx=hip_ctx)
    N = int(xyz.shape[1])
    sig = synth_sigmas(np.random.default_rng(3), N).astype(np.float32)
    if ions:
        at = np.linspace(0, N - 1, ions).astype(int)
        sig[at] = 0.0
        sig[at, 7] = 2.27
    assert len(np.unique(sig[sig != 0])) <= 15
    topo = _lib.Topology(hip_ctx, sig, 1.0)
    assert topo.has_wide_sigmas == bool(ions)
    topo.close()
    ref = xyz[0, ca].cpu().numpy()
    center = ref.astype(np.float64).mean(0)
    box = [16, 16, 16]
    streamed = torch.cat([f for _, f in batch.iterVoxelizeXTC(XTC, sig, center, box, 1.0, pbc=False, frames=frames, chunk=16,
                                                               ctx=hip_ctx, align=(ref, ca))])
    aligned = align.align_trajectory(xyz, torch.as_tensor(ref, device=dev), ca, np.arange(len(ca)), ctx=hip_ctx)
    coords = aligned.permute(1, 2, 0).contiguous()
    direct = torch.cat([f for _, f in batch.iterVoxelizeTrajectory(coords, sig, center, box, 1.0, chunk=16, ctx=hip_ctx)])
    torch.cuda.synchronize()
    assert torch.equal(streamed, direct)
    a = aligned.cpu().numpy()
    centers = oracle.grid_centers(center - 8.0, np.array(box), 1.0)
    worst = max(float(np.abs(streamed[f].cpu().numpy() - oracle.calculate_occupancy(centers, a[f], sig)).max()) for f in (0, 17, 39))
    print(f"aligned stream, getChannels-shaped sigmas, {ions} ions: {worst:.2e}")
    assert worst <= TOL


# ------------------------------------------------------------------------------------------------
# every launch plan and apply path on the hardware: the cases of tests/align_cases.py, which tests/test_align_cpu.py runs on the
# emulation -- the same inputs under the same conditions, the plan asserted through ctx.last_dist_kernel()
# ------------------------------------------------------------------------------------------------
class Hardware:
    """the driver of tests/align_cases.py on the device: numpy in, numpy out.  Every transforms and RMSD call is made twice and must
    give the same bits both times."""

    def __init__(self, ctx):
        import torch
        from moleculekit_amd import align
        self.torch, self.align, self.ctx = torch, align, ctx
        self.dev = torch.device("cuda", ctx.device)

    def up(self, a):
        return self.torch.as_tensor(np.array(a), device=self.dev)            # (a copy: the shared cases are read-only arrays)

    @staticmethod
    def same_bits(a, b):
        return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(np.int64 if a.itemsize == 8 else np.int32)
                                                                   == b.view(np.int64 if b.itemsize == 8 else np.int32)).all())

    def transforms(self, xyz, ref, sel, refsel, frames=None, refframe=0, matching=False, cus=None):
        A = self.align
        d_xyz, d_ref = A._xyz3("xyz", self.up(xyz)), A._xyz3("ref", self.up(ref))
        ctx, dev = A._torch_ctx(d_xyz, self.ctx)
        d_sel, d_refsel = A._dev_sel(np.asarray(sel), d_xyz.shape[1], "sel", dev), A._dev_sel(np.asarray(refsel), d_ref.shape[1], "refsel", dev)
        d_fr, K = A._dev_frames(frames, int(d_xyz.shape[0]), dev)
        runs = []
        for _ in range(2):                                                     # float64 fit RMSD: what the kernel writes, not its float32 copy
            aff, fit = A._transforms(ctx, dev, d_xyz, d_ref, d_sel, d_refsel, d_sel.numel(), d_fr, K, refframe, matching)
            runs.append((aff.cpu().numpy(), fit.cpu().numpy()))
        assert self.same_bits(runs[0][0], runs[1][0]) and self.same_bits(runs[0][1], runs[1][1]), "two runs of the transforms differ"
        return runs[0]

    def apply(self, xyz, affine, frames=None):
        return self.align.apply_transforms(self.up(xyz), self.up(affine), frames=frames, ctx=self.ctx).cpu().numpy()

    def apply_at(self, base, off_in, outbuf, off_out, N, F, affine, frames):
        n = 3 * N * F
        d_base = self.up(base)
        d_out = d_base if outbuf is None else self.up(outbuf)
        src = d_base[off_in:off_in + n].view(F, N, 3)
        dst = d_out[off_out:off_out + n].view(F, N, 3)
        assert src.data_ptr() == d_base.data_ptr() + 4 * off_in and dst.data_ptr() == d_out.data_ptr() + 4 * off_out and d_base.data_ptr() % 16 == 0
        assert d_out.data_ptr() % 16 == 0
        got = self.align.apply_transforms(src, self.up(affine), frames=frames, out=dst, ctx=self.ctx)
        assert got.data_ptr() == dst.data_ptr()
        return d_out.cpu().numpy()

    def rmsd_trajectory(self, xyz, ref, alnsel, rmsdsel, frames=None):
        d_xyz, d_ref = self.up(xyz), self.up(ref)
        a = self.align.rmsd_trajectory(d_xyz, d_ref, alnsel, alnsel, rmsdsel, rmsdsel, frames=frames, ctx=self.ctx).cpu().numpy()
        b = self.align.rmsd_trajectory(d_xyz, d_ref, alnsel, alnsel, rmsdsel, rmsdsel, frames=frames, ctx=self.ctx).cpu().numpy()
        assert self.same_bits(a, b), "two runs of the RMSD differ"
        return a

    def last_kernel(self):
        return self.ctx.last_dist_kernel()


@pytest.fixture(scope="module")
def hw(hip_ctx):
    return Hardware(hip_ctx)


@pytest.mark.parametrize("F", C.WIDTH_FRAMES)
@pytest.mark.parametrize("n", C.WIDTH_SIZES)
def test_group_widths_and_partial_waves(hw, n, F):
    """G = 8 / 16 / 32 / 64 by the selection's size, below, at and above every width; 13 and 37 frames leave waves and blocks partly
    filled; one reference frame and matching frames, all frames and a list out of order"""
    for matching in (False, True):
        for listed in (False, True):
            C.check_width(hw, n, F, matching, listed)


def test_matching_frames_segmented(hw):
    C.check_segmented_match(hw)


def test_unsegmented_long_walk_and_its_segmented_twin(hw):
    cus = hw.ctx.device_info()["compute_units"]
    if 8 * cus > C.LONG_WALK["F"]:
        pytest.skip(f"{cus} compute units: the plan cuts a 300-atom selection into segments even on {C.LONG_WALK['F']} frames")
    C.check_two_plans(hw, C.LONG_WALK["F"], C.LONG_WALK["every"])


@pytest.mark.parametrize("N", C.APPLY_SIZES)
def test_apply_every_placement_gives_the_same_bits(hw, N):
    C.check_apply_alignment(hw, N)


def test_rmsd_over_another_selection(hw):
    C.check_rmsd(hw)


@pytest.mark.parametrize("matching", [False, True])
def test_host_route_equals_tensor_route(hw, matching):
    """_pp_align (host arrays in the reference's layout: mkamd_align_host) against align_trajectory on the transposed tensor"""
    c = C.route_case()
    for frames in C.ROUTE_FRAMES:
        fr = np.arange(c.F) if frames is None else np.array(frames)
        host = hw.align._pp_align(c.coords, c.refs if matching else c.ref, c.sel, c.sel, fr, 0, matching, inplace=False, ctx=hw.ctx)
        dev = hw.align.align_trajectory(hw.up(c.xyz), hw.up(c.refs_fm if matching else c.ref_fm), c.sel, frames=fr, matchingframes=matching,
                                        ctx=hw.ctx).cpu().numpy()
        assert host.dtype == np.float32 and np.array_equal(C.bits(host), C.bits(dev.transpose(1, 2, 0))), (matching, frames)
        assert not np.array_equal(host[:, :, fr], c.coords[:, :, fr])                      # (the alignment did something)


@pytest.mark.parametrize("kind", ["coplanar", "collinear"])
def test_degenerate_selections(hw, kind):
    C.check_degenerate(hw, kind)


def test_zero_covariance_gives_identity(hw):
    C.check_coincident(hw)


def test_empty_selection_gives_nan(hw):
    C.check_empty(hw)
