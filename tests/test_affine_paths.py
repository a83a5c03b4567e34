"""CPU tier: the fused per-item affine (LatticeProblem::affine) on every path of the voxelizer, on the emulated kernels.

The contract (csrc/mk_affine.h, csrc/pipeline.h): voxelizing WITH an affine gives, bit for bit, what voxelizing the coordinates
k_align_apply writes gives -- on every path.  The affine is read at seven places of kernels.h (bin_atom for the chain,
k_prepass_items and k_bin_solo; k_bin_direct; the TOPO binning; exact_recompute and exact_fixup_atom behind k_tail,
k_exact_shells and k_exact_redo), each of which finds its item index its own way.

Every case here is built BACKWARDS: the target coordinates are those of a case of tests/cases.py (so the transformed atoms sit
where that case was designed to be hard), every item gets a transform of its own -- a proper rotation from a random quaternion
plus a translation of tens of Angstrom, one item the identity -- and the inputs are the targets moved by the inverse
transforms.  Two references per run:
  * bits:   E_align.apply writes float32(M x + t); the same entry point, path and knobs voxelize that with affine=None;
  * values: the oracle on those float32 coordinates, within cases.TOL.
Periodic items: the C ABI takes a box together with an affine (include/mkamd_voxel.h (3b), (3c): the atom is voxelized at
float32(M x + t), the minimum image is taken of THAT position), so the pair is run and must meet both references; only the
Python streams refuse it (an aligned frame's box is no longer axis-aligned).
"""
import functools

import numpy as np
import pytest

from tests import emu_align_build as E_align
from tests import emu_build as E
from tests.cases import LATTICE_CASES, TOL, oracle_lattice


# ---- transforms and backwards-built inputs ---------------------------------------------------------------------------
def quat_rotation(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def random_affines(rng, B, identity_at=1):
    """float64 [B, 12]: a proper rotation from a random quaternion and a translation of 20 .. 60 A per item; item `identity_at`
    keeps the identity"""
    A = np.zeros((B, 12))
    for b in range(B):
        R, t = np.eye(3), np.zeros(3)
        if b != identity_at:
            R = quat_rotation(rng.normal(size=4))
            assert abs(np.linalg.det(R) - 1.0) < 1e-12
            d = rng.normal(size=3)
            t = d / np.linalg.norm(d) * rng.uniform(20.0, 60.0)
        A[b, :9], A[b, 9:] = R.ravel(), t
    return A


def move_back(target, offs, A):
    """the inputs whose transforms land on `target`: x = R^T (x' - t) in double, rounded to float32"""
    src = np.empty_like(target)
    with np.errstate(all="ignore"):
        for b in range(len(offs) - 1):
            s, e = int(offs[b]), int(offs[b + 1])
            R, t = A[b, :9].reshape(3, 3), A[b, 9:]
            src[s:e] = ((target[s:e].astype(np.float64) - t) @ R).astype(np.float32)
    return src


def apply_emulated(src, offs, A):
    """k_align_apply (the emulated kernel) on every item: float32(M x + t)"""
    out = src.copy()
    for b in range(len(offs) - 1):
        s, e = int(offs[b]), int(offs[b + 1])
        if e > s:
            out[s:e] = E_align.apply(src[s:e][None], A[b:b + 1])[0]
    return out


def ulps_from_numpy(src, offs, A, applied):
    """worst distance, in float32 ulps, of `applied` from float32(float64(M) x + t) computed by numpy (finite values only; where
    numpy's value is not finite the kernel's must not be either)"""
    worst = 0.0
    with np.errstate(all="ignore"):
        for b in range(len(offs) - 1):
            s, e = int(offs[b]), int(offs[b + 1])
            exp = (src[s:e].astype(np.float64) @ A[b, :9].reshape(3, 3).T + A[b, 9:]).astype(np.float32)
            fin = np.isfinite(exp)
            assert np.array_equal(fin, np.isfinite(applied[s:e]))
            if fin.any():
                d = np.abs(applied[s:e][fin].astype(np.float64) - exp[fin]) / np.spacing(np.abs(exp[fin])).astype(np.float64)
                worst = max(worst, float(d.max()))
    return worst


@functools.lru_cache(maxsize=None)
def built(name):
    """case `name` of tests/cases.py with at least three items (a one-item case: three copies of its item, each under a transform
    of its own), built backwards -> dict(src, applied, affine, offs, sigmas, origins, nv, vs, box, expected)"""
    case = LATTICE_CASES[name]()
    coords, offs, sig, origins, box = case["coords"], case["atom_offsets"], np.asarray(case["sigmas"]), case["origins"], case["box"]
    B = len(offs) - 1
    if B < 3:
        assert B == 1
        n = len(coords)
        coords, sig, origins = np.tile(coords, (3, 1)), np.tile(sig, (3, 1)), np.tile(origins, (3, 1))
        box = None if box is None else np.tile(box, (3, 1))
        offs, B = np.arange(4, dtype=np.int64) * n, 3
    rng = np.random.default_rng(sum(map(ord, name)))
    A = random_affines(rng, B)
    src = move_back(coords, offs, A)
    applied = apply_emulated(src, offs, A)
    with np.errstate(all="ignore"):
        expected = oracle_lattice(applied, offs, np.asarray(sig, np.float64), origins, case["nvoxels"], case["voxelsize"], box)
    return dict(src=src, applied=applied, affine=A, offs=offs, sigmas=sig, origins=origins, nv=case["nvoxels"], vs=case["voxelsize"],
                box=box, expected=expected, target=coords)


@functools.lru_cache(maxsize=None)
def untransformed(name):
    """what a voxelizer that ignores the affine would give: the inputs as they are"""
    c = built(name)
    out, _ = E.voxelize_lattice(c["src"], c["offs"], c["sigmas"], c["origins"], c["nv"], c["vs"], box=c["box"])
    return out


def gap(got, expected):
    return float(np.abs(np.asarray(got, np.float64).reshape(expected.shape) - expected).max())


# ---- the plain entry -------------------------------------------------------------------------------------------------
# path -> knobs of E.voxelize_lattice.  direct1: the first call on a workspace has no class table (the pass gives up, the chain
# serves it); the second one is binned by k_bin_direct.  items_kernel: the workgroup-per-item kernel runs when no team does.
PLAIN_PATHS = {
    "chain": dict(prepass_mode=0),
    "per_item": dict(prepass_mode=1),
    "default": dict(),
    "direct1": dict(direct=1, prepass_mode=0, repeat=2),
    "solo": dict(direct=2),
    "team": dict(tile_team=1),
    "one_wave_per_tile": dict(tile_team=0),
    "items_kernel": dict(tile_items=1, tile_team=0),
    "general": dict(force_general=True),
    "k4": dict(tile_k=4),
    "k8": dict(tile_k=8),
    "sigmas_f32": dict(),
    "sigmas_f64": dict(),
}
PLAIN_CASES = ["cfg3_small", "ragged_batch", "channels11", "dense_with_wide_sigmas", "cutoff_adversarial_1A", "voxel07"]
# cases whose atoms carry one sigma each, one channel group, open boundaries: k_bin_direct takes them
DIRECT_TAKES = {"cfg3_small", "ragged_batch", "dense_with_wide_sigmas", "voxel07"}


def run_plain(c, path, coords, affine, words=None):
    sig = c["sigmas"]
    if path == "sigmas_f32":
        sig = sig.astype(np.float32)
    elif path == "sigmas_f64":
        sig = sig.astype(np.float64)
    return E.voxelize_lattice(coords, c["offs"], sig, c["origins"], c["nv"], c["vs"], box=c["box"], affine=affine, direct_words=words,
                              **PLAIN_PATHS[path])


@pytest.mark.parametrize("path", list(PLAIN_PATHS))
@pytest.mark.parametrize("name", PLAIN_CASES)
def test_plain_entry_with_affine(name, path):
    c = built(name)
    words = np.zeros(4, np.uint32)
    fused, e1 = run_plain(c, path, c["src"], c["affine"], words)
    ref, e0 = run_plain(c, path, c["applied"], None)
    assert e1 == 0 and e0 == 0
    if path == "direct1" and name in DIRECT_TAKES:
        assert words[0] == 0, "k_bin_direct gave up: the chain served the call"
    if path == "solo" and c["sigmas"].shape[1] <= 8:
        assert words[0] == 0, "k_bin_solo did not run"
    assert np.array_equal(fused, ref), f"{np.count_nonzero(fused != ref)} values differ from the pre-applied run"
    g = gap(fused, c["expected"])
    print(f"{name}/{path}: worst gap to the oracle {g:.2e}")
    assert np.all(np.isfinite(fused)) and g <= TOL
    assert np.abs(fused - untransformed(name)).max() > 0.1


@pytest.mark.parametrize("tile_k", [4, 8])
@pytest.mark.parametrize("name", ["ragged_batch", "cutoff_adversarial_1A"])
def test_plain_entry_paths_agree_with_affine(name, tile_k):
    """every path gives the same bits as every other with the affine present, at one tile depth (the tile kernels expand d^2 about the
    tile's centre, so K = 4 and K = 8 differ in the last bits, with or without an affine).  ragged_batch's sigmas are float32 to begin
    with; cutoff_adversarial's float64 values are not float32 numbers, so that case keeps its dtype."""
    c = built(name)
    first = None
    for path in PLAIN_PATHS:
        if path in ("k4", "k8") or (name == "cutoff_adversarial_1A" and path == "sigmas_f32"):
            continue
        sig = c["sigmas"].astype({"sigmas_f32": np.float32, "sigmas_f64": np.float64}.get(path, c["sigmas"].dtype))
        out, err = E.voxelize_lattice(c["src"], c["offs"], sig, c["origins"], c["nv"], c["vs"], affine=c["affine"],
                                      **{**PLAIN_PATHS[path], "tile_k": tile_k})
        assert err == 0
        first = out if first is None else first
        assert np.array_equal(out, first), path


# ---- the topology entry ----------------------------------------------------------------------------------------------
NV_TOPO = [24, 24, 24]


@functools.lru_cache(maxsize=None)
def topo_molecule(kind):
    """frames of ONE molecule on a 24^3 grid at 1 A, built backwards.  `none`: no sigma above 1.81 A; `few`: four ions (2.27 A);
    `many`: 300 ions.  The ions sit on voxel centres nudged by float32 ulps, so that each has ~30 voxels within 1e-5 A^2 of the
    cut-off shell: the places where the exact fix-up, and only it, decides the value."""
    from tests.synth import synth_sigmas
    rng = np.random.default_rng({"none": 51, "few": 52, "many": 53}[kind])
    n_ions = {"none": 0, "few": 4, "many": 300}[kind]
    n_rest, F = 230, 3
    sig = np.concatenate([synth_sigmas(rng, n_rest), np.zeros((n_ions, 8))])
    sig[n_rest:, 0] = 2.27
    sig[n_rest::2, 5] = 2.75                                     # (every second ion: two wide channels)
    order = rng.permutation(len(sig))                             # the ions spread over the molecule
    sig = sig[order]
    base = np.concatenate([rng.uniform(1.0, 23.0, size=(n_rest, 3)), rng.integers(2, 22, size=(n_ions, 3)).astype(np.float64)])[order]
    ion = np.concatenate([np.zeros(n_rest, bool), np.ones(n_ions, bool)])[order]
    frames = []
    for _ in range(F):
        c = base.copy()
        c[~ion] += rng.normal(0, 0.4, size=(n_rest, 3))
        c = c.astype(np.float32)
        steps = rng.integers(-3, 4, size=c.shape)
        nudged = c.copy()
        for _ in range(3):
            up = np.nextafter(nudged, np.float32(np.inf)); dn = np.nextafter(nudged, np.float32(-np.inf))
            nudged = np.where(steps > 0, up, np.where(steps < 0, dn, nudged))
            steps = steps - np.sign(steps)
        c[ion] = nudged[ion]
        frames.append(c)
    n = len(sig)
    target = np.concatenate(frames)
    offs = np.arange(F + 1, dtype=np.int64) * n
    A = random_affines(rng, F)
    src = move_back(target, offs, A)
    applied = apply_emulated(src, offs, A)
    origins = np.zeros((F, 3))
    expected = oracle_lattice(applied, offs, np.tile(sig, (F, 1)), origins, np.array(NV_TOPO), 1.0)
    return dict(src=src, applied=applied, affine=A, offs=offs, sigmas=sig, origins=origins, expected=expected, F=F, target=target)


TOPO_KNOBS = {
    "shells_and_redo": dict(exact_redo=0),
    "in_k_tail": dict(exact_redo=-1),
    "redo_list_overflows": dict(exact_redo=5),
    "workspace_kept": dict(repeat=2),
}


@pytest.mark.parametrize("knobs", list(TOPO_KNOBS))
@pytest.mark.parametrize("kind", ["none", "few", "many"])
def test_topology_entry_with_affine(kind, knobs):
    m = topo_molecule(kind)
    kw = TOPO_KNOBS[knobs]
    fused, e1, wide = E.voxelize_lattice_topo(m["src"], m["sigmas"], m["F"], m["origins"], NV_TOPO, 1.0, affine=m["affine"], **kw)
    ref, e0, _ = E.voxelize_lattice_topo(m["applied"], m["sigmas"], m["F"], m["origins"], NV_TOPO, 1.0, **kw)
    assert e1 == 0 and e0 == 0 and wide == (kind != "none")
    assert np.array_equal(fused, ref), f"{np.count_nonzero(fused != ref)} values differ from the pre-applied run"
    g = gap(fused, m["expected"])
    print(f"topology/{kind}/{knobs}: worst gap to the oracle {g:.2e}")
    assert g <= TOL
    # no value on the other side of the cut-off than the reference's: the fix-up found every shell where the transform put it
    assert not ((fused.astype(np.float64).reshape(m["expected"].shape) == 0) != (m["expected"] == 0))[..., [0, 5]].any()
    plain, e2 = E.voxelize_lattice(m["src"], m["offs"], np.tile(m["sigmas"], (m["F"], 1)), m["origins"], NV_TOPO, 1.0, affine=m["affine"],
                                   prepass_mode=0)
    assert e2 == 0 and np.array_equal(plain, fused)
    bare, _, _ = E.voxelize_lattice_topo(m["src"], m["sigmas"], m["F"], m["origins"], NV_TOPO, 1.0)
    assert np.abs(fused - bare).max() > 0.1


# ---- periodic items with an affine -----------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["chain", "per_item", "default", "team", "general"])
def test_periodic_plain_entry_with_affine(path):
    """pbc_small through the plain entry: the box is applied to the TRANSFORMED position (the C ABI's contract)"""
    c = built("pbc_small")
    assert c["box"] is not None and len(c["offs"]) - 1 >= 3
    fused, e1 = run_plain(c, path, c["src"], c["affine"])
    ref, e0 = run_plain(c, path, c["applied"], None)
    assert e1 == 0 and e0 == 0 and np.array_equal(fused, ref)
    g = gap(fused, c["expected"])
    print(f"pbc_small/{path}: worst gap to the oracle {g:.2e}")
    assert g <= TOL
    assert np.abs(fused - untransformed("pbc_small")).max() > 0.1


def test_periodic_topology_entry_with_affine():
    """cfg4_small (frames of one molecule in a 31 A box) through the topology entry"""
    c = built("cfg4_small")
    F = len(c["offs"]) - 1
    n = int(c["offs"][1])
    sig = np.asarray(c["sigmas"][:n], np.float64)
    assert np.array_equal(np.tile(sig, (F, 1)), c["sigmas"])
    fused, e1, wide = E.voxelize_lattice_topo(c["src"], sig, F, c["origins"], c["nv"], c["vs"], box=c["box"], affine=c["affine"])
    ref, e0, _ = E.voxelize_lattice_topo(c["applied"], sig, F, c["origins"], c["nv"], c["vs"], box=c["box"])
    assert e1 == 0 and e0 == 0 and not wide and np.array_equal(fused, ref)
    g = gap(fused, c["expected"])
    print(f"cfg4_small/topology: worst gap to the oracle {g:.2e}")
    assert g <= TOL
    plain, e2 = run_plain(c, "chain", c["src"], c["affine"])
    assert e2 == 0 and np.array_equal(plain, fused)
    bare, _, _ = E.voxelize_lattice_topo(c["src"], sig, F, c["origins"], c["nv"], c["vs"], box=c["box"])
    assert np.abs(fused - bare).max() > 0.1


# ---- non-finite coordinates ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["chain", "per_item", "default", "direct1", "solo", "general"])
def test_nonfinite_coordinates_under_an_affine(path):
    """NaN / inf / huge inputs stay non-finite (or huge) under the transform: the same error flag and the same bits as the
    pre-applied run, and nothing but the finite atoms in the grids"""
    c = built("nonfinite_coords")
    assert not np.isfinite(c["applied"]).all() and not np.isfinite(c["src"]).all()
    fused, e1 = run_plain(c, path, c["src"], c["affine"])
    ref, e0 = run_plain(c, path, c["applied"], None)
    assert e1 == e0 and np.array_equal(fused, ref)
    g = gap(fused, c["expected"])
    print(f"nonfinite_coords/{path}: worst gap to the oracle {g:.2e}")
    assert np.all(np.isfinite(fused)) and g <= TOL


# ---- k_align_apply itself --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PLAIN_CASES + ["pbc_small", "cfg4_small", "nonfinite_coords"])
def test_applied_coordinates_within_one_ulp_of_numpy(name):
    c = built(name)
    worst = ulps_from_numpy(c["src"], c["offs"], c["affine"], c["applied"])
    print(f"{name}: applied coordinates worst {worst:.2f} ulp from numpy's float32(M x + t)")
    assert worst <= 1.0
    # the identity item is untouched, and the construction did land on the case's own geometry
    # (an atom with an infinite coordinate is NaN all over after any matrix product, the identity's included: 0 x inf)
    fin = np.isfinite(c["target"]).all(axis=1) & (np.abs(c["target"]).max(axis=1) < 1e6)
    s, e = int(c["offs"][1]), int(c["offs"][2])
    assert np.array_equal(c["applied"][s:e][fin[s:e]], c["target"][s:e][fin[s:e]])
    assert np.abs(c["applied"][fin] - c["target"][fin]).max() < 2e-5


@pytest.mark.parametrize("kind", ["none", "few", "many"])
def test_applied_topology_frames_within_one_ulp_of_numpy(kind):
    m = topo_molecule(kind)
    worst = ulps_from_numpy(m["src"], m["offs"], m["affine"], m["applied"])
    print(f"topology/{kind}: applied coordinates worst {worst:.2f} ulp from numpy's float32(M x + t)")
    assert worst <= 1.0
    assert np.abs(m["applied"] - m["target"]).max() < 2e-5


# ---- which paths the shapes of the GPU tier take -----------------------------------------------------------------------
# kernels that read coordinates: each must be handed the call's affine (a launch that passed nullptr would bin, or re-decide, the
# untransformed positions)
READS_COORDS = ("k_bin_solo<", "k_bin_direct<", "k_bin_count<", "k_bin_fill<", "k_prepass_items<", "k_tail<", "k_exact_shells<", "k_exact_redo<")


def _launches(**problem):
    st, text = E.trace_lattice(affine=1, **problem)
    assert st == 0, text
    lines = [ln.split("launch ", 1)[1] for ln in text.splitlines() if ln.startswith("  launch ")]
    names = [ln.split(" grid ", 1)[0].replace("mkamd::", "") for ln in lines]
    for name, ln in zip(names, lines):
        if name.startswith(READS_COORDS) and " coords " in ln:
            assert " affine" in ln.split(" : ", 1)[1], ln
    return names, text


def _has(kernels, prefix):
    return any(k.startswith(prefix) for k in kernels)


def test_gpu_tier_shapes_select_the_paths_they_are_meant_to():
    """tests/test_gpu_affine.py cannot see which kernels served a call (all paths give the same bits); run_lattice's host side on
    the launch recorder, with an affine present, can.  The shapes are the GPU tier's (GPU_SHAPES there)."""
    g24 = dict(nx=24, ny=24, nz=24)
    # one molecule on one 24^3 grid: the one-launch pre-pass and a team of waves per tile
    k, _ = _launches(B=1, total_atoms=3000, **g24)
    assert _has(k, "k_bin_solo<") and _has(k, "k_voxelize_tiles_team<") and not _has(k, "k_bin_count<")
    # 64 ligand-sized items: the per-item pre-pass and the workgroup-per-item kernel
    k, _ = _launches(B=64, total_atoms=64 * 60, **g24)
    assert _has(k, "k_prepass_items<") and _has(k, "k_voxelize_items<") and not _has(k, "k_bin_solo<")
    # 8 items of 2 000 atoms on 48^3 grids: the per-item pre-pass and a wave per tile
    k, _ = _launches(B=8, total_atoms=8 * 2000, nx=48, ny=48, nz=48)
    assert _has(k, "k_prepass_items<") and _has(k, "k_voxelize_tiles<") and not _has(k, "k_voxelize_items<")
    # 40 items of 6 000 atoms in order: direct binning in front of the chain, plain tiles
    k, _ = _launches(B=40, total_atoms=40 * 6000, **g24)
    assert _has(k, "k_bin_direct<") and _has(k, "k_bin_count<") and _has(k, "k_bin_fill<") and _has(k, "k_voxelize_tiles<")
    # ... and under a promise: the chain alone beside the previous call's tile kernel, the lean tiles
    k, text = _launches(B=40, total_atoms=40 * 6000, pipelining=1, calls=2, **g24)
    assert not _has(k, "k_bin_direct<") and _has(k, "k_bin_count<") and _has(k, "k_voxelize_tiles_lean<") and "-> set 1" in text
    # topology calls of 16 and of 300 frames of a 3 000-atom molecule: the TOPO binning; with ions the split exact fix-up
    for F in (16, 300):
        k, _ = _launches(B=F, total_atoms=F * 3000, topo=1, **g24)
        assert any(x.startswith("k_bin_count<") and x.endswith("true>") for x in k), k
        assert not _has(k, "k_exact_shells<") and not _has(k, "k_exact_redo<")
        k, _ = _launches(B=F, total_atoms=F * 3000, topo=1, topo_wide=4, **g24)
        assert any(x.startswith("k_bin_count<") and x.endswith("true>") for x in k), k
        assert _has(k, "k_exact_shells<") and _has(k, "k_exact_redo<") and _has(k, "k_tail<")
    # the chain proper (items of more than 4 096 atoms, below 200 000 in all)
    k, _ = _launches(B=24, total_atoms=24 * 5000, **g24)
    assert _has(k, "k_bin_count<") and not _has(k, "k_bin_direct<") and not _has(k, "k_prepass_items<") and not _has(k, "k_bin_solo<")
