"""tests/moments_cases.py -- TEST INFRASTRUCTURE: the synthetic inputs the group-moment tests share between the CPU tier (kernels on
the SIMT emulation) and the GPU tier, the conditions both tiers hold the kernels to, and the loader of the fixture
(tests/golden/moments_cases.npz).

The shapes are the smallest at which these kernels can go wrong: group sizes 1, 2, 7, 8, 9, 63, 64, 65 and 1 025 mixed within one call
(below, at and above every lane-group width), 1 / 3 / 277 groups, 1 / 2 / 63 / 65 frames (below and above a wave of frames for the
frame mean), weights absent / random float32 masses, affine absent / random proper rotations and translations, atoms repeated across
groups, one group of 30 000 atoms on one frame (the segmented form by the plan's own choice) and coordinates 1 000 Angstrom from the
origin (the shift has to keep the second moment exact)."""
from __future__ import annotations

import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
MIXED_SIZES = (1, 2, 7, 8, 9, 63, 64, 65, 1025)


def rotations(F, rng, shift=0.0):
    """float64 [F, 12]: random proper rotations (unit quaternions) and translations (about `shift`)"""
    q = rng.normal(size=(F, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], axis=1)
    return np.ascontiguousarray(np.concatenate([R, rng.uniform(-20, 20, size=(F, 3)) + shift], axis=1))


def case(name):
    """-> namespace(xyz float32 [F, N, 3], groups list of index arrays, weights float32 [n_sel] or None, affine float64 [F, 12] or None)"""
    seeds = {"mixed": 1, "one": 2, "three": 3, "residues": 4, "large": 5}
    rng = np.random.default_rng(seeds[name])
    if name == "mixed":             # every lane-group width crossed in one call; weights, affine, 1 000 A from the origin, 2 frames
        F, N, sizes, offset, wts, aff = 2, 1400, MIXED_SIZES, 1000.0, True, True
    elif name == "one":             # one group, more frames than a wave
        F, N, sizes, offset, wts, aff = 65, 90, (65,), 0.0, False, False
    elif name == "three":           # three groups, one frame short of a wave
        F, N, sizes, offset, wts, aff = 63, 100, (7, 64, 9), 0.0, True, False
    elif name == "residues":        # 277 residue-sized groups (several per wave), one frame
        F, N, sizes, offset, wts, aff = 1, 4507, tuple(rng.integers(4, 25, size=277)), 0.0, False, True
    else:                           # one group of 30 000 atoms on one frame: the segmented form by the plan's own choice
        F, N, sizes, offset, wts, aff = 1, 30000, (30000,), 1000.0, True, False
    xyz = (rng.uniform(-30, 30, size=(F, N, 3)) + offset).astype(F32)
    # atoms repeated ACROSS groups (each group draws from the whole molecule), never within one
    groups = [np.sort(rng.choice(N, size=int(s), replace=False)) if s < N else rng.permutation(N) for s in sizes]
    n_sel = int(sum(sizes))
    weights = rng.choice(np.array([1.00794, 12.0107, 14.0067, 15.9994, 32.065], F32), size=n_sel).astype(F32) if wts else None
    affine = rotations(F, rng, shift=0.0) if aff else None
    return types.SimpleNamespace(name=name, xyz=xyz, groups=groups, weights=weights, affine=affine, F=F, N=N)


CASES = ("mixed", "one", "three", "residues", "large")


def ordered(a):
    """float32 bits as integers in the order of the values (adjacent floats differ by 1)"""
    i = np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def assert_one_ulp(got, want64, what):
    """the condition of `center`, `gyration` and `spherical`: at most one float32 ulp from float32(restatement) -- both sides are
    float64 evaluations of the same float32 inputs that differ only in the order of summation (about n 2^-53 relative), so the one
    rounding to float32 can differ by one ulp at a rounding boundary and no more -- and NaN exactly where the restatement has NaN"""
    got = np.asarray(got)
    assert got.dtype == F32, (what, got.dtype)
    want = np.asarray(want64, np.float64).astype(F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs"
    ok = ~np.isnan(want)
    d = np.abs(ordered(got[ok]) - ordered(want[ok]))
    assert d.size == 0 or d.max() <= 1, f"{what}: {int(d.max())} float32 ulp from the restatement ({int((d > 1).sum())} values)"


def assert_fluct(got, want64, F, group_size, xmax, what):
    """the condition of `fluct` (float64): |got - want| <= (F + group size + 8) 2^-52 max|x|^2"""
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want64.shape, (what, got.dtype, got.shape, want64.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want64)), f"{what}: NaN pattern differs"
    bound = (F + group_size + 8) * 2.0 ** -52 * float(xmax) ** 2
    err = np.nanmax(np.abs(got - want64)) if got.size else 0.0
    assert err <= bound, f"{what}: error {err:.3e}, bound {bound:.3e}"


def fixture():
    """what the golden generator recorded (tests/golden/moments_cases.npz)"""
    return np.load(os.path.join(HERE, "golden", "moments_cases.npz"))


def _stand_in(g, s, coords, box, masses=None):
    n = g["protein"].size
    return types.SimpleNamespace(coords=np.ascontiguousarray(coords, dtype=F32), box=np.asarray(box, F32), numFrames=int(coords.shape[2]),
                                 element=s["element"], name=s["name"], resname=s["resname"], resid=s["resid"],
                                 masses=np.zeros(n, F32) if masses is None else masses)


_REFERENCE = None


def reference_case():
    """What the reference's own tests of the four projections work on, rebuilt from tests/golden alone (computed once, shared, never
    changed): stand-in molecules of tests/golden/xtc/metricdistance_traj.xtc with the naming fields of sasa_cases.npz and the masses
    of the fixture --
      raw20 / raw0     the LAST 20 frames and frame 0 as decoded (with their boxes)
      mol20 / ref0     the same wrapped with the wrap_box restatement about the reference's centersel ("protein"), the fixture's bonds
      pdb              the coordinates of filtered.pdb itself, one frame, no box
      sel              the boolean selections (protein, ca, noh, mol, within8), g the fixture"""
    global _REFERENCE
    if _REFERENCE is None:
        import moments_restatement as R
        from moleculekit_amd.xtc import XTCread

        g = fixture()
        s = np.load(os.path.join(HERE, "golden", "sasa_cases.npz"))
        t = XTCread(os.path.join(HERE, "golden", "xtc", "metricdistance_traj.xtc"), frame=[0] + list(range(180, 200)))
        coords, box = np.ascontiguousarray(t.coords, dtype=F32), np.asarray(t.box, F32)
        prot = np.flatnonzero(g["protein"])
        wrapped = R.wrap_box(coords, box, prot, g["bonds"])
        sel = dict(protein=g["protein"], ca=g["protein_ca"], noh=g["protein_noh"], mol=g["resname_mol"], within8=g["within8_resid98"])
        _REFERENCE = types.SimpleNamespace(
            g=g, sel=sel, raw20=_stand_in(g, s, coords[:, :, 1:], box[:, 1:], g["masses"]), raw0=_stand_in(g, s, coords[:, :, :1], box[:, :1]),
            mol20=_stand_in(g, s, wrapped[:, :, 1:], box[:, 1:], g["masses"]), ref0=_stand_in(g, s, wrapped[:, :, :1], box[:, :1]),
            pdb=_stand_in(g, s, g["pdb_coords"][:, :, None], np.zeros((3, 1), F32)))
    return _REFERENCE


def residue_offsets(resid, idx):
    """offsets of the runs of equal sequenceID(resid) among the atoms idx (ascending)"""
    seq = np.cumsum(np.r_[0, resid[1:] != resid[:-1]])[idx]
    return np.r_[0, np.flatnonzero(np.diff(seq)) + 1, idx.size]
