"""tests/sasa_cases.py -- TEST INFRASTRUCTURE: the inputs the surface-area tests share between the CPU tier (kernels on the SIMT
emulation) and the GPU tier, and the fixture of the reference's own MetricSasa test (tests/golden/sasa_cases.npz)."""
from __future__ import annotations

import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F32 = np.float32
# radius + probe in nanometres of H, C, N, O, S and two wide ones (Rb, Sn): the mixed radii of the random globules
MIXED_RADII = np.array([0.12, 0.17, 0.155, 0.152, 0.18, 0.303, 0.217], F32) + F32(0.14)


def globule(n, seed, frames=1):
    """n atoms at protein density (100 per cubic nanometre): the n sites of a cubic lattice nearest the origin, each moved by up
    to 0.05 nm per axis (no two atoms closer than 0.11 nm).  float32 [frames, n, 3] in nm, radii float32 [n] (mixed)"""
    rng = np.random.default_rng(seed)
    a = 100.0 ** (-1.0 / 3.0)
    m = int(np.ceil((3.0 * n / (4.0 * np.pi)) ** (1.0 / 3.0))) + 2
    g = np.arange(-m, m + 1)
    sites = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    sites = sites[np.argsort((sites * sites).sum(1), kind="stable")[:n]] * a
    xyz = (sites[None] + rng.uniform(-0.05, 0.05, size=(frames, n, 3))).astype(F32)
    return xyz, rng.choice(MIXED_RADII, n).astype(F32)


def fixture():
    """the reference's MetricSasa test: a stand-in molecule (frames 0 and 1, Angstrom) and the reference-held arrays"""
    g = np.load(os.path.join(HERE, "golden", "sasa_cases.npz"))
    head = np.load(os.path.join(HERE, "golden", "xtc", "3ptb_traj_head_decoded.npz"))["coords"][:, :, :2]
    mol = types.SimpleNamespace(coords=np.ascontiguousarray(head * F32(10)), element=g["element"], name=g["name"], resname=g["resname"],
                                resid=g["resid"], chain=g["chain"], segid=g["segid"], numFrames=2)
    return mol, g


def fixture_nm():
    """(xyz float32 [2, 4480, 3] nm, radii float32 [4480] nm, residue mapping int32 [4480]) by the reference's unit conversion"""
    import sasa_restatement as R
    from moleculekit_amd._sasa_radii import ATOMIC_RADII

    mol, g = fixture()
    p = g["protein"]
    mapping = np.zeros(int(p.sum()), np.int32)
    mapping[g["residue_first_atoms"][1:]] = 1
    return R.to_nm(mol.coords[p]), R.radii_nm([ATOMIC_RADII[e] for e in g["element"][p]]), np.cumsum(mapping).astype(np.int32)
