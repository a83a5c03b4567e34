#!/usr/bin/env python3
"""Golden fixture for the shell densities (moleculekit_amd/shell.py).

The reference's tests/test_metricshell.py projects all 200 frames of `tests/test_projections/trajectory/{filtered.pdb, traj.xtc}`
with MetricShell("protein and name CA", "resname MOL and noh", periodic="selections") -- 4 shells of 3 Angstrom around the 277 CA
atoms, counting the 9 heavy atoms of MOL -- and compares with an array the reference holds
(`tests/test_projections/metricshell/refdata.npy`, 200 x 1108 float64, np.allclose).  This script stores what a test of the same
projection needs WITHOUT the reference: DATA only, nothing of the reference is run.

    MOLECULEKIT_REF_TESTS=<reference>/tests python3 tests/golden/make_golden_shell.py

  tests/golden/shell_cases.npz  (compressed: 99.3 % of the array is zeros)
    refdata [200, 1108] float64     the reference-held array
    ca [277], mol_heavy [9] int64   the two selections as atom indexes, derived from the fields of sasa_cases.npz

The trajectory is tests/golden/xtc/metricdistance_traj.xtc (the reference's traj.xtc, byte for byte).
"""
import os

import numpy as np

REF_TESTS = os.environ.get("MOLECULEKIT_REF_TESTS", "/root/reference/tests")
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    held = np.load(os.path.join(REF_TESTS, "test_projections", "metricshell", "refdata.npy"))
    assert held.shape == (200, 1108) and held.dtype == np.float64, (held.shape, held.dtype)
    g = np.load(os.path.join(OUT, "sasa_cases.npz"))
    ca = np.flatnonzero(g["protein"] & (g["name"] == "CA"))
    mol_heavy = np.flatnonzero((g["resname"] == "MOL") & (g["element"] != "H"))
    assert ca.size == 277 and mol_heavy.size == 9, (ca.size, mol_heavy.size)
    assert held.shape[1] == ca.size * 4
    print("zeros: %.1f %%" % (100.0 * float((held == 0).mean())))
    path = os.path.join(OUT, "shell_cases.npz")
    np.savez_compressed(path, refdata=held, ca=ca.astype(np.int64), mol_heavy=mol_heavy.astype(np.int64))
    print("wrote", path, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
