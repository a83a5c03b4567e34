#!/usr/bin/env python3
"""Golden fixture for the dihedral angles (moleculekit_amd/dihedral.py).

The reference's tests/test_metricdihedral.py projects all 200 frames of `tests/test_projections/trajectory/{filtered.pdb, traj.xtc}`
with MetricDihedral(protsel="protein") -- sin / cos of the 552 phi / psi angles of its 277 protein residues -- and compares with an
array the reference holds (`tests/test_projections/metricdihedral/ref.npy`, 200 x 1104 float32, np.allclose(atol=1e-3)); and it
projects `dialanine-peptide.pdb` (ACE ALA NME in water, 688 atoms) with the default selection against four literals.  This script
stores what tests of the same projections need WITHOUT the reference: DATA only, nothing of the reference is run.

    MOLECULEKIT_REF_TESTS=<reference>/tests python3 tests/golden/make_golden_dihedral.py

  tests/golden/dihedral_cases.npz  (compressed)
    ref [200, 1104] float32                 the reference-held array
    insertion [4507] <U1                    the insertion codes of filtered.pdb (all empty; the other fields are in sasa_cases.npz)
    dia_name, dia_resname, dia_resid, dia_chain, dia_segid, dia_insertion [688]; dia_coords [688, 3, 1] float32
    dia_sel [688] bool                      resname ACE ALA NME (what "protein or resname ACE NME" selects in that file)
    dia_expected [1, 4] float32             the literals of the reference's test_dialanine_ace_nme

The trajectory is tests/golden/xtc/metricdistance_traj.xtc (the reference's traj.xtc, byte for byte).
"""
import os

import numpy as np

REF_TESTS = os.environ.get("MOLECULEKIT_REF_TESTS", "/root/reference/tests")
OUT = os.path.dirname(os.path.abspath(__file__))


def pdb_fields(path):
    """the fixed columns of the ATOM / HETATM records of the first model"""
    rows = []
    with open(path) as fh:
        for line in fh:
            if line.startswith("ENDMDL"):
                break
            if line.startswith(("ATOM", "HETATM")):
                line = line.rstrip("\n").ljust(80)
                rows.append((line[12:16].strip(), line[17:21].strip(), int(line[22:26]), line[21].strip(), line[72:76].strip(),
                             line[26].strip(), float(line[30:38]), float(line[38:46]), float(line[46:54])))
    name, resname, resid, chain, segid, ins = (np.array([r[k] for r in rows]) for k in range(6))
    xyz = np.array([r[6:9] for r in rows], np.float32)
    return name, resname, resid.astype(np.int64), chain.astype("<U1"), segid.astype("<U4"), ins.astype("<U1"), xyz


def main():
    held = np.load(os.path.join(REF_TESTS, "test_projections", "metricdihedral", "ref.npy"))
    assert held.shape == (200, 1104) and held.dtype == np.float32, (held.shape, held.dtype)
    g = np.load(os.path.join(OUT, "sasa_cases.npz"))
    name, resname, resid, chain, segid, ins, _ = pdb_fields(os.path.join(REF_TESTS, "test_projections", "trajectory", "filtered.pdb"))
    assert np.array_equal(name, g["name"]) and np.array_equal(resid, g["resid"]) and np.array_equal(resname, g["resname"])
    assert not np.any(ins != "")
    dn, drn, dri, dch, dsg, dins, xyz = pdb_fields(os.path.join(REF_TESTS, "test_projections", "metricdihedral", "dialanine-peptide.pdb"))
    assert dn.size == 688
    sel = np.isin(drn, ("ACE", "ALA", "NME"))
    assert sel.sum() == 22, sel.sum()
    path = os.path.join(OUT, "dihedral_cases.npz")
    np.savez_compressed(path, ref=held, insertion=ins, dia_name=dn, dia_resname=drn, dia_resid=dri, dia_chain=dch, dia_segid=dsg,
                        dia_insertion=dins, dia_coords=np.ascontiguousarray(xyz[:, :, None]), dia_sel=sel,
                        dia_expected=np.array([[-0.71247578, -0.70169669, 0.27399951, -0.96172982]], np.float32))
    print("wrote", path, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
