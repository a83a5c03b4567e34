"""CPU tier of the dihedral angles (moleculekit_amd/dihedral.py).

1. The numpy restatement of the reference (tests/dihedral_restatement.py) against the array the reference holds for its own
   MetricDihedral test (its assertion: allclose, atol 1e-3), and against the four literals of its dialanine test.
2. The kernels' source on the SIMT emulation (tests/emu/emu_dihedral.cpp, -ffp-contract=off), both lane assignments forced:
   the terms (p1, p2) BIT-EQUAL to the restatement on every case of tests/dihedral_cases.py; angle, degrees and sin / cos at least
   as close to the float64 function of those terms as the restatement is (E_ref is computed here from the restatement, over
   >= 100 000 values, no margin); collinear and NaN cases exactly.
3. The topology (phi / psi of the real system in the held array's column order, chi1-chi5 of every residue type under both naming
   conventions, caps, two chains, insertion codes, the ambiguous-atom error) and the host logic of dihedral.py with the emulation
   standing in for the library.
"""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dihedral_cases as C  # noqa: E402
import dihedral_restatement as R  # noqa: E402

F32, U32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def E():
    import emu_dihedral_build
    emu_dihedral_build.build()
    return emu_dihedral_build


@pytest.fixture(scope="module")
def real():
    from moleculekit_amd.dihedral import Dihedral
    mol, g = C.fixture()
    dih = Dihedral.proteinDihedrals(mol, mol.protein)
    quads = np.array(Dihedral.dihedralsToIndexes(mol, dih, mol.protein), np.int64)
    return mol, g, dih, quads, R.terms(mol.coords, quads)


KERNELS = (("k_dihedral_frames", 2), ("k_dihedral_atoms", 1))        # (name, the `avoid` bit that forces it)


def check_terms(E, coords, quads, box=None):
    """the restatement's terms, after asserting that BOTH lane assignments (forced) reproduce their bits"""
    want = R.terms(coords, quads, box)
    wraps = box is not None and bool(np.any(np.asarray(box) != 0))
    for name, avoid in KERNELS:
        got = E.dihedrals(coords, quads, box, "terms", avoid=avoid)
        assert name in E.last_kernel() and E.last_kernel().endswith("<true>") == wraps, E.last_kernel()
        assert got.dtype == F32 and got.shape == want.shape
        assert C.bit_equal(got, want), f"{name}: {int((got.view(U32) != want.view(U32)).sum())} of {want.size} terms differ"
        assert E.last_workspace() == 0
    return want


def check_accuracy(run, sets, label):
    """item 2 of the contract over a list of (coords, quads, box): the worst error of `run(coords, quads, box, mode, avoid)` against the
    float64 function of the restatement's terms must not exceed the restatement's own worst error E_ref -- no margin"""
    for name, avoid in KERNELS:
        worst = {m: [0.0, 0.0] for m in ("radians", "degrees", "sincos")}
        count = 0
        for coords, quads, box in sets:
            t = R.terms(coords, quads, box)
            rad, deg, sc = R.truth(t)
            count += sc.size
            for mode, want, ref in (("radians", rad, R.radians(t)), ("degrees", deg, R.project(t, False)), ("sincos", sc, R.project(t, True))):
                got = run(coords, quads, box, mode, avoid)
                assert got.dtype == F32 and got.shape == want.shape
                assert np.array_equal(np.isnan(got), np.isnan(want)), f"{label} {name} {mode}: NaN positions differ"
                worst[mode][0] = max(worst[mode][0], R.worst(got, want))
                worst[mode][1] = max(worst[mode][1], R.worst(ref, want))
        assert count >= 100000, count
        for mode, (e_dev, e_ref) in worst.items():
            print(f"{label} {name} {mode}: device {e_dev:.3e}  E_ref {e_ref:.3e}  ({count} values)")
            assert e_dev <= e_ref, f"{label} {name} {mode}: {e_dev:.3e} > E_ref {e_ref:.3e}"


def synthetic_sets():
    sets = [(c, q, None) for c, q in C.scale_cases(F=200, D=130)] + [(c, q, None) for c, q in C.shape_cases()]
    c, q, b = C.periodic_case(F=200)
    return sets + [(c, q, b)]


# ---------------------------------------------------------------------------------------------
# 1. the restatement against what the reference holds
# ---------------------------------------------------------------------------------------------
def test_restatement_is_the_reference_held_array_to_its_own_tolerance(real):
    _, g, _, quads, t = real
    got = R.project(t, True)
    assert got.shape == (200, 1104) and got.dtype == F32
    assert np.allclose(got, g["ref"], atol=1e-3)
    assert float(np.abs(got - g["ref"]).max()) < 1e-6                # (last bits: another libm's atan2f)


def test_restatement_gives_the_dialanine_literals():
    from moleculekit_amd.dihedral import Dihedral
    mol, sel, expected = C.dialanine()
    quads = Dihedral.dihedralsToIndexes(mol, Dihedral.proteinDihedrals(mol, sel), sel)
    assert len(quads) == 2
    assert np.allclose(expected, R.project(R.terms(mol.coords, quads), True))


# ---------------------------------------------------------------------------------------------
# 2. the kernels on the emulation
# ---------------------------------------------------------------------------------------------
def test_emu_terms_real_trajectory(E, real):
    mol, _, _, quads, t = real
    sub = slice(0, 70)                                               # (the emulation is slow: 70 frames, all 552 dihedrals)
    want = check_terms(E, np.ascontiguousarray(mol.coords[:, :, sub]), quads)
    assert C.bit_equal(want, t[sub])


def test_emu_terms_scales_and_shapes(E):
    for coords, quads in C.scale_cases() + C.shape_cases():
        check_terms(E, coords, quads)


def test_emu_terms_periodic_and_zero_box(E):
    coords, quads, box = C.periodic_case()
    want = check_terms(E, coords, quads, box)
    open_ = R.terms(coords, quads)
    assert not C.bit_equal(want, open_)                              # (the box matters in this case)
    assert C.bit_equal(check_terms(E, coords, quads, np.zeros_like(box)), open_)
    # the components exactly at +- box / 2 are NOT wrapped, the one an ulp beyond is: the restatement says so too
    n = coords.shape[0] - 8
    r12x = coords[n, 0] - coords[n + 1, 0]
    assert np.array_equal(r12x, box[0] / F32(2))


def test_emu_plan_chooses_by_frames(E):
    for F, name in ((1, "k_dihedral_atoms"), (7, "k_dihedral_atoms"), (63, "k_dihedral_atoms"), (64, "k_dihedral_frames"),
                    (200, "k_dihedral_frames")):
        coords, quads = C.random_case(40, 33, F, 5)
        E.dihedrals(coords, quads, None, "sincos")
        assert name in E.last_kernel(), (F, E.last_kernel())


def test_emu_collinear_and_nan_exactly(E):
    coords, quads = C.collinear_case()
    t = check_terms(E, coords, quads)
    assert np.all(t[:, 0] == 0) and np.all(t[:, 2] == 0)
    ncoords, nquads = C.nan_case()
    nt = check_terms(E, ncoords, nquads)
    hit = np.zeros(nt.shape[:2], bool)
    hit[2] = np.any(nquads == 5, axis=1)
    hit[65] |= np.any(nquads == 9, axis=1)
    assert np.array_equal(np.isnan(nt[..., 0]), hit) and np.array_equal(np.isnan(nt[..., 1]), hit)
    for _, avoid in KERNELS:
        sc = E.dihedrals(coords, quads, None, "sincos", avoid=avoid)
        assert np.all(sc[:, 0] == 0) and np.all(sc[:, 1] == 1) and np.all(sc[:, 4] == 0) and np.all(sc[:, 5] == 1)
        for mode in ("radians", "degrees"):
            a = E.dihedrals(coords, quads, None, mode, avoid=avoid)
            assert np.all(a[:, 0] == 0) and np.all(a[:, 2] == 0) and np.all(a[:, 1] != 0)
        for mode in ("radians", "degrees"):
            assert np.array_equal(np.isnan(E.dihedrals(ncoords, nquads, None, mode, avoid=avoid)), hit)
        assert np.array_equal(np.isnan(E.dihedrals(ncoords, nquads, None, "sincos", avoid=avoid)), np.repeat(hit, 2, axis=1))


def test_emu_accuracy_synthetic_sets(E):
    check_accuracy(lambda c, q, b, mode, avoid: E.dihedrals(c, q, b, mode, avoid=avoid), synthetic_sets(), "synthetic")


def test_emu_accuracy_real_trajectory(E, real):
    mol, _, _, quads, _ = real
    sets = [(np.ascontiguousarray(mol.coords[:, :, :100]), quads, None)]
    check_accuracy(lambda c, q, b, mode, avoid: E.dihedrals(c, q, b, mode, avoid=avoid), sets, "real")


def test_emu_refusals(E):
    coords, quads = C.random_case(10, 3, 2, 1)
    with pytest.raises(ValueError, match="mode"):
        E.dihedrals(coords, quads, None, 7)
    assert E.dihedrals(coords, np.zeros((0, 4), U32), None, "sincos").shape == (2, 0)


# ---------------------------------------------------------------------------------------------
# 3. topology
# ---------------------------------------------------------------------------------------------
def test_phi_psi_of_the_real_topology(real):
    mol, g, dih, quads, _ = real
    assert len(dih) == 552 and quads.shape == (552, 4)
    assert [d.dihedraltype for d in dih[:3]] == ["psi", "phi", "psi"] and dih[-1].dihedraltype == "phi"
    names = mol.name[quads]
    phi = np.array([d.dihedraltype == "phi" for d in dih])
    assert np.all(names[phi] == np.array(["C", "N", "CA", "C"])) and np.all(names[~phi] == np.array(["N", "CA", "C", "N"]))
    # the column order is the held array's: every column reproduces it (a permutation would not)
    got = R.project(R.terms(mol.coords, quads), True)
    assert float(np.abs(got - g["ref"]).max(axis=0).max()) < 1e-6


SIDE = {  # residue -> side-chain atom names (PDB naming; ILE's delta carbon is added by convention below)
    "ALA": "CB", "GLY": "", "ARG": "CB CG CD NE CZ NH1 NH2", "ASN": "CB CG OD1 ND2", "ASP": "CB CG OD1 OD2", "CYS": "CB SG",
    "GLN": "CB CG CD OE1 NE2", "GLU": "CB CG CD OE1 OE2", "HIS": "CB CG ND1 CD2 CE1 NE2", "ILE": "CB CG1 CG2", "LEU": "CB CG CD1 CD2",
    "LYS": "CB CG CD CE NZ", "MET": "CB CG SD CE", "PHE": "CB CG CD1 CD2 CE1 CE2 CZ", "PRO": "CB CG CD", "SER": "CB OG",
    "THR": "CB OG1 CG2", "TRP": "CB CG CD1 CD2 NE1 CE2 CE3 CZ2 CZ3 CH2", "TYR": "CB CG CD1 CD2 CE1 CE2 CZ OH", "VAL": "CB CG1 CG2",
}
EXPECTED_CHI = {  # residue -> chi1 .. chi5, written out (ILE chi2 ends in CD1 under amber names, CD under charmm names)
    "ARG": ["N CA CB CG", "CA CB CG CD", "CB CG CD NE", "CG CD NE CZ", "CD NE CZ NH1"],
    "ASN": ["N CA CB CG", "CA CB CG OD1"], "ASP": ["N CA CB CG", "CA CB CG OD1"], "CYS": ["N CA CB SG"],
    "GLN": ["N CA CB CG", "CA CB CG CD", "CB CG CD OE1"], "GLU": ["N CA CB CG", "CA CB CG CD", "CB CG CD OE1"],
    "HIS": ["N CA CB CG", "CA CB CG ND1"], "ILE": ["N CA CB CG1", "CA CB CG1 CD?"], "LEU": ["N CA CB CG", "CA CB CG CD1"],
    "LYS": ["N CA CB CG", "CA CB CG CD", "CB CG CD CE", "CG CD CE NZ"], "MET": ["N CA CB CG", "CA CB CG SD", "CB CG SD CE"],
    "PHE": ["N CA CB CG", "CA CB CG CD1"], "PRO": ["N CA CB CG", "CA CB CG CD"], "SER": ["N CA CB OG"], "THR": ["N CA CB OG1"],
    "TRP": ["N CA CB CG", "CA CB CG CD1"], "TYR": ["N CA CB CG", "CA CB CG CD1"], "VAL": ["N CA CB CG1"], "ALA": [], "GLY": [],
}


def every_residue(ff):
    names, resnames, resids = [], [], []
    for k, (res, side) in enumerate(sorted(SIDE.items())):
        atoms = ["N", "CA", "C", "O"] + side.split() + ([{"amber": "CD1", "charmm": "CD"}[ff]] if res == "ILE" else [])
        names += atoms
        resnames += [res] * len(atoms)
        resids += [k + 1] * len(atoms)
    n = len(names)
    return types.SimpleNamespace(name=np.array(names), resname=np.array(resnames), resid=np.array(resids), chain=np.full(n, "A"),
                                 segid=np.full(n, "P"), insertion=np.full(n, ""), coords=np.zeros((n, 3, 1), F32))


@pytest.mark.parametrize("ff", ["amber", "charmm"])
def test_chi_angles_of_every_residue_type(ff):
    from moleculekit_amd.dihedral import Dihedral
    mol = every_residue(ff)
    kinds = ("chi1", "chi2", "chi3", "chi4", "chi5")
    dih = Dihedral.proteinDihedrals(mol, "all", dih=kinds, ff=ff)
    got = Dihedral.dihedralsToIndexes(mol, dih)
    want, labels = [], []
    for k, res in enumerate(sorted(SIDE)):
        for c, quad in enumerate(EXPECTED_CHI[res]):
            quad = quad.replace("CD?", {"amber": "CD1", "charmm": "CD"}[ff])
            want.append([int(np.flatnonzero((mol.resid == k + 1) & (mol.name == a))[0]) for a in quad.split()])
            labels.append(kinds[c])
    assert got == want and [d.dihedraltype for d in dih] == labels
    if ff == "amber":                                               # the other convention's ILE atom is not in this molecule
        with pytest.raises(Exception, match="CD"):
            Dihedral.proteinDihedrals(mol, "all", dih=("chi2",), ff="charmm")
    # the per-residue order is phi, psi, omega, chi1 .. chi5 whatever the order asked for
    mixed = Dihedral.proteinDihedrals(mol, "all", dih=("chi1", "omega", "psi", "phi"), ff=ff)
    arg = [d.dihedraltype for d in mixed if d.atoms[1]["resid"] == 2 or (d.dihedraltype in ("psi", "omega") and d.atoms[0]["resid"] == 2)]
    assert arg == ["phi", "psi", "omega", "chi1"], arg
    with pytest.raises(RuntimeError, match="known residues"):
        mol.resname[:] = "XYZ"
        Dihedral.proteinDihedrals(mol, "all", dih=("chi1",), ff=ff)


def test_dialanine_caps_give_one_phi_and_one_psi():
    from moleculekit_amd.dihedral import Dihedral
    mol, sel, _ = C.dialanine()
    dih = Dihedral.proteinDihedrals(mol, sel)
    assert [d.dihedraltype for d in dih] == ["phi", "psi"]          # ACE has no N / CA: no psi; NME has no CA / C: no phi
    q = Dihedral.dihedralsToIndexes(mol, dih, sel)
    assert [list(mol.name[a]) for a in q] == [["C", "N", "CA", "C"], ["N", "CA", "C", "N"]]
    assert list(mol.resname[q[0]]) == ["ACE", "ALA", "ALA", "ALA"] and list(mol.resname[q[1]]) == ["ALA", "ALA", "ALA", "NME"]
    assert Dihedral.proteinDihedrals(mol, sel, dih=("omega",)) == []      # neither cap has a CA


def tripeptides(chains=("A", "B"), insertion=False):
    names, resids, ch, ins = [], [], [], []
    for c in chains:
        for r in (1, 2, 3):
            names += ["N", "CA", "C", "O"]
            resids += [r if not insertion else 5] * 4
            ch += [c] * 4
            ins += [("", "A", "B")[r - 1] if insertion else ""] * 4
    n = len(names)
    return types.SimpleNamespace(name=np.array(names), resname=np.full(n, "GLY"), resid=np.array(resids), chain=np.array(ch),
                                 segid=np.full(n, ""), insertion=np.array(ins), coords=np.zeros((n, 3, 1), F32))


def test_two_chains_and_insertion_codes():
    from moleculekit_amd.dihedral import Dihedral
    mol = tripeptides()
    q = Dihedral.dihedralsToIndexes(mol, Dihedral.proteinDihedrals(mol, "all", dih=("phi", "psi")))
    # per chain: psi(1), phi(2), psi(2), phi(3); nothing crosses from chain A (atoms 0-11) into chain B (12-23)
    assert q == [[0, 1, 2, 4], [2, 4, 5, 6], [4, 5, 6, 8], [6, 8, 9, 10],
                 [12, 13, 14, 16], [14, 16, 17, 18], [16, 17, 18, 20], [18, 20, 21, 22]]
    # the same resid three times, told apart by the insertion code
    mol = tripeptides(chains=("A",), insertion=True)
    q = Dihedral.dihedralsToIndexes(mol, Dihedral.proteinDihedrals(mol, "all", dih=("phi", "psi")))
    assert q == [[0, 1, 2, 4], [2, 4, 5, 6], [4, 5, 6, 8], [6, 8, 9, 10]]
    # a selection of one chain
    mol = tripeptides()
    q = Dihedral.dihedralsToIndexes(mol, Dihedral.proteinDihedrals(mol, mol.chain == "B"), mol.chain == "B")
    assert q[0] == [12, 13, 14, 16] and len(q) == 4


def test_ambiguous_and_missing_atoms_are_errors():
    from moleculekit_amd.dihedral import Dihedral
    mol = tripeptides()
    d = Dihedral({"name": "N", "resid": 1, "chain": "A"}, {"name": "CA", "resid": 1, "chain": "A"}, {"name": "C", "resid": 1, "chain": "A"},
                 {"name": "N", "resid": 2, "chain": "A"})
    assert Dihedral.dihedralsToIndexes(mol, d) == [[0, 1, 2, 4]]
    mol.chain[:] = "A"                                               # now every (name, resid) exists twice
    with pytest.raises(RuntimeError, match="Expected one atom"):
        Dihedral.dihedralsToIndexes(mol, d)
    with pytest.raises(RuntimeError, match="Expected one atom"):
        Dihedral.dihedralsToIndexes(tripeptides(), Dihedral({"name": "CB", "resid": 1, "chain": "A"}, *d.atoms[1:]))
    with pytest.raises(RuntimeError, match="Dictionary key"):
        Dihedral({"name": "N", "resno": 1}, {}, {}, {})
    with pytest.raises(TypeError, match="selection language"):
        Dihedral.proteinDihedrals(tripeptides(), "protein")


# ---------------------------------------------------------------------------------------------
# host logic: the emulation stands in for the library
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch, E):
    from moleculekit_amd import _lib
    calls = []

    def arr(addr, ctype, n):
        addr = getattr(addr, "value", addr)
        return np.ctypeslib.as_array((ctype * max(n, 1)).from_address(addr))[:n].copy() if addr else None

    class FakeLib:
        def mkamd_dihedrals_host(self, h, coords, N, F, box, box_frames, quads, D, mode, out):
            a = dict(N=N, F=F, D=D, mode=mode, box_frames=box_frames, quads=arr(quads, ctypes.c_uint32, 4 * D).reshape(D, 4),
                     coords=arr(coords, ctypes.c_float, N * 3 * F).reshape(N, 3, F), box=arr(box, ctypes.c_float, 3 * F))
            calls.append(a)
            got = E.dihedrals(a["coords"], a["quads"], None if a["box"] is None else a["box"].reshape(3, F), mode)
            np.ctypeslib.as_array((ctypes.c_float * got.size).from_address(getattr(out, "value", out)))[:] = got.reshape(-1)
            return 0

    class FakeCtx:
        _h = None

    monkeypatch.setattr(_lib, "load", lambda: FakeLib())
    monkeypatch.setattr(_lib, "default_context", lambda *a: FakeCtx())
    return calls


def test_metricdihedral_dialanine_through_the_host_path(fake):
    from moleculekit_amd.dihedral import MetricDihedral
    mol, sel, expected = C.dialanine()
    got = MetricDihedral(protsel=sel).project(mol)
    assert got.shape == (1, 4) and got.dtype == F32 and np.allclose(expected, got)      # the reference's own assertion
    assert fake[0]["mode"] == 3 and fake[0]["box"] is None and fake[0]["D"] == 2
    deg = MetricDihedral(protsel=sel, sincos=False).project(mol)
    assert deg.shape == (1, 2) and fake[1]["mode"] == 2
    assert np.allclose(np.sin(np.deg2rad(deg)), got[:, 0::2], atol=1e-3) and np.allclose(np.cos(np.deg2rad(deg)), got[:, 1::2], atol=1e-3)


def test_metricdihedral_real_projection_through_the_host_path(fake, real):
    from moleculekit_amd.dihedral import MetricDihedral
    mol, g, _, quads, t = real
    sub = types.SimpleNamespace(**{**vars(mol), "coords": np.ascontiguousarray(mol.coords[:, :, :64])})
    got = MetricDihedral(protsel=mol.protein).project(sub)
    assert got.shape == (64, 1104) and got.dtype == F32
    assert np.allclose(got, g["ref"][:64], atol=1e-3)
    restated = R.project(t[:64], True)
    e_ref = R.worst(restated, R.truth(t[:64])[2])
    assert float(np.abs(got - g["ref"][:64]).max()) <= float(np.abs(restated - g["ref"][:64]).max()) + e_ref
    assert np.array_equal(fake[0]["quads"], quads)


def test_host_argument_checks(fake):
    from moleculekit_amd.dihedral import dihedrals
    coords, quads = C.random_case(12, 5, 3, 2)
    assert dihedrals(coords, quads, out="terms").shape == (3, 5, 2) and dihedrals(coords, quads, out="radians").shape == (3, 5)
    assert dihedrals(coords, quads[0]).shape == (3, 2)
    assert dihedrals(coords, -1 - quads.astype(np.int64)).shape == (3, 10)          # negative indices count from the end
    assert dihedrals(coords, np.zeros((0, 4), int)).shape == (3, 0)
    with pytest.raises(ValueError, match="out must be"):
        dihedrals(coords, quads, out="angle")
    with pytest.raises(IndexError, match="out of range"):
        dihedrals(coords, quads + 12)
    with pytest.raises(ValueError, match=r"\(n_dihedrals, 4\)"):
        dihedrals(coords, quads[:, :3])
    with pytest.raises(TypeError, match="integer"):
        dihedrals(coords, quads.astype(float))
    with pytest.raises(ValueError, match="box must have shape"):
        dihedrals(coords, quads, box=np.zeros((3, 2), F32))
    with pytest.raises(ValueError, match="float32"):
        dihedrals(coords.astype(np.float64), quads)
    box = np.full((3, 3), 50, F32)
    dihedrals(coords, quads, box=box)
    assert np.array_equal(fake[-1]["box"].reshape(3, 3), box) and fake[-1]["box_frames"] == 3


def test_get_mapping(fake):
    from moleculekit_amd.dihedral import MetricDihedral
    mol, sel, _ = C.dialanine()
    m = MetricDihedral(protsel=sel).getMapping(mol)
    assert list(m["type"]) == ["dihedral"] * 4
    d = list(m["description"])
    assert d[0].startswith("Sine of angle of (ACE 1 C ") and d[1].startswith("Cosine of angle of (ACE 1 C ") and d[2].startswith("Sine of angle of (ALA 2 N ")
    assert list(m["atomIndexes"])[0] == list(m["atomIndexes"])[1] and len(list(m["atomIndexes"])[0]) == 4
    m = MetricDihedral(protsel=sel, sincos=False).getMapping(mol)
    assert [s.split(" (")[0] for s in m["description"]] == ["Angle of", "Angle of"]
    with pytest.raises(RuntimeError, match="Dihedral class"):
        MetricDihedral(dih=[[0, 1, 2, 3]])


def test_install_swaps_calc_of_a_stub_moleculekit(monkeypatch, fake):
    import moleculekit_amd.dihedral as Dm

    class Stub:
        def _calcDihedralAngles(self, mol, dihedrals, sincos=True):
            return "reference"

    mods = {"moleculekit": types.ModuleType("moleculekit"), "moleculekit.projections": types.ModuleType("moleculekit.projections"),
            "moleculekit.projections.metricdihedral": types.ModuleType("moleculekit.projections.metricdihedral")}
    mods["moleculekit.projections.metricdihedral"].MetricDihedral = Stub
    mods["moleculekit"].projections = mods["moleculekit.projections"]
    mods["moleculekit.projections"].metricdihedral = mods["moleculekit.projections.metricdihedral"]
    for name, m in mods.items():
        monkeypatch.setitem(sys.modules, name, m)
    mol, sel, expected = C.dialanine()
    quads = Dm.Dihedral.dihedralsToIndexes(mol, Dm.Dihedral.proteinDihedrals(mol, sel), sel)
    original = Dm.install()
    assert Dm.install() is original                                  # idempotent
    assert np.allclose(Stub()._calcDihedralAngles(mol, quads), expected)
    assert Stub()._calcDihedralAngles(mol, quads, sincos=False).shape == (1, 2)
    Dm.uninstall()
    Dm.uninstall()
    assert Stub()._calcDihedralAngles(mol, quads) == "reference"
