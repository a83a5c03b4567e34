"""CPU tier of the group moments (moleculekit_amd/moments.py): the kernels' bodies on the SIMT emulation over the
synthetic cases of tests/moments_cases.py under the conditions of the GPU tier, the launch plan, and the host logic of the four
projection classes (grouping, column order, dtypes, mapping rows, error messages, the pbc rule, the mass table, argument checks)."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emu_moments_build as E  # noqa: E402
import moments_cases as C  # noqa: E402
import moments_restatement as R  # noqa: E402

from moleculekit_amd import moments as M  # noqa: E402
from moleculekit_amd import _masses  # noqa: E402

FORMS = {"owned": (E.AVOID_SEGMENTED, "false>"), "segmented": (E.AVOID_OWNED, "k_mom_fold")}


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name in C.CASES:
        c = C.case(name)
        c.moved = R.apply_affine(c.xyz, c.affine) if c.affine is not None else c.xyz      # what the restatement is fed
        out[name] = c
    return out


# ------------------------------------------------------------------------------------------------
# the kernels on the emulation
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name", C.CASES)
def test_emulated_center_and_gyration(cases, name, form):
    c = cases[name]
    avoid, tag = FORMS[form]
    for out, restate in (("center", R.center), ("gyration", R.gyration)):
        got = E.group_moments(c.xyz, c.groups, c.weights, c.affine, out=out, avoid=avoid)
        assert tag in E.last_kernel(), E.last_kernel()
        C.assert_one_ulp(got, restate(c.moved, c.groups, c.weights), f"{name} {out} {form}")
        again = E.group_moments(c.xyz, c.groups, c.weights, c.affine, out=out, avoid=avoid)
        assert np.array_equal(got.view(np.int32), again.view(np.int32)), f"{name} {out} {form}: two runs differ"


def test_the_plan_segments_the_large_group_by_itself(cases):
    c = cases["large"]
    got = E.group_moments(c.xyz, c.groups, c.weights, c.affine, out="gyration")
    assert "k_mom_fold" in E.last_kernel() and E.plan(30000, 30000, 1)[1] > 8
    C.assert_one_ulp(got, R.gyration(c.moved, c.groups, c.weights), "large gyration")
    assert E.last_workspace() <= E.plan(30000, 30000, 1)[1] * 10 * 8 + 64
    # residues share a wave: 8 .. 32 lanes for groups of 4 .. 24 atoms, and nothing is segmented when the items fill the device
    assert E.plan(10, 24, 3000 * 2048)[:2] == (4, 1)
    assert E.plan(1, 1, 7)[:2] == (3, 1) and E.plan(1000, 1025, 2)[0] == 6


@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("name,pair", [("mixed", (5, 8)), ("mixed", (0, 1)), ("three", (0, 1)), ("residues", (3, 200))])
def test_emulated_spherical(cases, name, pair, form):
    c = cases[name]
    avoid, tag = FORMS[form]
    groups = [c.groups[pair[0]], c.groups[pair[1]]]
    got = E.group_moments(c.xyz, groups, None, c.affine, out="spherical", avoid=avoid)
    assert tag in E.last_kernel()
    C.assert_one_ulp(got, R.spherical(c.moved, *groups), f"{name} spherical {form}")


def test_emulated_spherical_of_coincident_centroids_is_nan_where_numpy_has_nan(cases):
    c = cases["three"]
    got = E.group_moments(c.xyz, [c.groups[1], c.groups[1]], None, None, out="spherical")
    want = R.spherical(c.xyz, c.groups[1], c.groups[1])
    assert np.all(got[:, 0] == 0) and np.all(np.isnan(got[:, 1])) and np.all(np.isnan(want[:, 1]))
    C.assert_one_ulp(got, want, "coincident spherical")


@pytest.mark.parametrize("given_ref", [False, True])
@pytest.mark.parametrize("name", ["mixed", "one", "three", "residues"])
def test_emulated_fluctuation(cases, name, given_ref):
    c = cases[name]
    atoms = np.concatenate(c.groups)
    offsets = np.r_[0, np.cumsum([g.size for g in c.groups])]
    groups = [np.arange(offsets[g], offsets[g + 1]) for g in range(len(c.groups))]
    ref = np.random.default_rng(7).normal(size=(atoms.size, 3)) * 3 + c.moved[0, atoms] if given_ref else None
    xmax = np.abs(c.moved).max()
    got = E.fluctuation(c.xyz, atoms, ref=ref, affine=c.affine)
    assert E.last_kernel() == ("" if given_ref else "mkamd::k_mom_mean + ") + "mkamd::k_mom_fluct_atoms"
    C.assert_fluct(got, R.fluctuation(c.moved, atoms, ref), c.F, 1, xmax, f"{name} fluct atoms")
    for form, (avoid, tag) in FORMS.items():
        got = E.fluctuation(c.xyz, atoms, ref=ref, groups=groups, affine=c.affine, avoid=avoid)
        assert tag in E.last_kernel() and E.last_kernel().startswith("mkamd::k_mom_mean") != given_ref
        C.assert_fluct(got, R.fluctuation(c.moved, atoms, ref, offsets), c.F, max(g.size for g in groups), xmax, f"{name} fluct groups {form}")
        again = E.fluctuation(c.xyz, atoms, ref=ref, groups=groups, affine=c.affine, avoid=avoid)
        assert np.array_equal(got.view(np.int64), again.view(np.int64))


def test_emulated_nan_stays_in_its_group(cases):
    c = cases["three"]
    xyz = c.xyz.copy()
    only = np.setdiff1d(c.groups[0], np.concatenate(c.groups[1:]))[0]
    xyz[5, only, 1] = np.nan
    for out, restate in (("center", R.center), ("gyration", R.gyration)):
        got = E.group_moments(xyz, c.groups, c.weights, None, out=out)
        with np.errstate(invalid="ignore"):
            want = restate(xyz, c.groups, c.weights)
        assert np.isnan(want).any()
        C.assert_one_ulp(got, want, f"nan {out}")


def test_emulated_calls_refuse_what_the_plan_cannot_run(cases):
    c = cases["three"]
    with pytest.raises(ValueError, match="two unweighted groups"):
        E.group_moments(c.xyz, c.groups, None, None, out="spherical")
    with pytest.raises(ValueError, match="two unweighted groups"):
        E.group_moments(c.xyz, c.groups[:2], c.weights[:71], None, out="spherical")
    with pytest.raises(ValueError, match="mode must be"):
        E.group_moments(c.xyz, c.groups, None, None, out=3)


# ------------------------------------------------------------------------------------------------
# the restatement against the reference-held data (what pins the yardstick of the GPU tier)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def held():
    """The reference's own tests of the four projections wrap the trajectory about "protein" first; neither filtered.psf nor
    filtered.pdb lists a bond, so every atom is a bonded group of its own there.  The frames (last 20, and frame 0) are wrapped with the
    wrap_box restatement and aligned with the float64 Kabsch, then the restatements are compared with the reference-held arrays and
    literals at the reference's own tolerances.

    NOT reproduced: metricsphericalcoordinate/res.npy.  The reference's test of that projection replaces the bonds by GUESSED ones
    (mol._guessBonds()) before it wraps; with the stored (empty) bond list the ligand's 23 atoms wrap one by one and the result is up
    to 29.8 Angstrom / 0.83 rad / 5.6 rad from the held array (the bound is 1e-4), so that array is stored but no test compares with it
    (DESIGN.md section 12); the spherical mode keeps its synthetic checks."""
    return C.reference_case()


def _frames(mol):
    return np.ascontiguousarray(mol.coords.transpose(2, 0, 1))


def test_wrap_box_restatement_moves_only_what_left_the_box(held):
    moved = np.flatnonzero((held.mol20.coords != held.raw20.coords).any(axis=(1, 2)))
    assert 0 < moved.size < 100 and not held.sel["protein"][moved].all()
    centre = held.raw20.coords[held.sel["protein"]].mean(axis=0)
    assert np.all(np.abs(held.mol20.coords - centre[None]) <= held.raw20.box[None] / 2 + 1e-3)
    # bonded groups: union-find over a chain and a pair -> starts 0, 3, 4, 6 (+ n)
    assert R.bonded_groups(np.array([[1, 2], [0, 1], [4, 5]]), 7).tolist() == [0, 3, 4, 6, 7]
    # a bonded pair moves together or not at all: its running-mean centre decides
    x = np.array([[[11.0]] * 3, [[13.5]] * 3, [[1.0]] * 3], np.float32)      # centre 12.25: 11.25 from atom 2, the half box is 10
    out = R.wrap_box(x, np.full((3, 1), 20, np.float32), [2], np.array([[0, 1]]))
    assert out[:2, 0, 0].tolist() == [-9.0, -6.5] and out[2, 0, 0] == 1.0
    alone = R.wrap_box(x, np.full((3, 1), 20, np.float32), [2], np.zeros((0, 2), np.int64))          # unbonded: atom 0 (10.0 away) stays
    assert alone[:2, 0, 0].tolist() == [11.0, -6.5]


def test_restated_gyration_reproduces_the_reference_literals(held):
    prot = np.flatnonzero(held.sel["protein"])
    got = R.gyration(_frames(held.mol20), [prot], held.g["masses"][prot])[:, 0, 0]
    assert np.all(np.abs(got - held.g["gyration_last20"]) < 1e-3)


def test_restated_coordinates_reproduce_the_reference_literals(held):
    ca = np.flatnonzero(held.sel["ca"])
    last = _frames(held.mol20)[-1:]
    assert np.all(np.abs(R.center(last, [[a] for a in ca])[0, -20:] - held.g["coord_last20"]) < 1e-3)
    aligned = R.kabsch_align(last, ca, held.raw0.coords[ca, :, 0])           # (the refmol of that test is frame 0 as read, not wrapped)
    assert np.all(np.abs(R.center(aligned, [[a] for a in ca])[0, -20:] - held.g["coord_align_last20"]) < 1e-3)


def test_restated_fluctuations_reproduce_the_reference_arrays(held):
    ca, noh = np.flatnonzero(held.sel["ca"]), np.flatnonzero(held.sel["noh"])
    frames, ref0 = _frames(held.mol20), held.ref0.coords[:, :, 0]
    offsets = C.residue_offsets(held.mol20.resid, noh)
    on_ref = R.kabsch_align(frames, ca, ref0[ca])
    ref_self = R.kabsch_align(ref0[None], ca, ref0[ca])[0].astype(np.float64)      # the refmol aligned onto itself, float32 positions
    assert np.allclose(R.fluctuation(on_ref, ca, ref_self[ca]), held.g["fluct_atom_ref"], atol=1e-3)
    assert np.allclose(R.fluctuation(on_ref, noh, ref_self[noh], offsets), held.g["fluct_residue_ref"], atol=1e-3)
    on_first = R.kabsch_align(frames, ca, frames[0, ca])
    assert np.allclose(R.fluctuation(on_first, ca), held.g["fluct_atom_mean"], atol=1e-3)
    assert np.allclose(R.fluctuation(on_first, noh, None, offsets), held.g["fluct_residue_mean"], atol=1e-3)


def test_fixture_selections(held):
    s = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sasa_cases.npz"))
    assert np.array_equal(held.sel["protein"], s["protein"])
    assert np.array_equal(held.sel["ca"], s["protein"] & (s["name"] == "CA")) and held.sel["ca"].sum() == 277
    assert np.array_equal(held.sel["noh"], s["protein"] & (s["element"] != "H"))
    assert np.array_equal(held.sel["mol"], s["resname"] == "MOL") and held.sel["within8"][s["resid"] == 98].all()
    assert held.g["bonds"].shape == (0, 2) and held.g["masses"].shape == (4507,)


# ------------------------------------------------------------------------------------------------
# host logic
# ------------------------------------------------------------------------------------------------
def _mol(box=None):
    """12 atoms: resid VALUES 5 5 5 7 7 5 5 9 9 9 7 7 -- the value 5 and the value 7 come back after other residues"""
    resid = np.array([5, 5, 5, 7, 7, 5, 5, 9, 9, 9, 7, 7])
    return types.SimpleNamespace(
        coords=np.random.default_rng(0).normal(size=(12, 3, 4)).astype(np.float32), numFrames=4, resid=resid, box=box,
        resname=np.array(["ALA"] * 3 + ["GLY"] * 2 + ["SER"] * 2 + ["MOL"] * 3 + ["LYS"] * 2), name=np.array(["N", "CA", "C"] * 4),
        element=np.array(["N", "C", "C", "N", "C", "C", "O", "Cl", "H", "S", "C", "C"]), masses=np.zeros(12, np.float32))


def test_coordinate_groups_by_the_value_of_resid_and_fluctuation_by_sequence():
    mol = _mol()
    idx, groups = M.MetricCoordinate(np.arange(1, 12), groupsel="residue")._groups(mol)
    assert [g.tolist() for g in groups] == [[1, 2, 5, 6], [3, 4, 10, 11], [7, 8, 9]]          # np.unique of the values
    seq = M.MetricFluctuation("all", trajalnsel="all", mode="residue")._residues(mol, np.arange(12))
    assert seq.tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 3, 3, 4, 4]                             # sequenceID: five residues
    assert M.MetricCoordinate("all", groupsel="all")._groups(mol)[1][0].tolist() == list(range(12))
    with pytest.raises(RuntimeError, match="Invalid groupsel option"):
        M.MetricCoordinate("all", groupsel="chain")._groups(mol)


def test_mappings_follow_the_reference():
    mol = _mol()
    m = M.MetricCoordinate(np.array([0, 4]), pbc=False).getMapping(mol)
    assert list(m["description"]) == ["X coordinate of ALA 5 N", "X coordinate of GLY 7 CA", "Y coordinate of ALA 5 N",
                                      "Y coordinate of GLY 7 CA", "Z coordinate of ALA 5 N", "Z coordinate of GLY 7 CA"]
    assert list(m["type"]) == ["coordinate"] * 6 and [int(i) for i in m["atomIndexes"]] == [0, 4, 0, 4, 0, 4]
    m = M.MetricCoordinate("all", groupsel="residue", groupreduce="centroid").getMapping(mol)
    assert list(m["description"]) == [f"{c} centroid coordinate of group" for c in "XYZ" for _ in range(3)]
    m = M.MetricGyration("all").getMapping(mol)
    assert list(m["type"]) == ["rog"] * 4 and list(m["description"]) == ["Radius of gyration", "x component", "y component", "z component"]
    m = M.MetricFluctuation(np.arange(2, 8), trajalnsel="all", mode="residue").getMapping(mol)
    assert list(m["description"]) == ["Mean fluctuation of ALA 5", "Mean fluctuation of GLY 7", "Mean fluctuation of SER 5", "Mean fluctuation of MOL 9"]
    assert [int(i) for i in m["atomIndexes"]] == [2, 3, 5, 7]
    m = M.MetricFluctuation(np.array([1, 9]), trajalnsel="all").getMapping(mol)
    assert list(m["description"]) == ["Fluctuation of ALA 5 CA", "Fluctuation of MOL 9 N"]
    m = M.MetricSphericalCoordinate(mol, np.array([0, 1]), np.array([7]), trajalnsel="all").getMapping(mol)
    assert list(m["type"]) == ["r", "theta", "phi"] and [a.tolist() for a in m["atomIndexes"][0]] == [[0, 1], [7]]


def test_the_reference_messages_for_empty_selections_and_bad_arguments():
    mol = _mol()
    none = np.zeros(12, bool)
    with pytest.raises(ValueError, match="Atom selection cannot be None"):
        M.MetricCoordinate(None)
    with pytest.raises(ValueError, match="Atom selection cannot be None"):
        M.MetricGyration(None)
    with pytest.raises(RuntimeError, match="Atom selection resulted in 0 atoms."):
        M.MetricCoordinate(none, pbc=False).project(mol)
    with pytest.raises(RuntimeError, match="Atom selection resulted in 0 atoms."):
        M.MetricGyration(none, pbc=False).project(mol)
    with pytest.raises(RuntimeError, match="Alignment selection resulted in 0 atoms."):
        M.MetricCoordinate("all", trajalnsel=none, pbc=False).project(mol)
    with pytest.raises(RuntimeError, match="Atom selection for `targetcom` resulted in 0 atoms."):
        M.MetricSphericalCoordinate(mol, none, "all", trajalnsel="all", pbc=False).project(mol)
    with pytest.raises(RuntimeError, match="Atom selection for `refcom` resulted in 0 atoms."):
        M.MetricSphericalCoordinate(mol, "all", none, trajalnsel="all", pbc=False).project(mol)
    with pytest.raises(RuntimeError, match="Invalid mode"):
        M.MetricFluctuation("all", trajalnsel="all", mode="chain", pbc=False).project(mol)
    with pytest.raises(TypeError, match="no selection language"):
        M.MetricFluctuation("all", pbc=False).project(mol)                     # the reference's default trajalnsel is a string
    with pytest.raises(TypeError, match="no selection language"):
        M.MetricCoordinate("protein", pbc=False).project(mol)


def test_gyration_refuses_a_selection_without_mass(monkeypatch):
    monkeypatch.setitem(M.ATOMIC_MASSES, "X0", 0.0)
    with pytest.raises(RuntimeError, match="The molecule selection has 0 total mass"):
        M.MetricGyration("all")._masses(types.SimpleNamespace(masses=np.zeros(2), element=np.array(["X0", "X0"])), np.arange(2))


def test_the_pbc_rule():
    box = np.full((3, 4), 60, np.float32)
    for metric in (M.MetricCoordinate("all"), M.MetricGyration("all"), M.MetricFluctuation("all", trajalnsel="all"),
                   M.MetricSphericalCoordinate(_mol(), np.array([0]), np.array([1]), trajalnsel="all")):
        assert metric._pbc is True                                              # the reference's default stays
        with pytest.raises(NotImplementedError, match="wrap the molecule first .* or pass pbc=False"):
            metric.project(_mol(box))
    # a missing or all-zero box: pbc=True is the no-op it is in the reference (the call then gets as far as the library)
    M._check_pbc(_mol(None), True)
    M._check_pbc(_mol(np.zeros((3, 4), np.float32)), True)
    M._check_pbc(_mol(box), False)


def test_masses_table():
    assert set(_masses.CHECKED) <= set(_masses.ATOMIC_MASSES)
    with pytest.raises(KeyError):
        _masses.masses_for(["Xx"])
    g = C.fixture()
    recorded = dict(zip(g["mass_elements"].tolist(), g["mass_values"].tolist()))
    assert sorted(_masses.CHECKED) == sorted(recorded), "CHECKED lists the fixture's elements"
    for el in _masses.CHECKED:
        assert np.float32(_masses.ATOMIC_MASSES[el]) == np.float32(recorded[el]), el
    # groupreduce="com" takes element masses as float32; MetricGyration falls back to them where a mass is 0
    mol = _mol()
    assert M._element_masses(mol, np.array([0, 7])).tolist() == [14.0067, 35.453]
    assert M.MetricGyration("all")._masses(mol, np.arange(3)).tolist() == [14.0067, 12.0107, 12.0107]
    mol.masses = np.arange(1, 13, dtype=np.float32)
    assert M.MetricGyration("all")._masses(mol, np.arange(3)).tolist() == [1, 2, 3]


def test_argument_validation():
    assert M._csr([[3, 1], [2]], 5)[1].tolist() == [0, 2, 3]
    assert M._csr((np.array([3, 1, 2]), np.array([0, 2, 3])), 5)[0].tolist() == [3, 1, 2]
    assert M._csr([[-1]], 5)[0].tolist() == [4]
    with pytest.raises(ValueError, match="an empty group"):
        M._csr([[1], []], 5)
    with pytest.raises(IndexError, match="out of range"):
        M._csr([[5]], 5)
    with pytest.raises(TypeError, match="integer atom indices"):
        M._csr([[0.5]], 5)
    with pytest.raises(ValueError, match="offsets must run from 0"):
        M._csr((np.arange(3), np.array([1, 3])), 5)
    with pytest.raises(ValueError, match="one entry per group atom"):
        M._weights(np.ones(2), 3)
    with pytest.raises(ValueError, match="out must be one of"):
        M.group_moments(np.zeros((2, 3, 1), np.float32), [[0]], out="fluct")
    with pytest.raises(ValueError, match="exactly two unweighted groups"):
        M.group_moments(np.zeros((2, 3, 1), np.float32), [[0]], out="spherical")
    with pytest.raises(ValueError, match="expected float32"):
        M.group_moments(np.zeros((2, 3, 1)), [[0]])
    with pytest.raises(ValueError, match="contiguous groups"):
        M._fluct_groups([[1], [0]], 2)
    assert M._fluct_groups([[0, 1], [2]], 3).tolist() == [0, 2, 3]
    with pytest.raises(ValueError, match=r"ref must have shape \(2, 3\)"):
        M.fluctuation(np.zeros((2, 3, 1), np.float32), [0, 1], ref=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="alnsel picks 1 atoms"):
        M.group_moments(np.zeros((2, 3, 1), np.float32), [[0]], align=([0], np.zeros((2, 3))))
    with pytest.raises(TypeError, match="CUDA tensor"):
        M.group_moments_trajectory(np.zeros((1, 2, 3), np.float32), [[0]])
    with pytest.raises(TypeError, match="CUDA tensor"):
        M.fluctuation_trajectory(np.zeros((1, 2, 3), np.float32), [0])


def test_no_cpu_path():
    from moleculekit_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible; the refusal path is exercised on CPU-only boxes")
    coords = np.zeros((3, 3, 2), np.float32)
    with pytest.raises(RuntimeError):
        M.group_moments(coords, [[0, 1]])
    with pytest.raises(RuntimeError):
        M.fluctuation(coords, [0, 1])
    with pytest.raises(RuntimeError):
        M.MetricGyration("all", pbc=False).project(_mol())


# ------------------------------------------------------------------------------------------------
# install(): the four hook bodies run against a stub moleculekit, the library replaced by the emulated kernels
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def emulated_library(monkeypatch):
    """moments.group_moments / moments.fluctuation on the emulation: float64 Kabsch for the alignment, the emulated kernels after it"""
    def to_frames(coords, align):
        frames = np.ascontiguousarray(np.asarray(coords, np.float32).transpose(2, 0, 1))
        return frames if align is None else R.kabsch_align(frames, np.asarray(align[0]), align[1])

    def group_moments(coords, groups, *, weights=None, align=None, out="center", ctx=None):
        atoms, offsets = M._csr(groups, coords.shape[0])
        groups = [atoms[offsets[g]:offsets[g + 1]] for g in range(offsets.size - 1)]
        return E.group_moments(to_frames(coords, align), groups, weights, None, out=out)

    def fluctuation(coords, atoms, *, ref=None, groups=None, align=None, ctx=None):
        offsets = M._fluct_groups(groups, len(atoms))
        runs = None if offsets is None else [np.arange(offsets[g], offsets[g + 1]) for g in range(offsets.size - 1)]
        return E.fluctuation(to_frames(coords, align), atoms, ref=ref, groups=runs)

    monkeypatch.setattr(M, "group_moments", group_moments)
    monkeypatch.setattr(M, "fluctuation", fluctuation)


class _StubMol(types.SimpleNamespace):
    wrapped = 0

    def copy(self):
        return _StubMol(**{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in vars(self).items()})

    def wrap(self, sel):
        self.wrapped += 1
        self.wrapsel = sel

    def atomselect(self, sel):
        if isinstance(sel, str) and sel == "all":
            return np.ones(self.coords.shape[0], bool)
        a = np.asarray(sel)
        if a.dtype == bool:
            return a
        m = np.zeros(self.coords.shape[0], bool)
        m[a] = True
        return m


class _StubProjection:
    """the reference's Projection base as far as the hooks use it"""

    def __init__(self):
        self._cache = {}

    def _getMolProp(self, mol, prop):
        return self._cache[prop] if prop in self._cache else self._calculateMolProp(mol, [prop])[prop]


def _stub_moleculekit(monkeypatch):
    class Coordinate(_StubProjection):
        def __init__(self, atomsel, refmol=None, trajalnsel=None, refalnsel=None, centersel="all", groupsel=None, groupreduce="com", pbc=True):
            super().__init__()
            self._atomsel, self._refmol, self._trajalnsel, self._centersel = atomsel, refmol, trajalnsel, centersel
            self._groupsel, self._groupreduce, self._pbc = groupsel, groupreduce, pbc
            if refmol is not None:
                self._refalnsel = refalnsel if refalnsel is not None else trajalnsel
                self._cache["refalnsel"] = refmol.atomselect(self._refalnsel)

        def _calculateMolProp(self, mol, props):
            named = {"atomsel": self._atomsel, "trajalnsel": self._trajalnsel, "centersel": self._centersel, "targetcom": getattr(self, "_targetcom", None),
                     "refcom": getattr(self, "_refcom", None)}
            out = {p: (None if named.get(p) is None else mol.atomselect(named[p])) for p in props if p != "masses"}
            if "masses" in props:
                out["masses"] = mol.masses[mol.atomselect(self._atomsel)]
            return out

        def project(self, mol):
            return "reference"

    class Gyration(Coordinate):
        def project(self, mol):
            return "reference"

    class Fluctuation(Coordinate):
        def __init__(self, atomsel, refmol=None, trajalnsel=None, refalnsel=None, centersel="all", pbc=True, mode="atom"):
            super().__init__(atomsel, refmol, trajalnsel, refalnsel, centersel, pbc=pbc)
            self._mode = mode

        def project(self, mol):
            return "reference"

    class Spherical(Coordinate):
        def __init__(self, refmol, targetcom, refcom, trajalnsel, refalnsel=None, centersel="all", pbc=True):
            super().__init__("all", None, trajalnsel, None, centersel, pbc=pbc)
            self._refmol, self._targetcom, self._refcom = refmol, targetcom, refcom
            self._refalnsel = refmol.atomselect(trajalnsel if refalnsel is None else refalnsel)

        def project(self, mol):
            return "reference"

    mods = {"moleculekit": types.ModuleType("moleculekit"), "moleculekit.projections": types.ModuleType("moleculekit.projections"),
            "moleculekit.util": types.ModuleType("moleculekit.util"), "moleculekit.periodictable": types.ModuleType("moleculekit.periodictable")}
    mods["moleculekit.util"].sequenceID = lambda resid: np.cumsum(np.r_[0, np.asarray(resid)[1:] != np.asarray(resid)[:-1]])
    mods["moleculekit.periodictable"].periodictable = {e: types.SimpleNamespace(mass=m) for e, m in _masses.ATOMIC_MASSES.items()}
    for short, cls_name, cls in (("metriccoordinate", "MetricCoordinate", Coordinate), ("metricgyration", "MetricGyration", Gyration),
                                 ("metricfluctuation", "MetricFluctuation", Fluctuation),
                                 ("metricsphericalcoordinate", "MetricSphericalCoordinate", Spherical)):
        m = types.ModuleType("moleculekit.projections." + short)
        setattr(m, cls_name, cls)
        mods["moleculekit.projections." + short] = m
    for name, m in mods.items():
        monkeypatch.setitem(sys.modules, name, m)
    return Coordinate, Gyration, Fluctuation, Spherical


def test_install_runs_the_four_hooks_of_a_stub_moleculekit(monkeypatch, emulated_library):
    Coordinate, Gyration, Fluctuation, Spherical = _stub_moleculekit(monkeypatch)
    rng = np.random.default_rng(5)
    base = rng.normal(size=(12, 3)) * 5
    coords = (base[:, :, None] + 0.3 * rng.normal(size=(12, 3, 4))).astype(np.float32)
    mol = _StubMol(coords=coords, box=np.zeros((3, 4), np.float32), resid=_mol().resid, element=_mol().element,
                   masses=np.arange(1, 13, dtype=np.float32), numFrames=4)
    # a refmol whose atoms are in ANOTHER order: the alignment pairs trajalnsel [2, 5, 7, 9] with refalnsel [3, 5, 7, 10], index arrays
    refmol = _StubMol(coords=np.ascontiguousarray(coords[[0, 1, 3, 2, 4, 5, 6, 7, 8, 10, 9, 11], :, :1]), box=np.zeros((3, 1), np.float32),
                      resid=_mol().resid, element=_mol().element, masses=np.zeros(12, np.float32), numFrames=1)
    traj_aln, ref_aln = np.array([2, 5, 7, 9]), np.array([3, 5, 7, 10])
    frames = np.ascontiguousarray(coords.transpose(2, 0, 1))
    moved = R.kabsch_align(frames, traj_aln, refmol.coords[ref_aln, :, 0])
    saved = M.install()
    try:
        assert M.install() == saved and all(s(None, None) == "reference" for s in saved)          # idempotent; the originals are returned
        sel = np.array([1, 4, 6, 8])
        got = Coordinate(sel, refmol, traj_aln, ref_aln, pbc=False).project(mol)
        C.assert_one_ulp(got, R.center(moved, [[a] for a in sel]), "hook: coordinate on an index refalnsel")
        got = Coordinate(np.arange(12), None, None, groupsel="residue", groupreduce="com", pbc=True).project(mol)
        groups = [np.flatnonzero(mol.resid == u) for u in np.unique(mol.resid)]
        w = np.array([_masses.ATOMIC_MASSES[e] for e in mol.element[np.concatenate(groups)]], np.float32)
        C.assert_one_ulp(got, R.center(frames, groups, w), "hook: residue centres of mass")
        got = Gyration(sel, refmol, traj_aln, ref_aln, pbc=False).project(mol)
        C.assert_one_ulp(got, R.gyration(moved, [sel], mol.masses[sel])[:, 0], "hook: gyration")
        got = Spherical(refmol, np.array([0, 1]), np.array([6, 8, 11]), traj_aln, ref_aln, pbc=False).project(mol)
        C.assert_one_ulp(got, R.spherical(moved, [0, 1], [6, 8, 11]), "hook: spherical")
        got = Fluctuation(np.arange(2, 9), None, traj_aln, mode="residue", pbc=False).project(mol)
        on_first = R.kabsch_align(frames, traj_aln, frames[0, traj_aln])
        want = R.fluctuation(on_first, np.arange(2, 9), None, C.residue_offsets(mol.resid, np.arange(2, 9)))
        assert got.dtype == np.float64 and np.allclose(got, want, rtol=0, atol=1e-9)
    finally:
        M.uninstall()
    assert Coordinate(sel, pbc=False).project(mol) == "reference"
