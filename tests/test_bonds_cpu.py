"""CPU tier: the bond guesser.

The numpy restatement of the reference's search (tests/bonds_restatement.py) is held against what the compiled reference returned on
the golden cases (tests/golden/bond_cases.npz); the product's kernels and launch plan, compiled on the SIMT emulation
(tests/emu/emu_bonds.cpp), are held against the restatement on every case, with a thread per owner, with a wave per owner and with
the plan's own choice.  Then the Python layer: the radii, the grid, the errors, the empty results, the wrap path with guessed bonds,
``install`` / ``uninstall``.

Pass criterion (the issue's): equal arrays, rows in order.  There is no tolerance anywhere.
"""
import logging
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bonds_cases as C  # noqa: E402
import bonds_restatement as R  # noqa: E402

import moleculekit_amd.bonds as B  # noqa: E402
import moleculekit_amd.wrap as W  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "bond_cases.npz")
PLANS = {"unforced": 0, "wave": 1, "thread": 2}          # emu_bonds_build.AVOID_THREAD forces the wave kernels and the other way round


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def emu():
    import emu_bonds_build
    emu_bonds_build.build()
    return emu_bonds_build


@pytest.fixture
def emulated_library(emu, monkeypatch):
    """bonds.py on the emulated kernels instead of the device"""
    def host_call(coords, radii, flags, grid_cutoff, max_boxes, cutoff_incr, ctx=None):
        try:
            pairs, grid, _ = emu.guess_bonds(coords, grid_cutoff, flags, radii, max_boxes, cutoff_incr)
        except ValueError as e:
            raise B._library_error(e, grid_cutoff) from None
        return pairs.astype(np.int32), grid

    monkeypatch.setattr(B, "_host_call", host_call)


def same_list(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.ndim == 2 and got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64)), f"{what}: the lists differ"


def test_the_cases_are_the_cases_they_are_meant_to_be():
    C.check()


@pytest.mark.parametrize("name", C.GOLDEN)
def test_restatement_gives_the_references_list(golden, name):
    c = C.case(name)
    for key in ("coords", "radii", "is_h"):                     # the inputs the reference saw are the inputs generated here
        assert np.array_equal(golden[f"{name}/{key}"], c[key]) and golden[f"{name}/{key}"].dtype == c[key].dtype, key
    assert float(golden[f"{name}/grid_cutoff"]) == c["grid_cutoff"]
    same_list(C.restated(name)[0], golden[f"{name}/pairs"], name)
    if "element" in c:
        same_list(R.guess(c["coords"], c["element"], c["name"]), golden[f"{name}/pairs"], name + " through guess")


def test_the_fixtures_bonds_are_the_references(golden):
    same_list(golden["3ptb/pairs"], np.load(os.path.join(HERE, "golden", "channels_3ptb.npz"))["bonds"], "3ptb")


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", C.GOLDEN)
def test_emulated_kernels_give_the_restatements_list(emu, name, plan):
    c = C.case(name)
    want, det = C.restated(name)
    pairs, grid, max_occ = emu.guess_bonds(c["coords"], c["grid_cutoff"], c["is_h"], c["radii"], avoid=PLANS[plan])
    same_list(pairs, want, f"{name} / {plan}")
    assert grid == det["grid"] and max_occ == det["max_occ"]
    crowded = det["max_occ"] >= 64
    expected = {"unforced": emu.WAVE_KERNEL if crowded else emu.THREAD_KERNEL, "wave": emu.WAVE_KERNEL, "thread": emu.THREAD_KERNEL}[plan]
    assert emu.last_kernel() == expected
    # two words a box, seven (and two) an atom, the scans' chunk sums and the status words: the list apart
    boxes, n = grid[0] * grid[1] * grid[2], len(c["coords"])
    assert emu.last_workspace() <= 8 * boxes + 28 * n + 8 + 64 + 48 + 16


def test_the_crowded_case_takes_the_wave_kernels_unforced(emu):
    assert C.restated("crowded")[1]["max_occ"] >= 64 and max(C.restated(n)[1]["max_occ"] for n in C.GOLDEN if n != "crowded") < 64
    c = C.case("crowded")
    emu.guess_bonds(c["coords"], c["grid_cutoff"], c["is_h"], c["radii"])
    assert emu.last_kernel() == emu.WAVE_KERNEL


@pytest.mark.parametrize("plan", list(PLANS))
def test_over_cap_returns_the_status_not_a_list(emu, plan):
    c = C.over_cap()
    with pytest.raises(ValueError, match=r"crowded box: box 0 .* holds 4097 atoms, more than the 4096"):
        emu.guess_bonds(c["coords"], c["grid_cutoff"], c["is_h"], c["radii"], avoid=PLANS[plan])
    # one atom fewer is inside the cap: no bond among coincident atoms
    pairs, grid, max_occ = emu.guess_bonds(c["coords"][:-1], c["grid_cutoff"], c["is_h"][:-1], c["radii"][:-1], avoid=PLANS[plan])
    assert len(pairs) == 0 and grid[:3] == (1, 1, 1) and max_occ == C.BOX_CAP


def test_the_pipeline_refuses_bad_arguments(emu):
    c = C.case("one_box")
    bad = c["coords"].copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite coordinates"):
        emu.guess_bonds(bad, c["grid_cutoff"], c["is_h"], c["radii"])
    bad[3, 1] = -np.inf
    with pytest.raises(ValueError, match="non-finite coordinates"):
        emu.guess_bonds(bad, c["grid_cutoff"], c["is_h"], c["radii"])
    for cutoff in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="grid_cutoff"):
            emu.guess_bonds(c["coords"], cutoff, c["is_h"], c["radii"])
    with pytest.raises(ValueError, match="max_boxes"):
        emu.guess_bonds(c["coords"], c["grid_cutoff"], c["is_h"], c["radii"], max_boxes=0.5)
    with pytest.raises(ValueError, match="max_boxes"):
        emu.guess_bonds(c["coords"], c["grid_cutoff"], c["is_h"], c["radii"], max_boxes=2.0 ** 28 + 1)
    with pytest.raises(ValueError, match="cutoff_incr"):
        emu.guess_bonds(c["coords"], c["grid_cutoff"], c["is_h"], c["radii"], cutoff_incr=1.0)
    pairs, _, _ = emu.guess_bonds(c["coords"][:1], c["grid_cutoff"], c["is_h"][:1], c["radii"][:1])
    assert pairs.shape == (0, 2)
    pairs, _, _ = emu.guess_bonds(c["coords"][:0], c["grid_cutoff"], c["is_h"][:0], c["radii"][:0])
    assert pairs.shape == (0, 2)


# ------------------------------------------------------------------------------------------------
# radii and grid
# ------------------------------------------------------------------------------------------------
def test_bond_radii_rules():
    element = np.array(["C", "Cl", "CL", "CL", "", "Xx", "H", "ZN", "Zn", "X", "X", "X"])
    name = np.array(["CA", "CL1", "CL1", "hl1", "o2", "Q1", "H1", "ZN", "ZN", "f1", "S1", "n"])
    r = B.bond_radii(element, name)
    assert r.dtype == np.float32 and r.shape == (12,)
    want = [1.7, 2.27, 1.5, 1.0, 1.3, 1.5, 1.0, 1.5, 1.39, 1.2, 1.9, 1.4]      # table; name rule for "CL" (C) and "hl1" (H); default 1.5
    assert np.array_equal(r, np.array(want, np.float32))
    assert np.array_equal(r, R.radii_of(element, name))
    c = C.case("3ptb")
    assert np.array_equal(B.bond_radii(c["element"], c["name"]), c["radii"])


@pytest.mark.parametrize("span", [1e4, 1e5, 1e6, 1e7])
def test_bond_grid_on_the_unwrapped_spans(emu, span):
    c = C.case("unwrapped_1e%d" % round(np.log10(span)))
    mn, mx = c["coords"].min(axis=0), c["coords"].max(axis=0)
    want = C.restated("unwrapped_1e%d" % round(np.log10(span)))[1]["grid"]
    assert B.bond_grid(mn, mx, 2.04) == want == emu.bond_grid(mn, mx, 2.04)
    assert want[0] * want[1] * want[2] <= 4e6 and want[3] > 2.04
    # one step back the grid was too large: the loop stopped where the reference's stops
    back = R.grid_of(mn, mx, want[3] / 1.26, max_boxes=float("inf"))
    assert back[0] * back[1] * back[2] > 4e6


def test_bond_grid_at_the_box_budget(emu):
    mn, mx = np.zeros(3, np.float32), np.array([99.5, 99.5, 39.5], np.float32)         # 100 x 100 x 40 boxes of side 1
    assert B.bond_grid(mn, mx, 1.0, max_boxes=400000) == (100, 100, 40, 1.0) == emu.bond_grid(mn, mx, 1.0, max_boxes=400000)
    for grid in (B.bond_grid(mn, mx, 1.0, max_boxes=399999), emu.bond_grid(mn, mx, 1.0, max_boxes=399999)):
        assert grid == R.grid_of(mn, mx, 1.0, max_boxes=399999) and grid[3] == 1.26 and grid[0] * grid[1] * grid[2] <= 399999
    assert B.bond_grid(mn, mx, 1.0) == (100, 100, 40, 1.0)
    for cutoff in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="grid_cutoff"):
            B.bond_grid(mn, mx, cutoff)
        with pytest.raises(ValueError, match="grid_cutoff"):
            emu.bond_grid(mn, mx, cutoff)


# ------------------------------------------------------------------------------------------------
# the reference's two functions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pair_edges", "3ptb_shuffled", "unwrapped_1e6"])
def test_the_references_functions_on_the_emulated_library(emulated_library, golden, caplog, name):
    c = C.case(name)
    with caplog.at_level(logging.WARNING, logger="moleculekit_amd.bonds"):
        pairs = B.bond_grid_search(c["coords"], c["grid_cutoff"], c["is_h"], c["radii"])
    assert pairs.dtype == np.uint32
    same_list(pairs, golden[f"{name}/pairs"], name)
    g = C.restated(name)[1]["grid"]
    assert ("unwrapped simulation" in caplog.text) == (g[0] * g[1] * g[2] > 1e6) == name.startswith("unwrapped")
    if "element" in c:
        pairs = B.guess_bonds(C.as_mol(c, frame=2, frames=4))          # frame mol.frame, and no other
        assert pairs.dtype == np.uint32
        same_list(pairs, golden[f"{name}/pairs"], name + " through guess_bonds")


def test_errors_and_empty_results(emulated_library):
    c = C.case("one_box")
    bad = c["coords"].copy()
    bad[0, 0] = np.inf
    with pytest.raises(ValueError, match="finite"):
        B.bond_grid_search(bad, c["grid_cutoff"], c["is_h"], c["radii"])
    with pytest.raises(ValueError, match="grid_cutoff"):
        B.bond_grid_search(c["coords"], 0.0, c["is_h"], c["radii"])
    with pytest.raises(ValueError, match="grid_cutoff"):
        B.bond_grid_search(c["coords"], float("nan"), c["is_h"], c["radii"])
    with pytest.raises(RuntimeError, match=r"Frame 3 \(defined in mol.frame\) is out of range"):
        B.guess_bonds(C.as_mol(c, frame=3, frames=3))
    one = types.SimpleNamespace(numAtoms=1, frame=0, numFrames=1, coords=np.zeros((1, 3, 1), np.float32), element=np.array(["C"]), name=np.array(["CA"]))
    none = types.SimpleNamespace(numAtoms=0, frame=5, numFrames=0, coords=np.zeros((0, 3, 0), np.float32), element=np.array([]), name=np.array([]))
    for mol in (one, none):
        out = B.guess_bonds(mol)
        assert out.shape == (0, 2) and out.dtype == np.uint32
    far = np.array([[0, 0, 0], [5, 0, 0], [0, 7, 0]], np.float32)          # a search that finds nothing
    out = B.bond_grid_search(far, 2.04, np.zeros(3, np.uint32), np.full(3, 1.7, np.float32))
    assert out.shape == (0, 2) and out.dtype == np.uint32
    over = C.over_cap()
    with pytest.raises(ValueError, match="crowded box.*holds 4097 atoms"):
        B.bond_grid_search(over["coords"], over["grid_cutoff"], over["is_h"], over["radii"])


def test_tensor_entry_refuses_host_arrays():
    c = C.case("one_box")
    with pytest.raises(TypeError, match="CUDA tensor"):
        B.guess_bonds_tensor(c["coords"], c["radii"], c["is_h"])


# ------------------------------------------------------------------------------------------------
# wrap with guessed bonds; the hooks
# ------------------------------------------------------------------------------------------------
def _water_mol(frames=2):
    c = C.case("water")
    n = 30                                                               # ten waters: contiguous groups of three
    coords = np.repeat(c["coords"][:n, :, None], frames, axis=2).copy()
    return types.SimpleNamespace(coords=coords, box=np.full((3, frames), 40.0, np.float32), boxangles=np.full((3, frames), 90.0, np.float32),
                                 bonds=np.zeros((0, 2), np.uint32), numAtoms=n, frame=1, numFrames=frames, element=c["element"][:n], name=c["name"][:n])


def test_wrap_molecule_hands_wrap_the_groups_of_file_and_guessed_bonds(emulated_library, monkeypatch):
    seen = {}

    def fake_wrap(coords, box, groups, centersel=None, center=None, ctx=None):
        seen.update(groups=np.asarray(groups).tolist())
        return coords

    monkeypatch.setattr(W, "wrap", fake_wrap)
    mol = _water_mol()
    with pytest.raises(NotImplementedError, match="guessBonds=True: this package does not guess bonds; pass a molecule whose bonds are read from a topology"):
        W.wrap_molecule(mol, guessBonds=True)
    W.wrap_molecule(mol, guessBonds=True, guess_on_device=True)
    assert seen["groups"] == list(range(0, 31, 3))                      # the waters
    guessed = R.guess(mol.coords[:, :, 1], mol.element, mol.name)
    assert seen["groups"] == W.bonded_groups(guessed, 30).tolist()
    mol.bonds = np.array([[2, 3], [8, 9]], np.uint32)                   # file bonds tie waters 0-1 and 2-3 together
    W.wrap_molecule(mol, guessBonds=True, guess_on_device=True)
    assert seen["groups"] == [0, 6, 12, 15, 18, 21, 24, 27, 30] == W.bonded_groups(np.vstack((mol.bonds, guessed)), 30).tolist()
    W.wrap_molecule(mol, fileBonds=False, guessBonds=True, guess_on_device=True)
    assert seen["groups"] == list(range(0, 31, 3))
    W.wrap_molecule(mol, guess_on_device=True)                          # guessBonds=False: the keyword alone changes nothing
    assert seen["groups"] == [0, 1, 2] + list(range(4, 9)) + list(range(10, 31)) == W.bonded_groups(mol.bonds, 30).tolist()
    mol.bonds = np.array([[0, 29]], np.uint32)
    with pytest.raises(ValueError, match="not one contiguous run"):
        W.wrap_molecule(mol, guessBonds=True, guess_on_device=True)


@pytest.fixture
def stub_moleculekit(monkeypatch):
    pkg, molecule, guesser = types.ModuleType("moleculekit"), types.ModuleType("moleculekit.molecule"), types.ModuleType("moleculekit.bondguesser")

    class Molecule(types.SimpleNamespace):
        def wrap(self, wrapsel="all", fileBonds=True, guessBonds=False, wrapcenter=None, unitcell="rectangular"):
            self.reference_calls = getattr(self, "reference_calls", 0) + 1

        def _guessBonds(self):
            from moleculekit.bondguesser import guess_bonds                  # at call time, as the reference does
            return guess_bonds(self)

    def guess_bonds(mol):
        return "the reference's guess_bonds"

    def bond_grid_search(coords, grid_cutoff, is_hydrogen, radii, max_boxes=4e6, cutoff_incr=1.26):
        return "the reference's bond_grid_search"

    molecule.Molecule = Molecule
    guesser.guess_bonds, guesser.bond_grid_search = guess_bonds, bond_grid_search
    pkg.molecule, pkg.bondguesser = molecule, guesser
    for name, mod in (("moleculekit", pkg), ("moleculekit.molecule", molecule), ("moleculekit.bondguesser", guesser)):
        monkeypatch.setitem(sys.modules, name, mod)
    return pkg


def test_wrap_install_with_guess_keeps_guessed_bonds_on_the_device(stub_moleculekit, emulated_library, monkeypatch):
    ref = stub_moleculekit.molecule
    original = ref.Molecule.wrap
    calls = []
    monkeypatch.setattr(W, "wrap", lambda coords, box, groups, centersel=None, center=None, ctx=None: calls.append(np.asarray(groups).tolist()) or coords)
    assert W.install(guess=True) is original and ref._mkamd_wrap_guess is True
    mol = ref.Molecule(**vars(_water_mol()))
    mol.wrap(guessBonds=True)
    assert calls == [list(range(0, 31, 3))] and not hasattr(mol, "reference_calls")
    apart = ref.Molecule(**vars(_water_mol()))
    apart.bonds = np.array([[0, 29]], np.uint32)                        # not contiguous with the guessed bonds either: the original
    apart.wrap(guessBonds=True)
    assert apart.reference_calls == 1 and len(calls) == 1
    assert W.install() is original and ref._mkamd_wrap_guess is False     # the last call's value holds
    mol.wrap(guessBonds=True)
    assert mol.reference_calls == 1 and len(calls) == 1
    W.install(guess=True)
    W.uninstall()
    assert ref.Molecule.wrap is original and ref._mkamd_wrap_guess is False and ref._mkamd_reference_wrap is None
    W.uninstall()


def test_install_swaps_the_guesser_and_uninstall_restores(stub_moleculekit, emulated_library):
    guesser, ref = stub_moleculekit.bondguesser, stub_moleculekit.molecule
    originals = (guesser.guess_bonds, guesser.bond_grid_search)
    assert B.install() == originals and B.install() == originals       # idempotent
    assert guesser.guess_bonds is B.guess_bonds and guesser.bond_grid_search is B.bond_grid_search
    assert ref.Molecule.wrap.__name__ == "wrap" and not hasattr(ref, "_mkamd_reference_wrap")      # independent of the wrap hook
    c = C.case("one_box")
    mol = ref.Molecule(**vars(C.as_mol(c)))
    same_list(mol._guessBonds(), C.restated("one_box")[0], "Molecule._guessBonds after install")
    B.uninstall()
    assert (guesser.guess_bonds, guesser.bond_grid_search) == originals and guesser._mkamd_reference_bonds is None
    assert mol._guessBonds() == "the reference's guess_bonds"
    B.uninstall()
