"""CPU tier of the periodic wrap (moleculekit_amd/wrap.py, csrc/wrap_kernels.h).

The restatement (tests/wrap_restatement.py) is pinned to the reference's known answer on its own fixture; the kernels and their launch
plan, compiled for the host (tests/emu_wrap_build.py, -ffp-contract=off), must give the restatement's bits on every case of
tests/wrap_cases.py under every launch plan; the host logic of wrap.py is checked without a device."""
import logging
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emu_wrap_build as E  # noqa: E402
import moments_restatement as MR  # noqa: E402
import wrap_cases as C  # noqa: E402
import wrap_restatement as R  # noqa: E402

from moleculekit_amd import moments as M  # noqa: E402
from moleculekit_amd import wrap as W  # noqa: E402

PLANS = {"default": (0, "k_wrap_lanes + mkamd::k_wrap_waves"), "waves_only": (E.AVOID_LANES, "k_wrap_waves"), "lanes_only": (E.AVOID_WAVES, "k_wrap_lanes")}


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def test_the_cases_restate_the_kernels_constants():
    assert E.small_max() == C.SMALL_MAX and E.chunk() == C.CHUNK
    assert E.small_max(E.AVOID_LANES) == 0 and E.small_max(E.AVOID_WAVES) > 2 ** 30
    sizes = set(np.diff(C.cases()["sizes_center"].starts.astype(np.int64)).tolist())
    assert {1, 2, 3, 63, 64, 65, 134, C.SMALL_MAX - 1, C.SMALL_MAX, C.SMALL_MAX + 1, C.CHUNK - 1, C.CHUNK, C.CHUNK + 1, 3384} <= sizes
    assert sorted(int(n[7:]) for n in C.cases() if n.startswith("frames_")) == [1, 2, 63, 64, 65, 130]
    for name, c in C.cases().items():
        assert c.xyz.nbytes < 4 << 20, name
        if c.xyz.shape[0] > 1 and name != "edge":
            assert np.all(c.box[:, 0] != c.box[:, 1]), name                     # a different box per frame


def test_restatement_extends_the_bond_form_unchanged():
    c = C.cases()["frames_2"]
    s = c.starts.astype(np.int64)
    bonds = np.concatenate([np.stack([np.arange(a, b - 1), np.arange(a + 1, b)], axis=1) for a, b in zip(s[:-1], s[1:])])
    assert MR.bonded_groups(bonds, int(s[-1])).tolist() == s.tolist()
    via_bonds = MR.wrap_box(R.from_frame_major(c.xyz), c.box, c.centersel, bonds)
    C.assert_same_bits(R.to_frame_major(via_bonds), C.expected("frames_2"), "starts form against the bond form")
    assert R.wrap_box_bonds is MR.wrap_box


def test_restatement_on_the_edges():
    c = C.cases()["edge"]
    want = C.expected("edge")
    f32 = np.float32
    x0, w0 = c.xyz[0], want[0]                                                  # frame 0: box 30, 31.7, 8; centre 0
    half = np.array([30.0, 31.7, 8.0], f32) / f32(2)
    assert np.array_equal(w0[0], half) and np.array_equal(w0[1], -half)         # exactly at +- box / 2: not moved
    assert np.all(w0[2] < 0) and np.all(w0[3] > 0)                              # one ulp beyond: moved by one box
    assert np.array_equal(w0[4:6], x0[4:6]) and np.all(w0[6:8] < 0) and np.all(w0[8:11] > 0)
    # +-1.5 and +-2.5 boxes: half away from zero gives 2 and 3 boxes (rint: 2 and 2)
    assert [w0[11 + 2 * k, 2] for k in range(4)] == [-4.0, 4.0, -4.0, 4.0]
    assert [w0[12 + 2 * k, 0] for k in range(4)] == [-15.0, 15.0, -15.0, 15.0]
    # a thousand boxes away: the translation is a rounded product, what is left is not exactly inside the cell but close
    far = slice(19, 31)
    assert np.all(np.abs(w0[far]) <= half * f32(1.001)) and np.all(np.abs(x0[far]) > 900 * half)
    # NaN / infinity: only that group's axis
    assert np.isnan(w0[31, 0]) and np.isnan(x0[31, 0]) and w0[32, 0] == x0[32, 0] and w0[31, 1] == f32(40.0) - f32(31.7)
    # (the chain over inf and 41 gives inf + (41 - inf) / 2 = NaN: that axis does not move; x does, z does not)
    assert np.array_equal(w0[33:35, 1], x0[33:35, 1]) and np.array_equal(w0[33:35, 0], x0[33:35, 0] - f32(60.0))
    assert np.isnan(w0[35, 0]) and np.array_equal(w0[35, 1:], [f32(1.0), f32(-13.0) + f32(16.0)])      # -inf - (-inf)
    assert np.isfinite(w0[36:38]).all() and np.all(np.abs(w0[36:38]) <= half + 1)
    # frame 1: a zero box length on y turns what is off the centre on y into NaN, x and z are wrapped as ever; frame 2: all zero
    assert np.isnan(want[1][2, 1]) and np.array_equal(want[1][:, [0, 2]][:31], w0[:, [0, 2]][:31])
    assert np.isnan(want[2][:31][c.xyz[2][:31] != 0]).all()
    assert np.isfinite(want[3][36:38]).all()


def test_known_answer_of_the_reference_on_its_fixture():
    """the two assertions of the reference's test_orthogonal_wrapping, on the restatement"""
    coords, box, starts, center = C.fixture()
    assert coords.shape == (167262, 3, 1) and starts.size == 43130
    assert np.allclose(box[:, 0], [94.93, 95.56, 178.05], atol=0.01)
    assert np.linalg.norm(coords[:, :, 0].mean(axis=0) - center) > 100
    wrapped, moved = C.fixture_expected(False)
    assert np.linalg.norm(wrapped[:, :, 0].mean(axis=0) - center) < 1
    assert int(moved.any(axis=(1, 2)).sum()) == 37824
    sizes = np.diff(starts.astype(np.int64))
    assert (sizes == 3).sum() == 42635 and (sizes == 1).sum() == 249 and sorted(sizes[sizes > 134].tolist()) == [467, 1360, 1603, 3384]


# ------------------------------------------------------------------------------------------------
# the emulated kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("name", sorted(C.cases()))
def test_emulated_kernels_give_the_restatements_bits(name, plan):
    avoid, kernels = PLANS[plan]
    c = C.cases()[name]
    before = c.xyz.copy()
    got = E.wrap_box(c.xyz, c.box, c.starts, c.centersel, c.center, avoid=avoid)
    assert np.array_equal(before.view(np.uint32), c.xyz.view(np.uint32)), "out of place leaves the input untouched"
    C.assert_same_bits(got, C.expected(name), f"{name} / {plan}, out of place")
    if plan != "default" or np.diff(c.starts.astype(np.int64)).max() > C.SMALL_MAX:
        assert kernels in E.last_kernel(), E.last_kernel()
    assert ("k_wrap_centre" in E.last_kernel()) == (c.centersel is not None and len(c.centersel) > 0)
    inplace = c.xyz.copy()
    assert E.wrap_box(inplace, c.box, c.starts, c.centersel, c.center, avoid=avoid, inplace=True) is inplace
    C.assert_same_bits(inplace, C.expected(name), f"{name} / {plan}, in place")


def test_the_centre_selection_inside_moving_groups_is_a_hazard_the_plan_answers():
    """the case's centre selection is a group that itself moves: had its centre been taken after that group was written, in place, the
    other groups would land elsewhere"""
    c = C.cases()["sizes_sel_inside_moving"]
    want = C.expected("sizes_sel_inside_moving")
    sel = c.centersel.astype(np.int64)
    assert np.any(want[:, sel] != c.xyz[:, sel])
    centre_before = R.box_centre(R.from_frame_major(c.xyz), sel, None)
    centre_after = R.box_centre(R.from_frame_major(want), sel, None)
    assert np.any(np.abs(centre_before - centre_after) > 1)


@pytest.mark.parametrize("with_sel", [False, True])
def test_emulated_kernels_on_the_fixture(with_sel):
    coords, box, starts, center = C.fixture()
    want, _ = C.fixture_expected(with_sel)
    sel = np.arange(coords.shape[0], dtype=np.uint32)[C.PROTEIN_6X18] if with_sel else None
    got = E.wrap_box(R.to_frame_major(coords), box, starts, sel, None if with_sel else center)
    C.assert_same_bits(got, R.to_frame_major(want), "6X18")


def test_pipeline_refuses_bad_arguments():
    assert E.check_starts([0, 3, 5], 5) is None
    assert "begin at 0" in E.check_starts([1, 3, 5], 5)
    assert "increase" in E.check_starts([0, 3, 3, 5], 5) and "increase" in E.check_starts([0, 4, 3, 5], 5)
    assert "number of atoms" in E.check_starts([0, 3, 5], 6)
    c = C.cases()["frames_1"]
    with pytest.raises(ValueError, match="both group kernels"):
        E.wrap_box(c.xyz, c.box, c.starts, c.centersel, None, avoid=3)
    # starts that run past the atoms do not fault: the kernels clamp every group to the array
    bad = c.starts.copy()
    bad[-1] += 1000
    E.wrap_box(c.xyz, c.box, bad, c.centersel, None)


# ------------------------------------------------------------------------------------------------
# host logic
# ------------------------------------------------------------------------------------------------
def test_bonded_groups_against_random_bond_lists():
    rng = np.random.default_rng(5)
    for trial in range(20):
        sizes = rng.integers(1, 40, rng.integers(1, 30))
        starts = np.r_[0, np.cumsum(sizes)]
        bonds = []
        for a, b in zip(starts[:-1], starts[1:]):                               # a random spanning tree of each run, plus a few cycles
            order = rng.permutation(np.arange(a, b))
            for k in range(1, order.size):
                bonds.append((order[k], order[rng.integers(0, k)]))
            for _ in range(rng.integers(0, 3)):
                bonds.append(tuple(rng.integers(a, b, 2)))
        bonds = np.array(bonds, np.int64).reshape(-1, 2)[rng.permutation(len(bonds))] if bonds else np.zeros((0, 2), np.int64)
        got = W.bonded_groups(bonds, int(starts[-1]))
        assert got.dtype == np.uint32 and got.tolist() == starts.tolist()
        assert got.tolist() == MR.bonded_groups(bonds, int(starts[-1])).tolist()
    assert W.bonded_groups(None, 4).tolist() == [0, 1, 2, 3, 4]
    assert W.bonded_groups(np.zeros((0, 2), int), 0).tolist() == [0]
    long_chain = np.stack([np.arange(4999), np.arange(1, 5000)], axis=1)
    assert W.bonded_groups(long_chain, 5001).tolist() == [0, 5000, 5001]
    with pytest.raises(ValueError, match="not one contiguous run"):
        W.bonded_groups(np.array([[0, 2]]), 3)                                   # atom 1 sits between the two bonded atoms
    with pytest.raises(IndexError):
        W.bonded_groups(np.array([[0, 3]]), 3)


def _mol(F=2, box=20.0, angles=90.0):
    rng = np.random.default_rng(2)
    return types.SimpleNamespace(coords=rng.normal(0, 30, (7, 3, F)).astype(np.float32), box=np.full((3, F), box, np.float32),
                                 boxangles=np.full((3, F), angles, np.float32), bonds=np.array([[0, 1], [1, 2], [4, 5]], np.uint32))


def test_wrap_molecule_keeps_the_references_behaviours(caplog):
    with pytest.raises(ValueError, match="Invalid unit cell type: cubic. Must be one of: rectangular, triclinic, compact"):
        W.wrap_molecule(_mol(), unitcell="Cubic")
    mol = _mol(box=0.0)
    before = mol.coords.copy()
    with caplog.at_level(logging.WARNING, logger="moleculekit_amd.wrap"):
        assert W.wrap_molecule(mol) is None
    assert "Zero box size detected in `Molecule.box`; skipping wrap." in caplog.text and np.array_equal(mol.coords, before)
    mol = _mol()
    mol.box = mol.box[:, :1]
    with pytest.raises(RuntimeError, match="Detected different number of simulation frames in `Molecule.box` and `Molecule.coords`"):
        W.wrap_molecule(mol)
    with pytest.raises(NotImplementedError, match="'rectangular', 'triclinic' and 'compact'"):
        W.wrap_molecule(_mol(angles=60.0))
    with pytest.raises(NotImplementedError, match="guessBonds"):
        W.wrap_molecule(_mol(), guessBonds=True)
    mol = _mol()
    mol.bonds = np.array([[0, 2]], np.uint32)
    with pytest.raises(ValueError, match="not one contiguous run"):
        W.wrap_molecule(mol)
    with pytest.raises(TypeError, match="no selection language"):
        W.wrap_molecule(_mol(), "protein")


def test_wrap_molecule_hands_the_library_what_the_reference_hands_its_loop(monkeypatch):
    seen = {}

    def fake_wrap(coords, box, groups, centersel=None, center=None, ctx=None):
        seen.update(groups=np.asarray(groups).tolist(), centersel=None if centersel is None else np.asarray(centersel).tolist(),
                    center=None if center is None else np.asarray(center).tolist())
        return coords + 1

    monkeypatch.setattr(W, "wrap", fake_wrap)
    mol = _mol()
    before = mol.coords.copy()
    held = mol.coords
    W.wrap_molecule(mol, np.array([False, True, True, False, False, False, True]))
    assert seen == dict(groups=[0, 3, 4, 6, 7], centersel=[1, 2, 6], center=None)
    assert mol.coords is held and np.array_equal(mol.coords, before + 1)        # in place, as the reference
    W.wrap_molecule(mol, wrapcenter=[1, 2, 3], fileBonds=False)
    assert seen == dict(groups=list(range(8)), centersel=None, center=[1.0, 2.0, 3.0])
    W.wrap_molecule(mol)
    assert seen["centersel"] == list(range(7))


@pytest.fixture
def stub_moleculekit(monkeypatch):
    pkg, molecule = types.ModuleType("moleculekit"), types.ModuleType("moleculekit.molecule")

    class Molecule(types.SimpleNamespace):
        def wrap(self, wrapsel="all", fileBonds=True, guessBonds=False, wrapcenter=None, unitcell="rectangular"):
            self.reference_calls = getattr(self, "reference_calls", 0) + 1

        def atomselect(self, sel, indexes=False, guessBonds=False):
            assert sel == "protein" and indexes
            return np.array([0, 1, 2])

    molecule.Molecule = Molecule
    pkg.molecule = molecule
    for name, mod in (("moleculekit", pkg), ("moleculekit.molecule", molecule)):
        monkeypatch.setitem(sys.modules, name, mod)
    return molecule


def test_install_swaps_molecule_wrap_and_uninstall_restores(stub_moleculekit, monkeypatch):
    ref = stub_moleculekit
    original = ref.Molecule.wrap
    calls = []
    monkeypatch.setattr(W, "wrap", lambda coords, box, groups, centersel=None, center=None, ctx=None:
                        calls.append(None if centersel is None else np.asarray(centersel).tolist()) or coords)
    assert W.install() is original and W.install() is original                  # idempotent
    assert ref.Molecule.wrap is not original and ref._mkamd_reference_wrap is original
    mol = ref.Molecule(**vars(_mol()))
    mol.wrap("protein")                                                         # a selection string: the molecule's own atomselect
    assert calls == [[0, 1, 2]] and not hasattr(mol, "reference_calls")
    mol.wrap(wrapcenter=[0, 0, 0])
    assert calls[-1] is None
    # what the device does not do goes back to the reference: triclinic boxes, guessed bonds, groups that are not contiguous
    tri = ref.Molecule(**vars(_mol(angles=70.0)))
    tri.wrap("protein", unitcell="compact")
    guessed = ref.Molecule(**vars(_mol()))
    guessed.wrap(guessBonds=True)
    apart = ref.Molecule(**vars(_mol()))
    apart.bonds = np.array([[0, 2]], np.uint32)
    apart.wrap()
    assert (tri.reference_calls, guessed.reference_calls, apart.reference_calls) == (1, 1, 1) and len(calls) == 2
    W.uninstall()
    assert ref.Molecule.wrap is original and ref._mkamd_reference_wrap is None
    W.uninstall()


def test_the_rows_that_travel_are_wrapped_as_if_everything_had():
    c = C.cases()["frames_2"]
    coords = R.from_frame_major(c.xyz)
    starts = c.starts.astype(np.int64)
    centersel = np.array([5, 0, 3, 30, 300])
    named = np.array([2, 40, 41, 387])                                           # atoms of groups 1, 4 (65 atoms) and 5 (300 atoms)
    rows, packed = W.travel_rows(starts, named, centersel)
    gids = np.searchsorted(starts, named, side="right") - 1
    whole = np.concatenate([np.arange(starts[g], starts[g + 1]) for g in np.unique(gids)])
    assert rows.tolist() == sorted(set(whole.tolist()) | set(centersel.tolist())) and rows.size < coords.shape[0]
    assert packed[0] == 0 and packed[-1] == rows.size and W._starts(packed, rows.size) is not None
    sub = R.wrap_box(coords[rows.astype(np.int64)], c.box, packed, np.searchsorted(rows, centersel), None)
    full = R.wrap_box(coords, c.box, c.starts, centersel, None)
    at = np.searchsorted(rows, whole)
    C.assert_same_bits(sub[at], full[whole], "every atom of the named atoms' groups")


def test_argument_validation_without_a_device():
    x = np.zeros((2, 5, 3), np.float32)
    with pytest.raises(TypeError, match="CUDA tensor"):
        W.wrap_trajectory(x, np.ones((3, 2), np.float32), [0, 5], center=[0, 0, 0])
    with pytest.raises(ValueError, match="not both"):
        W._centre_inputs([1], [0, 0, 0], 5)
    with pytest.raises(ValueError, match="is required"):
        W._centre_inputs(None, None, 5)
    with pytest.raises(ValueError, match="is required"):
        W._centre_inputs(np.zeros(0, int), None, 5)
    sel, cen = W._centre_inputs(np.zeros(0, int), [1, 2, 3], 5)                  # an empty selection with a centre given
    assert sel is None and cen.tolist() == [1, 2, 3]
    assert W._centre_inputs([3, 1, -1], None, 5)[0].tolist() == [3, 1, 4]       # the order is kept
    assert W._centre_inputs(np.array([True, False, True, False, False]), None, 5)[0].tolist() == [0, 2]
    with pytest.raises(IndexError):
        W._centre_inputs([5], None, 5)
    for bad in ([1, 5], [0, 3, 3, 5], [0, 4], [0]):
        with pytest.raises(ValueError, match="starts must run from 0"):
            W._starts(bad, 5)
    coords = np.zeros((5, 3, 2), np.float32)
    with pytest.raises(ValueError, match="box must have shape"):
        W.wrap(coords, np.ones((3, 3)), [0, 5], center=[0, 0, 0])
    with pytest.raises(ValueError, match="float32"):
        W.wrap(coords.astype(np.float64), np.ones((3, 2)), [0, 5], center=[0, 0, 0])


def test_wrap_on_device_is_opt_in():
    box = np.full((3, 4), 60, np.float32)
    mol = types.SimpleNamespace(coords=np.zeros((6, 3, 4), np.float32), box=box, bonds=np.zeros((0, 2), np.uint32), numFrames=4,
                                resid=np.arange(6), element=np.array(["C"] * 6), masses=np.ones(6, np.float32))
    for cls, args in ((M.MetricCoordinate, ("all",)), (M.MetricGyration, ("all",)), (M.MetricFluctuation, ("all",)),
                      (M.MetricSphericalCoordinate, (mol, np.array([0]), np.array([1])))):
        assert cls(*args, trajalnsel="all")._wrap_on_device is False
        assert cls(*args, trajalnsel="all", wrap_on_device=True)._wrap_on_device is True
        with pytest.raises(NotImplementedError, match="wrap the molecule first .* or pass pbc=False"):
            cls(*args, trajalnsel="all", wrap_on_device=False).project(mol)
    # opted in, the selection language is still not there: the reference's default centersel is a string
    with pytest.raises(TypeError, match="no selection language"):
        M.MetricCoordinate("all", wrap_on_device=True).project(mol)
