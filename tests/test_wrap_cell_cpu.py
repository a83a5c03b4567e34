"""CPU tier of the periodic wrap of triclinic boxes (moleculekit_amd/wrap.py, csrc/wrap_cell_kernels.h).

The restatement (tests/wrap_cell_restatement.py) must give the compiled reference's bits on the golden subset
(tests/golden/wrap_cell_cases.npz); the kernels and their launch plan, compiled for the host (tests/emu_wrap_cell_build.py,
-ffp-contract=off), must give the restatement's bits on every case of tests/wrap_cell_cases.py under every launch plan and unit cell;
the host logic of wrap.py is checked without a device."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emu_wrap_cell_build as E  # noqa: E402
import wrap_cell_cases as C  # noqa: E402
import wrap_cell_restatement as R  # noqa: E402

from moleculekit_amd import wrap as W  # noqa: E402

PLANS = {"default": (0, "k_wrap_cell_lanes + mkamd::k_wrap_cell_waves"), "waves_only": (E.AVOID_LANES, "k_wrap_cell_prep + mkamd::k_wrap_cell_waves"),
         "lanes_only": (E.AVOID_WAVES, "k_wrap_cell_lanes")}


# ------------------------------------------------------------------------------------------------
# the cases, the restatement
# ------------------------------------------------------------------------------------------------
def test_the_cases_cover_what_they_must():
    import emu_wrap_build

    assert emu_wrap_build.small_max() == C.SMALL_MAX and emu_wrap_build.chunk() == C.CHUNK
    assert E.max_steps() == R.MAX_STEPS == W.WRAP_CELL_MAX_STEPS == 4096
    assert E.MODES == W.CELL_MODES and [E.MODES[m] for m in R.MODES] == [0, 1, 2]
    sizes = set(np.diff(C.cases()["dodeca_sizes_center"].starts.astype(np.int64)).tolist())
    assert {1, 2, 3, 15, 16, 17, 63, 64, 65, 134, 255, 256, 257, 700} <= sizes
    assert sorted(int(n[12:]) for n in C.cases() if n.startswith("octa_frames_")) == [1, 2, 63, 64, 65]
    assert {n.split("_")[0] for n in C.cases()} >= set(C.BOXES)
    for name, c in C.cases().items():
        assert c.xyz.nbytes < 4 << 20, name
        if c.xyz.shape[0] > 1:
            assert np.any(c.boxvectors[:, :, 0] != c.boxvectors[:, :, 1]), name             # a different box per frame
        assert W._check_boxvectors(c.boxvectors) is None and E.check_boxvectors(c.boxvectors) is None
    assert set(C.GOLDEN) | set(C.HOST_ONLY) <= set(C.cases()) and not set(C.HOST_ONLY) & set(C.device_cases())
    # groups up to +-5 cells away: the triclinic loops take several steps
    c = C.cases()["octa_frames_2"]
    frac = np.linalg.solve(c.boxvectors[:, :, 0].T, c.xyz[0].astype(np.float64).T).T
    assert np.abs(frac).max() > 4


def test_the_golden_inputs_are_the_cases():
    g = C.golden()
    for name in C.GOLDEN:
        c = C.cases()[name]
        C.assert_same_bits(c.xyz, g[f"{name}/xyz"], name)
        assert np.array_equal(c.boxvectors, g[f"{name}/boxvectors"]) and np.array_equal(c.starts, g[f"{name}/starts"]), name
        assert np.array_equal(np.zeros(0, np.uint32) if c.centersel is None else c.centersel, g[f"{name}/centersel"]), name
        assert np.array_equal(np.zeros(3, np.float32) if c.center is None else c.center, g[f"{name}/center"]), name


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("name", C.GOLDEN)
def test_restatement_gives_the_references_bits(name, mode):
    want = C.golden()[f"{name}/{mode}"]
    got, status = C.expected(name, mode)
    C.assert_same_bits(got, want, f"{name} / {mode}")
    assert not status.any()
    assert np.any(got != C.cases()[name].xyz)


def test_the_face_case_sits_on_the_faces():
    """which side of a face a centre lands on is the compiled reference's say (the golden bits); here: that the case is what it claims"""
    c = C.cases()["face"]
    g = C.golden()
    bm = np.array(R.box_middle(c.boxvectors[:, :, 0]))
    assert bm.tolist() == [32.0, 40.0, 32.0]
    tri, rect = g["face/triclinic"][0], g["face/rectangular"][0]
    x = c.xyz[0]
    # frame 0: an atom exactly on the lower triclinic face stays (fractional coordinate 0 is inside), one on the upper face moves
    # down a cell; recentred coordinates are x + box_middle
    assert tri[1].tolist() == [-16.0 + 32.0, 40.0, 32.0] and tri[4].tolist() == [16.0 - 32.0 + 32.0, 40.0, 32.0]
    # one ulp below the lower face: a cell up is float32(48 - 2^-19) = 48, which is ON the upper face, so a cell down again to 16 -- the
    # atom ends on the lower face, moved by its one ulp (the centre is rounded to float32 after every step)
    assert x[0, 0] == np.nextafter(np.float32(-16), np.float32(-np.inf)) and tri[0].tolist() == [16.0, 40.0, 32.0]
    assert tri[2, 0] == x[2, 0] + np.float32(32) and x[2, 0] == np.nextafter(np.float32(-16), np.float32(np.inf))      # above it: stays
    # dx exactly + half the diagonal stays, - half moves up (the interval is (-h, h])
    assert rect[4, 0] == 16.0 + 32.0 and rect[1, 0] == -16.0 + 32.0 + 32.0
    assert x[1].tolist() == [-16.0, 0.0, 0.0] and x[4].tolist() == [16.0, 0.0, 0.0]


def test_known_answers():
    """what the reference gives on such boxes, seen when its module was compiled: fractional group centres in [0, 1) (triclinic), every
    group at the nearest of its 125 images (compact; dodecahedron and octahedron), centres within half the diagonal (rectangular).
    Compared with a tolerance: these centres are plain means."""
    for name in ("dodeca_sizes_center", "octa_frames_2", "hexa_sel_one_atom", "skew_sel_everything", "ortho_center"):
        c = C.cases()[name]
        s = c.starts.astype(np.int64)
        sizes = np.diff(s)
        for f in range(c.xyz.shape[0]):
            b = c.boxvectors[:, :, f]
            middle = 0.5 * b.sum(axis=0)

            def centres(r):
                return np.add.reduceat(r[f].astype(np.float64), s[:-1], axis=0) / sizes[:, None]

            tri = centres(C.expected(name, "triclinic")[0])
            frac = np.linalg.solve(b.T, tri.T).T
            assert frac.min() > -1e-4 and frac.max() < 1 + 1e-4, (name, f, frac.min(), frac.max())
            rect = centres(C.expected(name, "rectangular")[0]) - middle
            assert np.all(np.abs(rect) <= 0.5 * np.diag(b) + 1e-3), (name, f)
            comp = centres(C.expected(name, "compact")[0]) - middle
            if name.startswith(("dodeca", "octa")):
                k = np.arange(-2, 3)
                images = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) @ b          # [125, 3]
                d = np.linalg.norm(comp[:, None, :] + images[None], axis=2)
                assert np.all(np.linalg.norm(comp, axis=1) <= d.min(axis=1) + 1e-3), (name, f)
            # the triclinic and the compact cell hold the same images: they differ by whole box vectors.  (Not so the rectangular
            # mode: the reference moves along each axis by the box's DIAGONAL entry, which is no lattice vector where a box vector leans.)
            diff = np.linalg.solve(b.T, (tri - middle - comp).T).T
            assert np.abs(diff - np.round(diff)).max() < 1e-3, (name, f)


def test_restatement_where_the_references_loops_do_not_end():
    c = C.cases()["inf"]
    for mode in R.MODES:
        r, status = C.expected("inf", mode)
        assert status.tolist() == [1, 0, 0], mode
        assert not np.isfinite(r[0, 0, 1]) and not np.isfinite(r[1, int(c.starts[3]) - 1, 2])
        g1 = slice(int(c.starts[1]), int(c.starts[2]))
        assert np.isfinite(r[:, g1]).all()                                                  # the other groups are wrapped as ever
        far, status = C.expected("far_1000", mode)
        assert not status.any() and np.isfinite(far).all(), mode                              # 1 000 cells: under the cap
        assert np.abs(far).max() < 200 and np.abs(C.cases()["far_1000"].xyz).max() > 30000


# ------------------------------------------------------------------------------------------------
# the emulated kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", sorted(PLANS))
@pytest.mark.parametrize("name", sorted(C.cases()))
def test_emulated_kernels_give_the_restatements_bits(name, plan):
    avoid, kernels = PLANS[plan]
    c = C.cases()[name]
    before = c.xyz.copy()
    for mode in R.MODES:
        want, want_status = C.expected(name, mode)
        got, status = E.wrap_cell(c.xyz, c.boxvectors, c.starts, mode, c.centersel, c.center, avoid=avoid)
        assert np.array_equal(before.view(np.uint32), c.xyz.view(np.uint32)), "out of place leaves the input untouched"
        C.assert_same_bits(got, want, f"{name} / {mode} / {plan}, out of place")
        assert status.tolist() == want_status.tolist(), (name, mode, plan)
        if plan != "default" or np.diff(c.starts.astype(np.int64)).max() > C.SMALL_MAX:
            assert kernels in E.last_kernel(), E.last_kernel()
        assert "k_wrap_cell_prep" in E.last_kernel()
        assert ("k_wrap_centre" in E.last_kernel()) == (c.centersel is not None and len(c.centersel) > 0)
        inplace = c.xyz.copy()
        res, status = E.wrap_cell(inplace, c.boxvectors, c.starts, mode, c.centersel, c.center, avoid=avoid, inplace=True)
        assert res is inplace and status.tolist() == want_status.tolist()
        C.assert_same_bits(inplace, want, f"{name} / {mode} / {plan}, in place")


def test_the_centre_selection_inside_moving_groups_is_a_hazard_the_plan_answers():
    c = C.cases()["dodeca_sel_inside_moving"]
    want, _ = C.expected("dodeca_sel_inside_moving", "triclinic")
    sel = c.centersel.astype(np.int64)
    before = R.box_centre(R.from_frame_major(c.xyz), sel, None)
    after = R.box_centre(R.from_frame_major(want), sel, None)
    assert np.any(np.abs(before - after) > 1)


BAD_BOXES = {"zero": ((2, 2), 0.0, "must be positive"), "negative": ((1, 1), -31.0, "must be positive"), "nan": ((2, 0), np.nan, "not finite"),
             "inf": ((0, 0), np.inf, "not finite"), "upper": ((0, 2), 0.5, "not lower triangular")}


@pytest.mark.parametrize("what", sorted(BAD_BOXES))
def test_degenerate_frames_are_refused_by_the_checks_and_flagged_by_the_plan(what):
    (i, j), value, text = BAD_BOXES[what]
    c = C.cases()["octa_frames_2"]
    bv = c.boxvectors.copy()
    bv[i, j, 1] = value                                                                     # frame 1 only
    assert text in E.check_boxvectors(bv)
    with pytest.raises(ValueError, match=text):
        W._check_boxvectors(bv)
    for plan in sorted(PLANS):
        for mode in R.MODES:
            want, want_status = R.wrap_cell_frames(c.xyz, bv, c.starts, mode, c.centersel, c.center)
            assert want_status.tolist() == [0, 1, 0]
            assert np.array_equal(want[1], c.xyz[1]) and np.array_equal(want[0], C.expected("octa_frames_2", mode)[0][0])
            got, status = E.wrap_cell(c.xyz, bv, c.starts, mode, c.centersel, c.center, avoid=PLANS[plan][0])
            C.assert_same_bits(got, want, f"{what} / {mode} / {plan}")                    # the frame is copied through, the other wrapped
            assert status.tolist() == [0, 1, 0]
            inplace = c.xyz.copy()
            E.wrap_cell(inplace, bv, c.starts, mode, c.centersel, c.center, avoid=PLANS[plan][0], inplace=True)
            C.assert_same_bits(inplace, want, f"{what} / {mode} / {plan}, in place")
    assert "degenerate" in E.status_error([0, 1, 0]) and "degenerate" in W.status_error([0, 1, 0])


def test_status_words_name_their_conditions():
    assert E.status_error([0, 0, 0]) is None and W.status_error(np.zeros(3, np.int32)) is None
    for status in ([1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]):
        assert E.status_error(status) == W.status_error(status)
    assert W.status_error([1, 0, 1]) == "Too many triclinic vectors!!"
    assert "4096 steps" in W.status_error([1, 0, 0])


def test_pipeline_refuses_bad_arguments():
    c = C.cases()["octa_frames_1"]
    with pytest.raises(ValueError, match="both group kernels"):
        E.wrap_cell(c.xyz, c.boxvectors, c.starts, "compact", c.centersel, None, avoid=3)
    with pytest.raises(ValueError, match="mode must be 0"):
        E.wrap_cell(c.xyz, c.boxvectors, c.starts, 3, c.centersel, None)
    # starts that run past the atoms do not fault: the kernels clamp every group to the array
    bad = c.starts.copy()
    bad[-1] += 1000
    E.wrap_cell(c.xyz, c.boxvectors, bad, "triclinic", c.centersel, None)


# ------------------------------------------------------------------------------------------------
# host logic
# ------------------------------------------------------------------------------------------------
def test_box_vectors_against_the_references_recorded_values():
    """bit-equal where numpy's cos / sin are the recording machine's; they are the platform's, so up to 2 ulp of float64 is allowed, and
    a snapped zero must be a zero"""
    g = C.golden()
    want = g["bv/vectors"]
    got = W.box_vectors(g["bv/lengths"], g["bv/angles"])
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got == 0, want == 0)
    assert np.all(np.abs(got - want) <= 2 * np.spacing(np.abs(want)))
    assert np.all(got[0, 1] == 0) and np.all(got[0, 2] == 0) and np.all(got[1, 2] == 0)
    k = 5                                                                                   # 30, 40, 50 at exactly 90 degrees: cos(pi / 2) is snapped
    assert got[:, :, k].tolist() == [[30.0, 0.0, 0.0], [0.0, 40.0, 0.0], [0.0, 0.0, 50.0]]
    assert got[1, 0, k + 2] != 0 and got[1, 0, k + 1] == 0                                  # near 90: 40 cos(90.001) is kept, 40 cos(90) is not
    # float32 inputs are widened first, as Molecule.boxvectors does; one frame as 1-D arrays
    L, A = g["bv/lengths"][:, -1], g["bv/angles"][:, -1]
    assert np.array_equal(W.box_vectors(L.astype(np.float32), A.astype(np.float32))[:, :, 0], got[:, :, -1])
    assert np.array_equal(W.box_vectors(np.zeros((3, 4)), np.zeros((3, 4))), np.zeros((3, 3, 4)))
    with pytest.raises(AssertionError, match="Box angles should not be 0"):
        W.box_vectors(np.ones((3, 2)), np.array([[90.0, 0.0], [90.0, 90.0], [90.0, 90.0]]))
    with pytest.raises(ValueError, match="shape"):
        W.box_vectors(np.ones((3, 2)), np.ones((3, 3)))


def test_argument_validation_without_a_device():
    x = np.zeros((2, 5, 3), np.float32)
    bv = np.repeat(np.diag([10.0, 11.0, 12.0])[:, :, None], 2, axis=2)
    with pytest.raises(ValueError, match="Invalid unit cell type: cubic"):
        W.wrap_cell_trajectory(x, bv, [0, 5], "cubic", center=[0, 0, 0])
    with pytest.raises(TypeError, match="CUDA tensor"):
        W.wrap_cell_trajectory(x, bv, [0, 5], "compact", center=[0, 0, 0])
    coords = np.zeros((5, 3, 2), np.float32)
    with pytest.raises(ValueError, match=r"boxvectors must have shape \(3, 3, 2\)"):
        W.wrap_cell(coords, bv[:, :, :1], [0, 5], "compact", center=[0, 0, 0])
    for (i, j), value, text in BAD_BOXES.values():
        bad = bv.copy()
        bad[i, j, 1] = value
        with pytest.raises(ValueError, match=text):
            W.wrap_cell(coords, bad, [0, 5], "triclinic", center=[0, 0, 0])                 # refused before the library is touched
    with pytest.raises(ValueError, match="Invalid unit cell type"):
        W.wrap_cell(coords, bv, [0, 5], "cubic", center=[0, 0, 0])
    with pytest.raises(ValueError, match="not both"):
        W.wrap_cell(coords, bv, [0, 5], "compact", centersel=[1], center=[0, 0, 0])
    with pytest.raises(ValueError, match="starts must run from 0"):
        W.wrap_cell(coords, bv, [0, 4], "compact", center=[0, 0, 0])


def _mol(angles, F=3):
    rng = np.random.default_rng(2)
    ang = np.full((3, F), 90.0, np.float32)
    ang[:, : len(angles)] = np.asarray(angles, np.float32).T
    return types.SimpleNamespace(coords=rng.normal(0, 30, (7, 3, F)).astype(np.float32), box=np.full((3, F), 20.0, np.float32), boxangles=ang,
                                 bonds=np.array([[0, 1], [1, 2], [4, 5]], np.uint32))


def test_wrap_molecule_sends_a_triclinic_box_to_the_cell_path_only_when_asked(monkeypatch):
    seen = []

    def fake_cell(coords, boxvectors, groups, unitcell, centersel=None, center=None, rows=None, ctx=None):
        seen.append(("cell", unitcell, np.asarray(boxvectors).copy(), np.asarray(groups).tolist(),
                     None if centersel is None else np.asarray(centersel).tolist(), None if center is None else np.asarray(center).tolist()))
        return coords + 1

    def fake_box(coords, box, groups, centersel=None, center=None, ctx=None):
        seen.append(("box", np.asarray(box).copy()))
        return coords + 2

    monkeypatch.setattr(W, "wrap_cell", fake_cell)
    monkeypatch.setattr(W, "wrap", fake_box)
    # mixed frames: one frame of three is not at 90 degrees -- the whole call takes the cell path (the reference's rule)
    mol = _mol([[90, 90, 90], [60, 60, 90]])
    with pytest.raises(NotImplementedError, match="'rectangular', 'triclinic' and 'compact'"):
        W.wrap_molecule(mol)
    assert not seen
    before, held = mol.coords.copy(), mol.coords
    for unitcell in ("rectangular", "Compact", "triclinic"):
        W.wrap_molecule(mol, np.array([1, 2, 6]), unitcell=unitcell, triclinic_on_device=True)
        kind, cell, bv, groups, centersel, center = seen[-1]
        assert (kind, cell, groups, centersel, center) == ("cell", unitcell.lower(), [0, 3, 4, 6, 7], [1, 2, 6], None)
        assert np.array_equal(bv, W.box_vectors(mol.box, mol.boxangles)) and bv.shape == (3, 3, 3) and abs(bv[2, 0, 1] - 10.0) < 1e-12
    assert mol.coords is held and np.array_equal(mol.coords, before + 3)                    # in place, as the reference
    W.wrap_molecule(mol, wrapcenter=[1, 2, 3], fileBonds=False, unitcell="compact", triclinic_on_device=True)
    assert seen[-1][3:] == (list(range(8)), None, [1.0, 2.0, 3.0])
    # every angle 90: wrap_box's path, whatever the unit cell
    n = len(seen)
    W.wrap_molecule(_mol([[90, 90, 90]]), unitcell="compact", triclinic_on_device=True)
    W.wrap_molecule(_mol([[90, 90, 90]]), unitcell="triclinic")
    assert [s[0] for s in seen[n:]] == ["box", "box"]
    with pytest.raises(NotImplementedError, match="guessBonds"):
        W.wrap_molecule(_mol([[60, 60, 90]]), guessBonds=True, triclinic_on_device=True)
    with pytest.raises(ValueError, match="Invalid unit cell type"):
        W.wrap_molecule(_mol([[60, 60, 90]]), unitcell="cubic", triclinic_on_device=True)


@pytest.fixture
def stub_moleculekit(monkeypatch):
    pkg, molecule = types.ModuleType("moleculekit"), types.ModuleType("moleculekit.molecule")

    class Molecule(types.SimpleNamespace):
        def wrap(self, wrapsel="all", fileBonds=True, guessBonds=False, wrapcenter=None, unitcell="rectangular"):
            self.reference_calls = getattr(self, "reference_calls", 0) + 1

    molecule.Molecule = Molecule
    pkg.molecule = molecule
    for name, mod in (("moleculekit", pkg), ("moleculekit.molecule", molecule)):
        monkeypatch.setitem(sys.modules, name, mod)
    return molecule


def test_install_triclinic_sends_triclinic_boxes_to_the_device(stub_moleculekit, monkeypatch):
    ref = stub_moleculekit
    original = ref.Molecule.wrap
    calls = []
    monkeypatch.setattr(W, "wrap_cell", lambda coords, bv, groups, unitcell, centersel=None, center=None, rows=None, ctx=None:
                        calls.append(unitcell) or coords)
    monkeypatch.setattr(W, "wrap", lambda coords, box, groups, centersel=None, center=None, ctx=None: calls.append("box") or coords)
    try:
        assert W.install() is original
        tri = ref.Molecule(**vars(_mol([[70, 70, 70]])))
        tri.wrap(unitcell="compact")
        assert tri.reference_calls == 1 and not calls                                       # install() as ever: the original
        assert W.install(triclinic=True) is original and ref.Molecule.wrap is not original
        tri.wrap(unitcell="compact")
        tri.wrap(np.array([0, 1]), unitcell="triclinic")
        tri.wrap()
        assert calls == ["compact", "triclinic", "rectangular"] and tri.reference_calls == 1
        ref.Molecule(**vars(_mol([[90, 90, 90]]))).wrap(unitcell="compact")
        assert calls[-1] == "box"
        guessed = ref.Molecule(**vars(_mol([[70, 70, 70]])))
        guessed.wrap(guessBonds=True)
        apart = ref.Molecule(**vars(_mol([[70, 70, 70]])))
        apart.bonds = np.array([[0, 2]], np.uint32)
        apart.wrap(unitcell="compact")
        assert (guessed.reference_calls, apart.reference_calls) == (1, 1) and len(calls) == 4
        W.install()                                                                         # the last call's value holds
        tri.wrap(unitcell="compact")
        assert tri.reference_calls == 2
        W.install(triclinic=True)
    finally:
        W.uninstall()
    assert ref.Molecule.wrap is original and ref._mkamd_reference_wrap is None and ref._mkamd_wrap_triclinic is False
    W.install()
    tri.wrap(unitcell="compact")                                                            # uninstall() cleared the flag
    assert tri.reference_calls == 3
    W.uninstall()
