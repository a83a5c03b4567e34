"""CPU tier of the proximity selection (moleculekit_amd/within.py): the product's kernels and launch plan on the host
SIMT emulation (tests/emu_within_build.py), held against what the compiled reference left in its results array on the golden cases
(tests/golden/within_cases.npz).  Reads nothing of the reference: tests/golden only.

Pass criterion: equal boolean arrays; no tolerance.  The reference ORs into its results array, the kernels write one byte per query, so
what is compared is ``preset | kernel bytes``.
"""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emu_within_build as E  # noqa: E402
import within_cases as C  # noqa: E402
import within_restatement as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "within_cases.npz")
PLANS = {"unforced": 0, "pairs": E.AVOID_CELLS, "cells": E.AVOID_PAIRS}
# where the cell path cannot run, the plan hands over to the all-pairs kernel: several frames, nothing to search, or the reasons
# within_pipeline.h names
HANDS_OVER = {"crowded_box": "a box holds more sources than the cap", "nan_source": "a source coordinate is not finite",
              "inf_source": "a source coordinate is not finite", "cutoff_inf": "sq_cutoff is not finite", "cutoff_1e20": "sq_cutoff is not finite",
              "cutoff_nan": "sq_cutoff is not finite", "one_by_one": "the grid is one box", "cutoff_negative_single_source": "the grid is one box",
              "3ptb_ligand_5A": "the grid is one box"}                 # (nine ligand atoms inside one 5 A box)
NOTHING_TO_SEARCH = ("empty_sel1", "empty_sel2")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def golden_inputs(golden, name):
    c = {k: golden[f"{name}/{k}"] for k in ("coords", "sel1", "sel2", "mn", "mx")}
    c["cutoff"] = float(golden[f"{name}/cutoff"])
    c["preset"] = golden[f"{name}/preset"] if f"{name}/preset" in golden.files else None
    return c


def golden_result(golden, name):
    return golden[f"{name}/results"]


def expected_kernel(name, plan, frames=1):
    if name in NOTHING_TO_SEARCH:
        return ""
    if plan != "cells" or frames > 1 or name in HANDS_OVER:
        return E.PAIRS_KERNEL
    return E.CELLS_KERNEL


def emulated(c, plan="unforced", no_cull=False):
    gate = np.stack([c["mn"], c["mx"]], axis=1)
    out, info = E.within(c["coords"], c["sel1"], c["sel2"], c["cutoff"], gate, avoid=PLANS[plan], no_cull=no_cull)
    if c["preset"] is not None:
        out = out | c["preset"]
    return out, E.last_kernel(), E.left()


def test_the_cases_are_what_they_are_meant_to_be():
    C.check()


@pytest.mark.parametrize("name", C.GOLDEN)
def test_fixture_holds_the_cases_and_the_restatement_gives_the_golden(golden, name):
    c, g = C.case(name), golden_inputs(golden, name)
    for k in ("coords", "sel1", "sel2", "mn", "mx"):
        assert c[k].dtype == g[k].dtype and c[k].tobytes() == g[k].tobytes(), k
    assert (c["cutoff"] == g["cutoff"] or (np.isnan(c["cutoff"]) and np.isnan(g["cutoff"]))) and (c["preset"] is None) == (g["preset"] is None)
    assert np.array_equal(C.restated(name), golden_result(golden, name))


@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", C.GOLDEN)
def test_emulated_pipeline_gives_the_golden(golden, name, plan):
    c = golden_inputs(golden, name)
    got, kernel, left = emulated(c, plan)
    assert np.array_equal(got, golden_result(golden, name)), f"{name} / {plan}: {int((got != golden_result(golden, name)).sum())} results differ"
    assert kernel == expected_kernel(name, plan, c["coords"].shape[0])
    if plan == "cells" and name in HANDS_OVER:
        assert left == HANDS_OVER[name]
    if plan == "pairs":
        assert left == ""
    if plan == "unforced":                                            # the plan's own choice: the cell list from 2 048 sources on (crowded_box)
        assert left == (HANDS_OVER.get(name, "") if len(c["sel2"]) >= 2048 and c["coords"].shape[0] == 1 else "")


@pytest.mark.parametrize("name", ["crowded_box", "nan_source", "cutoff_inf"])
def test_the_cell_path_hands_over_without_an_error(golden, name):
    got, kernel, left = emulated(golden_inputs(golden, name), "cells")
    assert kernel == E.PAIRS_KERNEL and left == HANDS_OVER[name] and np.array_equal(got, golden_result(golden, name))


@pytest.mark.parametrize("plan", ["pairs", "cells"])
@pytest.mark.parametrize("name", C.GOLDEN)
def test_the_cull_never_changes_a_result(golden, name, plan):
    c = golden_inputs(golden, name)
    with_cull, _, _ = emulated(c, plan)
    without, _, _ = emulated(c, plan, no_cull=True)
    assert np.array_equal(with_cull, without)


def test_the_cull_rule_for_non_finite_sources_and_cutoffs():
    # sources with a non-finite coordinate stay out of the box (they are within of nothing), so a far query is culled although an inf
    # source "contains" it; a cutoff whose square overflows turns the cull off and every finite pair is within
    xyz = np.array([[[0, 0, 0], [1000, 0, 0], [np.inf, 0, 0], [1, 1, 1], [np.nan, 1, 1]]], np.float32)
    for no_cull in (False, True):
        out, _ = E.within(xyz, [0, 1], [2, 3, 4], 3.0, no_cull=no_cull)
        assert out.tolist() == [[True, False]]
        out, _ = E.within(xyz, [0, 1], [2, 3, 4], 1e20, no_cull=no_cull)
        assert out.tolist() == [[True, True]]
        out, _ = E.within(xyz, [0, 1], [2, 4], 3.0, no_cull=no_cull)       # no finite source at all: an empty box culls everyone
        assert out.tolist() == [[False, False]]


def test_real_density_runs_over_the_cell_list():
    # the golden 3PTB cases search around nine ligand atoms, which fit one or two boxes; around the PROTEIN the grid has hundreds
    c = C.case("3ptb_ligand_5A")
    xyz = c["coords"]
    water = np.setdiff1d(np.arange(xyz.shape[1]), C.case("3ptb_protein_of_ligand")["sel1"]).astype(np.uint32)
    protein = C.case("3ptb_protein_of_ligand")["sel1"]
    want = R.frames(xyz, water, protein, 3.5)
    for plan in PLANS:
        out, info = E.within(xyz, water, protein, 3.5, avoid=PLANS[plan])
        assert np.array_equal(out, want) and want.any() and not want.all()
        assert E.last_kernel() == (E.CELLS_KERNEL if plan == "cells" else E.PAIRS_KERNEL) and (plan != "cells" or info[:3].prod() > 100)


def test_the_plan_takes_the_cell_list_from_2048_sources_on_one_frame():
    rng = np.random.default_rng(21)
    xyz = (rng.random((1, 2048 + 40, 3)) * 30.0).astype(np.float32)
    q = np.arange(2048, 2088)
    for n2, kernel in ((2047, E.PAIRS_KERNEL), (2048, E.CELLS_KERNEL)):
        out, _ = E.within(xyz, q, np.arange(n2), 2.0)
        assert E.last_kernel() == kernel and np.array_equal(out, R.frames(xyz, q, np.arange(n2), 2.0)) and out.any() and not out.all()
    out, _ = E.within(np.concatenate([xyz, xyz]), q, np.arange(2048), 2.0)                       # two frames: the all-pairs kernel
    assert E.last_kernel() == E.PAIRS_KERNEL and np.array_equal(out[0], out[1])


def test_no_gate_means_the_pair_test_alone(golden):
    for name in ("cutoff_negative_single_source", "nan_bounds_all_axes", "cutoff_negative_wide_source"):
        c = golden_inputs(golden, name)
        for plan in PLANS:
            out, _ = E.within(c["coords"], c["sel1"], c["sel2"], c["cutoff"], None, avoid=PLANS[plan])
            assert np.array_equal(out, C.ungated(name)) and out.any()


# ------------------------------------------------------------------------------------------------
# the Python layer, with a context whose host entry is the emulator
# ------------------------------------------------------------------------------------------------
class EmuContext:
    """stands in for _lib.Context: within_distance_host of coords [N, 3, F] through the emulated pipeline"""

    def __init__(self):
        self.calls = 0

    def within_distance_host(self, coords, sel1, sel2, cutoff, gate=None):
        assert coords.dtype == np.float32 and coords.flags.c_contiguous and sel1.dtype == np.uint32 and sel2.dtype == np.uint32
        self.calls += 1
        out, _ = E.within(np.ascontiguousarray(np.transpose(coords, (2, 0, 1))), sel1, sel2, cutoff, gate)
        return out.astype(np.uint8)


@pytest.fixture(scope="module")
def W():
    from moleculekit_amd import within
    return within


def test_within_distance_ors_in_place(W, golden):
    for name in ("results_preset", "self_in_source", "cutoff_negative_wide_source", "unsorted_duplicates"):
        c = golden_inputs(golden, name)
        results = np.zeros(len(c["sel1"]), bool) if c["preset"] is None else c["preset"][0].copy()
        held = results
        assert W.within_distance(c["coords"][0], c["cutoff"], c["sel1"], c["sel2"], c["mn"][0], c["mx"][0], results, ctx=EmuContext()) is None
        assert held is results and np.array_equal(results, golden_result(golden, name)[0])
    results = np.ones(3, bool)                                        # nothing is ever cleared
    W.within_distance(np.zeros((4, 3), np.float32), 0.0, np.arange(3, dtype=np.uint32), np.array([3], np.uint32), np.zeros(3, np.float32),
                      np.zeros(3, np.float32), results, ctx=EmuContext())
    assert results.all()


def test_within_over_frames_and_frame_lists(W, golden):
    c = golden_inputs(golden, "traj3")
    mol = C.Mol(c)
    ungated = C.ungated("traj3")
    got = W.within(mol.coords, c["sel1"], c["sel2"], c["cutoff"], ctx=EmuContext())
    assert got.dtype == bool and got.shape == (300, 3) and np.array_equal(got.T, ungated)
    got = W.within(mol.coords, c["sel1"], c["sel2"], c["cutoff"], frames=[2, 0], ctx=EmuContext())
    assert np.array_equal(got.T, ungated[[2, 0]])
    mask1, mask2 = mol.atomselect(c["sel1"]), mol.atomselect(c["sel2"])
    assert np.array_equal(W.within(mol.coords, mask1, mask2, c["cutoff"], ctx=EmuContext()).T, ungated)


@pytest.mark.parametrize("exclusive", [False, True])
def test_within_molecule_equals_the_per_frame_golden(W, golden, exclusive):
    # the golden of "3ptb_ligand_5A" is "all atoms within 5 of the ligand" with the numpy bounds: what within_molecule computes
    c = golden_inputs(golden, "3ptb_ligand_5A")
    mol = C.Mol(c)
    src = mol.atomselect(c["sel2"])
    want = golden_result(golden, "3ptb_ligand_5A")[0].copy()
    if exclusive:
        want[src] = False
    ctx = EmuContext()
    got = W.within_molecule(mol, src, 5.0, exclusive=exclusive, ctx=ctx)
    assert got.shape == (mol.numAtoms, 1) and np.array_equal(got[:, 0], want) and ctx.calls == 1
    assert np.array_equal(W.within_molecule(mol, c["sel2"], 5.0, exclusive=exclusive, ctx=EmuContext())[:, 0], want)       # through mol.atomselect
    # several frames in one call, each with its own bounds; a negative cutoff keeps the reference's gate
    t = golden_inputs(golden, "traj3")
    tm = C.Mol(t)
    tsrc = np.zeros(tm.numAtoms, bool)
    tsrc[t["sel2"][t["sel2"] != 350]] = True                         # (without the NaN atom: numpy's min / max would be NaN)
    for cutoff in (3.5, -3.5):
        got = W.within_molecule(tm, tsrc, cutoff, frames=[0, 1, 2], exclusive=exclusive, ctx=EmuContext())
        for f in range(3):
            want = np.zeros(tm.numAtoms, bool)
            xyz = t["coords"][f]
            R.within_distance(xyz, cutoff, np.arange(tm.numAtoms), np.flatnonzero(tsrc), xyz[tsrc].min(axis=0), xyz[tsrc].max(axis=0), want)
            if exclusive:
                want[tsrc] = False
            assert np.array_equal(got[:, f], want), (cutoff, f)
    ctx = EmuContext()
    assert not W.within_molecule(tm, np.zeros(tm.numAtoms, bool), 3.5, frames=[0, 1], ctx=ctx).any() and ctx.calls == 0     # an empty source


def test_argument_errors_are_refused(W):
    xyz = np.zeros((5, 3, 2), np.float32)
    u = lambda *a: np.array(a, np.uint32)   # noqa: E731
    ctx = EmuContext()
    with pytest.raises(ValueError, match="out of range"):
        W.within(xyz, u(0, 5), u(1), 3.0, ctx=ctx)
    with pytest.raises(ValueError, match="out of range"):
        W.within(xyz, u(0), np.array([-1]), 3.0, ctx=ctx)
    with pytest.raises(ValueError, match="float32"):
        W.within(xyz.astype(np.float64), u(0), u(1), 3.0, ctx=ctx)
    with pytest.raises(ValueError, match="integer index"):
        W.within(xyz, np.array([0.0]), u(1), 3.0, ctx=ctx)
    with pytest.raises(ValueError, match="mask must have shape"):
        W.within(xyz, np.ones(4, bool), u(1), 3.0, ctx=ctx)
    with pytest.raises(ValueError, match="frames"):
        W.within(xyz, u(0), u(1), 3.0, frames=[2], ctx=ctx)
    with pytest.raises(ValueError, match="bounds"):
        W.within(xyz, u(0), u(1), 3.0, ctx=ctx, _gate=np.zeros((1, 2, 3), np.float32))
    res = np.zeros(1, bool)
    f3 = np.zeros(3, np.float32)
    with pytest.raises(ValueError, match="uint32"):
        W.within_distance(xyz[:, :, 0], 3.0, np.array([0]), u(1), f3, f3, res, ctx=ctx)
    with pytest.raises(ValueError, match="results"):
        W.within_distance(xyz[:, :, 0], 3.0, u(0), u(1), f3, f3, np.zeros(2, bool), ctx=ctx)
    with pytest.raises(ValueError, match="results"):
        W.within_distance(xyz[:, :, 0], 3.0, u(0), u(1), f3, f3, np.zeros(1, np.uint8), ctx=ctx)
    with pytest.raises(ValueError, match="shape"):
        W.within_distance(xyz[:, :, 0], 3.0, u(0), u(1), np.zeros(2, np.float32), f3, res, ctx=ctx)
    with pytest.raises(ValueError, match="float32"):
        W.within_distance(xyz[:, :, 0], 3.0, u(0), u(1), np.zeros(3), f3, res, ctx=ctx)
    with pytest.raises(ValueError, match="natoms, 3"):
        W.within_distance(xyz, 3.0, u(0), u(1), f3, f3, res, ctx=ctx)
    assert ctx.calls == 0
    with pytest.raises(TypeError, match="CUDA tensor"):
        W.within_trajectory(xyz, u(0), u(1), 3.0)


def test_the_emulated_plan_refuses_bad_sizes():
    import ctypes
    info = np.zeros(8)
    L = ctypes.c_longlong
    st = E.lib().emu_within(None, L(-1), L(1), None, L(0), None, L(0), ctypes.c_float(1.0), None, 0, 0, None, info.ctypes.data_as(ctypes.c_void_p))
    assert st == 1 and E.lib().emu_within_last_error().decode() == "negative size"


def test_install_swaps_both_names_and_uninstall_restores(W, monkeypatch):
    pkg, utils, sel_pkg, sel = (types.ModuleType("moleculekit"), types.ModuleType("moleculekit.atomselect_utils"),
                                types.ModuleType("moleculekit.atomselect"), types.ModuleType("moleculekit.atomselect.atomselect"))

    def reference_within_distance(*a):
        raise AssertionError("the reference's loop was called")

    utils.within_distance = reference_within_distance
    sel.within_distance = reference_within_distance                  # (from moleculekit.atomselect_utils import within_distance)
    pkg.atomselect_utils, pkg.atomselect, sel_pkg.atomselect = utils, sel_pkg, sel
    for name, mod in (("moleculekit", pkg), ("moleculekit.atomselect_utils", utils), ("moleculekit.atomselect", sel_pkg),
                      ("moleculekit.atomselect.atomselect", sel)):
        monkeypatch.setitem(sys.modules, name, mod)
    assert W.install() is reference_within_distance
    assert utils.within_distance is W.within_distance and sel.within_distance is W.within_distance
    assert W.install() is reference_within_distance                  # idempotent
    assert utils.within_distance is W.within_distance
    W.uninstall()
    assert utils.within_distance is reference_within_distance and sel.within_distance is reference_within_distance
    W.uninstall()
    assert utils.within_distance is reference_within_distance and sel.within_distance is reference_within_distance
    assert W.install() is reference_within_distance and sel.within_distance is W.within_distance
    W.uninstall()


def test_the_library_declares_the_entry_points():
    from moleculekit_amd import _lib
    for sym in ("mkamd_within_distance_dev", "mkamd_within_distance_host", "mkamd_ctx_set_within_plan"):
        assert sym in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mkamd_distance.h")).read()
    assert all(f"int {s}(" in header for s in ("mkamd_within_distance_dev", "mkamd_within_distance_host", "mkamd_ctx_set_within_plan"))
