"""CPU tier of the shell densities (moleculekit_amd/shell.py).

1. The numpy restatement of the reference's histogram (tests/shell_restatement.py, distances from the compiled oracle) EQUAL to the
   array the reference holds for its own MetricShell test.
2. The kernels' source on the SIMT emulation (tests/emu/emu_shell.cpp, -ffp-contract=off): counts EQUAL to the restatement's, in
   both lane assignments.
3. shell_thresholds by brute force; the workspace bound; the host logic of shell.py with the emulation standing in for the library.
"""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shell_cases as C  # noqa: E402
import shell_restatement as R  # noqa: E402

F32, U32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def E():
    import emu_shell_build
    emu_shell_build.build()
    return emu_shell_build


@pytest.fixture(scope="module")
def real():
    mol, g = C.fixture()
    edges, vol = R.edges_and_volumes(4, 3)
    chains = C.selection_chains(4507, g["mol_heavy"])
    return mol, g, edges, vol, chains, R.counts(R.oracle_dist, mol.coords, mol.box, g["ca"], g["mol_heavy"], chains, edges)


def both_kernels(E, coords, box, sel1, sel2, chains, edges, *, symmetric=False, pbc=True, truncate=None):
    """the restatement's counts, after asserting that BOTH lane assignments (forced) reproduce them"""
    from moleculekit_amd.shell import shell_thresholds
    want = R.counts(R.oracle_dist, coords, box, sel1, sel2, chains, edges, symmetric=symmetric, pbc=pbc, truncate=truncate)
    thr = shell_thresholds(edges, truncate)
    for avoid, name in ((E.AVOID_ATOMS, "k_shell_frames"), (E.AVOID_FRAMES, "k_shell_atoms")):
        got = E.shell_counts(coords, box, sel1, sel2, chains, thr, symmetric=symmetric, pbc=pbc, avoid=avoid)
        assert name in E.last_kernel() and (E.last_kernel().endswith("<true>") == bool(pbc))
        assert got.dtype == np.int32 and np.array_equal(got, want), f"{name}: {int((got != want).sum())} of {want.size} counts differ"
    return want


# ---------------------------------------------------------------------------------------------
# 1. the restatement against the reference-held array
# ---------------------------------------------------------------------------------------------
def test_restatement_equals_the_reference_held_array(real):
    _, g, _, vol, _, counts = real
    got = R.density(counts, vol)
    assert got.dtype == np.float64 and got.shape == (200, 1108)
    assert np.array_equal(got, g["refdata"])
    assert counts.sum() > 1000                                   # (not an empty comparison: 99.3 % zeros, the rest counts)


def test_fixture_selections_are_the_reference_test_s(real):
    mol, g, *_ = real
    assert np.all(mol.name[g["ca"]] == "CA") and len(g["ca"]) == 277
    assert np.all(mol.resname[g["mol_heavy"]] == "MOL") and np.all(mol.element[g["mol_heavy"]] != "H") and len(g["mol_heavy"]) == 9


# ---------------------------------------------------------------------------------------------
# 2. the kernels on the emulation
# ---------------------------------------------------------------------------------------------
def test_emu_real_trajectory_both_lane_assignments(E, real):
    mol, g, edges, _, chains, counts = real
    assert np.array_equal(both_kernels(E, mol.coords, mol.box, g["ca"], g["mol_heavy"], chains, edges), counts)
    # left to itself the plan runs lanes along the 200 frames
    from moleculekit_amd.shell import shell_thresholds
    E.shell_counts(mol.coords, mol.box, g["ca"], g["mol_heavy"], chains, shell_thresholds(edges))
    assert E.last_kernel() == "mkamd::k_shell_frames<true>"


@pytest.mark.parametrize("F", [1, 3, 70])
@pytest.mark.parametrize("n2", [1, 63, 1000])
@pytest.mark.parametrize("n1", [1, 7, 64, 300])
def test_emu_random_periodic_boxes(E, n1, n2, F):
    coords, box, sel1, sel2, chains = C.random_case(n1, n2, F, seed=1000 * n1 + 10 * n2 + F)
    want = both_kernels(E, coords, box, sel1, sel2, chains, R.edges_and_volumes(4, 3)[0])
    if n2 >= 63:
        assert want.sum() > 0


def test_emu_plan_chooses_by_frames_and_atoms(E):
    from moleculekit_amd.shell import shell_thresholds
    thr = shell_thresholds(np.arange(0, 15, 3))
    for n2, F, name in ((1000, 1, "k_shell_atoms"), (1000, 70, "k_shell_frames"), (9, 3, "k_shell_atoms"), (2, 40, "k_shell_frames")):
        coords, box, sel1, sel2, chains = C.random_case(3, n2, F, seed=5)
        E.shell_counts(coords, box, sel1, sel2, chains, thr)
        assert name in E.last_kernel(), (n2, F, E.last_kernel())


@pytest.mark.parametrize("mode", ["selections", "chains"])
def test_emu_symmetric(E, mode):
    coords, box = C.random_system(90, 5, seed=11, box_len=20.0)
    sel = np.sort(np.random.default_rng(3).permutation(90)[:70]).astype(U32)
    chains = C.selection_chains(90, sel) if mode == "selections" else np.random.default_rng(4).integers(0, 3, 90).astype(U32)
    want = both_kernels(E, coords, box, sel, sel, chains, R.edges_and_volumes(4, 3)[0], symmetric=True)
    assert want.sum() > 0
    # the rectangle counts the atom itself at distance 0 -- in no shell: the same numbers
    assert np.array_equal(both_kernels(E, coords, box, sel, sel, chains, R.edges_and_volumes(4, 3)[0]), want)


def test_emu_three_chains(E):
    coords, box, sel1, sel2, _ = C.random_case(40, 200, 6, seed=21, box_len=18.0)
    chains = np.random.default_rng(22).integers(0, 3, coords.shape[0]).astype(U32)
    edges = R.edges_and_volumes(4, 3)[0]
    want = both_kernels(E, coords, box, sel1, sel2, chains, edges)
    assert not np.array_equal(want, both_kernels(E, coords, box, sel1, sel2, chains, edges, pbc=False))       # (images matter here)


@pytest.mark.parametrize("truncate", [7.5, 7.3, 6, 6.0, 100.0, 0.5])
def test_emu_truncate_inside_a_shell_and_on_an_edge(E, truncate):
    coords, box, sel1, sel2, chains = C.random_case(20, 150, 4, seed=31, box_len=40.0)
    edges = R.edges_and_volumes(4, 3)[0]
    want = both_kernels(E, coords, box, sel1, sel2, chains, edges, truncate=truncate)
    if truncate < 12:
        # the quirk: every far atom lands in the shell that holds `truncate`
        s = int(np.searchsorted(edges, truncate, side="left")) - 1
        assert np.all(want.sum(axis=2) == 150) and np.all(want[:, :, s + 1:] == 0)


@pytest.mark.parametrize("numshells,shellwidth", [(4, 0.7), (32, 0.7), (1, 3), (1, 2.5), (4, 3), (32, 1), (9, 2), (17, 1.1)])
def test_emu_shell_numbers_and_float_widths(E, numshells, shellwidth):
    coords, box, sel1, sel2, chains = C.random_case(9, 400, 3, seed=41, box_len=14.0)
    edges = R.edges_and_volumes(numshells, shellwidth)[0]
    assert len(edges) == numshells + 1
    want = both_kernels(E, coords, box, sel1, sel2, chains, edges)
    assert want.sum() > 0


def test_emu_overlapping_unequal_and_duplicate_selections(E):
    coords, box = C.random_system(120, 4, seed=51, box_len=16.0)
    edges = R.edges_and_volumes(4, 3)[0]
    sel1, sel2 = np.arange(0, 80, dtype=U32), np.arange(40, 120, dtype=U32)
    want = both_kernels(E, coords, box, sel1, sel2, C.selection_chains(120, sel2), edges)
    assert want.sum() > 0
    dup1, dup2 = np.array([5, 5, 7, 5, 90], U32), np.array([3, 3, 3, 50, 51, 50, 5], U32)
    want = both_kernels(E, coords, box, dup1, dup2, C.selection_chains(120, dup2), edges)
    assert np.array_equal(want[:, 0], want[:, 1]) and np.array_equal(want[:, 0], want[:, 3])


def test_emu_nan_coordinate_and_zero_box(E):
    coords, box, sel1, sel2, chains = C.random_case(12, 100, 3, seed=61, box_len=15.0)
    edges = R.edges_and_volumes(4, 3)[0]
    clean = both_kernels(E, coords, box, sel1, sel2, chains, edges)
    bad = coords.copy()
    bad[sel2[3], 1, 1] = np.nan
    bad[sel1[2], 0, 2] = np.nan
    want = both_kernels(E, bad, box, sel1, sel2, chains, edges)
    assert np.all(want[2, 2] == 0) and np.array_equal(want[0], clean[0]) and want[1].sum() <= clean[1].sum()
    both_kernels(E, bad, box, sel1, sel2, chains, edges, truncate=7.5)               # (a NaN is not "above" truncate either)
    # periodic with a zero box: every wrapped separation is NaN in the reference, and in no shell
    zero = np.zeros_like(box)
    want = both_kernels(E, coords, zero, sel1, sel2, chains, edges)
    assert want.sum() == 0
    inf = coords.copy()
    inf[sel2[0], 0, 0] = np.inf
    both_kernels(E, inf, box, sel1, sel2, chains, edges, pbc=False)
    w = both_kernels(E, inf, box, sel1, sel2, chains, edges, pbc=False, truncate=4.0)
    assert np.all(w[0].sum(axis=1) == 100)                                            # (an infinite distance IS above truncate)


def test_emu_exact_edges_and_one_ulp_either_side(E):
    coords, box, sel1, sel2, chains = C.edge_case()
    edges = R.edges_and_volumes(4, 3)[0]
    from oracle import oracle
    d2 = oracle.dist_trajectory(coords, box, sel1, sel2, chains, False, False, squared=True)[0]
    d = oracle.dist_trajectory(coords, box, sel1, sel2, chains, False, False)[0]
    for r in (3.0, 6.0, 9.0):
        r2 = F32(r * r)
        # the case holds what it says: d2 exactly r^2, and its float32 neighbours on both sides; d exactly r and its neighbours
        assert {float(np.nextafter(r2, F32(0))), float(r2), float(np.nextafter(r2, F32(1e9)))} <= set(d2.tolist())
        assert {float(np.nextafter(F32(r), F32(0))), float(r), float(np.nextafter(F32(r), F32(100)))} <= set(d.tolist())
    for pbc in (False, True):
        want = both_kernels(E, coords, box, sel1, sel2, chains, edges, pbc=pbc)       # (one chain: nothing wraps)
        assert want[0, 0].tolist() == [int(((d > lo) & (d <= hi)).sum()) for lo, hi in zip(edges[:-1], edges[1:])]


@pytest.mark.parametrize("width", [3, 1, 0.7, 2.5, 1.1, 0.1, 7])
def test_shell_thresholds_by_brute_force(width):
    from moleculekit_amd.shell import shell_thresholds
    edges = np.arange(width * 33, step=width)[:33]
    thr = shell_thresholds(edges)
    assert thr.dtype == F32 and thr.shape == edges.shape and thr[0] == 0
    for e, t in zip(edges, thr):
        x = t
        for _ in range(64):
            x = np.nextafter(x, F32(-1))
        around = [x]
        for _ in range(128):
            around.append(np.nextafter(around[-1], F32(np.inf)))
        around = np.array(around, F32)
        around = around[around >= 0]
        # what the reference asks of the float32 root against the edge (int or float64: numpy compares in float64)
        assert np.array_equal(around <= t, np.sqrt(around).astype(np.float64) <= float(e)), (width, e)
    # truncate: every edge at or above float32(truncate) is passed by everything
    tr = 2.5 * width
    t2 = shell_thresholds(edges, truncate=tr)
    assert np.array_equal(np.isinf(t2), edges >= float(F32(tr))) and np.array_equal(t2[~np.isinf(t2)], thr[~np.isinf(t2)])


def test_shell_thresholds_refuses_bad_edges():
    from moleculekit_amd.shell import shell_thresholds
    for bad in ([3], [0, 3, 2], [-1, 2], [0, np.nan], [[0, 1]]):
        with pytest.raises(ValueError):
            shell_thresholds(bad)
    with pytest.raises(TypeError):
        shell_thresholds(["a", "b"])


def test_emu_workspace_does_not_grow_with_the_second_selection(E):
    """nothing proportional to n1 * n2: doubling n2 at fixed n1 and F may add at most the linear term F * n2 * 16 bytes"""
    from moleculekit_amd.shell import shell_thresholds
    thr = shell_thresholds(np.arange(0, 15, 3))
    for avoid in (E.AVOID_ATOMS, E.AVOID_FRAMES):
        ws = []
        for n2 in (400, 800, 1600):
            coords, box, sel1, sel2, chains = C.random_case(64, n2, 2, seed=71)
            E.shell_counts(coords, box, sel1, sel2, chains, thr, avoid=avoid)
            ws.append(E.last_workspace())
        n1, F, S = 64, 2, 4
        assert ws[0] <= (n1 + 400) * F * 16 + F * n1 * (S + 1) * 4
        assert ws[1] - ws[0] <= 400 * F * 16 and ws[2] - ws[1] <= 800 * F * 16, ws


def test_emu_refusals(E):
    from moleculekit_amd.shell import shell_thresholds
    coords, box, sel1, sel2, chains = C.random_case(3, 5, 2, seed=81)
    with pytest.raises(ValueError, match="numshells"):
        E.shell_counts(coords, box, sel1, sel2, chains, np.zeros(34, F32))
    with pytest.raises(ValueError, match="numshells"):
        E.shell_counts(coords, box, sel1, sel2, chains, np.zeros(1, F32))
    with pytest.raises(ValueError, match="non-decreasing"):
        E.shell_counts(coords, box, sel1, sel2, chains, np.array([0, 9, 4], F32))
    with pytest.raises(ValueError, match="non-decreasing"):
        E.shell_counts(coords, box, sel1, sel2, chains, np.array([0, np.nan, 4], F32))
    with pytest.raises(ValueError, match="symmetric"):
        E.shell_counts(coords, box, sel1, sel2, chains, shell_thresholds([0, 3]), symmetric=True)
    # empty selections: a cleared result
    assert E.shell_counts(coords, box, sel1, sel2[:0], chains, shell_thresholds([0, 3, 6])).tolist() == np.zeros((2, 3, 2), int).tolist()
    assert E.shell_counts(coords, box, sel1[:0], sel2, chains, shell_thresholds([0, 3, 6])).shape == (2, 0, 2)


# ---------------------------------------------------------------------------------------------
# 3. host logic: the emulation stands in for the library
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch, E):
    from moleculekit_amd import _lib
    calls = []

    def arr(addr, ctype, n):
        return np.ctypeslib.as_array((ctype * max(n, 1)).from_address(addr))[:n].copy() if addr else None

    class FakeLib:
        def mkamd_shell_counts_host(self, h, coords, N, F, box, s1, n1, s2, n2, ch, symmetric, pbc, thr, n_edges, out):
            a = dict(N=N, F=F, sel1=arr(s1, ctypes.c_uint32, n1), sel2=arr(s2, ctypes.c_uint32, n2), chains=arr(ch, ctypes.c_uint32, N),
                     symmetric=symmetric, pbc=pbc, thr=arr(thr, ctypes.c_float, n_edges),
                     coords=arr(coords, ctypes.c_float, N * 3 * F).reshape(N, 3, F), box=arr(box, ctypes.c_float, 3 * F).reshape(3, F))
            calls.append(a)
            got = E.shell_counts(a["coords"], a["box"], a["sel1"], a["sel2"], a["chains"], a["thr"], symmetric=symmetric, pbc=pbc)
            np.ctypeslib.as_array((ctypes.c_int32 * got.size).from_address(out))[:] = got.reshape(-1)
            return 0

    class FakeCtx:
        _h = None

    monkeypatch.setattr(_lib, "load", lambda: FakeLib())
    monkeypatch.setattr(_lib, "default_context", lambda *a: FakeCtx())
    return calls


def test_metricshell_projects_the_reference_test_through_the_host_path(fake, real):
    from moleculekit_amd.shell import MetricShell
    mol, g, *_ = real
    ca = np.zeros(4507, bool)
    ca[g["ca"]] = True
    got = MetricShell(ca, g["mol_heavy"], periodic="selections").project(mol)
    k = fake[-1]
    assert got.dtype == np.float64 and np.array_equal(got, g["refdata"])
    assert (k["symmetric"], k["pbc"]) == (0, 1) and np.array_equal(k["sel1"], g["ca"]) and np.array_equal(k["sel2"], g["mol_heavy"])
    assert k["chains"].sum() == 4507 + 9 and np.all(k["chains"][g["mol_heavy"]] == 2)


def small_mol(with_box=True):
    coords = np.zeros((3, 3, 1), F32)
    coords[1, :, 0] = [0.5, 0, 0]
    coords[2, :, 0] = [0, 1.5, 0]
    return types.SimpleNamespace(coords=coords, box=np.full((3, 1), 20, F32) if with_box else None, name=np.array(["CL"] * 3),
                                 resname=np.array(["CL"] * 3), resid=np.arange(3), chain=np.array(["A", "A", "B"]), numFrames=1, numAtoms=3)


def test_metricshell_simple_is_the_reference_s_own_small_test(fake):
    """the reference's test_metricshell_simple: three atoms, both parameter sets, its literals"""
    from moleculekit_amd.shell import MetricShell
    mol = small_mol()
    got = MetricShell("all", "all", periodic=None).project(mol)
    assert fake[-1]["symmetric"] == 1 and fake[-1]["pbc"] == 0
    assert np.allclose(got, [[0.01768388256576615, 0, 0, 0, 0.01768388256576615, 0, 0, 0, 0.01768388256576615, 0, 0, 0]])
    got = MetricShell([0, 1, 2], np.ones(3, bool), numshells=2, shellwidth=1, periodic=None).project(mol)
    assert np.allclose(got, [[0.23873241, 0.03410463, 0.23873241, 0.03410463, 0.0, 0.06820926]])


def test_metricshell_argument_errors(fake):
    from moleculekit_amd.shell import MetricShell, shell_counts, shell_counts_trajectory
    mol = small_mol()
    with pytest.raises(DeprecationWarning, match="pbc"):
        MetricShell("all", "all", periodic=None, pbc=True)
    with pytest.raises(RuntimeError, match="Invalid periodic option"):
        MetricShell("all", "all", periodic="box")
    with pytest.raises(ValueError, match="numshells"):
        MetricShell("all", "all", periodic=None, numshells=33)
    with pytest.raises(ValueError, match="numshells"):
        MetricShell("all", "all", periodic=None, numshells=0)
    for box in (None, np.zeros((3, 1), F32)):
        mol.box = box
        for periodic in ("chains", "selections"):
            with pytest.raises(RuntimeError, match="No periodic box dimensions"):
                MetricShell("all", [0], periodic=periodic).project(mol)
    mol.box = np.full((3, 2), 20, F32)
    with pytest.raises(RuntimeError, match="Different number of frames"):
        MetricShell("all", [0], periodic="chains").project(mol)
    mol.box = None
    assert MetricShell("all", [0], periodic=None).project(mol).shape == (1, 12)          # (no box needed without a periodic mode)
    assert fake[-1]["symmetric"] == 0
    with pytest.raises(TypeError, match="selection language"):
        MetricShell("name CL", "all", periodic=None).project(mol)
    with pytest.raises(IndexError):
        MetricShell([3], "all", periodic=None).project(mol)
    with pytest.raises(IndexError):
        MetricShell(np.ones(4, bool), "all", periodic=None).project(mol)
    n = len(fake)
    c, b, ch = mol.coords, np.zeros((3, 1), F32), np.zeros(3, U32)
    with pytest.raises(ValueError, match="dtype"):
        shell_counts(c.astype(np.float64), b, [0], [1], ch, [0, 3])
    with pytest.raises(ValueError, match="natoms, 3, nframes"):
        shell_counts(np.zeros((3, 2, 1), F32), b, [0], [1], ch, [0, 3])
    with pytest.raises(ValueError, match="box"):
        shell_counts(c, np.zeros((3, 2), F32), [0], [1], ch, [0, 3])
    with pytest.raises(ValueError, match="chains"):
        shell_counts(c, b, [0], [1], ch[:2], [0, 3])
    with pytest.raises(ValueError, match="symmetric"):
        shell_counts(c, b, [0, 1], [1, 0], ch, [0, 3], symmetric=True)
    with pytest.raises(ValueError, match="numshells"):
        shell_counts(c, b, [0], [1], ch, np.arange(34))
    with pytest.raises(TypeError, match="CUDA"):
        shell_counts_trajectory(c, b, [0], [1], ch, [0, 3])
    assert len(fake) == n
    # sel1 order is the output order; a box of another shape is fine without pbc
    got = shell_counts(c, None, [2, 0], [0, 1, 2], ch, [0, 1, 2], pbc=False)
    assert got.tolist() == [[[0, 2], [1, 1]]]
    # "chains": the chain letters digitized; "selections": 2 on sel2
    mol.box = np.full((3, 1), 20, F32)
    MetricShell("all", [0], periodic="chains").project(mol)
    assert fake[-1]["chains"].tolist() == [0, 0, 1] and fake[-1]["pbc"] == 1
    MetricShell("all", [0], periodic="selections").project(mol)
    assert fake[-1]["chains"].tolist() == [2, 1, 1]


def test_metricshell_get_mapping_strings():
    from moleculekit_amd.shell import MetricShell
    mol = small_mol()
    mol.resname = np.array(["CL", "NA", "CL"])
    m = MetricShell([2, 0], "all", periodic=None, numshells=2, shellwidth=1.5).getMapping(mol)
    assert list(m["type"]) == ["shell"] * 4 and list(m["atomIndexes"]) == [0, 0, 2, 2]
    assert list(m["description"]) == ["Density of sel2 atoms in shell 0.0-1.5 A centered on atom CL 0 CL",
                                      "Density of sel2 atoms in shell 1.5-3.0 A centered on atom CL 0 CL",
                                      "Density of sel2 atoms in shell 0.0-1.5 A centered on atom CL 2 CL",
                                      "Density of sel2 atoms in shell 1.5-3.0 A centered on atom CL 2 CL"]
    m = MetricShell("all", "all", periodic=None).getMapping(mol)
    assert len(m["type"]) == 12 and list(m["description"])[5] == "Density of sel2 atoms in shell 3-6 A centered on atom NA 1 CL"


def test_install_swaps_project_of_a_stub_moleculekit(monkeypatch):
    from moleculekit_amd import shell as S
    seen = []

    class RefMetricShell:
        numshells, shellwidth, symmetrical = 5, 2, True
        metricdistance = types.SimpleNamespace(sel1="name CL", sel2="name CL", periodic="selections", truncate=7.5)

        def project(self, mol):
            seen.append("reference")

    ref_project = RefMetricShell.project
    pkg, proj, mod = types.ModuleType("moleculekit"), types.ModuleType("moleculekit.projections"), types.ModuleType("moleculekit.projections.metricshell")
    mod.MetricShell = RefMetricShell
    proj.metricshell, pkg.projections = mod, proj
    for name, m in (("moleculekit", pkg), ("moleculekit.projections", proj), ("moleculekit.projections.metricshell", mod)):
        monkeypatch.setitem(sys.modules, name, m)
    monkeypatch.setattr(S, "_project", lambda mol, sel1, sel2, periodic, numshells, shellwidth, truncate, symmetrical:
                        seen.append(("gpu", int(sel1.sum()), int(sel2.sum()), periodic, numshells, shellwidth, truncate, symmetrical)))
    mol = types.SimpleNamespace(atomselect=lambda s: np.array([True, True, False]) if s == "name CL" else np.ones(3, bool))
    assert S.install() is ref_project
    assert S.install() is ref_project            # idempotent
    RefMetricShell().project(mol)
    S.uninstall()
    S.uninstall()
    RefMetricShell().project(mol)
    assert seen == [("gpu", 2, 2, "selections", 5, 2, 7.5, True), "reference"]
    assert RefMetricShell.project is ref_project
