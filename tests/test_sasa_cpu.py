"""CPU tier of the surface area (moleculekit_amd/sasa.py).

1. The float32 restatement (tests/sasa_restatement.py) against the arrays the reference holds for its own MetricSasa test, at the
   reference's tolerances on every entry: atom 0.1, residue 0.3 square Angstrom (one sphere point of a carbon is 0.126).
2. The kernels' source on the SIMT emulation (tests/emu/emu_sasa.cpp, -ffp-contract=off) BIT-EQUAL to the restatement.
3. The host logic of sasa.py with a fake library.
"""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sasa_cases as C  # noqa: E402
import sasa_restatement as R  # noqa: E402

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.fixture(scope="module")
def E():
    import emu_sasa_build
    emu_sasa_build.build()
    return emu_sasa_build


@pytest.fixture(scope="module")
def restated():
    """the restatement on the fixture's two frames: (xyz nm, radii nm, residue mapping, areas float32 [2, 4480] in square nm)"""
    xyz, rad, mapping = C.fixture_nm()
    return xyz, rad, mapping, R.areas(xyz, rad, 960)


# ---------------------------------------------------------------------------------------------
# 1. the arithmetic, settled against the reference's held arrays
# ---------------------------------------------------------------------------------------------
def test_restatement_reproduces_reference_held_atom_areas(restated):
    _, g = C.fixture()
    got = restated[3] * 100
    d = np.abs(got - g["sasa_atom"])
    print(f"atom entries outside 0.1: {int((d > 0.1).sum())} of {d.size}; max |diff| {d.max():.3g}")
    assert got.shape == (2, 4480)
    assert np.allclose(got, g["sasa_atom"], atol=0.1), f"{int((d > 0.1).sum())} entries outside 0.1, max {d.max()}"


def test_restatement_reproduces_reference_held_residue_areas(restated):
    _, g = C.fixture()
    _, _, mapping, area = restated
    got = R.scatter(area, mapping, np.ones(4480, bool), np.zeros((2, 277), F32)) * 100
    d = np.abs(got - g["sasa_residue"])
    print(f"residue entries outside 0.3: {int((d > 0.3).sum())} of {d.size}; max |diff| {d.max():.3g}")
    assert np.allclose(got, g["sasa_residue"], atol=0.3), f"{int((d > 0.3).sum())} entries outside 0.3, max {d.max()}"


def test_restatement_selection_of_one_atom(restated):
    """the reference's test_selection_and_filtering: atom 20 alone within 1e-2 of the full run, and different without the others"""
    xyz, rad, _, area = restated
    sel = np.zeros(4480, bool)
    sel[20] = True
    one = R.sasa(xyz, rad, 960, sel=sel)[:, [20]] * 100
    assert np.allclose(one, area[:, [20]] * 100, atol=1e-2)
    alone = R.sasa(xyz[:, [20]], rad[[20]], 960) * 100
    assert not np.allclose(alone, area[:, [20]] * 100, atol=1e-2)


# ---------------------------------------------------------------------------------------------
# 2. the kernels on the emulation, bit for bit
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 60, 960, 1000])
def test_emu_sphere_points_bit_equal(E, n):
    assert np.array_equal(bits(E.sphere_points(n)), bits(R.sphere_points(n)))


def test_emu_fixture_frames_bit_equal(E, restated):
    xyz, rad, mapping, area = restated
    assert np.array_equal(bits(E.sasa(xyz, rad, 960)), bits(area))
    exp = R.scatter(area, mapping, np.ones(4480, bool), np.zeros((2, 277), F32))
    assert np.array_equal(bits(E.sasa(xyz, rad, 960, mapping=mapping)), bits(exp))
    # from Angstrom, the division by 10 in the kernel
    mol, g = C.fixture()
    xa = np.ascontiguousarray(np.transpose(mol.coords[g["protein"]], (2, 0, 1)))
    assert np.array_equal(bits(E.sasa(xa, rad, 960, coord_div=10.0)), bits(area))


@pytest.mark.parametrize("n_points", [1, 60, 960, 1000])
@pytest.mark.parametrize("n", [1, 2, 7, 300, 5000])
def test_emu_globules_bit_equal(E, n, n_points):
    xyz, rad = C.globule(n, seed=n + n_points)
    assert np.array_equal(bits(E.sasa(xyz, rad, n_points)), bits(R.sasa(xyz, rad, n_points)))


def test_emu_isolated_and_buried_atoms(E):
    n = 960
    r = F32(0.31)
    got = E.sasa(np.zeros((1, 1, 3), F32), np.array([r]), n)
    assert got[0, 0] == ((F32(4.0 * np.pi / n) * F32(n)) * r) * r
    # an atom inside a much larger one: every point buried
    xyz = np.array([[[0.0, 0.0, 0.0], [0.05, 0.0, 0.0]]], F32)
    got = E.sasa(xyz, np.array([0.2, 1.0], F32), n)
    assert got[0, 0] == 0.0 and got[0, 1] > 0.0
    assert np.array_equal(bits(got), bits(R.sasa(xyz, np.array([0.2, 1.0], F32), n)))


def test_emu_selection_mapping_and_prefilled_output(E):
    xyz, rad = C.globule(300, seed=5, frames=3)
    rng = np.random.default_rng(5)
    sel = rng.random(300) < 0.4
    mapping = np.cumsum(rng.random(300) < 0.2).astype(np.int32)
    pre = np.full((3, int(mapping.max()) + 1), -1, F32)
    got = E.sasa(xyz, rad, 60, mapping=mapping, sel=sel, out=pre.copy())
    exp = R.sasa(xyz, rad, 60, mapping=mapping, sel=sel, out=pre.copy())
    assert np.array_equal(bits(got), bits(exp))
    untouched = np.setdiff1d(np.arange(pre.shape[1]), mapping[sel])
    assert len(untouched) and np.all(got[:, untouched] == -1)


def test_emu_more_neighbours_than_the_list_holds(E):
    """every atom of a dense cluster is everybody's neighbour: the points are tested against the frame's atoms directly"""
    xyz, _ = C.globule(E.max_neighbours() + 200, seed=2)
    xyz = (xyz * F32(0.25)).astype(F32)
    rad = np.full(xyz.shape[1], 0.9, F32)
    sel = np.zeros(xyz.shape[1], bool)
    sel[::97] = True
    assert np.array_equal(bits(E.sasa(xyz, rad, 60, sel=sel)), bits(R.sasa(xyz, rad, 60, sel=sel)))


def test_emu_refusals(E):
    xyz = np.array([[[0.0, 0.0, 0.0], [1e-6, 0.0, 0.0], [1.0, 0.0, 0.0]]], F32)
    out = np.full((1, 3), 7, F32)
    with pytest.raises(ValueError, match="on top of one another"):
        E.sasa(xyz, np.full(3, 0.3, F32), 60, out=out)
    assert np.all(out == 7)                                   # refused, not computed
    far = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.0]]], F32)
    with pytest.raises(ValueError, match="non-decreasing"):
        E.sasa(far, np.full(3, 0.3, F32), 60, mapping=np.array([0, 1, 0], np.int32), out=np.zeros((1, 2), F32))
    with pytest.raises(ValueError, match="outside"):
        E.sasa(far, np.full(3, 0.3, F32), 60, mapping=np.array([0, 1, 2], np.int32), out=np.zeros((1, 2), F32))
    with pytest.raises(ValueError, match="n_points"):
        E.sasa(far, np.full(3, 0.3, F32), 0)
    # the coincidence is looked for around SELECTED atoms only, as the reference does
    sel = np.array([False, False, True])
    assert np.array_equal(bits(E.sasa(xyz, np.full(3, 0.3, F32), 60, sel=sel)), bits(R.sasa(xyz, np.full(3, 0.3, F32), 60, sel=sel)))


def test_emu_runs_are_bitwise_equal(E):
    xyz, rad = C.globule(300, seed=9, frames=2)
    mapping = (np.arange(300) // 11).astype(np.int32)
    assert np.array_equal(bits(E.sasa(xyz, rad, 960, mapping=mapping)), bits(E.sasa(xyz, rad, 960, mapping=mapping)))


# ---------------------------------------------------------------------------------------------
# 3. host logic (a fake library)
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def fake(monkeypatch):
    from moleculekit_amd import _lib
    calls = []

    class FakeLib:
        def mkamd_sasa_host(self, h, coords, N, F, keep, n, radii, n_points, mapping, mask, div, out, n_out):
            calls.append(dict(coords=coords, N=N, F=F, keep=keep, n=n, n_points=n_points, div=div, n_out=n_out,
                              radii=np.ctypeslib.as_array((ctypes.c_float * n).from_address(radii)).copy(),
                              mapping=np.ctypeslib.as_array((ctypes.c_int32 * n).from_address(mapping)).copy(),
                              mask=np.ctypeslib.as_array((ctypes.c_int32 * n).from_address(mask)).copy(),
                              keep_list=None if keep is None else np.ctypeslib.as_array((ctypes.c_uint32 * n).from_address(keep)).copy()))
            return 0

    class FakeCtx:
        _h = None

    monkeypatch.setattr(_lib, "load", lambda: FakeLib())
    monkeypatch.setattr(_lib, "default_context", lambda *a: FakeCtx())
    return calls


def test_sasa_refuses_wrong_dtypes_and_shapes(fake):
    from moleculekit_amd import sasa as S
    c = np.zeros((4, 3, 2), F32)
    with pytest.raises(ValueError, match="dtype"):
        S.sasa(c.astype(np.float64), np.ones(4))
    with pytest.raises(ValueError, match="natoms, 3, nframes"):
        S.sasa(np.zeros((4, 2, 2), F32), np.ones(4))
    with pytest.raises(TypeError):
        S.sasa([[0, 0, 0]], np.ones(1))
    with pytest.raises(ValueError, match="radii"):
        S.sasa(c, np.ones(3))
    with pytest.raises(ValueError, match="atom_mapping"):
        S.sasa(c, np.ones(4), atom_mapping=np.zeros(4))
    with pytest.raises(ValueError, match="non-decreasing"):
        S.sasa(c, np.ones(4), atom_mapping=np.array([0, 1, 0, 1]))
    with pytest.raises(ValueError, match="n_points"):
        S.sasa(c, np.ones(4), n_points=0)
    with pytest.raises(IndexError):
        S.sasa(c, np.ones(4), sel=[4])
    with pytest.raises(TypeError, match="CUDA"):
        S.sasa_trajectory(np.zeros((2, 4, 3), F32), np.ones(4))
    assert not fake


def test_sasa_host_call_arguments(fake):
    from moleculekit_amd import sasa as S
    c = np.random.default_rng(0).normal(size=(6, 3, 4)).astype(F32)
    out = S.sasa(c, np.full(5, 3.1), n_points=60, keep=np.array([True, True, False, True, True, True]), sel=[0, -1],
                 atom_mapping=[0, 0, 1, 1, 2])
    k = fake[-1]
    assert out.shape == (4, 3) and out.dtype == F32
    assert k["coords"] == c.ctypes.data and (k["N"], k["F"], k["n"], k["n_points"], k["div"], k["n_out"]) == (6, 4, 5, 60, 10.0, 3)
    assert k["keep_list"].tolist() == [0, 1, 3, 4, 5] and k["mask"].tolist() == [1, 0, 0, 0, 1] and k["mapping"].tolist() == [0, 0, 1, 1, 2]
    assert np.array_equal(bits(k["radii"]), bits(np.full(5, F32(3.1) / F32(10))))
    S.sasa(c, np.full(6, 3.1))
    assert fake[-1]["keep"] is None and fake[-1]["n"] == 6 and fake[-1]["mapping"].tolist() == list(range(6))


def test_metricsasa_masks_indices_and_setdiff_error(fake):
    from moleculekit_amd.sasa import MetricSasa
    mol, g = C.fixture()
    p = g["protein"]
    out = MetricSasa(p).project(mol)
    k = fake[-1]
    assert out.shape == (2, 4480) and np.all(out == 0)        # one column per selected atom (the fake adds nothing)
    assert k["n"] == 4507 and k["mask"].sum() == 4480
    out = MetricSasa(np.flatnonzero(p), filtersel=p, mode="residue").project(mol)
    k = fake[-1]
    assert out.shape == (2, 277) and k["n"] == 4480 and k["n_out"] == 277 and np.array_equal(k["keep_list"], np.flatnonzero(p))
    import sasa_restatement
    from moleculekit_amd._sasa_radii import ATOMIC_RADII
    assert np.array_equal(bits(k["radii"]), bits(sasa_restatement.radii_nm([ATOMIC_RADII[e] for e in g["element"][p]])))
    assert np.array_equal(k["mapping"], C.fixture_nm()[2])
    out = MetricSasa([20], filtersel=p).project(mol)
    assert out.shape == (2, 1) and fake[-1]["mask"].tolist() == [0] * 20 + [1] + [0] * 4459
    # the reference's test_set_diff_error: index 3000 selected, everything but index 3000 kept
    with pytest.raises(RuntimeError, match="subset of `filtersel`"):
        MetricSasa([3000], filtersel=np.arange(4507) != 3000).project(mol)
    with pytest.raises(ValueError, match="mode"):
        MetricSasa(p, mode="chain").project(mol)
    with pytest.raises(TypeError, match="selection language"):
        MetricSasa("protein").project(mol)
    with pytest.raises(KeyError):                              # Cl has a radius, an unknown element has none
        mol.element = mol.element.copy()
        mol.element[0] = "Xx"
        MetricSasa(p).project(mol)


def test_metricsasa_get_mapping_matches_the_reference_list():
    from moleculekit_amd.sasa import MetricSasa
    mol, g = C.fixture()
    p = g["protein"]
    m = MetricSasa(p, mode="atom").getMapping(mol)
    assert np.array_equal(m.atomIndexes, np.arange(4480))
    m = MetricSasa(p, mode="residue").getMapping(mol)
    assert np.array_equal(m.atomIndexes, g["residue_first_atoms"])
    assert list(m.type)[:2] == ["SASA", "SASA"] and list(m.description)[:2] == ["SASA of GLU 1 N", f"SASA of {g['resname'][17]} {g['resid'][17]} N"]


def test_element_radii_table():
    from moleculekit_amd._sasa_radii import ATOMIC_RADII, CHECKED
    assert {e: ATOMIC_RADII[e] for e in CHECKED} == {"H": 0.12, "C": 0.17, "N": 0.155, "O": 0.152, "S": 0.18}
    with pytest.raises(KeyError):
        ATOMIC_RADII["Xx"]


def test_install_swaps_project_of_a_stub_moleculekit(monkeypatch):
    from moleculekit_amd import sasa as S
    seen = []

    class RefMetricSasa:
        _sel, _filtersel, _probeRadius, _numSpherePoints, _mode = "protein", "all", 0.14, 960, "atom"

        def project(self, mol):
            seen.append("reference")

    ref_project = RefMetricSasa.project
    pkg, proj, mod = types.ModuleType("moleculekit"), types.ModuleType("moleculekit.projections"), types.ModuleType("moleculekit.projections.metricsasa")
    mod.MetricSasa = RefMetricSasa
    proj.metricsasa, pkg.projections = mod, proj
    for name, m in (("moleculekit", pkg), ("moleculekit.projections", proj), ("moleculekit.projections.metricsasa", mod)):
        monkeypatch.setitem(sys.modules, name, m)
    monkeypatch.setattr(S, "_project", lambda mol, sel, filtersel, probe, n, mode: seen.append(("gpu", int(sel.sum()), int(filtersel.sum()), probe, n, mode)))
    mol = types.SimpleNamespace(atomselect=lambda s: np.array([True, True, False]) if s == "protein" else np.ones(3, bool))
    assert S.install() is ref_project
    assert S.install() is ref_project            # idempotent
    RefMetricSasa().project(mol)
    S.uninstall()
    S.uninstall()
    RefMetricSasa().project(mol)
    assert seen == [("gpu", 2, 3, 0.14, 960, "atom"), "reference"]
    assert RefMetricSasa.project is ref_project
