"""CPU tier of the steric-clash search (moleculekit_amd/clashes.py, moleculekit_amd/distance.py: find_clashes).

Pass criterion, here and in tests/test_gpu_clashes.py: the three arrays -- pairs, distances, overlaps -- EQUAL what the compiled
reference returned on the golden cases (tests/golden/clash_cases.npz), rows in order, with no tolerance: every float32 operation of
the pair test is the reference's.  Held against the golden arrays: the numpy restatement (tests/clashes_restatement.py) and the
product's kernels under their launch plan on the host emulation (tests/emu/emu_clashes.cpp), with a thread per owner, a wave per owner
and the plan's own choice.  Also: the arithmetic the reference's result rests on (numpy's float32 einsum is the unfused sum of
squares), the vectorised exclusion table against the restatement's set, the host-side argument errors, ``find_clashes`` on the
emulated library, and ``install`` / ``uninstall`` against a stub module.
"""
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import clashes_cases as C  # noqa: E402
import clashes_restatement as R  # noqa: E402
from moleculekit_amd import bonds as B  # noqa: E402
from moleculekit_amd import clashes as CL  # noqa: E402
from moleculekit_amd import distance as D  # noqa: E402

F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(HERE, "golden", "clash_cases.npz")
PLANS = {"unforced": 0, "wave": 1, "thread": 2}          # AVOID_THREAD forces the wave kernels and the other way round


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def emu():
    import emu_clashes_build
    emu_clashes_build.build()
    return emu_clashes_build


def golden_inputs(golden, name):
    """the case as the fixture holds it: what went to the reference"""
    src = str(golden[f"{name}/inputs_of"]) if f"{name}/inputs_of" in golden else name
    eb, e14, guess = (bool(v) for v in golden[f"{name}/flags"])
    c = {k: golden[f"{src}/{k}"] for k in ("coords", "element", "name", "bonds")}
    c.update(sel1=golden[f"{name}/sel1"] if f"{name}/sel1" in golden else None, sel2=golden[f"{name}/sel2"] if f"{name}/sel2" in golden else None,
             overlap=float(golden[f"{name}/overlap"]), exclude_bonded=eb, exclude_14=e14, guess_bonds=guess)
    c["bonds_used"] = golden[f"{src}/bonds_used"] if guess else c["bonds"]
    return c


def golden_result(golden, name):
    return golden[f"{name}/pairs"], golden[f"{name}/distances"], golden[f"{name}/overlaps"]


def same_result(got, want, what):
    (gp, gd, go), (wp, wd, wo) = (tuple(np.asarray(x) for x in got[:3]), want)
    assert gp.dtype == np.int64 and gd.dtype == F32 and go.dtype == F32, f"{what}: dtypes {gp.dtype}, {gd.dtype}, {go.dtype}"
    assert gp.shape == wp.shape and gd.shape == wd.shape and go.shape == wo.shape, f"{what}: {gp.shape} rows, the reference has {wp.shape}"
    assert np.array_equal(gp, wp), f"{what}: pairs differ, first at row {int(np.flatnonzero((gp != wp).any(axis=1))[0])}"
    assert gd.tobytes() == wd.tobytes(), f"{what}: distances differ in {int((gd != wd).sum())} rows"
    assert go.tobytes() == wo.tobytes(), f"{what}: overlaps differ in {int((go != wo).sum())} rows"


def library_inputs(c):
    """what the library's entry points take, from a case: radii, masks (mask2 None: self mode), the exclusion table, the cutoff"""
    n = len(c["coords"])
    radii = CL.clash_radii(c["element"])
    mask1 = R.mask_of(c["sel1"], n)
    mask2 = R.mask_of(c["sel2"], n) if c["sel2"] is not None else None
    if mask2 is not None and np.array_equal(mask1, mask2):
        mask2 = None
    ex = CL.clash_exclusions(c["bonds_used"], n, c["exclude_bonded"], c["exclude_14"]) if (c["exclude_bonded"] or c["exclude_14"]) else None
    return radii, mask1, mask2, ex, CL.clash_cutoff(radii.max(), c["overlap"])


def emulated(emu, c, plan="unforced"):
    radii, mask1, mask2, ex, cutoff = library_inputs(c)
    if not mask1.any() or (mask2 is not None and not mask2.any()):
        return R.empty()
    p, d, o, info = emu.find_clashes(c["coords"], radii, mask1, mask2, None if ex is None else ex.start, None if ex is None else ex.partner,
                                     c["overlap"], cutoff, avoid=PLANS[plan])
    return (*R.canonical(p, d, o), info) if len(p) else (p, d, o, info)


# ------------------------------------------------------------------------------------------------
# the contract
# ------------------------------------------------------------------------------------------------
def test_the_cases_are_the_cases_they_are_meant_to_be():
    C.check()


@pytest.mark.parametrize("name", C.GOLDEN)
def test_the_fixture_holds_the_cases_inputs(golden, name):
    c, g = C.case(name), golden_inputs(golden, name)
    for k in ("coords", "element", "name", "bonds"):
        assert np.array_equal(c[k], g[k]) and c[k].dtype == g[k].dtype, k
    for k in ("sel1", "sel2"):
        assert (c[k] is None) == (g[k] is None) and (c[k] is None or np.array_equal(c[k], g[k])), k
    assert (c["overlap"], c["exclude_bonded"], c["exclude_14"], c["guess_bonds"]) == (g["overlap"], g["exclude_bonded"], g["exclude_14"], g["guess_bonds"])
    assert np.array_equal(C.bonds_used(name), g["bonds_used"]), "the restated guesser's bonds are not the reference's"


@pytest.mark.parametrize("name", C.GOLDEN)
def test_restatement_gives_the_references_arrays(golden, name):
    same_result(C.restated(name), golden_result(golden, name), name)


def test_golden_ties_are_in_pair_order(golden):
    for name in C.GOLDEN:
        p, _, o = golden_result(golden, name)
        assert np.all(np.diff(o) <= 0), name
        tie = np.diff(o) == 0
        key = p[:, 0] * 10 ** 6 + p[:, 1]
        assert np.all(np.diff(key)[tie] > 0), name
    assert len(set(golden["ties/overlaps"].tolist())) == 1 and len(golden["ties/overlaps"]) == 8


def test_einsum_on_float32_rows_is_the_unfused_sum_of_squares():
    """the reference takes dist2 from numpy.einsum("ij,ij->i"): on float32 rows of three it is (dx dx + dy dy) + dz dz with every operation
    rounded on its own -- what the pair kernels compute -- and neither of the fused forms a compiler would contract it into"""
    rng = np.random.default_rng(301)
    rows = (rng.normal(size=(10 ** 6, 3)) * rng.choice([1e-3, 0.3, 2.0, 40.0, 3e4], size=(10 ** 6, 1))).astype(F32)
    bits = rng.integers(0x3A000000, 0x47000000, size=(200000, 3), dtype=np.int64).astype(np.uint32).view(F32)       # 2^-11 .. 2^15, every mantissa
    bits[::2] *= F32(-1)
    edge = np.array([[0, 0, 0], [1, 1, 1], [3, 4, 12], [np.nextafter(F32(1), F32(2)), 1, 1], [1e-20, 1e-20, 1e-20], [1e19, 1e19, 1e19]], F32)
    with np.errstate(over="ignore", under="ignore"):
        for d in (rows, bits, edge):
            got = np.einsum("ij,ij->i", d, d)
            assert got.dtype == F32 and got.tobytes() == R.dist2_f32(d).tobytes()
        d = np.concatenate([rows, bits])
        got = np.einsum("ij,ij->i", d, d)
        x, y, z = (d[:, k].astype(F64) for k in range(3))                # (a float32 product is exact in float64)
        xx, yy = (d[:, 0] * d[:, 0]).astype(F32), (d[:, 1] * d[:, 1]).astype(F32)
        fused_chain = (((x * x).astype(F32).astype(F64) + y * y).astype(F32).astype(F64) + z * z).astype(F32)       # fma(dz, dz, fma(dy, dy, dx dx))
        fused_last = ((xx + yy).astype(F32).astype(F64) + z * z).astype(F32)                                         # fma(dz, dz, dx dx + dy dy)
    assert int((got != fused_chain).sum()) > 1000 and int((got != fused_last).sum()) > 1000


def test_thresholds_are_float32_and_strict(golden):
    c = C.case("threshold_edges")
    rows = {tuple(r) for r in golden["threshold_edges/pairs"].tolist()}
    radii = R.radii_of(c["element"])
    for label, first, clash in c["labels"]:
        assert ((first, first + 1) in rows) == clash, label
        d = np.sqrt(R.dist2_f32(c["coords"][first:first + 1] - c["coords"][first + 1:first + 2])).astype(F32)[0]
        thr = R.threshold_of(radii[first:first + 1], radii[first + 1:first + 2], c["overlap"])[0]
        want = {"below": np.nextafter(thr, F32(0)), "at": thr, "above": np.nextafter(thr, F32(np.inf))}[label.split("_")[1]]
        assert d == want, label
    cutoff = R.cutoff_of(radii, c["overlap"])
    inside, outside = (next(f for lab, f, _ in c["labels"] if lab == k) for k in ("CC_below_inside_cutoff", "CC_below_outside_cutoff"))
    d2 = R.dist2_f64(c["coords"][[inside, outside]], c["coords"][[inside + 1, outside + 1]])
    assert d2[0] <= cutoff * cutoff < d2[1]                              # the same float32 distance on either side of the kd-tree's radius


# ------------------------------------------------------------------------------------------------
# host logic of the product
# ------------------------------------------------------------------------------------------------
def test_clash_radii_rules():
    r = CL.clash_radii(np.array(["C", "H", "Xx", "Rf", "Cs", "CL", "Cl"]))
    assert r.dtype == F32 and r.tolist() == [F32(1.7), F32(1.1), F32(1.7), F32(1.7), F32(3.43), F32(1.7), F32(1.75)]
    assert CL.clash_cutoff(F32(1.7), 0.6) == 2.0 * float(F32(1.7)) - 0.6
    for name in ("elements", "3ptb"):
        assert np.array_equal(CL.clash_radii(C.case(name)["element"]), R.radii_of(C.case(name)["element"]))


@pytest.mark.parametrize("name", ["excl_11", "excl_10", "excl_01", "excl_00", "cross_overlap", "overlap_06", "3ptb"])
def test_exclusion_table_is_the_restatements_set(name):
    c = C.case(name)
    bonds = C.bonds_used(name)
    for eb, e14 in ((True, True), (True, False), (False, True), (False, False)) if name != "3ptb" else ((True, True),):
        ex = CL.clash_exclusions(bonds, len(c["coords"]), eb, e14)
        want = R.excluded_set(bonds.astype(np.int64), eb, e14) if (eb or e14) else set()
        assert ex.start.dtype == np.uint32 and ex.partner.dtype == np.uint32 and ex.start.shape == (len(c["coords"]) + 1,)
        assert ex.start[0] == 0 and ex.start[-1] == len(ex.partner) == len(want)
        p = ex.pairs()
        assert {tuple(r) for r in p.tolist()} == want and np.all(p[:, 0] <= p[:, 1])
        assert np.all(np.diff(p[:, 0] * 10 ** 6 + p[:, 1]) > 0)                       # rows ascending: the kernels search them


def test_exclusion_table_on_random_graphs():
    rng = np.random.default_rng(302)
    for _ in range(60):
        n, nb = int(rng.integers(1, 40)), int(rng.integers(0, 70))
        bonds = rng.integers(0, n, size=(nb, 2))
        for eb, e14 in ((True, True), (True, False), (False, True)):
            assert {tuple(r) for r in CL.clash_exclusions(bonds, n, eb, e14).pairs().tolist()} == R.excluded_set(bonds, eb, e14)
    with pytest.raises(ValueError, match="out of range"):
        CL.clash_exclusions([(0, 5)], 5)
    assert len(CL.clash_exclusions(np.zeros((0, 2), np.uint32), 4).partner) == 0


def test_host_side_argument_errors():
    c = C.case("overlap_06")
    mol = C.as_mol(c)
    with pytest.raises(ValueError, match="out of range"):
        D.find_clashes(mol, sel1=np.array([0, 60]), ctx=object())
    with pytest.raises(ValueError, match="shape"):
        D.find_clashes(mol, sel1=np.ones(59, bool), ctx=object())
    with pytest.raises(ValueError, match="boolean mask or an integer"):
        D.find_clashes(mol, sel1=np.array([0.5, 1.0]), ctx=object())
    bad = C.as_mol(c)
    bad.coords[7, 1, 0] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        D.find_clashes(bad, ctx=object())
    p, d, o = D.find_clashes(bad, sel1=np.array([1, 2, 3]), sel2=np.zeros(60, bool), ctx=object())      # an empty selection: no call
    assert p.shape == (0, 2) and p.dtype == np.int64 and d.dtype == F32 and o.dtype == F32 and d.shape == o.shape == (0,)
    with pytest.raises(TypeError, match="CUDA tensor"):
        CL.find_clashes_tensor(c["coords"], CL.clash_radii(c["element"]), np.ones(60, bool))


# ------------------------------------------------------------------------------------------------
# the kernels under their launch plan, emulated
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", list(PLANS))
@pytest.mark.parametrize("name", C.GOLDEN)
def test_emulated_kernels_give_the_references_arrays(emu, golden, name, plan):
    got = emulated(emu, golden_inputs(golden, name), plan)
    same_result(got, golden_result(golden, name), f"{name} / {plan}")
    if len(got) == 4 and got[3][5] > 0:                                    # a call that reached the pair kernels
        assert emu.last_kernel() == {"unforced": emu.WAVE_KERNEL, "wave": emu.WAVE_KERNEL, "thread": emu.THREAD_KERNEL}[plan]


def test_the_fill_order_is_the_same_under_both_plans(emu, golden):
    for name in ("cross_overlap", "lanes65", "faces"):
        c = golden_inputs(golden, name)
        radii, mask1, mask2, ex, cutoff = library_inputs(c)
        runs = [emu.find_clashes(c["coords"], radii, mask1, mask2, None if ex is None else ex.start, None if ex is None else ex.partner, c["overlap"],
                                 cutoff, avoid=a)[:3] for a in (1, 2, 1)]
        for other in runs[1:]:
            assert all(x.tobytes() == y.tobytes() for x, y in zip(runs[0], other)) and len(runs[0][0])


def test_the_one_box_cases_fill_a_waves_lanes(emu, golden):
    for name, count in (("lanes64", 64), ("lanes65", 65), ("crowded", 100)):
        info = emulated(emu, golden_inputs(golden, name))[3]
        assert info[4] == count and info[5] == count and info[6] == count, (name, info)


def test_many_owners_in_sparse_boxes_take_the_thread_kernels_unforced(emu):
    """17 576 owners, no crowded box: above the wave-per-owner plan's owner count (8 192).  Both plans give the same rows; a slab of them is
    held against the restatement"""
    c = C.lattice()
    radii = CL.clash_radii(c["element"])
    mask = np.ones(len(radii), bool)
    cutoff = CL.clash_cutoff(radii.max(), c["overlap"])
    thread = emu.find_clashes(c["coords"], radii, mask, None, None, None, c["overlap"], cutoff)
    assert emu.last_kernel() == emu.THREAD_KERNEL and thread[3][5] == len(radii) > 8192 and thread[3][4] < 64
    wave = emu.find_clashes(c["coords"], radii, mask, None, None, None, c["overlap"], cutoff, avoid=emu.AVOID_THREAD)
    assert emu.last_kernel() == emu.WAVE_KERNEL
    assert all(x.tobytes() == y.tobytes() for x, y in zip(thread[:3], wave[:3])) and len(thread[0]) > 1000
    slab = np.flatnonzero(c["coords"][:, 0] < 6.0)
    want = R.find_clashes(c["coords"], radii, C.NO_BONDS, sel1=slab, sel2=None, overlap=c["overlap"])
    p, d, o = R.canonical(*thread[:3])
    keep = np.isin(p[:, 0], slab) & np.isin(p[:, 1], slab)
    same_result((p[keep], d[keep], o[keep]), want, "lattice slab")


@pytest.mark.parametrize("plan", list(PLANS))
def test_over_cap_returns_the_status_not_a_list(emu, plan):
    c = C.over_cap()
    radii = CL.clash_radii(c["element"])
    with pytest.raises(ValueError, match=r"crowded box: box 0 .* holds 4097 atoms, more than the 4096"):
        emu.find_clashes(c["coords"], radii, np.ones(len(radii), bool), None, None, None, 0.6, CL.clash_cutoff(radii.max(), 0.6), avoid=PLANS[plan])


def test_the_pipeline_refuses_bad_arguments(emu):
    c = C.case("overlap_06")
    radii = CL.clash_radii(c["element"])
    ones = np.ones(60, bool)
    bad = c["coords"].copy()
    bad[3, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        emu.find_clashes(bad, radii, ones, None, None, None, 0.6, 2.8)
    unselected = ones.copy()
    unselected[3] = False
    assert len(emu.find_clashes(bad, radii, unselected, None, None, None, 0.6, 2.8)[0])          # ... in no selection: not looked at
    with pytest.raises(ValueError, match="finite"):
        emu.find_clashes(c["coords"], radii, ones, None, None, None, 0.6, np.inf)
    with pytest.raises(ValueError, match="max_boxes"):
        emu.find_clashes(c["coords"], radii, ones, None, None, None, 0.6, 2.8, max_boxes=0.5)
    with pytest.raises(ValueError, match="both arrays or neither"):
        emu.find_clashes(c["coords"], radii, ones, None, np.zeros(61, np.uint32), None, 0.6, 2.8)


def test_clash_grid_keeps_neighbours_in_adjacent_boxes(emu):
    """the box side is at least |cutoff| plus the margin of the float32 box arithmetic, at least 1 A, and grows with the grid"""
    nx, ny, nz, side = emu.clash_grid([0, 0, 0], [30, 30, 30], 2.8)
    assert side == 2.8 * (1 + 1 / 1024) and (nx, ny, nz) == (11, 11, 11) and F32(side) == C.grid_side(2.8)
    assert emu.clash_grid([0, 0, 0], [30, 30, 30], -2.8) == (nx, ny, nz, side)
    assert emu.clash_grid([0, 0, 0], [30, 30, 30], 0.0)[3] == 1 + 1 / 1024 and emu.clash_grid([0, 0, 0], [30, 30, 30], 0.25)[3] == 1 + 1 / 1024
    nx, ny, nz, side = emu.clash_grid([0, 0, 0], [1e5, 10, 10], 2.8)                  # a long axis: the margin follows the box count
    assert nx * ny * nz <= 4e6 and side >= 2.8 * (1 + nx / 2097152.0) > 2.8 * (1 + 1 / 1024)
    nx, ny, nz, side = emu.clash_grid([0, 0, 0], [3000, 3000, 3000], 2.8)             # ... and the escalation of the bond guesser's grid
    assert nx * ny * nz <= 4e6 and side > 2.8 * 1.26


# ------------------------------------------------------------------------------------------------
# find_clashes on the emulated library; the hook
# ------------------------------------------------------------------------------------------------
class EmulatedContext:
    """Context.find_clashes_host on the emulated kernels (the final order is then the restatement's sort, not the library's)"""

    def __init__(self, emu):
        self.emu = emu
        self.calls = 0

    def find_clashes_host(self, coords, radii, sel1, sel2, ex_start, ex_partner, overlap, cutoff, max_boxes=4e6):
        self.calls += 1
        assert coords.dtype == F32 and radii.dtype == F32 and sel1.dtype == np.uint32 and (sel2 is None or sel2.dtype == np.uint32)
        p, d, o, info = self.emu.find_clashes(coords, radii, sel1, sel2, ex_start, ex_partner, overlap, cutoff, max_boxes)
        p, d, o = R.canonical(p, d, o) if len(p) else (p, d, o)
        return p.astype(np.int32), d, o, info


@pytest.fixture
def emulated_library(emu, monkeypatch):
    """distance.find_clashes and bonds.guess_bonds on the emulated kernels instead of the device"""
    import emu_bonds_build

    def host_call(coords, radii, flags, grid_cutoff, max_boxes, cutoff_incr, ctx=None):
        pairs, grid, _ = emu_bonds_build.guess_bonds(coords, grid_cutoff, flags, radii, max_boxes, cutoff_incr)
        return pairs.astype(np.int32), grid

    monkeypatch.setattr(B, "_host_call", host_call)
    return EmulatedContext(emu)


@pytest.mark.parametrize("name", C.GOLDEN)
def test_find_clashes_on_the_emulated_library(emulated_library, golden, name):
    c = C.case(name)
    got = D.find_clashes(C.as_mol(c, frame=1, frames=3), ctx=emulated_library, **C.kwargs(c))
    same_result(got, golden_result(golden, name), name + " through find_clashes")


def test_find_clashes_takes_string_selections_from_the_molecule(emulated_library, golden):
    c = C.case("cross_disjoint")
    mol = C.as_mol(c)
    asked = []
    mol.atomselect = lambda sel: asked.append(sel) or R.mask_of(c["sel1"] if sel == "first" else c["sel2"], 48)
    got = D.find_clashes(mol, "first", "second", overlap=c["overlap"], guess_bonds=False, ctx=emulated_library)
    same_result(got, golden_result(golden, "cross_disjoint"), "string selections")
    assert asked == ["first", "second"]
    del mol.atomselect
    same_result(D.find_clashes(mol, "all", None, overlap=c["overlap"], guess_bonds=False, ctx=emulated_library),
                R.find_clashes(c["coords"], R.radii_of(c["element"]), c["bonds"], overlap=c["overlap"]), '"all" needs no atomselect')


def test_install_swaps_find_clashes_and_uninstall_restores(monkeypatch):
    pkg, dist = types.ModuleType("moleculekit"), types.ModuleType("moleculekit.distance")

    def find_clashes(mol, sel1=None, sel2=None, overlap=0.6, exclude_bonded=True, exclude_14=True, guess_bonds=True):
        return "the reference's find_clashes"

    dist.find_clashes = find_clashes
    pkg.distance = dist
    monkeypatch.setitem(sys.modules, "moleculekit", pkg)
    monkeypatch.setitem(sys.modules, "moleculekit.distance", dist)
    assert CL.install() is find_clashes and CL.install() is find_clashes           # idempotent
    assert dist.find_clashes is D.find_clashes
    CL.uninstall()
    assert dist.find_clashes is find_clashes
    CL.uninstall()
    assert dist.find_clashes is find_clashes and CL.install() is find_clashes and dist.find_clashes is D.find_clashes
    CL.uninstall()
