"""CPU tier of the alignment row (moleculekit_amd/align.py, csrc/align_kernels.h): the kernels through the host SIMT emulation
(tests/emu_align_build.py) against the float64 Kabsch restatement of tests/align_cases.py, the cases the GPU tier runs on the hardware
(tests/align_cases.py: the same inputs under the same conditions), and the host logic of the drop-in."""
import os
import sys
import types

import numpy as np
import pytest

from tests import align_cases as C
from tests.align_cases import apply64, fit_rmsd64, kabsch64, np_pp_align, rot, traj, within_ulp

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "align_cases.npz")


@pytest.fixture(scope="module")
def E():
    from tests import emu_align_build
    emu_align_build.build()
    return emu_align_build


@pytest.mark.parametrize("N,nsel,F", [(7, 7, 5), (50, 23, 9), (301, 300, 3), (1000, 1, 2), (5000, 5000, 1), (130, 64, 17)])
def test_transforms_and_apply_match_float64_kabsch(E, N, nsel, F):
    rng = np.random.default_rng(N + nsel + F)
    xyz, ref = traj(rng, N, F)
    sel = np.sort(rng.choice(N, nsel, replace=False))
    aff, fit = E.transforms(xyz, ref, sel, sel)
    out = E.apply(xyz, aff)
    for f in range(F):
        R, t = kabsch64(xyz[f][sel], ref[sel])
        assert abs(np.linalg.det(aff[f, :9].reshape(3, 3)) - 1.0) < 1e-12
        if nsel >= 3:
            assert np.abs(aff[f, :9] - R.ravel()).max() < 1e-9
            assert within_ulp(out[f], apply64(xyz[f], R, t))
            exp = fit_rmsd64(xyz[f][sel], ref[sel], R, t)
            assert abs(fit[f] - exp) <= 1e-9 * exp
        else:                                                    # one atom: R = I, the atom lands on its reference
            assert np.array_equal(aff[f, :9], np.eye(3).ravel())
            assert np.abs(out[f][sel] - ref[sel]).max() <= 2 * np.spacing(np.float32(np.abs(ref[sel]).max()))


def test_segmented_sums_equal_plans(E):
    """few frames x a large selection: the selection is split over segments (fewer CUs assumed: fewer segments); the results
    agree to rounding and every plan is deterministic"""
    rng = np.random.default_rng(3)
    xyz, ref = traj(rng, 4000, 2)
    sel = np.arange(4000)
    assert E.plan(4000, 2)["segs"] > 1
    a1, r1 = E.transforms(xyz, ref, sel, sel, cus=256)
    a2, r2 = E.transforms(xyz, ref, sel, sel, cus=1)
    assert np.abs(a1 - a2).max() < 1e-9
    b1, s1 = E.transforms(xyz, ref, sel, sel, cus=256)
    assert np.array_equal(a1, b1) and np.array_equal(r1, s1)
    m1 = E.rmsd(xyz, ref, sel, sel, a1, cus=256)
    m2 = E.rmsd(xyz, ref, sel, sel, a1, cus=1)
    assert np.abs(m1 - m2).max() <= 2 * np.spacing(m1.max())
    assert np.allclose(m1, r1, rtol=1e-5)


def test_reflected_copy_gives_proper_rotation(E):
    rng = np.random.default_rng(11)
    P = rng.normal(scale=5, size=(30, 3)).astype(np.float32)
    xyz = (P * np.array([-1, 1, 1], np.float32))[None]
    aff, fit = E.transforms(xyz, P, np.arange(30), np.arange(30))
    R = aff[0, :9].reshape(3, 3)
    assert abs(np.linalg.det(R) - 1.0) < 1e-12
    Rk, tk = kabsch64(xyz[0], P)
    assert np.abs(R - Rk).max() < 1e-9
    assert abs(fit[0] - fit_rmsd64(xyz[0], P, Rk, tk)) < 1e-9 * fit[0]


@pytest.mark.parametrize("kind", ["coplanar", "collinear"])
def test_degenerate_selections(E, kind):
    C.check_degenerate(E, kind)


def test_one_atom_and_zero_covariance_give_identity(E):
    C.check_coincident(E)


def test_empty_selection_gives_nan(E):
    C.check_empty(E)


def test_matching_frames_and_frame_lists(E):
    rng = np.random.default_rng(9)
    xyz, ref = traj(rng, 40, 8)
    refs, _ = traj(rng, 40, 8)
    sel = np.arange(0, 40, 3)
    frames = np.array([6, 1, 4])
    aff, _ = E.transforms(xyz, refs, sel, sel, frames=frames, matching=True)
    out = E.apply(xyz, aff, frames=frames)
    for i, f in enumerate(frames):
        R, t = kabsch64(xyz[f][sel], refs[f][sel])
        assert within_ulp(out[f], apply64(xyz[f], R, t))
    untouched = [f for f in range(8) if f not in frames]
    assert np.array_equal(out[untouched], xyz[untouched])
    aff2, _ = E.transforms(xyz, refs, sel, sel, frames=frames, refframe=5)
    for i, f in enumerate(frames):
        R, t = kabsch64(xyz[f][sel], refs[5][sel])
        assert np.abs(aff2[i, :9] - R.ravel()).max() < 1e-9


@pytest.mark.parametrize("N", [1, 5, 333, 1025, 2049])
def test_apply_any_alignment(E, N):
    """3N not a multiple of 4, frames whose start is not 16-byte aligned, input and output in different phases"""
    rng = np.random.default_rng(N)
    F = 3
    base = rng.normal(scale=100, size=F * N * 3 + 8).astype(np.float32)
    aff = np.concatenate([np.stack([rot(rng).ravel() for _ in range(F)]), rng.uniform(-50, 50, (F, 3))], axis=1)
    for off_in, off_out in ((0, 0), (1, 1), (3, 2), (2, 0)):
        src = base[off_in:off_in + F * N * 3]
        outbuf = np.full(F * N * 3 + 8, 7.0, np.float32)
        dst = outbuf[off_out:off_out + F * N * 3]
        E.apply_raw(src, N, aff, np.array([2, 0]), dst)
        x = src.reshape(F, N, 3)
        y = dst.reshape(F, N, 3)
        for i, f in enumerate([2, 0]):
            A = aff[i]
            exp = (x[f].astype(np.float64) @ A[:9].reshape(3, 3).T + A[9:]).astype(np.float32)
            assert np.array_equal(y[f], exp)
        assert np.all(y[1] == 7.0)
        assert np.all(outbuf[:off_out] == 7.0) and np.all(outbuf[off_out + F * N * 3:] == 7.0)


def test_apply_in_place(E):
    rng = np.random.default_rng(2)
    xyz, ref = traj(rng, 77, 4)
    aff, _ = E.transforms(xyz, ref, np.arange(77), np.arange(77))
    exp = E.apply(xyz, aff)
    E.apply(xyz, aff, out=xyz)
    assert np.array_equal(xyz, exp)


def test_rmsd_after_alignment(E):
    rng = np.random.default_rng(4)
    xyz, ref = traj(rng, 60, 6)
    aln = np.arange(0, 60, 2)
    rsel = np.arange(1, 60, 2)
    aff, _ = E.transforms(xyz, ref, aln, aln)
    got = E.rmsd(xyz, ref, rsel, rsel, aff)
    moved = E.apply(xyz, aff)
    for f in range(6):
        d = moved[f][rsel].astype(np.float64) - ref[rsel].astype(np.float64)
        assert got[f] == np.float32(np.sqrt((d * d).sum() / len(rsel)))


def test_runs_are_bitwise_equal(E):
    rng = np.random.default_rng(8)
    xyz, ref = traj(rng, 500, 5)
    sel = np.arange(500)
    a1, r1 = E.transforms(xyz, ref, sel, sel)
    a2, r2 = E.transforms(xyz, ref, sel, sel)
    assert np.array_equal(a1, a2) and np.array_equal(r1, r2)
    assert np.array_equal(E.apply(xyz, a1), E.apply(xyz, a2))


# ---- the cases of tests/align_cases.py: what the GPU tier runs on the hardware, here on the emulation ------------------------------
@pytest.mark.parametrize("F", C.WIDTH_FRAMES)
@pytest.mark.parametrize("n", C.WIDTH_SIZES)
def test_group_widths_and_partial_waves(E, n, F):
    for matching in (False, True):
        for listed in (False, True):
            C.check_width(E, n, F, matching, listed)


def test_matching_frames_segmented(E):
    C.check_segmented_match(E)


def test_unsegmented_long_walk_and_its_segmented_twin(E):
    """(the 4 096 frames that make the device's plan walk 300 atoms with one lane group run in the GPU tier only; here 8 frames on a plan
    for one compute unit take the same form)"""
    assert E.plan(300, 8, cus=1)["segs"] == 1 and E.plan(300, 4096)["segs"] == 1 and E.plan(300, 3)["segs"] > 1
    C.check_two_plans(E, 8, 1, cus=1)


@pytest.mark.parametrize("N", C.APPLY_SIZES)
def test_apply_every_placement_gives_the_same_bits(E, N):
    C.check_apply_alignment(E, N)


def test_rmsd_over_another_selection(E):
    C.check_rmsd(E)


@pytest.mark.parametrize("matching", [False, True])
def test_route_case_matches_the_restatement(E, matching):
    """the data the GPU tier hands to _pp_align and to align_trajectory (equal bits there), here against the float64 restatement in the
    reference's layout"""
    c = C.route_case()
    for frames in C.ROUTE_FRAMES:
        fr = None if frames is None else np.array(frames)
        aff, _ = E.transforms(c.xyz, c.refs_fm if matching else c.ref_fm, c.sel, c.sel, frames=fr, matching=matching)
        got = E.apply(c.xyz, aff, frames=fr).transpose(1, 2, 0)
        exp = np_pp_align(c.coords, c.refs if matching else c.ref, c.sel, c.sel, range(c.F) if frames is None else frames, 0, matching)
        assert within_ulp(got, exp)


# ---- the fixture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["selfalign", "refmol", "matching", "selected"])
def test_restatement_reproduces_reference_held_arrays(case):
    g = np.load(GOLDEN)
    lig = g["lig_coords"]
    sel, refsel = g[f"{case}_sel"], g[f"{case}_refsel"]
    if case == "selfalign":
        refc = lig
    elif case == "matching":
        refc = np.roll(lig, 3, axis=2)
    else:
        refc = lig[sel][:, :, 3:4]
    out = np_pp_align(lig, refc, sel, refsel, g[f"{case}_frames"], int(g[f"{case}_refframe"]), bool(g[f"{case}_matching"]))
    assert np.abs(out - g[f"{case}_held"]).max() < 1e-3
    assert np.abs(out - g[f"{case}_real"]).max() < 1e-3


# ---- host logic of the drop-in -------------------------------------------------------------------------------------------
def test_pp_align_refuses_non_float32():
    from moleculekit_amd import align
    c = np.zeros((4, 3, 2), np.float64)
    with pytest.raises(ValueError, match="dtype"):
        align._pp_align(c, c, np.arange(4), np.arange(4), [0, 1], 0, False)
    with pytest.raises(TypeError):
        align._pp_align(c.tolist(), c, np.arange(4), np.arange(4), [0, 1], 0, False)


def test_pp_align_index_and_mask_selections():
    from moleculekit_amd import align
    mask = np.array([True, False, True, True])
    assert align._index(mask, 4, "sel").tolist() == [0, 2, 3]
    assert align._index(np.array([-1, 0]), 4, "sel").tolist() == [3, 0]
    with pytest.raises(IndexError):
        align._index(np.array([4]), 4, "sel")
    with pytest.raises(IndexError):
        align._index(np.array([True, False]), 4, "sel")


def test_pp_align_host_call_arguments(monkeypatch):
    """what the drop-in hands to the library: contiguous float32 buffers, uint32 selections, in place on the caller's array
    (or a copy), the reference read from the caller's array before anything is written (aliasing: a snapshot), NaN for an
    empty selection is the library's to produce -- the call is made, not refused"""
    from moleculekit_amd import _lib, align
    calls = []

    class FakeLib:
        def mkamd_align_host(self, h, coords, N, F, ref, Nr, Fr, sel, refsel, n, frames, K, refframe, matching):
            calls.append(dict(coords=coords, ref=ref, N=N, F=F, n=n, K=K, refframe=refframe, matching=matching, sel=sel))
            return 0

    class FakeCtx:
        _h = None

    monkeypatch.setattr(_lib, "load", lambda: FakeLib())
    monkeypatch.setattr(_lib, "default_context", lambda *a: FakeCtx())
    c = np.random.default_rng(0).normal(size=(6, 3, 4)).astype(np.float32)
    assert align._pp_align(c, c, np.arange(6), np.arange(6), range(4), 0, False, inplace=True) is None
    assert calls[-1]["coords"] == c.ctypes.data and calls[-1]["K"] == 4 and calls[-1]["n"] == 6
    out = align._pp_align(c, c, np.ones(6, bool), np.ones(6, bool), [3, 1], -1, False)
    assert out is not c and calls[-1]["coords"] == out.ctypes.data and calls[-1]["refframe"] == 3
    align._pp_align(c, c, np.zeros(0, np.int64), np.zeros(0, np.int64), [0], 0, False, inplace=True)
    assert calls[-1]["n"] == 0
    with pytest.raises(ValueError, match="matchingframes"):
        align._pp_align(c, c[:, :, :2].copy(), np.arange(6), np.arange(6), [0], 0, True)
    with pytest.raises(ValueError):
        align._pp_align(c, c, np.arange(6), np.arange(5), [0], 0, False)
    strided = np.asfortranarray(c)
    align._pp_align(strided, c, np.arange(6), np.arange(6), [0], 0, False, inplace=True)   # non-contiguous: written back


def test_install_swaps_pp_align_of_a_stub_moleculekit(monkeypatch):
    from moleculekit_amd import align

    seen = []

    def ref_pp_align(coords, refcoords, sel, refsel, frames, refframe, matchingframes, inplace=False):
        seen.append("reference")

    stub_pkg = types.ModuleType("moleculekit")
    stub = types.ModuleType("moleculekit.align")
    stub._pp_align = ref_pp_align
    stub_pkg.align = stub
    monkeypatch.setitem(sys.modules, "moleculekit", stub_pkg)
    monkeypatch.setitem(sys.modules, "moleculekit.align", stub)
    monkeypatch.setattr(align, "_pp_align", lambda *a, **k: seen.append("gpu"))

    def molecule_align():                   # molecule.py:765: imported at call time
        from moleculekit.align import _pp_align
        _pp_align(None, None, None, None, [0], 0, False, inplace=True)

    assert align.install() is ref_pp_align
    assert align.install() is ref_pp_align          # idempotent
    molecule_align()
    align.uninstall()
    molecule_align()
    assert seen == ["gpu", "reference"]
    assert stub._pp_align is ref_pp_align


def test_align_with_pbc_raises():
    from moleculekit_amd import batch
    c = np.zeros((4, 3, 2), np.float32)
    with pytest.raises(ValueError, match="align"):
        next(batch.iterVoxelizeTrajectory(c, np.ones((4, 1), np.float32), [0, 0, 0], [8, 8, 8], box=np.full((3, 2), 30, np.float32),
                                          align=(c[:, :, 0], np.arange(4))))
    xtc = os.path.join(HERE, "golden", "xtc", "metricdistance_traj.xtc")
    with pytest.raises(ValueError, match="pbc"):
        next(batch.iterVoxelizeXTC(xtc, np.ones((4507, 1), np.float32), [0, 0, 0], [8, 8, 8], pbc=True,
                                   align=(np.zeros((3, 3), np.float32), np.arange(3))))
