"""CPU tier of the explicit-centre occupancy path: k_occupancy_centers (csrc/kernels.h) behind run_centers (csrc/pipeline.h) on
the host SIMT emulation, at every workgroup width the launch rule picks (4, 8 and 16 waves, one and two channel groups), against
the oracle at the project's tolerance and -- where the kernel promises it -- bit for bit.  tests/test_gpu_centers.py makes the
same comparisons on the device; the cases are tests/centers_cases.py."""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import centers_cases as CC
from tests import emu_build as E
from tests.cases import TOL


def note(waves):
    return f"mkamd::k_occupancy_centers, {waves} waves"


def expected(case):
    return oracle.calculate_occupancy(case.centers, case.coords, np.asarray(case.sigmas, np.float64), box=case.box)


def run(case, rows=None):
    centers = case.centers if rows is None else case.centers[:rows]
    return E.occupancy_centers(centers, case.coords, case.sigmas, box=case.box)


def check(got, want, what=""):
    """|got - want| <= TOL and NaN where the oracle has NaN (it never has: `value > old` keeps them out)"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    err = np.abs(got.astype(np.float64) - want)
    worst = float(np.nanmax(err)) if err.size else 0.0
    print(f"{what}: worst |emulated - oracle| = {worst:.3e}")
    assert worst <= TOL, (what, worst)
    return worst


@functools.lru_cache(maxsize=None)
def block_whole(C):
    """(the emulated kernel's result for the whole centre list, the kernel note, the oracle's result): once per module"""
    case = CC.block_case(C)
    got = run(case)
    kernel = E.last_dist_kernel()
    want = expected(case)
    got.setflags(write=False); want.setflags(write=False)
    return got, kernel, want


# ---- the block rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 8, 9, 16])
def test_block_rule_on_each_side_of_both_thresholds(C):
    G = -(-C // CC.CHANNEL_GROUP)
    rng = np.random.default_rng(C)
    coords = rng.uniform(-1.0, 1.0, (1, 3)).astype(np.float32)
    sigmas = np.full((1, C), 2.0)
    sizes = CC.threshold_sizes(G)
    assert sizes == CC.THRESHOLDS[G]                       # the literal table of centers_cases.py
    centers = rng.uniform(-5.0, 5.0, (sizes[-1][0], 3))
    want = oracle.calculate_occupancy(centers, coords, sigmas)
    for V, waves in sizes:
        got = E.occupancy_centers(centers[:V], coords, sigmas)
        assert E.last_dist_kernel() == note(waves), (V, C)
        check(got, want[:V], f"threshold V = {V}, C = {C}")


# ---- every block size on one atom set: oracle, then bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 9])
def test_block_case_against_the_oracle_at_four_waves(C):
    got, kernel, want = block_whole(C)
    assert kernel == note(4)
    # the case says something: a good part of the ORACLE's values is far above the tolerance
    assert np.mean(want > 100 * TOL) >= 0.25
    check(got, want, f"block_case({C}), 4 waves")


@pytest.mark.parametrize("C", [3, 9])
def test_prefixes_at_eight_and_sixteen_waves_give_the_rows_of_the_whole_call(C):
    """The same centres in a shorter call run in wider workgroups, whose waves are dealt other atoms: the minimum is taken over
    bit patterns and the epilogue is shared, so not a bit may differ."""
    whole, _, want = block_whole(C)
    case = CC.block_case(C)
    for rows, waves in CC.block_prefixes(C)[1:]:
        got = run(case, rows)
        assert E.last_dist_kernel() == note(waves), (rows, C)
        assert np.array_equal(got, whole[:rows]), (rows, C, float(np.abs(got - whole[:rows]).max()))
        check(got, want[:rows], f"block_case({C}), {waves} waves")


@pytest.mark.parametrize("C", [3, 9])
def test_atom_order_does_not_change_a_bit(C):
    """Atoms, with their sigma rows, in another order land in other chunks and other waves: the same bits at every width."""
    whole, _, _ = block_whole(C)
    case = CC.block_case(C)
    perm = np.random.default_rng(11).permutation(len(case.coords))
    for rows, waves in CC.block_prefixes(C):
        got = E.occupancy_centers(case.centers[:rows], case.coords[perm], case.sigmas[perm])
        assert E.last_dist_kernel() == note(waves)
        assert np.array_equal(got, whole[:rows]), (rows, C)


@pytest.mark.parametrize("C", [3, 9])
def test_centre_order_permutes_the_rows(C):
    whole, _, _ = block_whole(C)
    case = CC.block_case(C)
    perm = np.random.default_rng(12).permutation(len(case.centers))
    got = E.occupancy_centers(case.centers[perm], case.coords, case.sigmas)
    assert E.last_dist_kernel() == note(4)
    assert np.array_equal(got, whole[perm])


def test_float32_sigmas_equal_float64_sigmas_of_the_same_values():
    case = CC.block_case(9)
    rows = CC.block_prefixes(9)[2][0]
    s32 = case.sigmas.astype(np.float32)
    assert np.array_equal(E.occupancy_centers(case.centers[:rows], case.coords, s32),
                          E.occupancy_centers(case.centers[:rows], case.coords, s32.astype(np.float64)))
    sp = CC.special_case(np.float32)
    assert sp.sigmas.dtype == np.float32
    assert np.array_equal(run(sp), E.occupancy_centers(sp.centers, sp.coords, sp.sigmas.astype(np.float64)))


# ---- sizes, edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CC.SHAPE_C)
def test_shapes_around_chunk_block_and_group_boundaries(C):
    worst = 0.0
    for (N, V, c), case in CC.shape_cases():
        if c != C:
            continue
        got = run(case)
        assert got.shape == (V, C) and E.last_dist_kernel() == note(16)
        if N == 0:
            assert not got.any()                           # every element written, with zero
        worst = max(worst, check(got, expected(case), f"N = {N}, V = {V}, C = {C}"))
    print(f"shapes, C = {C}: worst {worst:.3e}")


def test_cutoff_is_strict():
    """Zero on and outside the shell, the oracle's value inside, one double ulp either way in every coordinate.  Row 3,
    (3 - 1 ulp, 4, 0), is ON the shell only when d^2 is summed with one rounding per operation, as the reference does."""
    case, where = CC.cutoff_case()
    got, want = run(case), expected(case)
    assert where[3] == "on" and set(where) == {"on", "in", "out"}
    for row, w in enumerate(where):
        if w == "in":
            assert np.all(want[row] > 1e-2)                # (sigma 3.5 at 5 A: 1.4e-2 -- a wrong decision shows)
        else:
            assert np.all(want[row] == 0.0) and np.all(got[row] == 0.0), (row, w, got[row])
    check(got, want, "cut-off")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_special_sigmas_and_centres_on_atoms(dtype):
    case = CC.special_case(dtype)
    want = expected(case)
    assert (want[:70] == 1.0).any() and (want == 0.0).any()
    check(run(case), want, f"special sigmas, {np.dtype(dtype).name}")


@pytest.mark.parametrize("name", ["nonfinite_case", "far_case", "periodic_case"])
def test_edge_case(name):
    case = getattr(CC, name)()
    want = expected(case)
    assert np.mean(want > 100 * TOL) >= 0.05
    check(run(case), want, name)


# ---- the in-place maximum of calculate_occupancy's pairwise route -------------------------------------------------------------
def test_in_place_maximum_keeps_larger_values_and_nans():
    case, pre = CC.jitter_case()
    want = CC.in_place_max(expected(case), pre)
    res = pre.copy()
    st, route = E.calculate_occupancy(case.centers, case.coords, case.sigmas, res)
    assert (st, route) == (0, 2)                           # the pairwise kernel, not the lattice path
    assert np.array_equal(np.isnan(res), np.isnan(pre)) and np.isnan(pre).any()
    assert np.nanmax(np.abs(res - want)) <= TOL
    assert np.array_equal(res[pre == 2.0], pre[pre == 2.0]) and np.all(res[pre == -1.0] >= 0.0)
    # no atoms / no centres: nothing is touched
    for coords, centers in ((case.coords[:0], case.centers), (case.coords, case.centers[:0])):
        res = pre[:len(centers)].copy()
        st, _ = E.calculate_occupancy(centers, coords, case.sigmas[:len(coords)], res)
        assert st == 0 and np.array_equal(res, pre[:len(centers)], equal_nan=True)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_backend_usable():
    """Each refusal by its message.  The good calls in between only show that the emulated entry still answers: it builds a
    fresh backend for every call, so no state outlives a refusal here -- that a refused call leaves ONE context usable is the
    GPU tier's to show (tests/test_gpu_centers.py, one hip_ctx)."""
    case = CC.shape_case(65, 65, 9)
    want = expected(case)

    def good_call():
        check(run(case), want, "after a refusal")

    for box in ([10.0, 30.0, 30.0], [30.0, 0.0, 30.0], [30.0, 30.0, np.nan]):
        with pytest.raises(RuntimeError, match="periodic box edges must be > 10 A"):
            E.occupancy_centers(case.centers, case.coords, case.sigmas, box=np.array(box))
        good_call()
    with pytest.raises(RuntimeError, match="n_channels > 0"):
        E.occupancy_centers(case.centers, case.coords, np.zeros((65, 0)))
    good_call()
    one = np.zeros((1, 3))
    with pytest.raises(RuntimeError, match="at most 524280 channels"):
        E.occupancy_centers(one, one.astype(np.float32), np.full((1, CC.MAX_CHANNELS + 1), 2.0))
    good_call()
