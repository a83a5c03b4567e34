"""GPU tier (-m gpu) of the explicit-centre occupancy path: k_occupancy_centers at every workgroup width the launch rule picks
(4, 8 and 16 waves, one and two channel groups) through the host entry (batch.occupancy_centers), the drop-in
(occupancy_utils.calculate_occupancy) and the device entry (Context.occupancy_centers_dev: device pointers on the caller's
stream), against the oracle at the project's tolerance and -- where the kernel promises it -- bit for bit.  The comparisons of
tests/test_emu_centers.py on the hardware's v_rcp_f32 / v_exp_f32 / ds_min_u32 and with the waves of a block really
concurrent; the cases are tests/centers_cases.py.  Every test prints the worst difference it saw (pytest -s)."""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import centers_cases as CC
from tests.cases import TOL

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GUARD = 64


def note(waves):
    return f"mkamd::k_occupancy_centers, {waves} waves"


def expected(case):
    return oracle.calculate_occupancy(case.centers, case.coords, np.asarray(case.sigmas, np.float64), box=case.box)


def run(ctx, case, rows=None):
    from moleculekit_amd import batch
    centers = case.centers if rows is None else case.centers[:rows]
    return batch.occupancy_centers(centers, case.coords, case.sigmas, box=case.box, ctx=ctx)


def check(got, want, what=""):
    """|got - want| <= TOL and NaN where the oracle has NaN (it never has: `value > old` keeps them out)"""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    err = np.abs(got.astype(np.float64) - want)
    worst = float(np.nanmax(err)) if err.size else 0.0
    print(f"{what}: worst |gpu - oracle| = {worst:.3e}")
    assert worst <= TOL, (what, worst)
    return worst


@functools.lru_cache(maxsize=None)
def _block_oracle(C):
    want = expected(CC.block_case(C))
    want.setflags(write=False)
    return want


_whole = {}


def block_whole(ctx, C):
    """(the host entry's result for the whole centre list, the kernel note, the oracle's result): once per module"""
    if C not in _whole:
        got = run(ctx, CC.block_case(C))
        got.setflags(write=False)
        _whole[C] = (got, ctx.last_dist_kernel())
    return _whole[C] + (_block_oracle(C),)


def dev_call(ctx, stream, centers, coords, sigmas, box, V=None, N=None, null=()):
    """Context.occupancy_centers_dev on torch tensors made on `stream` (which the context has been given): the output is a slice
    of a sentinel-filled buffer with GUARD floats in front and behind -> (the slice, the two guards) as numpy arrays."""
    import torch
    dev = torch.device("cuda", 0)
    V = len(centers) if V is None else V
    N = len(coords) if N is None else N
    C = sigmas.shape[1]
    with torch.cuda.stream(stream):
        t = lambda a: torch.as_tensor(np.array(a), device=dev)          # (a copy: the shared cases are read-only arrays)
        d = dict(centers=t(centers), coords=t(coords), sigmas=t(sigmas))
        buf = torch.full((GUARD + len(centers) * C + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        d["features"] = buf[GUARD:GUARD + len(centers) * C]
        assert len(centers) == 0 or d["features"].data_ptr() == buf.data_ptr() + 4 * GUARD
        for name in null:
            d[name] = None
        bx = None if box is None else np.ascontiguousarray(box, np.float64)
        ctx.occupancy_centers_dev(d["centers"], V, d["coords"], N, d["sigmas"], sigmas.dtype == np.float64, C, bx, d["features"])
        stream.synchronize()
        host = buf.cpu().numpy()
    return host[GUARD:len(host) - GUARD].reshape(len(centers), C), host[:GUARD], host[len(host) - GUARD:]


@pytest.fixture()
def side_stream(hip_ctx):
    import torch
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    hip_ctx.set_stream(stream.cuda_stream)
    try:
        yield stream
    finally:
        hip_ctx.set_stream(None)


# ---- the block rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 8, 9, 16])
def test_block_rule_on_each_side_of_both_thresholds(hip_ctx, C):
    from moleculekit_amd import batch
    G = -(-C // CC.CHANNEL_GROUP)
    rng = np.random.default_rng(C)
    coords = rng.uniform(-1.0, 1.0, (1, 3)).astype(np.float32)
    sigmas = np.full((1, C), 2.0)
    sizes = CC.threshold_sizes(G)
    assert sizes == CC.THRESHOLDS[G]                       # the literal table of centers_cases.py
    centers = rng.uniform(-5.0, 5.0, (sizes[-1][0], 3))
    want = oracle.calculate_occupancy(centers, coords, sigmas)
    for V, waves in sizes:
        got = batch.occupancy_centers(centers[:V], coords, sigmas, ctx=hip_ctx)
        assert hip_ctx.last_dist_kernel() == note(waves), (V, C)
        check(got, want[:V], f"threshold V = {V}, C = {C}")


# ---- every block size on one atom set: oracle, then bit for bit -----------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 9])
def test_block_case_at_all_three_widths(hip_ctx, C):
    """The whole list at 4 waves against the oracle; its prefixes at 8 and 16 waves, whose waves are dealt other atoms, against
    the oracle and bit for bit against the rows of the whole call (the minimum is taken over bit patterns, the epilogue is
    shared); the drop-in on the same list gives those bits widened to double."""
    from moleculekit_amd.occupancy_utils import calculate_occupancy
    whole, kernel, want = block_whole(hip_ctx, C)
    case = CC.block_case(C)
    seen = {kernel}
    assert kernel == note(4)
    assert np.mean(want > 100 * TOL) >= 0.25               # the case says something (the ORACLE's values, not the product's)
    check(whole, want, f"block_case({C}), 4 waves")
    for rows, waves in CC.block_prefixes(C)[1:]:
        got = run(hip_ctx, case, rows)
        seen.add(hip_ctx.last_dist_kernel())
        assert hip_ctx.last_dist_kernel() == note(waves), (rows, C)
        assert np.array_equal(got, whole[:rows]), (rows, C, float(np.abs(got - whole[:rows]).max()))
        check(got, want[:rows], f"block_case({C}), {waves} waves")
    assert seen == {note(4), note(8), note(16)}
    res = np.zeros(whole.shape)
    calculate_occupancy(np.array(case.centers), np.array(case.coords), np.array(case.sigmas), res, ctx=hip_ctx)
    assert hip_ctx.last_dist_kernel() == note(4)
    assert np.array_equal(res, whole.astype(np.float64))


@pytest.mark.parametrize("C", [3, 9])
def test_atom_and_centre_order(hip_ctx, C):
    """Atoms, with their sigma rows, in another order land in other chunks and other waves: the same bits at every width.
    Centres in another order: the rows in that order."""
    from moleculekit_amd import batch
    whole, _, _ = block_whole(hip_ctx, C)
    case = CC.block_case(C)
    perm = np.random.default_rng(11).permutation(len(case.coords))
    for rows, waves in CC.block_prefixes(C):
        got = batch.occupancy_centers(case.centers[:rows], case.coords[perm], case.sigmas[perm], ctx=hip_ctx)
        assert hip_ctx.last_dist_kernel() == note(waves)
        assert np.array_equal(got, whole[:rows]), (rows, C)
    perm = np.random.default_rng(12).permutation(len(case.centers))
    got = batch.occupancy_centers(case.centers[perm], case.coords, case.sigmas, ctx=hip_ctx)
    assert hip_ctx.last_dist_kernel() == note(4)
    assert np.array_equal(got, whole[perm])


def test_float32_sigmas_equal_float64_sigmas_of_the_same_values(hip_ctx):
    from moleculekit_amd import batch
    case = CC.block_case(9)
    s32 = case.sigmas.astype(np.float32)
    for rows, _ in CC.block_prefixes(9):
        assert np.array_equal(batch.occupancy_centers(case.centers[:rows], case.coords, s32, ctx=hip_ctx),
                              batch.occupancy_centers(case.centers[:rows], case.coords, s32.astype(np.float64), ctx=hip_ctx))
    sp = CC.special_case(np.float32)
    assert np.array_equal(run(hip_ctx, sp), batch.occupancy_centers(sp.centers, sp.coords, sp.sigmas.astype(np.float64), ctx=hip_ctx))


# ---- sizes, edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CC.SHAPE_C)
def test_shapes_around_chunk_block_and_group_boundaries(hip_ctx, C):
    worst = 0.0
    for (N, V, c), case in CC.shape_cases():
        if c != C:
            continue
        got = run(hip_ctx, case)
        assert got.shape == (V, C) and hip_ctx.last_dist_kernel() == note(16)
        if N == 0:
            assert not got.any()                           # every element written, with zero
        err = np.abs(got - expected(case))
        assert not np.isnan(got).any() and (err.max() if err.size else 0.0) <= TOL, (N, V, C, float(err.max()))
        worst = max(worst, float(err.max()))
    print(f"shapes, C = {C}: worst |gpu - oracle| = {worst:.3e}")


def test_cutoff_is_strict(hip_ctx):
    """Zero on and outside the shell, the oracle's value inside, one double ulp either way in every coordinate.  Row 3,
    (3 - 1 ulp, 4, 0), is ON the shell only when d^2 is summed with one rounding per operation, as the reference does: with
    the sum contracted into v_fma_f64 the device answered 1.4e-2 and 6.6e-2 there."""
    case, where = CC.cutoff_case()
    got, want = run(hip_ctx, case), expected(case)
    assert where[3] == "on" and set(where) == {"on", "in", "out"}
    for row, w in enumerate(where):
        if w == "in":
            assert np.all(want[row] > 1e-2)                # (sigma 3.5 at 5 A: 1.4e-2 -- a wrong decision shows)
        else:
            assert np.all(want[row] == 0.0) and np.all(got[row] == 0.0), (row, w, got[row])
    check(got, want, "cut-off")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_special_sigmas_and_centres_on_atoms(hip_ctx, dtype):
    case = CC.special_case(dtype)
    want = expected(case)
    assert (want[:70] == 1.0).any() and (want == 0.0).any()
    check(run(hip_ctx, case), want, f"special sigmas, {np.dtype(dtype).name}")


@pytest.mark.parametrize("name", ["nonfinite_case", "far_case", "periodic_case"])
def test_edge_case(hip_ctx, name):
    case = getattr(CC, name)()
    want = expected(case)
    assert np.mean(want > 100 * TOL) >= 0.05
    check(run(hip_ctx, case), want, name)


# ---- the in-place maximum of calculate_occupancy's pairwise route -------------------------------------------------------------
def test_in_place_maximum_keeps_larger_values_and_nans(hip_ctx):
    from moleculekit_amd.occupancy_utils import calculate_occupancy
    case, pre = CC.jitter_case()
    want = CC.in_place_max(expected(case), pre)
    res = pre.copy()
    calculate_occupancy(case.centers, case.coords, case.sigmas, res, ctx=hip_ctx)
    assert hip_ctx.last_dist_kernel() == note(16)          # the pairwise kernel, not the lattice path
    assert np.array_equal(np.isnan(res), np.isnan(pre)) and np.isnan(pre).any()
    print(f"in-place maximum: worst |gpu - oracle| = {np.nanmax(np.abs(res - want)):.3e}")
    assert np.nanmax(np.abs(res - want)) <= TOL
    assert np.array_equal(res[pre == 2.0], pre[pre == 2.0]) and np.all(res[pre == -1.0] >= 0.0)
    # no atoms / no centres: nothing is touched
    for coords, centers in ((case.coords[:0], case.centers), (case.coords, case.centers[:0])):
        res = pre[:len(centers)].copy()
        calculate_occupancy(centers, coords, case.sigmas[:len(coords)], res, ctx=hip_ctx)
        assert np.array_equal(res, pre[:len(centers)], equal_nan=True)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_context_usable(hip_ctx):
    from moleculekit_amd import batch
    from moleculekit_amd._lib import MkamdError
    case = CC.shape_case(65, 65, 9)
    want = expected(case)

    def good_call():
        check(run(hip_ctx, case), want, "after a refusal")

    for box in ([10.0, 30.0, 30.0], [30.0, 0.0, 30.0], [30.0, 30.0, np.nan]):
        with pytest.raises(MkamdError, match="periodic box edges must be > 10 A"):
            batch.occupancy_centers(case.centers, case.coords, case.sigmas, box=np.array(box), ctx=hip_ctx)
        good_call()
    with pytest.raises(ValueError, match="n_channels > 0"):
        batch.occupancy_centers(case.centers, case.coords, np.zeros((65, 0)), ctx=hip_ctx)
    good_call()
    one = np.zeros((1, 3))
    with pytest.raises(ValueError, match="at most 524280 channels"):
        batch.occupancy_centers(one, one.astype(np.float32), np.full((1, CC.MAX_CHANNELS + 1), 2.0), ctx=hip_ctx)
    good_call()
    # the limit itself is served: one atom on one centre, 65 535 channel groups, every channel 1
    got = batch.occupancy_centers(one, one.astype(np.float32), np.full((1, CC.MAX_CHANNELS), 2.0), ctx=hip_ctx)
    assert got.shape == (1, CC.MAX_CHANNELS) and np.all(got == 1.0)
    good_call()


# ---- the device entry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 9])
def test_device_entry_gives_the_host_entry_bits_at_every_width(hip_ctx, side_stream, C):
    """Device pointers on a stream of the caller's, the output in the middle of a larger buffer: the slice carries the host
    entry's bits at 4, 8 and 16 waves, with float64 and with float32 sigmas, and nothing outside it is written."""
    from moleculekit_amd import batch
    whole, _, want = block_whole(hip_ctx, C)
    case = CC.block_case(C)
    s32 = case.sigmas.astype(np.float32)
    seen = set()
    for rows, waves in CC.block_prefixes(C):
        got, front, back = dev_call(hip_ctx, side_stream, case.centers[:rows], case.coords, case.sigmas, None)
        seen.add(hip_ctx.last_dist_kernel())
        assert hip_ctx.last_dist_kernel() == note(waves)
        assert np.all(front == SENTINEL) and np.all(back == SENTINEL)
        assert np.array_equal(got, whole[:rows]), (rows, C)
        check(got, want[:rows], f"device entry, block_case({C}), {waves} waves")
        got32, front, back = dev_call(hip_ctx, side_stream, case.centers[:rows], case.coords, s32, None)
        assert np.all(front == SENTINEL) and np.all(back == SENTINEL)
        assert np.array_equal(got32, batch.occupancy_centers(case.centers[:rows], case.coords, s32, ctx=hip_ctx)), (rows, C)
    assert seen == {note(4), note(8), note(16)}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_entry_with_a_box_and_on_edge_inputs(hip_ctx, side_stream, dtype):
    from moleculekit_amd import batch
    for name in ("periodic_case", "special_case", "nonfinite_case"):
        case = CC.special_case(dtype) if name == "special_case" else getattr(CC, name)()
        sig = case.sigmas.astype(dtype)
        want = oracle.calculate_occupancy(case.centers, case.coords, sig.astype(np.float64), box=case.box)
        got, front, back = dev_call(hip_ctx, side_stream, case.centers, case.coords, sig, case.box)
        assert np.all(front == SENTINEL) and np.all(back == SENTINEL)
        check(got, want, f"device entry, {name}, {np.dtype(dtype).name} sigmas")
        assert np.array_equal(got, batch.occupancy_centers(case.centers, case.coords, sig, box=case.box, ctx=hip_ctx))
    # the cut-off rows: zero on and outside the shell through this entry too
    case, where = CC.cutoff_case()
    got, front, back = dev_call(hip_ctx, side_stream, case.centers, case.coords, case.sigmas.astype(dtype), None)
    assert np.all(front == SENTINEL) and np.all(back == SENTINEL)
    assert not got[[w != "in" for w in where]].any()
    check(got, expected(case), "device entry, cut-off")
    # a ragged last block of centres and of atoms, no atoms at all
    for N, V in ((1025, 65), (0, 65)):
        case = CC.shape_case(N, V, 9)
        got, front, back = dev_call(hip_ctx, side_stream, case.centers, case.coords, case.sigmas.astype(dtype), None)
        assert np.all(front == SENTINEL) and np.all(back == SENTINEL)
        check(got, expected(case._replace(sigmas=case.sigmas.astype(dtype))), f"device entry, N = {N}, V = {V}")


def test_device_entry_refusals(hip_ctx, side_stream):
    case = CC.shape_case(65, 65, 9)
    for name, msg in (("centers", "centers/features pointer is NULL"), ("features", "centers/features pointer is NULL"),
                      ("coords", "coords/sigmas pointer is NULL"), ("sigmas", "coords/sigmas pointer is NULL")):
        with pytest.raises(ValueError, match=msg):
            dev_call(hip_ctx, side_stream, case.centers, case.coords, case.sigmas, None, null=(name,))
    # without atoms their pointers may be NULL; without centres nothing is read or written
    got, front, back = dev_call(hip_ctx, side_stream, case.centers, case.coords[:0], case.sigmas[:0], None, null=("coords", "sigmas"))
    assert not got.any() and np.all(front == SENTINEL) and np.all(back == SENTINEL)
    got, front, back = dev_call(hip_ctx, side_stream, case.centers, case.coords, case.sigmas, None, V=0)
    assert np.all(got == SENTINEL) and np.all(front == SENTINEL) and np.all(back == SENTINEL)
    got, front, back = dev_call(hip_ctx, side_stream, case.centers, case.coords, case.sigmas, None, V=0, null=("centers", "features"))
    assert np.all(got == SENTINEL)
    with pytest.raises(ValueError, match="n_channels > 0"):
        hip_ctx.occupancy_centers_dev(None, 0, None, 0, None, True, 0, None, None)
    got, front, back = dev_call(hip_ctx, side_stream, case.centers, case.coords, case.sigmas, None)
    check(got, expected(case), "device entry after the refusals")
