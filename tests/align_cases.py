"""tests/align_cases.py -- TEST INFRASTRUCTURE: the inputs and the conditions the alignment tests share between the CPU tier (the kernels
on the SIMT emulation, tests/test_align_cpu.py) and the GPU tier (tests/test_gpu_align.py), so that both run the same data under the
same bounds.  Everything is generated from the seeds recorded here; nothing is read from a fixture.

A tier hands the checks a driver `D`:

    D.transforms(xyz, ref, sel, refsel, frames=None, refframe=0, matching=False, cus=None) -> (affine float64 [K, 12], fit float64 [K])
    D.apply(xyz, affine, frames=None)              -> float32 [F, N, 3], a copy of xyz with the listed frames moved
    D.apply_at(base, off_in, outbuf, off_out, N, F, affine, frames)
                                                    -> the whole output buffer after k_align_apply read the frames at base[off_in:] and
                                                       wrote them at outbuf[off_out:] (outbuf None: in place in base)
    D.rmsd_trajectory(xyz, ref, alnsel, rmsdsel, frames=None) -> float32 [K]
    D.last_kernel()                                -> the note of the last transforms / RMSD call

`cus` (the compute-unit count the launch plan assumes) is the emulator's to honour; the hardware has the count it has.

The shapes are the smallest at which these kernels can go wrong: selections of 1 .. 65 atoms (below, at and above every lane-group
width 8 / 16 / 32 / 64) on 13 and 37 frames (partly filled waves at every width; 37 crosses a block of 32 frames at G = 8); a
selection cut into segments on a matching call (the 17-sum fold); 300 atoms walked by one lane group (five atoms per lane) and the
same frames segmented; k_align_apply at 1 / 5 / 333 atoms and around its 1 024-atom block, at every phase of input and output within
a 16-byte piece; an RMSD over a selection other than the alignment's, folded and not.

The bounds are those of the project's earlier tests of the same quantities (tests/test_align_cpu.py): rotation entries within 1e-9
and the fit RMSD within 1e-9 relative of a float64 SVD Kabsch, |det - 1| < 1e-12, moved coordinates at most one float32 ulp from
float32(x R^T + t) evaluated in float64 (the double-precision error, with or without contraction, is far below half a float32
spacing, so the result is one of the two neighbours).  The width cases sit 60 Angstrom from the origin per axis (`CENTER`), six
standard deviations of the structure: a coordinate that lands within 1e-3 of zero has a float32 spacing near the float64 rounding of
a translation of 1 000 Angstrom, where "one ulp" says nothing about the kernel."""
from __future__ import annotations

import types

import numpy as np

F32 = np.float32
ROT_TOL = 1e-9          # rotation entries against the float64 SVD Kabsch
FIT_TOL = 1e-9          # the fit RMSD, relative
DET_TOL = 1e-12         # |det R - 1|, |R R^T - 1|


# ---- float64 restatements and generators --------------------------------------------------------------------------------
def kabsch64(P, Q):
    """float64 Kabsch (SVD with the reflection sign): R, t with R P_i + t ~ Q_i"""
    P = np.asarray(P, np.float64)
    Q = np.asarray(Q, np.float64)
    cP, cQ = P.mean(0), Q.mean(0)
    H = (P - cP).T @ (Q - cQ)
    V, S, Wt = np.linalg.svd(H)
    W = Wt.T
    Z = np.eye(3)
    Z[2, 2] = np.sign(np.linalg.det(W) * np.linalg.det(V))
    R = W @ Z @ V.T
    return R, cQ - R @ cP


def apply64_d(x, R, t):
    return np.asarray(x, np.float64) @ R.T + t


def apply64(x, R, t):
    return apply64_d(x, R, t).astype(F32)


def fit_rmsd64(P, Q, R, t):
    d = apply64_d(P, R, t) - np.asarray(Q, np.float64)
    return np.sqrt((d * d).sum() / len(P))


def rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def traj(rng, N, F, noise=0.3, spread=10.0, center=0.0):
    """-> (xyz float32 [F, N, 3], ref float32 [N, 3]): rigid copies of a structure about `center`, up to 1 000 Angstrom away, plus noise"""
    ref = (rng.normal(size=(N, 3)) * spread + center).astype(F32)
    xyz = np.stack([(ref @ rot(rng).T + rng.uniform(-1000, 1000, 3) + rng.normal(scale=noise, size=(N, 3))).astype(F32)
                    for _ in range(F)])
    return xyz, ref


def rigid_copies(rng, ref, F, noise=0.3):
    """as traj's frames, all at once (thousands of frames): float32 [F, N, 3]"""
    q = rng.normal(size=(F, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z], axis=1).reshape(F, 3, 3)
    moved = np.einsum("nc,frc->fnr", ref.astype(np.float64), R) + rng.uniform(-1000, 1000, (F, 1, 3))
    return (moved + rng.normal(scale=noise, size=moved.shape)).astype(F32)


def within_ulp(got, exp, ulps=1):
    return np.all(np.abs(got.astype(np.float64) - exp.astype(np.float64)) <= ulps * np.spacing(np.abs(exp)).astype(np.float64))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == F32 else np.int64)


def np_pp_align(coords, refcoords, sel, refsel, frames, refframe, matching):
    """the float64 restatement in the reference's layout (snapshot of the reference frame)"""
    out = coords.copy()
    ref = refcoords.copy()
    for f in frames:
        Q = ref[refsel, :, f] if matching else ref[refsel, :, refframe]
        R, t = kabsch64(coords[sel, :, f], Q)
        out[:, :, f] = apply64(coords[:, :, f], R, t)
    return out


# ---- (a) lane-group widths and partly filled waves --------------------------------------------------------------------------
WIDTH_N = 130
WIDTH_SIZES = (1, 2, 3, 4, 8, 9, 16, 17, 32, 33, 64, 65)
WIDTH_FRAMES = (13, 37)
FRAME_LIST = (11, 0, 5, 12, 3)
CENTER = 60.0
# The seed of each (selection size, frames) case: 1000 n + F, except for the two-atom selections.  There the optimal residual is
# half the difference of the two pair distances, and E_P + E_Q - 2 lambda (about 1e-14 E absolute, E a few hundred square Angstrom)
# keeps 1e-9 relative only while the residual stays above about 0.01 Angstrom; one frame in ten of a draw falls below.  For n = 2 the
# seed is the first of 1000 n + F + 100 000 k at which the float64 Kabsch residual of every frame, against the single and against the
# matching reference, is at least MIN_PAIR_RESIDUAL: a property of the data, which width_case checks, not of the code under test.
WIDTH_SEEDS = {(n, F): 1000 * n + F for n in WIDTH_SIZES for F in WIDTH_FRAMES}
WIDTH_SEEDS[(2, 13)] = 102013
WIDTH_SEEDS[(2, 37)] = 802037
MIN_PAIR_RESIDUAL = 0.02


def group_width(n):
    """the lane-group width align_plan gives a selection of n atoms"""
    return 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64


_width_cache = {}


def width_case(n, F):
    """-> namespace(xyz [F, N, 3], ref [N, 3], refs [F, N, 3] (the matching call's reference), sel); computed once, never changed"""
    if (n, F) not in _width_cache:
        rng = np.random.default_rng(WIDTH_SEEDS[(n, F)])
        xyz, ref = traj(rng, WIDTH_N, F, center=CENTER)
        refs, _ = traj(rng, WIDTH_N, F, center=-CENTER)
        sel = np.sort(rng.choice(WIDTH_N, n, replace=False))
        if n == 2:
            assert min(fit_rmsd64(x[sel], Q[sel], *kabsch64(x[sel], Q[sel])) for f, x in enumerate(xyz) for Q in (ref, refs[f])) >= MIN_PAIR_RESIDUAL
        for a in (xyz, ref, refs, sel):
            a.setflags(write=False)
        _width_cache[(n, F)] = types.SimpleNamespace(xyz=xyz, ref=ref, refs=refs, sel=sel, n=n, F=F)
    return _width_cache[(n, F)]


def check_frame(aff, fit, moved, x, Q, sel, what):
    """one listed frame: its affine [12] and fit RMSD, its moved atoms [N, 3], against the frame x [N, 3] and the reference frame Q"""
    n = len(sel)
    R = aff[:9].reshape(3, 3)
    assert abs(np.linalg.det(R) - 1.0) < DET_TOL, what
    if n >= 3:
        Rk, tk = kabsch64(x[sel], Q[sel])
        assert np.abs(R - Rk).max() < ROT_TOL, (what, np.abs(R - Rk).max())
        assert within_ulp(moved, apply64(x, Rk, tk)), what
        exp = fit_rmsd64(x[sel], Q[sel], Rk, tk)
        assert abs(fit - exp) <= FIT_TOL * exp, (what, fit, exp)
        return
    assert within_ulp(moved, apply64(x, R, aff[9:])), what
    if n == 1:                                                   # one atom: R = I to the bit, the atom lands on its reference
        assert np.array_equal(aff[:9], np.eye(3).ravel()), what
        assert np.abs(moved[sel] - Q[sel]).max() <= 2 * np.spacing(F32(np.abs(Q[sel]).max())), what
        return
    # two atoms: the rotation about their axis is free; what is checked is that it is a rotation, that the reported fit is the residual
    # of the returned transform, and that no rotation does better
    assert np.abs(R @ R.T - np.eye(3)).max() < DET_TOL, what
    own = fit_rmsd64(x[sel], Q[sel], R, aff[9:])
    assert abs(fit - own) <= FIT_TOL * own, (what, fit, own)
    best = fit_rmsd64(x[sel], Q[sel], *kabsch64(x[sel], Q[sel]))
    assert own <= best * (1 + FIT_TOL), (what, own, best)


def check_transforms(D, xyz, ref, sel, frames, matching, G, folded, what):
    """transforms + apply of the listed frames (None: all): the note, every listed frame by check_frame, the others untouched"""
    aff, fit = D.transforms(xyz, ref, sel, sel, frames=frames, matching=matching)
    note = D.last_kernel()
    assert len(note) < 96 and f"k_align_sums<{'AL_MATCH' if matching else 'AL_SINGLE'}>" in note and f"G={G}" in note.split(), (what, note)
    assert ("k_align_fold" in note) == folded, (what, note)
    moved = D.apply(xyz, aff, frames=frames)
    listed = list(range(len(xyz))) if frames is None else list(frames)
    assert aff.shape == (len(listed), 12) and fit.shape == (len(listed),) and moved.dtype == F32
    for i, f in enumerate(listed):
        check_frame(aff[i], fit[i], moved[f], xyz[f], ref[f] if matching else ref, sel, f"{what}, frame {f}")
    others = np.setdiff1d(np.arange(len(xyz)), listed)
    assert np.array_equal(bits(moved[others]), bits(xyz[others])), what
    return aff, fit


def check_width(D, n, F, matching, listed):
    c = width_case(n, F)
    return check_transforms(D, c.xyz, c.refs if matching else c.ref, c.sel, np.array(FRAME_LIST) if listed else None, matching,
                            group_width(n), False, f"n={n} F={F} {'matching' if matching else 'single'}{' listed' if listed else ''}")


# ---- (b) plans ----------------------------------------------------------------------------------------------------------------
SEGMENTED_MATCH = dict(seed=21, N=4000, F=3)
LONG_WALK = dict(seed=22, N=300, F=4096, every=256)

_plan_cache = {}


def segmented_match_case():
    if "match" not in _plan_cache:
        rng = np.random.default_rng(SEGMENTED_MATCH["seed"])
        xyz, _ = traj(rng, SEGMENTED_MATCH["N"], SEGMENTED_MATCH["F"], center=CENTER)
        refs, _ = traj(rng, SEGMENTED_MATCH["N"], SEGMENTED_MATCH["F"], center=-CENTER)
        _plan_cache["match"] = types.SimpleNamespace(xyz=xyz, refs=refs, sel=np.arange(SEGMENTED_MATCH["N"]))
    return _plan_cache["match"]


def check_segmented_match(D):
    """matchingframes with the selection cut into segments: k_align_fold<17, 24> sums all 17 slots of the records"""
    c = segmented_match_case()
    return check_transforms(D, c.xyz, c.refs, c.sel, None, True, 64, True, "segmented matching")


def long_walk_case():
    """300 atoms x 4 096 frames (15 MB): the first frames of it are the few-frame (segmented) call's data"""
    if "walk" not in _plan_cache:
        rng = np.random.default_rng(LONG_WALK["seed"])
        ref = (rng.normal(size=(LONG_WALK["N"], 3)) * 10.0 + CENTER).astype(F32)
        _plan_cache["walk"] = types.SimpleNamespace(xyz=rigid_copies(rng, ref, LONG_WALK["F"]), ref=ref, sel=np.arange(LONG_WALK["N"]))
    return _plan_cache["walk"]


def check_two_plans(D, F_long, every, cus=None):
    """the first F_long frames in one call, one lane group walking all 300 atoms of a frame (no fold; `cus`: what makes the emulator's plan
    take that form on few frames), every `every`-th frame against kabsch64; then the first three frames alone, which the plan cuts into
    segments: two plans, one answer to 1e-9"""
    c = long_walk_case()
    xyz = c.xyz[:F_long]
    aff, fit = D.transforms(xyz, c.ref, c.sel, c.sel, cus=cus)
    note = D.last_kernel()
    assert "k_align_sums<AL_SINGLE>" in note and "G=64" in note.split() and "k_align_fold" not in note, note
    moved = D.apply(xyz, aff)
    for f in range(0, F_long, every):
        check_frame(aff[f], fit[f], moved[f], xyz[f], c.ref, c.sel, f"long walk, frame {f}")
    few, fit3 = check_transforms(D, c.xyz[:3], c.ref, c.sel, None, False, 64, True, "the long walk's first frames, segmented")
    assert np.abs(few - aff[:3]).max() < 1e-9 and np.abs(fit3 - fit[:3]).max() <= 1e-9 * fit[:3].max()


# ---- (c) k_align_apply at every alignment ---------------------------------------------------------------------------------------
APPLY_SIZES = (1, 5, 333, 1023, 1024, 1025, 2049)
APPLY_PLACEMENTS = ((0, 0), (1, 1), (3, 2), (2, 0))
APPLY_F, APPLY_FRAMES, APPLY_PAD = 3, (2, 0), 8
SENTINEL = F32(-7.25e7)


def check_apply_alignment(D, N):
    """the frames at every phase of a 16-byte piece, input and output in equal and in different phases, and in place off the piece:
    one ulp from the float64 restatement, the same bits at every placement, nothing else written"""
    rng = np.random.default_rng(N)
    F, frames, pad = APPLY_F, np.array(APPLY_FRAMES), APPLY_PAD
    n = F * N * 3
    x = rng.normal(scale=100, size=n).astype(F32)
    aff = np.concatenate([np.stack([rot(rng).ravel() for _ in frames]), rng.uniform(-50, 50, (len(frames), 3))], axis=1)
    xf = x.reshape(F, N, 3)
    exp = {f: apply64(xf[f], aff[i, :9].reshape(3, 3), aff[i, 9:]) for i, f in enumerate(frames)}
    first = None
    for off_in, off_out in APPLY_PLACEMENTS + (("in place", 1),):
        inplace = off_in == "in place"
        base = np.full(n + pad, SENTINEL, F32)
        o_in = off_out if inplace else off_in
        base[o_in:o_in + n] = x
        outbuf = None if inplace else np.full(n + pad, SENTINEL, F32)
        got = D.apply_at(base, o_in, outbuf, off_out, N, F, aff, frames)
        what = f"N={N} in {off_in} out {off_out}"
        assert got.dtype == F32 and got.shape == (n + pad,), what
        y = got[off_out:off_out + n].reshape(F, N, 3)
        for f in frames:
            assert within_ulp(y[f], exp[f]), what
        if first is None:
            first = y[frames].copy()
        assert np.array_equal(bits(y[frames]), bits(first)), f"{what}: not the bits of the (0, 0) placement"
        unlisted = xf[1] if inplace else np.full((N, 3), SENTINEL, F32)
        assert np.array_equal(bits(y[1]), bits(unlisted)), f"{what}: the frame that is not listed was written"
        assert np.all(bits(got[:off_out]) == bits(SENTINEL)) and np.all(bits(got[off_out + n:]) == bits(SENTINEL)), f"{what}: written past the view"


# ---- (d) RMSD over another selection than the alignment's ---------------------------------------------------------------------
RMSD_CASE = dict(seed=23, N=600, F=5)


def check_rmsd(D):
    rng = np.random.default_rng(RMSD_CASE["seed"])
    N, F = RMSD_CASE["N"], RMSD_CASE["F"]
    xyz, ref = traj(rng, N, F, center=CENTER)
    aln = np.arange(0, N, 2)
    odd = np.arange(1, N, 2)                                                   # 300 atoms on 5 frames: segments, k_align_fold<1, 1>
    few = np.sort(rng.choice(odd, 40, replace=False))                          # 40 atoms: one segment
    aff, _ = D.transforms(xyz, ref, aln, aln)
    moved = D.apply(xyz, aff)                                                  # the bits the RMSD kernel sums without storing them
    for rsel, folded in ((odd, True), (few, False)):
        got = D.rmsd_trajectory(xyz, ref, aln, rsel)
        note = D.last_kernel()
        assert "k_align_sums<AL_RMSD>" in note and "G=64" in note.split() and ("k_align_fold<1, 1>" in note) == folded, note
        assert got.dtype == F32 and got.shape == (F,)
        d = moved[:, rsel].astype(np.float64) - ref[rsel].astype(np.float64)
        # a double sum of n non-negative terms is off by at most n 2^-53 relative; the root and the one rounding to float32 leave one ulp
        assert within_ulp(got, np.sqrt((d * d).sum(axis=(1, 2)) / len(rsel)).astype(F32)), (folded, got)
        for frames in ([3], [4, 0, 2], [1, 1]):
            sub = D.rmsd_trajectory(xyz, ref, aln, rsel, frames=np.array(frames))
            assert np.array_equal(bits(sub), bits(got[frames])), (folded, frames)


# ---- (e) the host route's data -------------------------------------------------------------------------------------------------
ROUTE_CASE = (33, 13)                     # a width case, handed over in the reference's [N, 3, F] layout
ROUTE_FRAMES = (None, (11, 5, 12, 3))     # all frames; a list whose first listed frame is not frame 0 (the host route uploads a span)


def route_case():
    c = width_case(*ROUTE_CASE)
    t = lambda a: np.ascontiguousarray(a.transpose(1, 2, 0))
    return types.SimpleNamespace(coords=t(c.xyz), ref=np.ascontiguousarray(c.ref[:, :, None]), refs=t(c.refs), sel=c.sel, xyz=c.xyz,
                                 ref_fm=c.ref, refs_fm=c.refs, F=c.F)


# ---- (f) degenerate selections ---------------------------------------------------------------------------------------------------
def check_degenerate(D, kind):
    """the rotation is not unique: checked by the fit RMSD and the selection's residual only"""
    rng = np.random.default_rng(5)
    P = rng.normal(scale=5, size=(20, 3))
    P[:, 2] = 0.0
    if kind == "collinear":
        P[:, 1] = 0.0
    P = P.astype(F32)
    Rt = rot(rng)
    xyz = (P @ Rt.T + 50.0).astype(F32)[None]
    aff, fit = D.transforms(xyz, P, np.arange(20), np.arange(20))
    R = aff[0, :9].reshape(3, 3)
    assert abs(np.linalg.det(R) - 1.0) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    out = D.apply(xyz, aff)
    assert np.abs(out[0] - P).max() < 1e-3
    assert fit[0] < 1e-5


def check_coincident(D):
    """one point many times (a zero covariance): the identity, every atom on the reference"""
    xyz = np.zeros((2, 5, 3), F32)
    xyz[1] += 3.0
    ref = np.ones((5, 3), F32)
    aff, fit = D.transforms(xyz, ref, np.arange(5), np.arange(5))
    for f in range(2):
        assert np.array_equal(aff[f, :9], np.eye(3).ravel())
    out = D.apply(xyz, aff)
    assert np.array_equal(out, np.ones_like(xyz))


def check_empty(D):
    xyz, ref = traj(np.random.default_rng(1), 10, 2)
    aff, fit = D.transforms(xyz, ref, np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert np.all(np.isnan(aff[:, 9:])) and np.all(np.isnan(fit))
    assert np.all(np.isnan(D.apply(xyz, aff)))
