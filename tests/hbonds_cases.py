"""tests/hbonds_cases.py -- TEST INFRASTRUCTURE: the seeded cases of the hydrogen-bond tests (CPU and GPU tier, golden data).

A case is a dict of what goes to the compiled `calculate`: name, coords float32 [N, 3, F], box float32 [3, F], donors uint32 [nd, 2]
((heavy atom, hydrogen) rows; [nd, 1] with ignore_hs), acceptors uint32 [na], sel1 / sel2 uint32 [N] flags (intra: sel2 is a copy of
sel1, as the reference's wrapper passes it), dist_threshold, angle_threshold, intra, ignore_hs -- and `edge`: the case is exactly
collinear and sits ON its angle threshold, so it is exempt from the margin condition (the golden list decides it).

Donor groups are D-H bonds of about 1 A with random directions and per-frame jitter; acceptors sit 1.5 .. 3.2 A from a hydrogen, up to
90 degrees off the D-H line, or anywhere; every atom has a shuffled index in a larger array.  The lists are NOT filtered by the
selections (the wrapper's filter is an optimisation): rows and acceptors in neither selection reach the loop and are refused there.
`check_margins()` asserts the condition the comparisons rest on: no float64 angle of a pair that reached the angle test lies within
1e-4 degrees of the threshold in use.
"""
from __future__ import annotations

import numpy as np

F32, U32 = np.float32, np.uint32
MARGIN_DEG = 1e-4


def _unit(rng, n=None):
    v = rng.normal(size=(3,) if n is None else (n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _off_axis(rng, d, theta):
    """a unit vector `theta` radians off the unit vector d"""
    p = np.cross(d, _unit(rng))
    p /= np.linalg.norm(p)
    return np.cos(theta) * d + np.sin(theta) * p


def _flags(rng, n, counts):
    """(only sel1, only sel2, both, neither) counts -> shuffled (sel1, sel2) flags of n atoms (the rest: random)"""
    kinds = np.concatenate([np.full(c, k) for k, c in enumerate(counts)]) if counts is not None else rng.integers(0, 4, n)
    assert len(kinds) == n
    kinds = rng.permutation(kinds)
    return ((kinds == 0) | (kinds == 2)).astype(U32), ((kinds == 1) | (kinds == 2)).astype(U32)


def _random_case(name, seed, nd, acc, F, extent, box="zero", sel="inter", ignore_hs=False, dist=2.5, angle=120, near=0.7, shared=0,
                 share_heavy=0.3, nan_frames=(), jitter=0.1, don=None):
    """nd donor rows against acceptors.  `acc`: the acceptors' (only sel1, only sel2, both, neither) counts -- intra: (in sel1, 0, 0, not
    in it); `shared`: that many acceptors ARE donor heavy atoms (hydroxyl, water); `share_heavy`: the chance that a row reuses the heavy
    atom of the row before it (NH2, water); `don`: the donor rows' heavy atoms' (only sel1, only sel2, both, neither) counts (random
    where None; needs distinct heavy atoms that are no acceptors)."""
    rng = np.random.default_rng(seed)
    na = int(sum(acc))
    atoms = []                                                         # [F, 3] each

    def add(p, scale=1.0):                                             # a point, or a trajectory to follow, plus its own jitter
        atoms.append(np.asarray(p, np.float64) + scale * jitter * rng.normal(size=(F, 3)))
        return len(atoms) - 1

    donors, dirs = [], []
    for r in range(nd):
        if r and rng.random() < share_heavy:
            heavy = donors[-1][0]
        else:
            heavy = add(rng.uniform(0, extent, 3))
        d = _unit(rng)
        donors.append((heavy, add(atoms[heavy] + 1.0 * d, 0.3)))      # the hydrogen follows its heavy atom, with a little jitter of its own
        dirs.append(d)
    acceptors = []
    for j in range(na):
        if j < shared:
            acceptors.append(donors[int(rng.integers(nd))][0])
        elif rng.random() < near:
            r = int(rng.integers(nd))
            acceptors.append(add(atoms[donors[r][1]] + rng.uniform(1.5, 3.2) * _off_axis(rng, dirs[r], rng.uniform(0, np.pi / 2))))
        else:
            acceptors.append(add(rng.uniform(0, extent, 3)))
    n = len(atoms)
    N = n + 5
    perm = rng.permutation(N)[:n]
    coords = rng.uniform(-50, 50, (N, 3, F))
    for i, a in enumerate(atoms):
        coords[perm[i]] = a.T
    coords = coords.astype(F32)
    donors = perm[np.asarray(donors)].astype(U32).reshape(nd, 2)
    acceptors = perm[np.asarray(acceptors, np.int64)].astype(U32)
    order = rng.permutation(na)
    acceptors = acceptors[order]
    # flags: the acceptors' as counted (a shared acceptor is one atom with one pair of flags), every other atom's at random
    s1, s2 = _flags(rng, N, None)
    a1, a2 = _flags(rng, na, acc)
    first = {}
    for j, a in enumerate(acceptors):                                  # (an atom named twice keeps its first flags: the counts are of list entries)
        first.setdefault(int(a), j)
    for a, j in first.items():
        s1[a], s2[a] = a1[j], a2[j]
    if don is not None:
        assert shared == 0 and share_heavy == 0
        s1[donors[:, 0]], s2[donors[:, 0]] = _flags(rng, nd, don)
    intra = sel == "intra"
    if intra:
        s2 = s1.copy()
    elif sel == "disjoint":
        s2[s1 == 1] = 0
    bx = np.zeros((3, F), F32)
    if box != "zero":
        bx[:] = (extent + rng.uniform(0, 0.5, (3, F))).astype(F32)    # a different box in every frame
        if box == "zero_axis":
            bx[1] = 0
        coords += F32(extent / 2)                                      # the cell's faces cut through the groups: bonds and pairs cross them
        for ax in range(3):
            if bx[ax, 0] != 0:
                coords[:, ax, :] -= bx[ax] * np.floor(coords[:, ax, :] / bx[ax])
    for f in nan_frames:
        coords[:, :, f] = np.nan
    if ignore_hs:
        donors = np.unique(donors[:, 0])[:, None].astype(U32) if ignore_hs == "unique" else donors[:, :1].copy()
    return dict(name=name, coords=np.ascontiguousarray(coords, F32), box=bx, donors=np.ascontiguousarray(donors), acceptors=acceptors, sel1=s1, sel2=s2,
                dist_threshold=float(dist), angle_threshold=float(angle), intra=intra, ignore_hs=bool(ignore_hs), edge=False)


def _collinear_case(name, angle, F=64, seed=61):
    """D, H and two acceptors on one line, a fresh direction in every frame: A0 beyond the hydrogen (D-H...A of 180 degrees), A1 on the
    donor's side (0 degrees).  Every coordinate is a multiple of 2^-10 A and the vectors are exact multiples of one another, so the float32
    ratio comes out at +-1, just inside -- or just OUTSIDE, where the reference clamps it."""
    rng = np.random.default_rng(seed)
    q = 1024.0
    coords = np.zeros((4, 3, F))
    for f in range(F):
        step = np.round(_unit(rng) * 0.5 * q) / q                      # half the D-H bond
        d = np.round(rng.uniform(5, 25, 3) * q) / q
        coords[0, :, f], coords[1, :, f] = d, d + 2 * step            # D, H
        coords[2, :, f], coords[3, :, f] = d + 5 * step, d - 1 * step  # A0: 1.5 A beyond H; A1: 1.5 A from H through D
    ones = np.ones(4, U32)
    return dict(name=name, coords=coords.astype(F32), box=np.zeros((3, F), F32), donors=np.array([[0, 1]], U32), acceptors=np.array([2, 3], U32),
                sel1=ones, sel2=ones.copy(), dist_threshold=2.5, angle_threshold=float(angle), intra=True, ignore_hs=False, edge=angle in (0, 180))


def _hand_case(name, box_x=8.0, dist=4.5):
    """what a random case does not hit: an acceptor ON the hydrogen (d2_a == 0), a hydrogen ON its heavy atom (d2_b == 0), an acceptor
    whose x distance from the hydrogen is EXACTLY half the box (not wrapped: the test is |val| > box / 2) in both directions, a bond and a
    pair across the boundary, an acceptor that is its own donor's heavy atom.  Frame 1: the same with a zero x axis (open)."""
    pts = {
        "D0": (1.0, 1.0, 1.0), "H0": (2.0, 1.0, 1.0),                  # along +x
        "A_on_H0": (2.0, 1.0, 1.0),                                    # d2_a == 0
        "A_half+": (6.0, 1.0, 1.0), "A_half-": (-2.0, 1.0, 1.0),       # val = +4 and -4: exactly half of 8
        "D1": (3.0, 5.0, 5.0), "H1": (3.0, 5.0, 5.0),                  # d2_b == 0
        "A_near_H1": (3.0, 6.5, 5.0),
        "D2": (7.5, 3.0, 3.0), "H2": (0.5 + 8.0 * 0, 3.0, 3.0),        # the bond crosses the x face: 7.5 -> 8.5 = 0.5
        "A_across": (2.2, 3.0, 3.0), "A_across2": (7.0, 3.25, 3.0),
        "D3": (4.0, 7.0, 7.0), "H3": (4.0, 7.0, 6.0), "A_far": (4.0, 7.0, 1.0),
    }
    names = list(pts)
    coords = np.zeros((len(names), 3, 2))
    for i, k in enumerate(names):
        coords[i, :, 0] = coords[i, :, 1] = pts[k]
    ix = {k: i for i, k in enumerate(names)}
    donors = np.array([[ix["D0"], ix["H0"]], [ix["D1"], ix["H1"]], [ix["D2"], ix["H2"]], [ix["D3"], ix["H3"]]], U32)
    acceptors = np.array([ix[k] for k in ("A_on_H0", "A_half+", "A_half-", "A_near_H1", "A_across", "A_across2", "A_far", "D0", "D3", "D2")], U32)
    box = np.array([[box_x, 0.0], [8.0, 8.0], [8.0, 8.0]], F32)
    ones = np.ones(len(names), U32)
    return dict(name=name, coords=coords.astype(F32), box=box, donors=donors, acceptors=acceptors, sel1=ones, sel2=ones.copy(),
                dist_threshold=float(dist), angle_threshold=100.0, intra=True, ignore_hs=False, edge=False)


def build_cases():
    R = _random_case
    cases = [
        # name, seed, donor rows, acceptors (only sel1, only sel2, both, neither), frames, extent
        R("hb_1x1_f1", 1, 1, (0, 1, 1, 0), 1, 3.0, near=1.0),
        R("hb_2x(1,63)_f2", 2, 2, (1, 63, 0, 2), 2, 6.0, share_heavy=0.0, don=(1, 1, 0, 0)),
        R("hb_65x(64,1)_f3", 3, 65, (64, 1, 0, 3), 3, 12.0),
        R("hb_7x49_f63_overlap", 4, 7, (20, 19, 5, 5), 63, 6.0),
        R("hb_12x40_f64_box", 5, 12, (14, 13, 8, 5), 64, 7.0, box="box"),
        R("hb_9x30_f65_zero_axis", 6, 9, (10, 9, 7, 4), 65, 7.0, box="zero_axis"),
        R("hb_5x20_f130_disjoint", 7, 5, (9, 8, 0, 3), 130, 5.0, sel="disjoint"),
        R("hb_intra_20x(129)_f3", 8, 20, (129, 0, 0, 9), 3, 9.0, sel="intra", shared=6),
        R("hb_intra_65x65_f2_box", 9, 65, (65, 0, 0, 4), 2, 10.0, sel="intra", box="box", shared=10),
        R("hb_shared_waters_f5", 10, 16, (6, 6, 6, 2), 5, 5.0, shared=12, share_heavy=0.5),
        R("hb_dist3.2_angle150", 11, 10, (10, 10, 6, 2), 4, 5.0, dist=3.2, angle=150),
        R("hb_angle_0", 12, 6, (8, 8, 4, 0), 3, 4.0, angle=0),
        R("hb_nan_frame_f4", 13, 6, (7, 6, 4, 2), 4, 5.0, nan_frames=(2,)),
        R("hb_ignore_hs_nan_frame_f4", 13, 6, (7, 6, 4, 2), 4, 5.0, nan_frames=(2,), ignore_hs=True),
        R("hb_ignore_hs_dup_heavy_f3", 14, 12, (9, 9, 6, 2), 3, 5.0, ignore_hs=True, share_heavy=0.6, dist=3.5, shared=5),
        R("hb_ignore_hs_unique_f66_box", 15, 10, (9, 9, 6, 2), 66, 5.0, ignore_hs="unique", share_heavy=0.6, dist=3.5, box="box"),
        R("hb_ignore_hs_intra_70x130_f1", 16, 70, (130, 0, 0, 6), 1, 12.0, ignore_hs=True, sel="intra", dist=3.5, share_heavy=0.0),
        R("hb_66x(129)_f70_box", 17, 66, (60, 60, 9, 6), 70, 12.0, box="box"),
        _collinear_case("hb_collinear_angle120", 120),
        _collinear_case("hb_collinear_angle180", 180),
        _collinear_case("hb_collinear_angle0", 0),
        _hand_case("hb_hand_half_box"),
    ]
    return cases


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
    return _CASES


def case(name):
    return next(c for c in cases() if c["name"] == name)


# the cases whose reference results are committed (tests/golden/hbond_cases.npz): the small ones -- the file holds their coordinates
GOLDEN = ("hb_1x1_f1", "hb_2x(1,63)_f2", "hb_65x(64,1)_f3", "hb_7x49_f63_overlap", "hb_12x40_f64_box", "hb_9x30_f65_zero_axis", "hb_5x20_f130_disjoint",
          "hb_intra_20x(129)_f3", "hb_intra_65x65_f2_box", "hb_shared_waters_f5", "hb_dist3.2_angle150", "hb_angle_0", "hb_nan_frame_f4",
          "hb_ignore_hs_nan_frame_f4", "hb_ignore_hs_dup_heavy_f3", "hb_ignore_hs_unique_f66_box", "hb_ignore_hs_intra_70x130_f1",
          "hb_collinear_angle120", "hb_collinear_angle180", "hb_collinear_angle0", "hb_hand_half_box")
# golden cases that must both report a pair and drop one that reached the distance or the angle test (make_golden_hbonds.py asserts it)
# (at 180 degrees nothing is ever reported: float32(180 / 57.29578) IS acosf(-1), and the comparison is strict)
BOTH = tuple(n for n in GOLDEN if n not in ("hb_1x1_f1", "hb_collinear_angle180"))

ARGS = ("donors", "acceptors", "coords", "box", "sel1", "sel2")
PARAMS = ("dist_threshold", "angle_threshold", "intra", "ignore_hs")


def sublists(c):
    """the lengths of the acceptor sublists a case's donor rows are held against: in sel1, in sel2, in either"""
    a = c["acceptors"]
    if c["intra"]:
        return {int((c["sel1"][a] != 0).sum())}
    a1, a2 = c["sel1"][a] == 1, c["sel2"][a] == 1
    h = c["donors"][:, 0]
    d1, d2 = c["sel1"][h] == 1, c["sel2"][h] == 1
    out = set()
    if (d2 & ~d1).any():
        out.add(int(a1.sum()))
    if (d1 & ~d2).any():
        out.add(int(a2.sum()))
    if (d1 & d2).any():
        out.add(int((a1 | a2).sum()))
    return out


def collinear_ratios(c):
    """the float32 ratios of a collinear case BEFORE the clamp: [2 acceptors, F]"""
    from hbonds_restatement import F64, wrapped_vec
    co, bx = c["coords"], c["box"]
    va, d2a = wrapped_vec(co[c["acceptors"]], co[1][None], bx)
    vb, d2b = wrapped_vec(co[0][None], co[1][None], bx)
    dot = np.zeros(d2a.shape, F32)
    for ax in range(3):
        dot = (dot + (va[:, ax] * vb[:, ax]).astype(F32)).astype(F32)
    return (dot.astype(F64) / (np.sqrt(d2a) * np.sqrt(d2b)).astype(F32).astype(F64)).astype(F32)


_EXPECTED = {}


def expected(c):
    """the restatement's (frame_offsets, triples) of a case, computed once; the margin condition is asserted on the way"""
    if c["name"] not in _EXPECTED:
        from hbonds_restatement import calculate, threshold_margin
        offs, triples, tested, angle64 = calculate(*(c[k] for k in ARGS), **{k: c[k] for k in PARAMS}, details=True)
        if not c["edge"]:
            margin = threshold_margin(c["angle_threshold"], tested, angle64)
            assert margin >= MARGIN_DEG, f"{c['name']}: an angle lies {margin:.3g} degrees from the threshold; pick another seed"
        for a in (offs, triples):
            a.setflags(write=False)
        _EXPECTED[c["name"]] = (offs, triples, int(tested.sum()))
    return _EXPECTED[c["name"]][:2]


def check_margins():
    for c in cases():
        expected(c)
