"""tests/clashes_cases.py -- TEST INFRASTRUCTURE: the seeded cases of the steric-clash search, the smallest shapes at which each part of
it can go wrong.  A case is a dict of what ``find_clashes`` takes: ``coords`` float32 [N, 3], ``element`` and ``name`` [N], ``bonds``
(the molecule's file bonds, uint32 [nb, 2]), ``sel1`` / ``sel2`` (None, a boolean mask or an index array), ``overlap``,
``exclude_bonded``, ``exclude_14``, ``guess_bonds``.  ``check()`` asserts on the restatement (tests/clashes_restatement.py) that every
case is the case it is meant to be.

tests/golden/clash_cases.npz holds what the compiled reference returns for every name in GOLDEN (make_golden_clashes.py).
"""
from __future__ import annotations

import functools
import os
from types import SimpleNamespace

import numpy as np

import bonds_restatement as BR
import clashes_restatement as R

F32, F64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
BOX_CAP = 4096
NO_BONDS = np.zeros((0, 2), np.uint32)

OVERLAPS = {"overlap_06": 0.6, "overlap_02": 0.2, "overlap_0": 0.0, "overlap_m15": -1.5}
FLAGS = {"excl_11": (True, True), "excl_10": (True, False), "excl_01": (False, True), "excl_00": (False, False)}
GOLDEN = ("two_clash", "two_apart", "one_atom", "empty_sel1", "empty_sel2", *OVERLAPS, "cutoff_negative", "cutoff_zero", "lanes64", "lanes65",
          "planar", "faces", "cross_disjoint", "cross_overlap", "cross_equal", *FLAGS, "threshold_edges", "ties", "elements", "3ptb",
          "3ptb_noguess", "3ptb_cross_mask", "3ptb_cross_index", "crowded")
# cases whose inputs (coords, element, name, bonds) are another case's: the fixture stores them once
SAME_INPUTS = {"3ptb_noguess": "3ptb", "3ptb_cross_mask": "3ptb", "3ptb_cross_index": "3ptb", "overlap_02": "overlap_06", "overlap_0": "overlap_06",
               "overlap_m15": "overlap_06", "excl_10": "excl_11", "excl_01": "excl_11", "excl_00": "excl_11", "empty_sel2": "empty_sel1"}


def _case(coords, element, name=None, bonds=NO_BONDS, sel1=None, sel2=None, overlap=0.6, exclude_bonded=True, exclude_14=True, guess_bonds=False):
    element = np.asarray(element, dtype="<U2")
    name = np.asarray([e + "1" for e in element] if name is None else name, dtype="<U4")
    return {"coords": np.ascontiguousarray(coords, F32), "element": element, "name": name, "bonds": np.asarray(bonds, np.uint32).reshape(-1, 2),
            "sel1": sel1, "sel2": sel2, "overlap": overlap, "exclude_bonded": exclude_bonded, "exclude_14": exclude_14, "guess_bonds": guess_bonds}


def _cluster(seed, n, side, elements=("C", "N", "O", "H")):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, side, size=(n, 3)), rng.choice(elements, size=n)


def grid_side(cutoff):
    """the first box side of the library's grid (clash_pipeline.h: clash_grid), as float32"""
    return F32(max(abs(cutoff), 1.0) * (1.0 + 1.0 / 1024.0))


def _cutoff_case(overlap):
    """coincident atoms, close atoms and bonded atoms under an overlap that leaves the kd-tree's radius at or below zero"""
    coords = np.array([[0, 0, 0], [0, 0, 0], [0.25, 0, 0], [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [3, 3, 3]], F32)
    return _case(coords, ["C"] * 6, bonds=[(0, 2)], overlap=overlap)


def _heavy_far(coords, element):
    """... and one caesium far away that no selection holds: the kd-tree's radius, and with it the box side, follows ITS radius"""
    return np.concatenate([coords, [[400.0, 400.0, 400.0]]]), np.concatenate([element, ["Cs"]])


def _lanes(n):
    """n selected light atoms in a cube smaller than a box"""
    coords, element = _heavy_far(*_cluster(201, n, 5.0, elements=("H", "H", "O")))
    return _case(coords, element, sel1=np.arange(n))


def _planar():
    rng = np.random.default_rng(202)
    gx, gy = np.meshgrid(np.arange(9) * 1.9, np.arange(7) * 1.9, indexing="ij")
    coords = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 3.25)], axis=1)
    coords[:, :2] += rng.uniform(-0.3, 0.3, size=(len(coords), 2))
    order = rng.permutation(len(coords))
    return _case(coords[order], np.where(rng.random(len(coords)) < 0.2, "N", "C"))


def _faces():
    """carbons exactly on the grid's box faces, min + k * side in float32 arithmetic, the maximum corner among them, and a partner
    beside each that mostly sits across a face"""
    rng = np.random.default_rng(203)
    side = grid_side(R.cutoff_of(np.array([1.7], F32), 0.6))
    mn = np.array([-3.5, 10.25, 0.125], F32)
    lattice = np.array([[mn[0] + F32(i) * side, mn[1] + F32(j) * side, mn[2] + F32(k) * side] for i in range(4) for j in range(3) for k in range(3)], F32)
    step = rng.normal(size=lattice.shape)
    step = step / np.linalg.norm(step, axis=1, keepdims=True) * rng.uniform(1.3, 2.9, size=(len(lattice), 1))
    partners = np.clip(lattice + step, mn, lattice.max(axis=0)).astype(F32)
    coords = np.concatenate([lattice, partners])
    c = _case(coords[rng.permutation(len(coords))], ["C"] * len(coords))
    c["lattice"], c["min"], c["side"] = lattice, mn, side
    return c


def _cross(kind):
    """a dense cluster with a chain of bonds through it; the selections disjoint, partially overlapping, or equal (given twice)"""
    coords, element = _cluster(204, 48, 6.5)
    bonds = [(i, i + 1) for i in range(0, 47)]
    n = len(coords)
    if kind == "disjoint":
        sel1, sel2 = np.arange(0, 20), np.arange(20, n)
    elif kind == "overlap":
        sel1, sel2 = np.arange(0, 30), np.arange(18, n)                 # 18 .. 29 in both: (a, a), (a, b) and (b, a) rows
    else:
        sel1 = np.zeros(n, bool)
        sel1[5:40] = True
        sel2 = np.arange(5, 40)[::-1].copy()                           # the same atoms as an index array: self mode
    return _case(coords, element, bonds=bonds, sel1=sel1, sel2=sel2, overlap=0.0)


def _excl(flags):
    """a squeezed molecule: a 3-ring, a 4-ring, a 6-ring, a 5-chain, duplicate bonds, a self-bond and a hub with eight bonds, every
    part linked to the next, so close together that neighbours of every degree clash"""
    bonds = [(0, 1), (1, 2), (2, 0),                                   # 3-ring
             (3, 4), (4, 5), (5, 6), (6, 3),                           # 4-ring
             (7, 8), (8, 9), (9, 10), (10, 11), (11, 12), (12, 7),     # 6-ring
             (13, 14), (14, 15), (15, 16), (16, 17),                   # 5-chain
             (2, 3), (6, 7), (12, 13),                                 # links
             (1, 0), (4, 3), (4, 3), (15, 14),                         # duplicates, one reversed
             (9, 9),                                                   # a self-bond
             (18, 19), (18, 20), (18, 21), (18, 22), (18, 23), (18, 24), (18, 25), (18, 26), (17, 18),      # a hub: nine bonds
             (27, 26)]
    coords, element = _cluster(205, 30, 5.0, elements=("C", "N", "O"))   # atoms 28, 29 are bonded to nothing
    return _case(coords, element, bonds=bonds, overlap=0.0, exclude_bonded=flags[0], exclude_14=flags[1])


def _search_pair(rng, base, want, cutoff=None, tries=400000):
    """an atom b beside the atom at `base` with the float32 distance of the two at `want` (a float32), computed from the coordinates as
    stored; with `cutoff` = (value, passes?), also on the asked side of the kd-tree's float64 pre-filter"""
    u = rng.normal(size=(tries, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    b = (base.astype(F64) + u * (F64(want) + rng.uniform(-4e-7, 4e-7, size=(tries, 1)))).astype(F32)
    a = np.broadcast_to(base, b.shape)
    ok = np.sqrt(R.dist2_f32(a - b)).astype(F32) == want
    if cutoff is not None:
        ok &= (R.dist2_f64(a, b) <= F64(cutoff[0]) * F64(cutoff[0])) == cutoff[1]
    hit = np.flatnonzero(ok)
    return None if len(hit) == 0 else b[hit[0]]


def _threshold_edges():
    """isolated pairs 25 A apart along y: the float32 distance one ulp below, at and one ulp above the pair's threshold; for the pair of
    the largest radius also one ulp below the threshold on either side of the kd-tree's float64 cutoff.  ``labels``: (label, first
    atom, clash?)"""
    rng = np.random.default_rng(206)
    r = {"C": F32(1.7), "H": F32(1.1), "O": F32(1.52)}
    overlap = 0.6
    cutoff = R.cutoff_of(np.array([1.7], F32), overlap)
    spec = []
    for ea, eb in (("H", "H"), ("C", "O"), ("H", "C")):
        thr = R.threshold_of([r[ea]], [r[eb]], overlap)[0]
        spec += [(f"{ea}{eb}_below", ea, eb, np.nextafter(thr, F32(0)), None, True), (f"{ea}{eb}_at", ea, eb, thr, None, False),
                 (f"{ea}{eb}_above", ea, eb, np.nextafter(thr, F32(np.inf)), None, False)]
    thr = R.threshold_of([r["C"]], [r["C"]], overlap)[0]
    below = np.nextafter(thr, F32(0))
    spec += [("CC_below_inside_cutoff", "C", "C", below, (cutoff, True), True), ("CC_below_outside_cutoff", "C", "C", below, (cutoff, False), False),
             ("CC_at", "C", "C", thr, None, False)]
    coords, element, labels = [], [], []
    for k, (label, ea, eb, want, cut, clash) in enumerate(spec):
        base = np.array([0.5, 25.0 * k, -1.25], F32)
        b = _search_pair(rng, base, want, cut)
        if b is None:
            continue                                                  # (check() lists what must be there)
        labels.append((label, len(element), clash))
        coords += [base, b]
        element += [ea, eb]
    c = _case(np.array(coords, F32), element, overlap=overlap)
    c["labels"] = labels
    return c


def _ties():
    """two squares of carbons of side 2: eight edges of one length, and with it eight equal overlaps"""
    sq = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0]], F32)
    coords = np.concatenate([sq, sq + np.array([0, 0, 16], F32)])
    return _case(coords[[5, 0, 7, 2, 1, 4, 3, 6]], ["C"] * 8)


def _elements():
    coords, _ = _cluster(207, 40, 9.0)
    element = np.array((["Xx", "Rf", "Cs", "C", "H", "Fr", "O", "Db"] * 5))
    return _case(coords, element, overlap=0.2)


@functools.lru_cache(maxsize=None)
def _ptb():
    d = np.load(os.path.join(HERE, "golden", "channels_3ptb.npz"))
    protein = ~np.isin(d["resname"], ("BEN", "HOH", "CA"))
    return d["coords"].astype(F32), d["element"], d["name"], d["bonds"].astype(np.uint32), protein


def _3ptb(kind):
    coords, element, name, bonds, protein = _ptb()
    if kind == "default":
        return _case(coords, element, name, bonds, guess_bonds=True)
    if kind == "noguess":
        return _case(coords, element, name, bonds, guess_bonds=False)
    if kind == "cross_mask":
        return _case(coords, element, name, bonds, sel1=protein, sel2=~protein, overlap=0.0, guess_bonds=True)
    return _case(coords, element, name, bonds, sel1=np.flatnonzero(protein), sel2=np.flatnonzero(~protein), overlap=0.0, guess_bonds=True)


def _crowded():
    """100 hydrogens in a cube smaller than a box: every owner's box holds them all"""
    coords, element = _heavy_far(*_cluster(208, 100, 6.0, elements=("H",)))
    return _case(coords, element, sel1=np.arange(100))


def over_cap():
    """4 097 coincident atoms: one more than a box may hold"""
    n = BOX_CAP + 1
    return _case(np.full((n, 3), 1.25, F32), ["C"] * n)


def lattice(n_side=26):
    """17 576 carbons on a jittered 2.5 A lattice: more owners than the wave-per-owner plan takes unforced, no crowded box.  Not a
    golden case: the two plans are compared with each other on it"""
    rng = np.random.default_rng(209)
    g = np.stack(np.meshgrid(*([np.arange(n_side) * 2.5] * 3), indexing="ij"), axis=-1).reshape(-1, 3)
    return _case(g + rng.uniform(-0.45, 0.45, size=g.shape), ["C"] * len(g), overlap=1.0)


_BUILDERS = {"two_clash": lambda: _case([[0, 0, 0], [2.0, 0, 0]], ["C", "C"]), "two_apart": lambda: _case([[0, 0, 0], [3.0, 0, 0]], ["C", "C"]),
             "one_atom": lambda: _case([[1, 2, 3]], ["C"]),
             "empty_sel1": lambda: _case([[0, 0, 0], [2.0, 0, 0]], ["C", "C"], sel1=np.zeros(2, bool), sel2=np.ones(2, bool)),
             "empty_sel2": lambda: _case([[0, 0, 0], [2.0, 0, 0]], ["C", "C"], sel1=np.ones(2, bool), sel2=np.zeros(0, np.int64)),
             "cutoff_negative": lambda: _cutoff_case(4.0), "cutoff_zero": lambda: _cutoff_case(2.0 * float(F32(1.7))),
             "lanes64": lambda: _lanes(64), "lanes65": lambda: _lanes(65), "planar": _planar, "faces": _faces,
             "cross_disjoint": lambda: _cross("disjoint"), "cross_overlap": lambda: _cross("overlap"), "cross_equal": lambda: _cross("equal"),
             "threshold_edges": _threshold_edges, "ties": _ties, "elements": _elements, "3ptb": lambda: _3ptb("default"),
             "3ptb_noguess": lambda: _3ptb("noguess"), "3ptb_cross_mask": lambda: _3ptb("cross_mask"), "3ptb_cross_index": lambda: _3ptb("cross_index"),
             "crowded": _crowded}
for _name, _ov in OVERLAPS.items():
    _BUILDERS[_name] = functools.partial(lambda ov: _case(*_cluster(210, 60, 8.0), bonds=[(i, i + 1) for i in range(0, 59, 3)], overlap=ov), _ov)
for _name, _fl in FLAGS.items():
    _BUILDERS[_name] = functools.partial(_excl, _fl)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


def as_mol(c, frame=0, frames=1):
    """what find_clashes takes: the case's frame as frame `frame` of `frames` (the others NaN, so that reading one shows)"""
    coords = np.full((len(c["coords"]), 3, frames), np.nan, F32)
    coords[:, :, frame] = c["coords"]
    return SimpleNamespace(numAtoms=len(c["coords"]), frame=frame, numFrames=frames, coords=coords, element=c["element"], name=c["name"],
                           bonds=c["bonds"].copy())


def kwargs(c):
    return {k: c[k] for k in ("sel1", "sel2", "overlap", "exclude_bonded", "exclude_14", "guess_bonds")}


@functools.lru_cache(maxsize=None)
def bonds_used(name):
    """the bond list the exclusions are built from: the file bonds stacked on the restated guesser's"""
    c = case(name)
    if c["guess_bonds"]:
        return np.vstack((c["bonds"], BR.guess(c["coords"], c["element"], c["name"]))).astype(np.uint32)
    return c["bonds"]


@functools.lru_cache(maxsize=None)
def restated(name):
    """(pairs, distances, overlaps, details) of the restatement, computed once"""
    c = case(name)
    return R.find_clashes(c["coords"], R.radii_of(c["element"]), bonds_used(name), c["sel1"], c["sel2"], c["overlap"], c["exclude_bonded"],
                          c["exclude_14"], details=True)


def check():
    """every case is the case it is meant to be, on the restatement"""
    n = lambda name: len(restated(name)[0])   # noqa: E731
    assert n("two_clash") == 1 and n("two_apart") == 0 and n("one_atom") == 0 and n("empty_sel1") == 0 and n("empty_sel2") == 0
    # the overlaps: each looser value a longer list, a larger cutoff; exclusions at work in each
    sizes = [n(k) for k in OVERLAPS]
    assert sizes[0] > 0 and all(x < y for x, y in zip(sizes, sizes[1:])), sizes
    cuts = [restated(k)[3]["cutoff"] for k in OVERLAPS]
    assert all(x < y for x, y in zip(cuts, cuts[1:])) and all(restated(k)[3]["excluded"] > 0 for k in OVERLAPS)
    # cutoff <= 0: the kd-tree still finds candidates (it squares its radius), the float32 test keeps none
    d = restated("cutoff_negative")[3]
    assert d["cutoff"] < 0 and d["candidates"] >= 3 and n("cutoff_negative") == 0
    d = restated("cutoff_zero")[3]
    assert d["cutoff"] == 0.0 and d["candidates"] == 2 and n("cutoff_zero") == 0
    # one box, a wave's lanes full and one over
    for name, count in (("lanes64", 64), ("lanes65", 65)):
        c = case(name)
        assert len(c["sel1"]) == count and np.all(np.ptp(c["coords"][:count], axis=0) < grid_side(restated(name)[3]["cutoff"])) and n(name) > count
    c = case("planar")
    assert np.ptp(c["coords"][:, 2]) == 0 and np.all(np.ptp(c["coords"][:, :2], axis=0) > 3 * grid_side(restated("planar")[3]["cutoff"])) and n("planar") > 10
    f = case("faces")
    assert f["side"] == grid_side(restated("faces")[3]["cutoff"]) and np.array_equal(f["coords"].min(axis=0), f["min"])
    quot = ((f["lattice"] - f["min"]).astype(F32) / f["side"]).astype(F32)
    assert int((quot == np.floor(quot)).sum()) >= 60, "faces: atoms whose float32 quotient is a whole number"
    assert np.any(np.all(f["coords"] == f["lattice"].max(axis=0), axis=1)) and n("faces") > 5
    # cross mode
    p, _, _, d = restated("cross_disjoint")
    assert not d["self_mode"] and len(p) > 10 and np.all(p[:, 0] < 20) and np.all(p[:, 1] >= 20) and d["excluded"] > 0
    p, dist, _, d = restated("cross_overlap")
    rows = {tuple(r) for r in p.tolist()}
    both = set(range(18, 30))
    assert not d["self_mode"] and sum(a == b for a, b in rows) == 12 and all(dist[i] == 0 for i, (a, b) in enumerate(p.tolist()) if a == b)
    assert any((b, a) in rows for a, b in rows if a < b and a in both and b in both), "cross_overlap: a pair in both orders"
    bonded = {(i, i + 1) for i in range(47)}
    assert any((b, a) in bonded for a, b in rows if a > b), "cross_overlap: a bonded pair reported as (b, a)"
    assert not any((a, b) in bonded for a, b in rows), "cross_overlap: a bonded pair reported as (a, b)"
    p, _, _, d = restated("cross_equal")
    assert d["self_mode"] and len(p) > 10 and np.all(p[:, 0] < p[:, 1]) and p.min() >= 5 and p.max() < 40
    # exclusions: each flag combination its own set, each smaller list a subset of the larger
    ex = {k: R.excluded_set(case(k)["bonds"], *FLAGS[k]) for k in FLAGS}
    assert ex["excl_00"] == set() and ex["excl_10"] < ex["excl_11"] and ex["excl_01"] < ex["excl_11"] and not ex["excl_01"] <= ex["excl_10"]
    assert (9, 9) in ex["excl_10"] and (9, 9) not in ex["excl_01"]                     # the self-bond
    deg = np.bincount(np.unique(np.sort(case("excl_11")["bonds"].astype(np.int64), axis=1), axis=0).ravel(), minlength=30)
    assert deg.max() >= 8
    lists = {k: {tuple(r) for r in restated(k)[0].tolist()} for k in FLAGS}
    assert lists["excl_11"] < lists["excl_10"] < lists["excl_00"] and lists["excl_11"] < lists["excl_01"] < lists["excl_00"]
    assert all(restated(k)[3]["excluded"] > 0 for k in ("excl_11", "excl_10", "excl_01")) and len(lists["excl_11"]) > 20
    # threshold edges: every intended pair there, on its intended side
    c = case("threshold_edges")
    labels = [lab for lab, _, _ in c["labels"]]
    assert len(labels) == 12 and "CC_below_outside_cutoff" in labels and "CC_below_inside_cutoff" in labels, labels
    p, _, _, d = restated("threshold_edges")
    rows = {tuple(r) for r in p.tolist()}
    for label, first, clash in c["labels"]:
        assert ((first, first + 1) in rows) == clash, f"threshold_edges: {label} on the wrong side"
    assert d["prefilter_decided"] >= 1
    # ties
    _, _, o, _ = restated("ties")
    assert len(o) == 8 and len(set(o.tolist())) == 1
    # elements: the fall-backs and a radius above 3
    r = R.radii_of(case("elements")["element"])
    assert r[0] == F32(1.7) and r[1] == F32(1.7) and r[2] == F32(3.43) and r[5] == F32(3.48) and r[7] == F32(1.7) and n("elements") > 10
    # 3PTB
    assert n("3ptb") > 0 and n("3ptb_noguess") >= n("3ptb") and restated("3ptb")[3]["excluded"] > 1000
    pm, pi = restated("3ptb_cross_mask"), restated("3ptb_cross_index")
    assert not pm[3]["self_mode"] and len(pm[0]) > 0 and np.array_equal(pm[0], pi[0]) and np.array_equal(pm[2], pi[2])
    prot = _ptb()[4]
    assert prot[pm[0][:, 0]].all() and not prot[pm[0][:, 1]].any()
    c = case("crowded")
    assert np.all(np.ptp(c["coords"][:100], axis=0) < grid_side(restated("crowded")[3]["cutoff"])) and n("crowded") > 100
