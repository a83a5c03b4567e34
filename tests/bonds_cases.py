"""tests/bonds_cases.py -- TEST INFRASTRUCTURE: the seeded cases of the bond guesser, the smallest shapes at which each part of it can
go wrong.  A case is a dict: ``coords`` float32 [N, 3], ``radii`` float32 [N], ``is_h`` uint32 [N], ``grid_cutoff`` -- what
``bond_grid_search`` takes -- and, for the cases that go through ``guess_bonds``, ``element`` and ``name`` (the radii, the flags and
the cut-off are then what ``guess_bonds`` derives from them).  ``check()`` asserts on the restatement (tests/bonds_restatement.py)
that every case is the case it is meant to be.

tests/golden/bond_cases.npz holds what the compiled reference returns for every name in GOLDEN (make_golden_bonds.py).
"""
from __future__ import annotations

import functools
import os
from types import SimpleNamespace

import numpy as np

import bonds_restatement as R

F32, F64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))

GOLDEN = ("pair_edges", "one_box", "planar", "line", "boundaries", "neighbours14", "3ptb", "3ptb_shuffled", "water",
          "unwrapped_1e4", "unwrapped_1e5", "unwrapped_1e6", "unwrapped_1e7", "crowded")
GRID_SHAPES = ("one_box", "planar", "line", "boundaries")
# cases whose list must hold bonds AND whose grid must hold rejected pairs
MIXED = ("pair_edges", "one_box", "planar", "boundaries", "3ptb", "3ptb_shuffled", "water", "crowded")
BOX_CAP = 4096


def _mol_case(coords, element, name):
    element, name = np.asarray(element, dtype="<U2"), np.asarray(name, dtype="<U4")
    radii = R.radii_of(element, name)
    return {"coords": np.ascontiguousarray(coords, F32), "element": element, "name": name, "radii": radii,
            "is_h": (element == "H").astype(np.uint32), "grid_cutoff": R.default_cutoff(radii)}


def _f32_sum_sq(dx, dy):
    return F32(F32(F32(dx) * F32(dx)) + F32(F32(dy) * F32(dy)))


def _place(target):
    """(dx, dy) float32 with (dx dx + dy dy) + 0 == target in float32 arithmetic; dx a multiple of 2^-10, so that x0 + dx is exact for
    the x0 in use and the guesser's own subtraction returns dx"""
    target = F32(target)
    dx = F32(np.floor(np.sqrt(F64(target)) * 0.9 * 1024.0) / 1024.0)
    dy = F32(np.sqrt(F64(target) - F64(dx) * F64(dx)))
    lo = dy
    for _ in range(4096):
        lo = np.nextafter(lo, F32(0))
    cand = lo
    for _ in range(8192):
        if _f32_sum_sq(dx, cand) == target:
            return dx, cand
        cand = np.nextafter(cand, F32(np.inf))
    raise AssertionError(f"no float32 (dx, dy) reaches dist2 = {target!r}")


def _pair_edges():
    """isolated pairs 12 A apart along x; PAIRS: (label, first atom, bonded?) in the order of the atoms"""
    up = lambda v: np.nextafter(F32(v), F32(np.inf))   # noqa: E731
    r = {"C": F32(1.7), "Cl": F32(2.27), "H": F32(1.0)}
    cut2 = lambda a, b: F32(F32(0.6 * F64(F32(a + b))) * F32(0.6 * F64(F32(a + b))))   # noqa: E731
    gc = float(r["Cl"] * 1.2)                                       # the largest radius of the structure is chlorine's
    cutoff2 = F32(F32(gc) * F32(gc))
    just_ok = F32(0.001)                                            # float32(0.001) > 0.001: not "near identical"
    assert F64(just_ok) >= 0.001 > F64(np.nextafter(just_ok, F32(0)))
    spec = [  # label, elements, names, dist2 target or plain distance
        ("cc_at_cut", ("C", "C"), ("CA", "CB"), ("d2", cut2(r["C"], r["C"]))),
        ("cc_above_cut", ("C", "C"), ("CA", "CB"), ("d2", up(cut2(r["C"], r["C"])))),
        ("clcl_at_cutoff2", ("Cl", "Cl"), ("CL1", "CL2"), ("d2", cutoff2)),
        ("clcl_above_cutoff2", ("Cl", "Cl"), ("CL1", "CL2"), ("d2", up(cutoff2))),
        ("cc_below_001", ("C", "C"), ("CA", "CB"), ("d2", np.nextafter(just_ok, F32(0)))),
        ("cc_at_001", ("C", "C"), ("CA", "CB"), ("d2", just_ok)),
        ("cc_identical", ("C", "C"), ("CA", "CB"), ("d", 0.0)),
        ("hh_inside", ("H", "H"), ("H1", "H2"), ("d", 0.8)),
        ("hc_inside", ("H", "C"), ("H1", "CA"), ("d", 1.0)),
        ("CL_by_name_apart", ("CL", "CL"), ("CL1", "CL2"), ("d", 1.9)),      # "CL" misses the table: the name's C, 1.5 -> cut 1.8
        ("CL_by_name_bonded", ("CL", "CL"), ("CL1", "CL2"), ("d", 1.7)),
        ("default_bonded", ("Xx", "Xx"), ("Q1", "Q2"), ("d", 1.75)),           # neither table nor name rule: 1.5 -> cut 1.8
        ("default_apart", ("Xx", "Xx"), ("Q1", "Q2"), ("d", 1.85)),
    ]
    coords, element, name, labels = [], [], [], []
    for k, (label, els, nms, (kind, v)) in enumerate(spec):
        x0 = F32(12.0 * k)
        dx, dy = _place(v) if kind == "d2" else (F32(v), F32(0.0))
        assert kind == "d" or F32(F32(x0 + dx) - x0) == dx
        coords += [(x0, 0.0, 0.0), (F32(x0 + dx), dy, 0.0)]
        element += list(els)
        name += list(nms)
        labels.append(label)
    c = _mol_case(np.array(coords, F32), element, name)
    c["labels"] = labels
    c["bonded"] = {"cc_at_cut": True, "cc_above_cut": False, "clcl_above_cutoff2": False, "cc_below_001": False, "cc_at_001": True,
                   "cc_identical": False, "hh_inside": False, "hc_inside": True, "CL_by_name_apart": False, "CL_by_name_bonded": True,
                   "default_bonded": True, "default_apart": False}
    return c


def _one_box():
    rng = np.random.default_rng(101)
    coords = rng.uniform(0.0, 1.9, size=(12, 3))
    element = ["C", "N", "O", "H", "C", "H", "S", "C", "O", "H", "N", "C"]
    return _mol_case(coords, element, [e + "1" for e in element])


def _planar():
    rng = np.random.default_rng(102)
    gx, gy = np.meshgrid(np.arange(9) * 1.42, np.arange(7) * 1.42, indexing="ij")
    coords = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 3.25)], axis=1)
    coords[:, :2] += rng.uniform(-0.15, 0.15, size=(len(coords), 2))
    order = rng.permutation(len(coords))
    element = np.where(rng.random(len(coords)) < 0.2, "N", "C")
    return _mol_case(coords[order], element, [e + "1" for e in element])


def _line():
    rng = np.random.default_rng(103)
    coords = np.zeros((41, 3))
    coords[:, 0] = np.cumsum(rng.uniform(1.2, 2.3, size=41))
    coords[:, 1:] = (-7.5, 2.25)
    order = rng.permutation(41)
    return _mol_case(coords[order], ["C"] * 41, ["CA"] * 41)


def _boundaries():
    """carbons exactly on the grid's box boundaries, min + k * pairdist in float32 arithmetic, the maximum corner among them, and a
    partner beside each that mostly sits across a boundary"""
    rng = np.random.default_rng(104)
    pd = F32(float(F32(1.7) * 1.2))
    mn = np.array([-3.5, 10.25, 0.125], F32)
    lattice = np.array([[mn[0] + F32(i) * pd, mn[1] + F32(j) * pd, mn[2] + F32(k) * pd] for i in range(4) for j in range(3) for k in range(3)], F32)
    step = rng.normal(size=lattice.shape)
    step = step / np.linalg.norm(step, axis=1, keepdims=True) * rng.uniform(1.1, 1.9, size=(len(lattice), 1))
    partners = np.clip(lattice + step, mn, lattice.max(axis=0)).astype(F32)      # (the corners stay the lattice's)
    coords = np.concatenate([lattice, partners])
    order = rng.permutation(len(coords))
    c = _mol_case(coords[order], ["C"] * len(coords), ["CA"] * len(coords))
    c["lattice"], c["min"], c["pd"] = lattice, mn, pd
    return c


def _neighbours14():
    """eight carbons +-0.4 A around an interior grid vertex, one in each adjoining box, between two anchors that span the grid"""
    pd = float(F32(1.7) * 1.2)
    v = 2.0 * pd
    eight = np.array([[v + sx * 0.4, v + sy * 0.4, v + sz * 0.4] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])
    coords = np.concatenate([eight, [[0.0, 0.0, 0.0], [4.0 * pd + 0.5, 4.0 * pd + 0.5, 4.0 * pd + 0.5]]])
    order = np.random.default_rng(105).permutation(len(coords))
    return _mol_case(coords[order], ["C"] * len(coords), ["CA"] * len(coords))


@functools.lru_cache(maxsize=None)
def _ptb():
    d = np.load(os.path.join(HERE, "golden", "channels_3ptb.npz"))
    return d["coords"].astype(F32), d["element"], d["name"], d["bonds"]


def _3ptb(shuffled=False):
    coords, element, name, bonds = _ptb()
    if shuffled:
        p = np.random.default_rng(106).permutation(len(coords))
        return _mol_case(coords[p], element[p], name[p])
    c = _mol_case(coords, element, name)
    c["expected"] = bonds
    return c


def _water():
    rng = np.random.default_rng(107)
    n = 10
    centres = np.stack(np.meshgrid(*([np.arange(n) * 3.1] * 3), indexing="ij"), axis=-1).reshape(-1, 3) + rng.uniform(-0.3, 0.3, size=(n ** 3, 3))
    half = np.deg2rad(104.5) / 2.0
    coords = np.zeros((n ** 3, 3, 3))
    for w, c in enumerate(centres):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        coords[w, 0] = c
        coords[w, 1] = c + 0.9572 * (np.cos(half) * q[0] + np.sin(half) * q[1])
        coords[w, 2] = c + 0.9572 * (np.cos(half) * q[0] - np.sin(half) * q[1])
    return _mol_case(coords.reshape(-1, 3), ["O", "H", "H"] * n ** 3, ["OH2", "H1", "H2"] * n ** 3)


def _unwrapped(span):
    coords = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [span, 0.0, 0.0], [span, span, span]], F32)
    return {"coords": coords, "radii": np.full(4, 1.7, F32), "is_h": np.zeros(4, np.uint32), "grid_cutoff": 2.04}


def _crowded(n_target=None):
    """a compact 3PTB fragment and one atom far along the diagonal: the escalated box side exceeds the fragment"""
    coords, element, name, _ = _ptb()
    centre = coords.astype(F64).mean(axis=0)
    keep = np.flatnonzero(np.linalg.norm(coords - centre, axis=1) < 11.0)
    frag = coords[keep] - coords[keep].min(axis=0)
    far = frag.max(axis=0) + 5000.0
    return _mol_case(np.concatenate([frag, far[None, :]]), list(element[keep]) + ["C"], list(name[keep]) + ["CA"])


def over_cap():
    """4 097 coincident atoms: one more than a box may hold"""
    n = BOX_CAP + 1
    return {"coords": np.full((n, 3), 1.25, F32), "radii": np.full(n, 1.7, F32), "is_h": np.zeros(n, np.uint32), "grid_cutoff": 2.04}


_BUILDERS = {"pair_edges": _pair_edges, "one_box": _one_box, "planar": _planar, "line": _line, "boundaries": _boundaries,
             "neighbours14": _neighbours14, "3ptb": _3ptb, "3ptb_shuffled": lambda: _3ptb(True), "water": _water, "crowded": _crowded,
             "unwrapped_1e4": lambda: _unwrapped(1e4), "unwrapped_1e5": lambda: _unwrapped(1e5), "unwrapped_1e6": lambda: _unwrapped(1e6),
             "unwrapped_1e7": lambda: _unwrapped(1e7)}


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


def as_mol(c, frame=0, frames=1):
    """what guess_bonds takes: the case's frame as frame `frame` of `frames` (the others NaN, so that reading one shows)"""
    coords = np.full((len(c["coords"]), 3, frames), np.nan, F32)
    if frame < frames:
        coords[:, :, frame] = c["coords"]
    return SimpleNamespace(numAtoms=len(c["coords"]), frame=frame, numFrames=frames, coords=coords, element=c["element"], name=c["name"])


@functools.lru_cache(maxsize=None)
def restated(name):
    """(pairs, details) of the restatement, computed once"""
    c = case(name)
    return R.search(c["coords"], c["grid_cutoff"], c["is_h"], c["radii"], details=True)


def check():
    """every case is the case it is meant to be, on the restatement"""
    # pair_edges: each intended pair on its intended side
    c = case("pair_edges")
    pairs, det = restated("pair_edges")
    got = {tuple(sorted(p)) for p in pairs.tolist()}
    assert all(abs(int(i) - int(j)) == 1 and min(i, j) % 2 == 0 for i, j in got), "pair_edges: a bond between two pairs"
    for k, label in enumerate(c["labels"]):
        d2 = R.dist2_of(c["coords"], 2 * k, np.array([2 * k + 1]))[0]
        if label == "clcl_at_cutoff2":
            assert not d2 > det["cutoff2"]                           # (cut * cut then decides: the golden list says which way)
            continue
        if label == "clcl_above_cutoff2":
            assert d2 > det["cutoff2"] and d2 == np.nextafter(det["cutoff2"], F32(np.inf))
        assert ((2 * k, 2 * k + 1) in got) == c["bonded"][label], f"pair_edges: {label} on the wrong side"
    r = c["radii"]
    lab = c["labels"]
    assert r[2 * lab.index("clcl_at_cutoff2")] == F32(2.27) and r[2 * lab.index("CL_by_name_apart")] == F32(1.5) and r[2 * lab.index("default_apart")] == F32(1.5)
    # grid shapes
    assert restated("one_box")[1]["grid"][:3] == (1, 1, 1)
    g = restated("planar")[1]["grid"]
    assert g[2] == 1 and g[0] > 1 and g[1] > 1
    g = restated("line")[1]["grid"]
    assert g[1] == 1 and g[2] == 1 and g[0] > 8
    b = case("boundaries")
    g = restated("boundaries")[1]["grid"]
    assert min(g[:3]) >= 2 and F32(g[3]) == b["pd"] and np.array_equal(b["coords"].min(axis=0), b["min"])
    quot = ((b["lattice"] - b["min"]).astype(F32) / b["pd"]).astype(F32)
    assert int((quot == np.floor(quot)).sum()) >= 60, "boundaries: atoms whose float32 quotient is a whole number"
    assert np.any(np.all(b["coords"] == b["lattice"].max(axis=0), axis=1)), "boundaries: the atom at the maximum corner"
    # neighbours14: every non-self relation from the owner's side
    pairs, det = restated("neighbours14")
    assert len(pairs) == 28 and set(det["relations"].tolist()) >= set(range(1, 14)), sorted(set(det["relations"].tolist()))
    # 3ptb: the fixture's bonds, and rows the wrong way round among them
    pairs, _ = restated("3ptb")
    assert np.array_equal(pairs, case("3ptb")["expected"]) and int((pairs[:, 0] > pairs[:, 1]).sum()) == 597
    # shuffled: the box order no longer follows the box index
    c = case("3ptb_shuffled")
    _, flat = R.boxes_of(c["coords"], c["coords"].min(axis=0), restated("3ptb_shuffled")[1]["grid"])
    _, first = np.unique(flat, return_index=True)
    assert np.any(np.diff(first) < 0)
    # water: every O-H bond and nothing else
    pairs, _ = restated("water")
    assert len(pairs) == 2000 and np.all(pairs.min(axis=1) % 3 == 0) and np.all(pairs.max(axis=1) - pairs.min(axis=1) <= 2)
    for span in ("1e4", "1e5", "1e6", "1e7"):
        pairs, det = restated("unwrapped_" + span)
        assert pairs.tolist() == [[0, 1]]
        g = det["grid"]
        assert g[3] > 2.04 and g[0] * g[1] * g[2] <= 4e6 and g[0] > 100, (span, g)      # (an escalated grid)
    pairs, det = restated("crowded")
    assert 64 <= det["max_occ"] <= BOX_CAP and det["max_occ"] == len(case("crowded")["coords"]) - 1 and det["grid"][3] > 22.0
    for name in MIXED:
        pairs, det = restated(name)
        assert len(pairs) and det["rejected"], f"{name}: must hold bonds and rejected in-grid pairs"
