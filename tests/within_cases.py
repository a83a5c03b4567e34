"""tests/within_cases.py -- TEST INFRASTRUCTURE: the seeded cases of the proximity selection (``within_distance``)
and ``check()``, which asserts that every case is the case it is meant to be.  The compiled reference's answers to them are
tests/golden/within_cases.npz (tests/golden/make_golden_within.py).

A case: ``coords`` float32 [F, N, 3], ``sel1`` / ``sel2`` uint32 index arrays, ``cutoff`` (a Python float, as a caller passes it), the
gate bounds ``mn`` / ``mx`` float32 [F, 3] as they go to the reference (default: per frame the numpy min / max of the sources, as
atomselect.py computes them; zeros for an empty source) and ``preset`` bool [F, n1] or None: the results array on entry.
"""
import functools
import os

import numpy as np

import within_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
F32, U32 = np.float32, np.uint32
BOX_CAP = 4096
GOLDEN = ("strict_edge", "rounding_tellers", "cutoff_3p3", "cutoff_zero", "cutoff_negative_single_source", "cutoff_negative_wide_source",
          "cutoff_nan", "cutoff_inf", "cutoff_1e20", "cutoff_1e-30", "self_in_source", "unsorted_duplicates", "empty_sel2", "empty_sel1",
          "results_preset", "nan_query", "nan_source", "inf_source", "nan_bounds_all_axes", "one_by_one", "lanes65", "queries_outside_grid",
          "box_edges", "crowded_box", "3ptb_ligand_5A", "3ptb_protein_of_ligand", "traj3")
TELLER_MIN = 8


def _case(coords, sel1, sel2, cutoff, mn=None, mx=None, preset=None):
    coords = np.ascontiguousarray(coords, F32)
    if coords.ndim == 2:
        coords = coords[None]
    sel1, sel2 = np.ascontiguousarray(sel1, U32).reshape(-1), np.ascontiguousarray(sel2, U32).reshape(-1)
    F = coords.shape[0]
    if mn is None:
        with np.errstate(invalid="ignore"):
            mn = np.stack([coords[f][sel2].min(axis=0) if len(sel2) else np.zeros(3, F32) for f in range(F)])
            mx = np.stack([coords[f][sel2].max(axis=0) if len(sel2) else np.zeros(3, F32) for f in range(F)])
    mn, mx = np.ascontiguousarray(mn, F32).reshape(F, 3), np.ascontiguousarray(mx, F32).reshape(F, 3)
    return dict(coords=coords, sel1=sel1, sel2=sel2, cutoff=float(cutoff), mn=mn, mx=mx, preset=None if preset is None else np.array(preset, bool).reshape(F, -1))


def _ulp(v, k):
    v = F32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf if k > 0 else -np.inf))
    return v


def _strict_edge():
    # queries at the origin side, sources at (3, 4, 0) from them: diff == 25 exactly, and one ulp either side along x
    q = np.array([[0, 0, 0], [10, 0, 0], [20, 0, 0]], F32)
    s = np.array([[3, 4, 0], [_ulp(13, -1), 4, 0], [_ulp(23, 1), 4, 0]], F32)
    return _case(np.concatenate([q, s]), [0, 1, 2], [3, 4, 5], 5.0)


@functools.lru_cache(maxsize=None)
def _teller_pairs():
    """seeded search: pairs at about 5 A whose decision under the reference's sequence differs from an alternative's"""
    rng = np.random.default_rng(20260101)
    found = {k: [] for k in R.ALTERNATIVES}
    slot, used = 0, set()                                            # (one pair per lattice cell, 20 A apart)
    _, sq = R.f32_cutoff(5.0)
    for _ in range(400):
        n = 4096
        cell = slot + np.arange(n)
        base = (np.stack([cell % 8, (cell // 8) % 8, cell // 64], axis=1) * 20.0 + rng.random((n, 3))).astype(F32)
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1)[:, None]
        src = (base.astype(np.float64) + u * 5.0 * (1.0 + rng.uniform(-3e-7, 3e-7, n))[:, None]).astype(F32)
        d = base - src
        sqd = d * d
        ref = ((sqd[:, 0] + sqd[:, 1]) + sqd[:, 2]) < sq
        d64 = base.astype(np.float64) - src.astype(np.float64)
        f64 = ((d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1]) + d64[:, 2] * d64[:, 2]) < np.float64(sq)
        acc = np.zeros(n, F32)
        for k in range(3):
            acc = (acc.astype(np.float64) + d[:, k].astype(np.float64) * d[:, k].astype(np.float64)).astype(F32)
        dsq = acc < sq
        for i in np.flatnonzero((ref != f64) | (ref != dsq)):
            for name, alt in R.ALTERNATIVES.items():
                if len(found[name]) < TELLER_MIN + 2 and int(cell[i]) not in used and alt(base[i], src[i], 5.0) != bool(ref[i]):
                    found[name].append((base[i].copy(), src[i].copy()))
                    used.add(int(cell[i]))
                    break
        if all(len(v) >= TELLER_MIN + 2 for v in found.values()):
            break
    return found


def _rounding_tellers():
    pairs = [p for v in _teller_pairs().values() for p in v]
    q = np.array([p[0] for p in pairs], F32)
    s = np.array([p[1] for p in pairs], F32)
    n = len(pairs)
    return _case(np.concatenate([q, s]), np.arange(n), np.arange(n, 2 * n), 5.0)


def _cutoff_3p3():
    # float32(3.3)^2 in float32 is 10.889999...; 3.3^2 in double is 10.89 (rounded to float32: another value).  Sources along x at
    # distances whose float32 square lies between, below and above the two
    _, sq32 = R.f32_cutoff(3.3)
    sq64 = F32(3.3 * 3.3)
    lo, hi = (sq32, sq64) if sq32 < sq64 else (sq64, sq32)
    ds = []
    d = F32(np.sqrt(np.float64(lo)))
    for k in range(-6, 7):
        ds.append(_ulp(d, k))
    ds = np.array(ds, F32)
    q = np.stack([np.arange(len(ds)) * 16.0, np.zeros(len(ds)), np.zeros(len(ds))], axis=1).astype(F32)
    s = q.copy()
    s[:, 1] = ds                                                     # (along y: the difference 0 - d is exact)
    n = len(ds)
    return _case(np.concatenate([q, s]), np.arange(n), np.arange(n, 2 * n), 3.3)


def _cloud(seed, n, side):
    return (np.random.default_rng(seed).random((n, 3)) * side).astype(F32)


def _cutoff_case(cutoff, seed=3):
    c = _cloud(seed, 120, 12.0)
    return _case(c, np.arange(120), np.arange(0, 120, 3), cutoff)


def _negative_single():
    c = _cloud(5, 80, 8.0)
    return _case(c, np.arange(80), [17], -4.0)


def _negative_wide():
    # the gate closes where max - 4 < x < min + 4 on all three axes: with sources spread over 6 A that is the middle 2 A of their box
    c = _cloud(6, 600, 16.0)
    return _case(c, np.arange(600), np.flatnonzero(((c >= 5.0) & (c <= 11.0)).all(axis=1)), -4.0)


def _self_in_source():
    c = _cloud(7, 90, 14.0)
    return _case(c, np.arange(90), np.arange(30, 60), 3.0)


def _unsorted_duplicates():
    c = _cloud(8, 100, 12.0)
    rng = np.random.default_rng(80)
    return _case(c, rng.integers(0, 100, 150), rng.integers(0, 100, 40), 2.5)


def _results_preset():
    c = _cloud(9, 100, 16.0)
    preset = np.zeros(100, bool)
    preset[::7] = True
    return _case(c, np.arange(100), np.arange(0, 100, 10), 3.0, preset=preset)


def _nan_query():
    c = _cloud(10, 100, 10.0)
    c[3, 0] = np.nan
    c[4, 1] = np.nan
    c[5] = np.nan
    c[6, 2] = np.inf
    return _case(c, np.arange(50), np.arange(50, 100), 4.0)


def _nan_source():
    c = _cloud(11, 100, 10.0)
    c[60, 1] = np.nan
    c[61] = np.nan
    src = c[50:]
    ok = np.isfinite(src).all(axis=1)
    return _case(c, np.arange(50), np.arange(50, 100), 3.0, mn=src[ok].min(axis=0), mx=src[ok].max(axis=0))


def _inf_source():
    c = _cloud(12, 100, 10.0)
    c[70, 0] = np.inf
    c[71, 2] = -np.inf
    c[2, 0] = np.inf                                                 # a query at +inf too: inf - inf is NaN
    src = c[50:]
    ok = np.isfinite(src).all(axis=1)
    return _case(c, np.arange(50), np.arange(50, 100), 3.0, mn=src[ok].min(axis=0), mx=src[ok].max(axis=0))


def _nan_bounds():
    c = _cloud(13, 60, 8.0)
    return _case(c, np.arange(60), np.arange(0, 60, 4), 4.0, mn=[np.nan] * 3, mx=[np.nan] * 3)


def _lanes65():
    # 65 queries x 65 sources; the sources sit 100 A away from every query but the last source, which touches only the last query
    q = np.stack([np.arange(65) * 1.0, np.zeros(65), np.zeros(65)], axis=1)
    s = np.stack([np.arange(65) * 1.0, np.full(65, 100.0), np.zeros(65)], axis=1)
    q[64] = [500.0, 0.0, 0.0]
    s[64] = [501.0, 0.0, 0.0]
    return _case(np.concatenate([q, s]), np.arange(65), np.arange(65, 130), 2.0)


def _queries_outside_grid():
    rng = np.random.default_rng(14)
    src = rng.random((1500, 3)) * 40.0
    cut = 4.0
    inside = rng.random((300, 3)) * 40.0
    near, far = [], []
    for ax in range(3):
        for sign in (-1, 1):
            p = rng.random((60, 3)) * 40.0
            p[:, ax] = (40.0 + rng.random(60) * cut) if sign > 0 else (-rng.random(60) * cut)
            near.append(p)
            p = rng.random((20, 3)) * 40.0
            p[:, ax] = (40.0 + 2.0 * cut + rng.random(20) * 3 * cut) if sign > 0 else (-2.0 * cut - rng.random(20) * 3 * cut)
            far.append(p)
    huge = np.array([[1e30, 20, 20], [-1e30, 20, 20], [20, 1e30, 20], [20, 20, -1e30], [1e30, -1e30, 1e30], [3e38, 20, 20]])
    q = np.concatenate([inside] + near + far + [huge])
    return _case(np.concatenate([src, q]), np.arange(1500, 1500 + len(q)), np.arange(1500), cut)


def _box_edges():
    # sources on a jittered lattice of period 7 A (further apart than two cutoffs, so a query has ONE source near it); each query sits
    # at the cutoff -/+ 2 ulp from its source along an axis direction or a diagonal.  With a box side just above the cutoff nearly
    # every such pair straddles a box boundary, on every axis and diagonal
    cut = 3.0
    g = np.arange(0, 36, 7.0)
    rng = np.random.default_rng(15)
    src = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    src = (src + rng.uniform(-0.3, 0.3, src.shape)).astype(F32)
    dirs = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)], np.float64)
    qs = []
    for k, i in enumerate(rng.choice(len(src), 208, replace=False)):
        u = dirs[k % 26] / np.linalg.norm(dirs[k % 26])
        for eps in (-1, 1):
            qs.append(src[i].astype(np.float64) + u * np.float64(_ulp(cut, 2 * eps)))
    return _case(np.concatenate([src, np.array(qs)]), np.arange(len(src), len(src) + len(qs)), np.arange(len(src)), cut)


def _crowded_box():
    rng = np.random.default_rng(16)
    src = rng.random((5000, 3)) * 0.5 + 10.0
    far = rng.random((200, 3)) * 30.0
    q = np.concatenate([rng.random((300, 3)) * 30.0, rng.random((100, 3)) * 6.0 + 7.0])
    return _case(np.concatenate([src, far, q]), np.arange(5200, 5600), np.arange(5200), 3.0)


@functools.lru_cache(maxsize=None)
def _ptb():
    d = np.load(os.path.join(HERE, "golden", "channels_3ptb.npz"))
    return d["coords"].astype(F32), d["resname"] == "BEN", ~np.isin(d["resname"], ("BEN", "HOH", "CA"))


def _3ptb(kind):
    coords, ligand, protein = _ptb()
    if kind == "ligand_5A":
        return _case(coords, np.arange(len(coords)), np.flatnonzero(ligand), 5.0)
    return _case(coords, np.flatnonzero(protein), np.flatnonzero(ligand), 4.0)                  # "protein and within 4 of resname BEN"


def _traj3():
    rng = np.random.default_rng(17)
    c0 = rng.random((400, 3)) * 25.0
    c = np.stack([c0, c0 + rng.normal(size=c0.shape) * 1.5, c0 + rng.normal(size=c0.shape) * 3.0]).astype(F32)
    c[1, 350, 1] = np.nan                                            # a NaN source in the middle frame
    sel2 = np.arange(300, 400)
    mn = np.stack([np.nanmin(c[f][sel2], axis=0) for f in range(3)])
    mx = np.stack([np.nanmax(c[f][sel2], axis=0) for f in range(3)])
    return _case(c, np.arange(300), sel2, 3.5, mn=mn, mx=mx)


_BUILDERS = {
    "strict_edge": _strict_edge, "rounding_tellers": _rounding_tellers, "cutoff_3p3": _cutoff_3p3, "cutoff_zero": lambda: _self_in_source() | {"cutoff": 0.0},
    "cutoff_negative_single_source": _negative_single, "cutoff_negative_wide_source": _negative_wide, "cutoff_nan": lambda: _cutoff_case(float("nan")),
    "cutoff_inf": lambda: _cutoff_case(float("inf")), "cutoff_1e20": lambda: _cutoff_case(1e20), "cutoff_1e-30": lambda: _cutoff_case(1e-30),
    "self_in_source": _self_in_source, "unsorted_duplicates": _unsorted_duplicates, "empty_sel2": lambda: _case(_cloud(1, 20, 5.0), np.arange(20), [], 5.0),
    "empty_sel1": lambda: _case(_cloud(2, 20, 5.0), [], np.arange(20), 5.0), "results_preset": _results_preset, "nan_query": _nan_query,
    "nan_source": _nan_source, "inf_source": _inf_source, "nan_bounds_all_axes": _nan_bounds,
    "one_by_one": lambda: _case([[0, 0, 0], [1, 1, 1]], [0], [1], 2.0), "lanes65": _lanes65, "queries_outside_grid": _queries_outside_grid,
    "box_edges": _box_edges, "crowded_box": _crowded_box, "3ptb_ligand_5A": lambda: _3ptb("ligand_5A"),
    "3ptb_protein_of_ligand": lambda: _3ptb("protein_of_ligand"), "traj3": _traj3,
}
assert set(_BUILDERS) == set(GOLDEN)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def _restated(name):
    c = case(name)
    out = R.frames(c["coords"], c["sel1"], c["sel2"], c["cutoff"], gate=(c["mn"], c["mx"]), preset=c["preset"])
    out.setflags(write=False)
    return out


def restated(name):
    """bool [F, n1]: the restatement's results array after the call(s), gate and preset included (computed once, read-only)"""
    return _restated(name)


def ungated(name):
    """bool [F, n1]: what the pair test alone finds (no gate, no preset)"""
    c = case(name)
    return R.frames(c["coords"], c["sel1"], c["sel2"], c["cutoff"])


class Mol:
    """a duck-typed molecule: coords float32 [N, 3, F], numAtoms, numFrames, frame, atomselect for masks and index arrays"""

    def __init__(self, c, frame=0):
        self.coords = np.ascontiguousarray(np.transpose(c["coords"], (1, 2, 0)))
        self.numAtoms, self.numFrames, self.frame = self.coords.shape[0], self.coords.shape[2], frame

    def atomselect(self, sel):
        sel = np.asarray(sel)
        if sel.dtype == bool:
            return sel
        mask = np.zeros(self.numAtoms, bool)
        mask[sel] = True
        return mask


def check():
    """every case is the case it is meant to be (on the restatement)"""
    r = {n: restated(n) for n in GOLDEN}
    for n in GOLDEN:
        c = case(n)
        assert c["coords"].shape[1] <= 6000 and r[n].shape == (c["coords"].shape[0], len(c["sel1"])), n
    # strict_edge: diff == 25 is not within; one ulp closer is, one ulp further is not
    c = case("strict_edge")
    assert R.pair_diff(c["coords"][0][:1], c["coords"][0][3:4])[0, 0] == F32(25.0) and r["strict_edge"].tolist() == [[False, True, False]]
    # rounding_tellers: each alternative decides at least TELLER_MIN of the pairs differently from the restatement
    c = case("rounding_tellers")
    n = len(c["sel1"])
    xyz = c["coords"][0]
    mine = np.array([bool(R.pair_diff(xyz[i:i + 1], xyz[n + i:n + i + 1])[0, 0] < R.f32_cutoff(5.0)[1]) for i in range(n)])
    assert np.array_equal(mine, r["rounding_tellers"][0]), "a teller query is decided by another source than its own"
    for name, alt in R.ALTERNATIVES.items():
        told = sum(alt(xyz[i], xyz[n + i], 5.0) != mine[i] for i in range(n))
        assert told >= TELLER_MIN, (name, told)
    assert mine.any() and not mine.all()
    # cutoff_3p3: some pair lies between the float32 square of float32(3.3) and the float32 rounding of 3.3^2 in double
    c = case("cutoff_3p3")
    n = len(c["sel1"])
    diffs = np.array([R.pair_diff(c["coords"][0][i:i + 1], c["coords"][0][n + i:n + i + 1])[0, 0] for i in range(n)])
    sq32, sq64 = R.f32_cutoff(3.3)[1], F32(3.3 * 3.3)
    assert sq32 != sq64 and ((diffs >= min(sq32, sq64)) & (diffs < max(sq32, sq64))).any() and r["cutoff_3p3"].any() and not r["cutoff_3p3"].all()
    assert np.array_equal(r["cutoff_3p3"][0], diffs < sq32)
    # the special cutoffs
    assert not r["cutoff_zero"].any() and len(np.intersect1d(case("cutoff_zero")["sel1"], case("cutoff_zero")["sel2"]))
    assert not r["cutoff_negative_single_source"].any() and ungated("cutoff_negative_single_source").sum() > 3
    w, wu = r["cutoff_negative_wide_source"], ungated("cutoff_negative_wide_source")
    assert w.any() and (wu & ~w).any(), "the wide source box keeps some hits and the gate removes others"
    assert not r["cutoff_nan"].any() and r["cutoff_inf"].all() and r["cutoff_1e20"].all() and not r["cutoff_1e-30"].any()
    assert np.isinf(R.f32_cutoff(1e20)[1]) and R.f32_cutoff(1e-30)[1] == 0 and R.f32_cutoff(1e-30)[0] > 0
    # index semantics
    c = case("self_in_source")
    assert r["self_in_source"][0][c["sel2"]].all() and not r["self_in_source"].all()
    c = case("unsorted_duplicates")
    assert len(np.unique(c["sel1"])) < len(c["sel1"]) and len(np.unique(c["sel2"])) < len(c["sel2"]) and (np.diff(c["sel1"].astype(int)) < 0).any()
    assert r["unsorted_duplicates"].any() and not r["unsorted_duplicates"].all()
    assert r["empty_sel2"].shape == (1, 20) and not r["empty_sel2"].any() and r["empty_sel1"].shape == (1, 0)
    c = case("results_preset")
    assert (c["preset"] & ~ungated("results_preset")).any() and (r["results_preset"] >= c["preset"]).all() and (r["results_preset"] & ~c["preset"]).any()
    # non-finite input
    assert not r["nan_query"][0][3:7].any() and r["nan_query"].any()
    for n in ("nan_source", "inf_source"):
        c = case(n)
        assert not np.isfinite(c["coords"][0][c["sel2"]]).all() and r[n].any() and not r[n].all()
    assert np.isinf(case("inf_source")["coords"][0][2, 0]) and not r["inf_source"][0][2]
    assert not r["nan_bounds_all_axes"].any() and ungated("nan_bounds_all_axes").any()
    assert r["one_by_one"].tolist() == [[True]]
    assert r["lanes65"][0].tolist() == [False] * 64 + [True]
    # queries_outside_grid: hits and misses among the queries within one cutoff outside the sources' cube; none further out
    c = case("queries_outside_grid")
    q = c["coords"][0][c["sel1"]]
    outside = ((q < 0) | (q > 40)).any(axis=1)
    beyond = ((q < -4.0) | (q > 44.0)).any(axis=1)
    res = r["queries_outside_grid"][0]
    assert res[outside & ~beyond].any() and (~res[outside & ~beyond]).any() and beyond.sum() >= 120 and not res[beyond].any() and res[~outside].any()
    assert (np.abs(q) >= 1e30).any()
    # box_edges: both decisions, from pairs within a few ulps of the cutoff
    assert r["box_edges"].any() and not r["box_edges"].all()
    # crowded_box: more sources than a box may hold within one box side of any grid the plan builds (side >= 1 A)
    c = case("crowded_box")
    s = c["coords"][0][c["sel2"]][:5000]
    assert (s.max(axis=0) - s.min(axis=0)).max() <= 0.5 and 5000 > BOX_CAP and r["crowded_box"].any() and not r["crowded_box"].all()
    for n in ("3ptb_ligand_5A", "3ptb_protein_of_ligand"):
        assert r[n].any() and not r[n].all()
    t = r["traj3"]
    assert t.shape == (3, 300) and all(t[f].any() for f in range(3)) and (t[0] != t[1]).any() and (t[1] != t[2]).any()
    assert np.isnan(case("traj3")["coords"][1][case("traj3")["sel2"]]).any()
