"""tests/rings_cases.py -- TEST INFRASTRUCTURE: the seeded cases of the ring-interaction tests (CPU and GPU tier, golden data).

A case is a dict: name, kind (0 pi-pi, 1 cation-pi, 2 sigma-hole), coords float32 [N, 3, F], box float32 [3, F], rings1 (a list of
uint32 atom-index arrays), second (pi-pi: rings2; cation-pi: cations uint32 [n]; sigma-hole: halides uint32 [n, 2]), thr (pi-pi: dist1,
angle1 max, dist2, angle2 min; the others: dist, angle min), and optionally raw = (ring_atoms, starts1, starts2): the lists as they go
to the compiled `calculate` where that is NOT what the reference's Python wrapper would build (both pi-pi lists naming the same
stretch of the atom list: the self-interaction skip).

Rings are planar polygons of 3, 5, 6 or 9 atoms with random centres, orientations and per-frame jitter; their atoms sit at shuffled,
non-contiguous indices of a larger atom array.  `flatten(case)` gives (ring_atoms, starts1, second) as the reference's wrappers build
them.  `check_margins()` asserts the condition the comparisons rest on: no float64 angle of a pair that passed the distance tests
lies within 1e-4 degrees of a threshold in use (so no pair's verdict hangs on the last bits of an arccos).
"""
from __future__ import annotations

import numpy as np

PIPI, CATIONPI, SIGMAHOLE = 0, 1, 2
F32 = np.float32
SIZES = (3, 5, 6, 9)
MARGIN_DEG = 1e-4
PIPI_DEFAULT = (4.4, 30.0, 5.5, 60.0)
CATIONPI_DEFAULT = (5.0, 60.0)
SIGMAHOLE_DEFAULT = (4.5, 60.0)


def _frame(rng):
    """a random orthonormal frame (rows: u, v, normal)"""
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def _polygon(k, radius, centre, frame):
    ang = 2 * np.pi * np.arange(k) / k
    return centre + radius * (np.cos(ang)[:, None] * frame[0] + np.sin(ang)[:, None] * frame[1])


class _System:
    """atoms are appended as [F, 3] trajectories and given shuffled indices at the end"""

    def __init__(self, seed, F, extent, jitter=0.15):
        self.rng = np.random.default_rng(seed)
        self.F, self.extent, self.jitter = F, extent, jitter
        self.atoms = []

    def add_atom(self, xyz):                                           # xyz [F, 3]
        self.atoms.append(np.asarray(xyz, np.float64))
        return len(self.atoms) - 1

    def moving(self, point):
        """a point that wanders a little from frame to frame"""
        return point + self.jitter * self.rng.normal(size=(self.F, 3))

    def add_ring(self, k=None, centre=None, radius=1.39, frame=None, rigid=False):
        rng = self.rng
        k = int(rng.choice(SIZES)) if k is None else k
        centre = rng.uniform(0, self.extent, 3) if centre is None else np.asarray(centre, np.float64)
        frame = _frame(rng) if frame is None else frame
        base = _polygon(k, radius, centre, frame)                      # [k, 3]
        drift = np.zeros((self.F, 3)) if rigid else self.jitter * rng.normal(size=(self.F, 3))
        wobble = 0.0 if rigid else 0.05
        return [self.add_atom(base[i] + drift + wobble * rng.normal(size=(self.F, 3))) for i in range(k)], centre, frame

    def finish(self, spare=7):
        """-> coords float32 [N, 3, F] and the map old index -> shuffled index"""
        n = len(self.atoms)
        N = n + spare
        perm = self.rng.permutation(N)[:n]
        coords = self.rng.uniform(-50, 50, (N, 3, self.F))
        for i, a in enumerate(self.atoms):
            coords[perm[i]] = a.T
        return coords.astype(F32), perm.astype(np.uint32)


def _box(kind, F, extent, rng):
    box = np.zeros((3, F), F32)
    if kind == "zero":
        return box
    box[:] = (extent + rng.uniform(0, 0.5, (3, F))).astype(F32)
    if kind == "zero_axis":
        box[1] = 0
    return box


def _random_case(name, kind, seed, n1, n2, F, extent, box="zero", thr=None, near=0.5, shared=0, fused=False, quiet_frames=()):
    """n1 rings against n2 rings / cations / halides.  `near`: the share of second partners placed where they interact with a ring
    (the rest are anywhere); `shared`: pi-pi, that many rings of the first list are ALSO in the second; `fused`: the first two rings of
    list 1 share two atoms; `quiet_frames`: frames blown up so far that nothing is in range."""
    sysm = _System(seed, F, extent)
    rng = sysm.rng
    rings1, info = [], []
    for r in range(n1):
        if fused and r == 1:
            # a five-ring sharing an edge (two atoms) with the first six-ring, in its plane
            atoms0, c0, fr0 = info[0]
            p0, p1 = (sysm.atoms[atoms0[0]], sysm.atoms[atoms0[1]])
            mid = (p0 + p1) / 2
            out = mid - (c0 + 0 * mid)
            out = out / np.linalg.norm(out, axis=1, keepdims=True)
            extra = [sysm.add_atom(mid + 1.2 * out + s * 0.7 * (p1 - p0)) for s in (1.0, 0.0, -1.0)]
            rings1.append([atoms0[1]] + extra + [atoms0[0]])
            info.append((rings1[-1], c0, fr0))
            continue
        atoms, c, fr = sysm.add_ring(k=6 if fused and r == 0 else None)
        rings1.append(atoms)
        info.append((atoms, c, fr))
    second = []
    for j in range(n2):
        host = info[int(rng.integers(n1))]
        close = rng.random() < near
        if kind == PIPI:
            if j < shared:
                second.append(list(rings1[j]))
                continue
            if close:
                # stacked, T-shaped or tilted above the host ring
                tilt = rng.choice([0.0, 0.3, 1.2, np.pi / 2])
                fr = host[2].copy()
                c, s = np.cos(tilt), np.sin(tilt)
                fr = np.stack([fr[0], c * fr[1] + s * fr[2], -s * fr[1] + c * fr[2]])
                centre = host[1] + rng.uniform(3.4, 5.2) * host[2][2] + rng.uniform(-0.8, 0.8) * host[2][0]
                atoms, _, _ = sysm.add_ring(centre=centre, frame=fr)
            else:
                atoms, _, _ = sysm.add_ring()
            second.append(atoms)
        else:
            if close:
                off = rng.uniform(-1.2, 1.2, 2)
                p = host[1] + rng.choice([-1, 1]) * rng.uniform(2.8, 4.6) * host[2][2] + off[0] * host[2][0] + off[1] * host[2][1]
            else:
                p = rng.uniform(0, extent, 3)
            a = sysm.add_atom(sysm.moving(p))
            if kind == CATIONPI:
                second.append(a)
            else:
                # the bonded carbon: roughly behind the halogen as seen from the ring, or anywhere
                d = _frame(rng)[0] if rng.random() < 0.4 else (p - host[1]) / np.linalg.norm(p - host[1])
                second.append([a, sysm.add_atom(sysm.moving(p + 1.8 * d))])
    coords, perm = sysm.finish()
    for f in quiet_frames:
        coords[:, :, f] *= F32(40)
    rings1 = [perm[np.asarray(r)] for r in rings1]
    if kind == PIPI:
        second = [perm[np.asarray(r)] for r in second]
    else:
        second = perm[np.asarray(second)]
    bx = _box(box, F, extent, rng)
    if box != "zero":
        # straddle the faces: shift everything so that the cell's faces cut through the rings, then put every atom back inside
        coords += F32(extent / 2)
        for ax in range(3):
            if bx[ax, 0] != 0:
                coords[:, ax, :] -= bx[ax] * np.floor(coords[:, ax, :] / bx[ax])
    default = {PIPI: PIPI_DEFAULT, CATIONPI: CATIONPI_DEFAULT, SIGMAHOLE: SIGMAHOLE_DEFAULT}[kind]
    return dict(name=name, kind=kind, coords=np.ascontiguousarray(coords, F32), box=bx, rings1=rings1, second=second,
                thr=tuple(thr or default))


def _stacked_case(F=256, seed=41):
    """a six-ring 3.5 A above an exact translated copy of itself, a fresh orientation in every frame.  Every coordinate and the
    translation are multiples of 2^-10 A: the copy is exact in float32, the two unit normals are the same bits, and their float32 dot
    product comes out at 1, just below or just ABOVE it -- where acos is NaN and the reference drops the pair."""
    rng = np.random.default_rng(seed)
    q = 1024.0
    coords = np.zeros((12, 3, F))
    for f in range(F):
        fr = _frame(rng)
        ring = np.round(_polygon(6, 1.39, rng.uniform(5, 25, 3), fr) * q) / q
        shift = np.round(3.5 * fr[2] * q) / q
        coords[:6, :, f] = ring
        coords[6:, :, f] = ring + shift
    coords = coords.astype(F32)
    assert np.array_equal(coords[6:] - coords[:6], np.broadcast_to((coords[6] - coords[0])[None], (6, 3, F)))
    return dict(name="pp_stacked_copy", kind=PIPI, coords=coords, box=np.zeros((3, F), F32), rings1=[np.arange(6, dtype=np.uint32)],
                second=[np.arange(6, 12, dtype=np.uint32)], thr=PIPI_DEFAULT)


def _wide_case(seed=43, F=3):
    """nine-rings 20 A across, interleaved: the centroids of a pair are a few A apart, but the first atoms of some pairs sit on opposite
    sides (> 15 A: the early exit drops the pair) and of others on the same side (reported)"""
    sysm = _System(seed, F, 30.0, jitter=0.05)
    fr = _frame(sysm.rng)
    rings1, rings2 = [], []
    for i, turn in enumerate((0.0, np.pi, 0.3)):
        c, s = np.cos(turn), np.sin(turn)
        fr_t = np.stack([c * fr[0] + s * fr[1], -s * fr[0] + c * fr[1], fr[2]])
        a, _, _ = sysm.add_ring(k=9, centre=np.array([15.0, 15.0, 15.0]) + 1.5 * i * fr[2], radius=10.0, frame=fr_t)
        (rings1 if i == 0 else rings2).append(a)
    a, _, _ = sysm.add_ring(k=6, centre=np.array([15.0, 15.0, 15.0]) + 3.6 * fr[2], frame=fr)
    rings2.append(a)
    coords, perm = sysm.finish()
    return dict(name="pp_wide_ring_early_exit", kind=PIPI, coords=coords, box=np.zeros((3, F), F32), rings1=[perm[np.asarray(r)] for r in rings1],
                second=[perm[np.asarray(r)] for r in rings2], thr=PIPI_DEFAULT)


def _degenerate_case(seed=47, F=5):
    """the first three atoms of ring 0 are collinear: its normal is 0 / 0, every angle with it NaN, nothing with it reported"""
    c = _random_case("pp_degenerate_normal", PIPI, seed, 3, 4, F, 6.0, near=1.0)
    r = c["rings1"][0]
    # multiples of 2^-8 A and their exact midpoint: a1 - a2 is exactly half of a0 - a2 and every component of the cross product is 0
    a0, a2 = (np.round(c["coords"][r[k]].astype(np.float64) * 256) / 256 for k in (0, 2))
    c["coords"][r[0]], c["coords"][r[2]], c["coords"][r[1]] = a0.astype(F32), a2.astype(F32), ((a0 + a2) / 2).astype(F32)
    return c


def _same_list_raw(seed=53, F=4):
    """both pi-pi lists name the SAME stretches of the atom list (what the wrapper never builds): identical rings are skipped"""
    c = _random_case("pp_same_list_raw", PIPI, seed, 5, 3, F, 7.0, near=1.0)
    atoms = np.concatenate(c["rings1"]).astype(np.uint32)
    starts = np.insert(np.cumsum([len(r) for r in c["rings1"]]), 0, 0).astype(np.uint32)
    c["second"] = [r.copy() for r in c["rings1"]]
    c["raw"] = (atoms, starts, starts.copy())
    return c


def build_cases():
    R = _random_case
    cases = [
        R("pp_1x1_f1", PIPI, 1, 1, 1, 1, 4.0, near=1.0),
        R("pp_2x3_f3", PIPI, 2, 2, 3, 3, 6.0, near=1.0),
        R("pp_63x64_f3", PIPI, 3, 63, 64, 3, 22.0),
        R("pp_65x130_f1", PIPI, 4, 65, 130, 1, 24.0),
        R("pp_130x65_f65_box", PIPI, 5, 130, 65, 65, 26.0, box="box"),
        R("pp_64x63_f64_zero_axis", PIPI, 6, 64, 63, 64, 22.0, box="zero_axis"),
        R("pp_3x2_f200_quiet", PIPI, 7, 3, 2, 200, 5.0, near=1.0, quiet_frames=tuple(range(0, 200, 3))),
        R("pp_dense_12x12_f5", PIPI, 8, 12, 12, 5, 2.0, near=0.0, thr=(6.5, 45.0, 7.5, 45.0)),
        R("pp_a1max0_a2min90", PIPI, 9, 20, 20, 3, 9.0, thr=(4.4, 0.0, 5.5, 90.0)),
        R("pp_thresholds", PIPI, 10, 20, 20, 3, 9.0, thr=(5.0, 20.0, 6.0, 70.0)),
        R("pp_shared_rings_fused", PIPI, 11, 6, 5, 3, 7.0, shared=3, fused=True),
        R("pp_9x7_f65_box", PIPI, 12, 9, 7, 65, 7.0, box="box"),
        R("pp_8x9_f3_zero_axis", PIPI, 13, 8, 9, 3, 7.0, box="zero_axis"),
        _stacked_case(),
        _wide_case(),
        _degenerate_case(),
        _same_list_raw(),
        R("cp_1x1_f1", CATIONPI, 21, 1, 1, 1, 4.0, near=1.0),
        R("cp_3x63_f3", CATIONPI, 22, 3, 63, 3, 8.0),
        R("cp_64x65_f64_box", CATIONPI, 23, 64, 65, 64, 20.0, box="box"),
        R("cp_130x130_f3_zero_axis", CATIONPI, 24, 130, 130, 3, 24.0, box="zero_axis"),
        R("cp_65x64_f200", CATIONPI, 25, 65, 64, 200, 20.0, quiet_frames=(0, 7, 199)),
        R("cp_2x1_f65_thresholds", CATIONPI, 26, 2, 1, 65, 4.0, near=1.0, thr=(6.0, 35.0)),
        R("cp_fused_5x9_f2", CATIONPI, 27, 5, 9, 2, 6.0, near=1.0, fused=True),
        R("cp_7x9_f65_box", CATIONPI, 28, 7, 9, 65, 7.0, box="box"),
        R("sh_1x1_f1", SIGMAHOLE, 31, 1, 1, 1, 4.0, near=1.0),
        R("sh_63x130_f3", SIGMAHOLE, 32, 63, 130, 3, 20.0),
        R("sh_64x63_f65_box", SIGMAHOLE, 33, 64, 63, 65, 20.0, box="box"),
        R("sh_3x65_f200", SIGMAHOLE, 34, 3, 65, 200, 8.0),
        R("sh_130x64_f1", SIGMAHOLE, 35, 130, 64, 1, 22.0),
        R("sh_2x2_f64_thresholds", SIGMAHOLE, 36, 2, 2, 64, 4.0, near=1.0, thr=(6.5, 20.0)),
        R("sh_6x8_f64_box", SIGMAHOLE, 37, 6, 8, 64, 7.0, box="box"),
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


# the cases whose reference results are committed (tests/golden/ring_cases.npz): the small ones -- the file holds their coordinates
GOLDEN = ("pp_2x3_f3", "pp_63x64_f3", "pp_9x7_f65_box", "pp_8x9_f3_zero_axis", "pp_dense_12x12_f5", "pp_a1max0_a2min90", "pp_thresholds",
          "pp_shared_rings_fused", "pp_stacked_copy", "pp_wide_ring_early_exit", "pp_degenerate_normal", "pp_same_list_raw",
          "cp_3x63_f3", "cp_7x9_f65_box", "cp_2x1_f65_thresholds", "cp_fused_5x9_f2",
          "sh_63x130_f3", "sh_6x8_f64_box", "sh_2x2_f64_thresholds")


def flatten(c):
    """(ring_atoms, starts1, second) as the reference's wrapper hands them to `calculate` (second: starts2 shifted behind the first
    list, the cations, or the halides) -- or the case's raw lists"""
    if "raw" in c:
        return c["raw"]
    r1 = c["rings1"]
    starts1 = np.insert(np.cumsum([len(r) for r in r1]), 0, 0).astype(np.uint32)
    if c["kind"] != PIPI:
        return np.hstack(r1).astype(np.uint32), starts1, np.asarray(c["second"], np.uint32)
    r2 = c["second"]
    starts2 = (np.insert(np.cumsum([len(r) for r in r2]), 0, 0) + starts1.max()).astype(np.uint32)
    return np.hstack((np.hstack(r1), np.hstack(r2))).astype(np.uint32), starts1, starts2


_EXPECTED = {}


def expected(c):
    """the restatement's (frame_offsets, pairs, distang) of a case, computed once; the margin condition is asserted on the way"""
    if c["name"] not in _EXPECTED:
        from rings_restatement import calculate, threshold_margin
        atoms, s1, second = flatten(c)
        offs, pairs, da, tested, angle = calculate(c["kind"], c["coords"], c["box"], atoms, s1, second, c["thr"], details=True)
        margin = threshold_margin(c["kind"], c["thr"] if c["kind"] == PIPI else tuple(c["thr"]) + (0, 0), tested, angle)
        assert margin >= MARGIN_DEG, f"{c['name']}: an angle lies {margin:.3g} degrees from a threshold; pick another seed"
        for a in (offs, pairs, da):
            a.setflags(write=False)
        _EXPECTED[c["name"]] = (offs, pairs, da)
    return _EXPECTED[c["name"]]


def check_margins():
    for c in cases():
        expected(c)
