"""tests/wrap_cell_cases.py -- TEST INFRASTRUCTURE: the cases of the periodic wrap of triclinic boxes that the CPU tier (emulated kernels)
and the GPU tier share.

Every case is frame-major float32 ``xyz [F, N, 3]``, float64 ``boxvectors [3, 3, F]``, group ``starts [G + 1]`` and a centre selection or a
centre; all three unit cells ("rectangular", "compact", "triclinic") run on each.  The expected result is the restatement's
(tests/wrap_cell_restatement.py), computed once per (case, mode) and never changed; the restatement itself is pinned to the compiled
reference on the GOLDEN subset (tests/golden/wrap_cell_cases.npz, written by tests/golden/make_golden_wrap_cell.py, which also stores
those cases' inputs: the tests compare them with what is generated here).  Every array stays below 4 MB.  SMALL_MAX and CHUNK restate
the two constants of csrc/wrap_kernels.h at which the kernels take another path.
"""
from __future__ import annotations

import functools
import os
from collections import namedtuple

import numpy as np

import wrap_cell_restatement as wcr
from wrap_cases import assert_same_bits, starts_of  # noqa: F401  (re-exported)

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wrap_cell_cases.npz")
SMALL_MAX = 16       # WRAP_SMALL_MAX: groups up to this size take the lane kernel
CHUNK = 256          # WRAP_CHUNK: atoms per LDS chunk of the wave kernels
SIZES = (1, 2, 3, SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, 63, 64, 65, 134, CHUNK - 1, CHUNK, CHUNK + 1, 700)
SMALL = (1, 2, 3, SMALL_MAX + 1, 65, CHUNK + 44)
FRAMES = (1, 2, 63, 64, 65)
MODES = wcr.MODES

# name -> (lengths, angles in degrees).  "ortho": angles of 90, handed over as vectors all the same
BOXES = {
    "dodeca": ((60.0, 60.0, 60.0), (60.0, 60.0, 90.0)),             # rhombic dodecahedron
    "octa": ((70.0, 70.0, 70.0), (109.4712, 109.4712, 109.4712)),    # truncated octahedron
    "hexa": ((55.0, 55.0, 80.0), (90.0, 90.0, 120.0)),               # hexagonal prism
    "skew": ((50.0, 62.0, 41.0), (75.0, 100.0, 115.0)),
    "ortho": ((44.0, 51.0, 38.0), (90.0, 90.0, 90.0)),
}
GOLDEN = ("dodeca_sizes_center", "octa_frames_2", "hexa_sel_one_atom", "skew_sel_everything", "ortho_center", "face", "nan")
HOST_ONLY = ("far_1000", "inf")          # the emulated kernels only: the GPU tier runs nothing the reference would not end on quickly

Case = namedtuple("Case", "xyz boxvectors starts centersel center")


def vectors_of(lengths, angles):
    """float64 [3, 3, F] from lengths [3, F] and angles [3, F]: the formula of the reference's unitcell.py, as wrap.box_vectors has it
    (tests/test_wrap_cell_cpu.py pins that function to recorded values of the reference)"""
    from moleculekit_amd.wrap import box_vectors

    return box_vectors(np.asarray(lengths, np.float64), np.asarray(angles, np.float64))


def _box(kind, F, rng):
    """the box `kind`, slightly different in every frame (lengths scaled by up to 2 %, as a barostat would)"""
    lengths, angles = BOXES[kind]
    scale = 1.0 + 0.02 * rng.uniform(-1.0, 1.0, F)
    L = np.array(lengths)[:, None] * scale[None, :]
    A = np.repeat(np.array(angles)[:, None], F, axis=1)
    return vectors_of(L, A)


def _random(kind, sizes, F, seed, spread=5.0):
    """groups of the given sizes whose centres lie up to +- spread cells away along every box vector"""
    rng = np.random.default_rng(seed)
    starts = starts_of(sizes)
    N = int(starts[-1])
    bv = _box(kind, F, rng)
    gid = np.repeat(np.arange(len(sizes)), sizes)
    frac = rng.uniform(-spread, spread, (F, len(sizes), 3))
    centres = np.einsum("fgi,ijf->fgj", frac, bv)                               # sum_i frac_i * vector_i
    xyz = (centres[:, gid, :] + rng.normal(0.0, 1.5, (F, N, 3))).astype(np.float32)
    return np.ascontiguousarray(xyz), bv, starts


def _face():
    """Single atoms exactly on the faces of the cells and one ulp either side, around the centre (0, 0, 0) given, in a box whose entries
    and ratios are exact in float32: diagonal 32 / 64 / 64, off-diagonals 16 / 16 / 16.  box_middle is (32, 40, 32), shm01 = 0.25,
    shm02 = 0.1875, shm12 = 0.25, shift_centre = 0: with the other two coordinates 0 the triclinic faces of axis x lie at x = -16 and
    16, of y at -32 and 32, of z at -32 and 32 -- which are the other two modes' dx = -+ half the diagonal as well."""
    f32 = np.float32
    bv = np.zeros((3, 3, 2))
    bv[:, :, 0] = [[32.0, 0.0, 0.0], [16.0, 64.0, 0.0], [16.0, 16.0, 64.0]]
    bv[:, :, 1] = [[64.0, 0.0, 0.0], [16.0, 32.0, 0.0], [-16.0, 16.0, 64.0]]
    rows = []
    for axis, half in ((0, 16.0), (1, 32.0), (2, 32.0)):
        for cells in (0, 1, -2):
            for face in (-half, half):
                v = f32(face + cells * 2 * half)
                for x in (np.nextafter(v, f32(-np.inf)), v, np.nextafter(v, f32(np.inf))):
                    p = np.zeros(3, f32)
                    p[axis] = x
                    rows.append(p)
    for p in ((16.0, 32.0, 32.0), (-16.0, -32.0, -32.0), (16.0, -32.0, 32.0), (48.0, 96.0, -96.0), (8.0, 32.0, 0.0), (-24.0, 0.0, -32.0)):
        rows.append(np.array(p, f32))                                           # several faces at once
    xyz = np.repeat(np.stack(rows)[None], 2, axis=0)
    return Case(np.ascontiguousarray(xyz), bv, starts_of([1] * len(rows)), None, np.zeros(3, f32))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case"""
    out = {}
    xyz, bv, starts = _random("dodeca", SIZES, 2, 11)
    out["dodeca_sizes_center"] = Case(xyz, bv, starts, None, np.array([3.0, -2.0, 11.0], np.float32))
    # a centre selection inside groups that move: all atoms of one group and twenty of another that lies cells away
    sizes = np.diff(starts.astype(np.int64))
    ga, gb = int(np.flatnonzero(sizes == CHUNK - 1)[0]), int(np.flatnonzero(sizes == CHUNK + 1)[0])
    inside = np.r_[np.arange(starts[gb], starts[gb + 1]), np.arange(starts[ga], starts[ga] + 20)[::-1]].astype(np.uint32)
    out["dodeca_sel_inside_moving"] = Case(xyz, bv, starts, inside, None)
    for F in FRAMES:
        x, b, s = _random("octa", SMALL, F, 100 + F)
        out[f"octa_frames_{F}"] = Case(x, b, s, np.array([5, 0, 3, 30, 300], np.uint32), None)
    x, b, s = _random("hexa", SMALL, 3, 7)
    out["hexa_sel_one_atom"] = Case(x, b, s, np.array([41], np.uint32), None)
    x, b, s = _random("skew", SMALL, 3, 8)
    out["skew_sel_everything"] = Case(x, b, s, np.arange(int(s[-1]), dtype=np.uint32), None)
    x, b, s = _random("ortho", SMALL, 3, 9)
    out["ortho_center"] = Case(x, b, s, None, np.array([-4.5, 100.25, 0.0], np.float32))
    out["face"] = _face()
    x, b, s = _random("skew", (1, 2, 3, SMALL_MAX + 1, 65), 2, 10)
    x = x.copy()
    x[0, 1, 2] = np.nan                                                         # group 1 (two atoms, a lane) of frame 0
    x[1, int(s[4]) + 7, 0] = np.nan                                             # group 4 (65 atoms, a wave) of frame 1
    out["nan"] = Case(x, b, s, np.array([0, 3, 4], np.uint32), None)            # (the selection holds no NaN)
    # what only the emulated kernels run: groups 1 000 cells away, an infinite coordinate (the cap)
    x, b, s = _random("dodeca", (1, 3, SMALL_MAX + 1), 2, 12)
    far = x.copy()
    far[:, int(s[1]):int(s[2])] += (1000.0 * b[2, :, 0]).astype(np.float32)
    far[:, int(s[2]):] -= (999.0 * (b[0, :, 0] + b[1, :, 0])).astype(np.float32)
    out["far_1000"] = Case(far, b, s, None, np.zeros(3, np.float32))
    inf = x.copy()
    inf[0, 0, 1] = np.inf                                                       # a lane's group
    inf[1, int(s[3]) - 1, 2] = -np.inf                                          # a wave's group, its last atom: the centre stays -inf
    out["inf"] = Case(inf, b, s, None, np.zeros(3, np.float32))
    for c in out.values():
        for a in (c.xyz, c.boxvectors, c.starts):
            a.setflags(write=False)
    return out


def device_cases():
    """the names the GPU tier runs"""
    return sorted(n for n in cases() if n not in HOST_ONLY)


@functools.lru_cache(maxsize=None)
def expected(name, mode):
    """(the restatement's result of a case under a mode, its status words), read-only"""
    c = cases()[name]
    r, status = wcr.wrap_cell_frames(c.xyz, c.boxvectors, c.starts, mode, c.centersel, c.center)
    r.setflags(write=False)
    status.setflags(write=False)
    return r, status


@functools.lru_cache(maxsize=None)
def golden():
    """the npz as a dict"""
    with np.load(GOLDEN_FILE) as z:
        return {k: z[k] for k in z.files}
