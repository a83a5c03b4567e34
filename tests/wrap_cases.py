"""tests/wrap_cases.py -- TEST INFRASTRUCTURE: the cases of the periodic wrap that the CPU tier (emulated kernels) and the GPU tier share.

Every case is frame-major float32 ``xyz [F, N, 3]``, ``box [3, F]``, group ``starts [G + 1]`` and a centre selection or a centre.  The
expected result is the restatement's (tests/wrap_restatement.py), computed once per case and never changed.  Every array stays below a
few MB.  SMALL_MAX and CHUNK restate the two constants of csrc/wrap_kernels.h at which the kernels take another path
(tests/test_wrap_cpu.py asserts them against the built emulator).
"""
from __future__ import annotations

import functools
import os
from collections import namedtuple

import numpy as np

import wrap_restatement as wr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL_MAX = 16       # WRAP_SMALL_MAX: groups up to this size take the lane kernel
CHUNK = 256          # WRAP_CHUNK: atoms per LDS chunk of the wave kernels
SIZES = (1, 2, 3, 63, 64, 65, 134, SMALL_MAX - 1, SMALL_MAX, SMALL_MAX + 1, CHUNK - 1, CHUNK, CHUNK + 1, 3384)
FRAMES = (1, 2, 63, 64, 65, 130)

Case = namedtuple("Case", "xyz box starts centersel center")


def starts_of(sizes):
    return np.r_[0, np.cumsum(sizes)].astype(np.uint32)


def _random(sizes, F, seed, spread=3.0):
    """groups of the given sizes scattered over +- spread boxes, a different box in every frame"""
    rng = np.random.default_rng(seed)
    starts = starts_of(sizes)
    N = int(starts[-1])
    box = rng.uniform(20.0, 40.0, (3, F)).astype(np.float32)
    gid = np.repeat(np.arange(len(sizes)), sizes)
    centres = rng.uniform(-spread, spread, (F, len(sizes), 3)) * box.T[:, None, :]
    xyz = (centres[:, gid, :] + rng.normal(0.0, 1.5, (F, N, 3))).astype(np.float32)
    return xyz, box, starts


def _edge():
    """single atoms and pairs on the decisions' edges, around the centre (0, 0, 0) given: per axis the box is 30, 31.7 and 8"""
    f32 = np.float32
    box1 = np.array([30.0, 31.7, 8.0], f32)
    half = box1 / f32(2)
    up = np.nextafter(half, f32(np.inf))
    rows, sizes = [], []

    def add(*atoms):
        rows.extend(atoms)
        sizes.append(len(atoms))

    add(half)                                                   # a centre exactly at + box / 2: not moved
    add(-half)
    add(up)                                                     # one ulp beyond: moved
    add(-up)
    add(half, half)                                             # the same with a chain of two steps
    add(up, up)
    add(-up, -up, -up)
    for q in (1.5, -1.5, 2.5, -2.5):                            # diff / box exactly +-1.5, +-2.5 on the axis whose box is 8: round gives
        add(np.array([0.0, 0.0, q * 8.0], f32))                 # 2 and 3 where rint gives 2 and 2
        add(np.array([q * 30.0, 0.0, 0.0], f32))                # (45, 75: exact in float32 as well)
    for k in (1000.3, -1000.3, 999.5, -1000.5):                 # +-1 000 boxes away: the product box * round(...) is rounded to float32
        add((box1.astype(np.float64) * k).astype(f32))
        add((box1.astype(np.float64) * k).astype(f32), (box1.astype(np.float64) * (k + 0.01)).astype(f32))
    add(np.array([np.nan, 40.0, 1.0], f32), np.array([1.0, 41.0, 9.0], f32))        # a NaN: only that group's axis is affected
    add(np.array([50.0, np.inf, 1.0], f32), np.array([51.0, 41.0, 9.0], f32))       # an infinity
    add(np.array([-np.inf, 1.0, -13.0], f32))
    add(np.array([70.0, -70.0, 70.0], f32), np.array([71.0, -71.0, 71.0], f32))     # an ordinary neighbour of those
    xyz = np.stack(rows).astype(f32)[None]                      # [1, N, 3]
    # frame 1: the same atoms, a zero box length on one axis; frame 2: an all-zero box among real ones; frame 3: another real box
    xyz = np.repeat(xyz, 4, axis=0)
    box = np.stack([box1, np.array([30.0, 0.0, 8.0], f32), np.zeros(3, f32), np.array([17.0, 23.0, 29.0], f32)], axis=1)
    return Case(np.ascontiguousarray(xyz), np.ascontiguousarray(box), starts_of(sizes), None, np.zeros(3, f32))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case"""
    out = {}
    xyz, box, starts = _random(SIZES, 2, 11)
    out["sizes_center"] = Case(xyz, box, starts, None, np.array([3.0, -2.0, 11.0], np.float32))
    # a centre selection inside groups that move: all atoms of one group and twenty of another that lies boxes away -- the cell's centre
    # falls near the first, the second is moved towards it, and a centre taken AFTER that move would lie elsewhere
    sizes = np.diff(starts.astype(np.int64))
    ga, gb = int(np.flatnonzero(sizes == CHUNK - 1)[0]), int(np.flatnonzero(sizes == CHUNK + 1)[0])
    inside = np.r_[np.arange(starts[gb], starts[gb + 1]), np.arange(starts[ga], starts[ga] + 20)[::-1]].astype(np.uint32)
    out["sizes_sel_inside_moving"] = Case(xyz, box, starts, inside, None)                   # (gb first, then ga's in reverse: the order is part of the result)
    small = (1, 2, 3, SMALL_MAX + 1, 65, CHUNK + 44)
    for F in FRAMES:
        x, b, s = _random(small, F, 100 + F)
        out[f"frames_{F}"] = Case(x, b, s, np.array([5, 0, 3, 30, 300], np.uint32), None)
    x, b, s = _random(small, 3, 7)
    out["sel_one_atom"] = Case(x, b, s, np.array([41], np.uint32), None)
    out["sel_everything"] = Case(x, b, s, np.arange(int(s[-1]), dtype=np.uint32), None)
    out["sel_empty_center_given"] = Case(x, b, s, np.zeros(0, np.uint32), np.array([-4.5, 100.25, 0.0], np.float32))
    out["edge"] = _edge()
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's result of a case, read-only"""
    c = cases()[name]
    r = wr.wrap_frames(c.xyz, c.box, c.starts, c.centersel, c.center)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def fixture():
    """the reference's own wrapping test system: (coords float32 [N, 3, 1] in Angstrom, box float32 [3, 1], group starts, the
    literal centre of its test)"""
    from moleculekit_amd import xtc

    t = xtc.XTCread(os.path.join(GOLDEN, "wrap", "wrap_6X18.xtc"))
    z = np.load(os.path.join(GOLDEN, "wrap_cases.npz"))
    coords = np.ascontiguousarray(t.coords, np.float32)
    coords.setflags(write=False)
    return coords, np.ascontiguousarray(t.box, np.float32), z["group_starts"], z["center"]


PROTEIN_6X18 = slice(0, 6814)      # the four chains are the first four groups (467 + 1360 + 1603 + 3384 atoms): what a centre selection takes


@functools.lru_cache(maxsize=None)
def fixture_expected(with_sel):
    coords, box, starts, center = fixture()
    sel = np.arange(coords.shape[0], dtype=np.uint32)[PROTEIN_6X18] if with_sel else None
    moved = []
    r = wr.wrap_box(coords, box, starts, sel, None if with_sel else center, moved=moved)
    r.setflags(write=False)
    return r, moved[0]


def assert_same_bits(got, want, what=""):
    """bit equality of two float32 arrays: the same positions hold a NaN, every other value has the same 32 bits.  (The payload and
    the sign of a NaN that an operation PRODUCES are the processor's choice -- x86 gives the negative default NaN, the GPU the positive
    one -- so NaNs are compared by position.)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), f"{what}: NaNs at different positions ({int(ng.sum())} against {int(nw.sum())})"
    a = np.where(ng, np.float32(0), got).view(np.uint32)
    b = np.where(nw, np.float32(0), want).view(np.uint32)
    bad = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} values differ in their bits, first at flat index {int(bad[0])}: " \
                          f"{got.reshape(-1)[bad[0]]!r} against {want.reshape(-1)[bad[0]]!r}"
