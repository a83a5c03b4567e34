"""tests/dcd_cases.py -- TEST INFRASTRUCTURE: the named DCD cases of the CPU and GPU tiers, and a pure-Python DCD synthesiser for the
flavours the reference's writer cannot produce (opposite endian, 64-bit record markers, a 4th dimension, X-PLOR headers, fixed
atoms, other title blocks).  tests/golden/make_golden_dcd.py turns every case into file bytes (synthesised here, or written by the
reference) and records what the reference's reader returns for them in tests/golden/dcd_cases.npz.
"""
from __future__ import annotations

import struct

import numpy as np

SEED = 20261021


def coords(rng, F, N, special=False):
    x = (rng.standard_normal((F, N, 3)) * 30).astype(np.float32)
    if special and N >= 9:                     # bit patterns that must pass through untouched: NaN payloads, -0, inf, a denormal
        u = x.view(np.uint32)
        u[0, 1, 0], u[0, 2, 1], u[-1, 3, 2] = 0x7fc12345, 0xffa00001, 0x80000000
        u[0, 4, 0], u[-1, 5, 1], u[0, 6, 2] = 0x7f800000, 0xff800000, 0x00000007
    return x


def synth_dcd(xyz, cell=None, big=False, rec64=False, fourth=None, xplor=False, fixed=None, titles=("synthesised", "by tests/dcd_cases.py"),
              istart=0, nsavc=1, delta=1.0, nset=None, version=24) -> bytes:
    """A DCD file of the frames ``xyz`` float32 [F, N, 3].  ``cell`` float64 [F, 6]: the six stored doubles per frame (A, gamma, B,
    beta, alpha, C -- cosines or degrees, as given); ``big``: big-endian; ``rec64``: 8-byte record markers; ``fourth`` float32 [F, N]: a
    4th-dimension plane per frame; ``xplor``: an X-PLOR header (version 0, DELTA a double); ``fixed``: 0-based indices of fixed atoms --
    frames after the first then hold the other atoms only."""
    xyz = np.asarray(xyz, np.float32)
    F, N, _ = xyz.shape
    e = ">" if big else "<"
    i32 = lambda v: struct.pack(e + "i", int(v))                                        # noqa: E731
    mark = (lambda v: struct.pack(e + "q", int(v))) if rec64 else i32
    rec = lambda payload: mark(len(payload)) + payload + mark(len(payload))             # noqa: E731
    fixed = np.zeros(0, np.int64) if fixed is None else np.asarray(sorted(fixed), np.int64)
    free = np.setdiff1d(np.arange(N), fixed)
    head = b"CORD" + i32(F if nset is None else nset) + i32(istart) + i32(nsavc) + i32(0) * 5 + i32(len(fixed))
    if xplor:
        head += struct.pack(e + "d", delta) + i32(0) * 9
    else:
        head += struct.pack(e + "f", delta) + i32(0 if cell is None else 1) + i32(0 if fourth is None else 1) + i32(0) * 7 + i32(version)
    assert len(head) == 84
    out = [rec(head), rec(i32(len(titles)) + b"".join(t.encode().ljust(80, b"\0")[:80] for t in titles)), rec(i32(N))]
    if len(fixed):
        out.append(rec(np.asarray(free + 1, e + "i4").tobytes()))
    for f in range(F):
        atoms = np.arange(N) if f == 0 or not len(fixed) else free
        if cell is not None:
            out.append(rec(np.asarray(cell[f], e + "f8").tobytes()))
        for k in range(3):
            out.append(rec(np.ascontiguousarray(xyz[f, atoms, k]).astype(e + "f4").tobytes()))
        if fourth is not None:
            out.append(rec(np.ascontiguousarray(np.asarray(fourth, np.float32)[f, atoms]).astype(e + "f4").tobytes()))
    return b"".join(out)


def cos_cell(lengths, angles_deg, F):
    """The six doubles as CHARMM / NAMD > 2.5 store them: A, cos(gamma), B, cos(beta), cos(alpha), C -- exact 0 for a right angle."""
    a, b, g = (0.0 if v == 90 else float(np.cos(np.deg2rad(v))) for v in angles_deg)
    row = np.array([lengths[0], g, lengths[1], b, a, lengths[2]], np.float64)
    return np.tile(row, (F, 1)) * (1 + 0.001 * np.arange(F))[:, None] ** np.array([1, 0, 1, 0, 0, 1])


def deg_cell(lengths, angles_deg, F):
    """... and as NAMD 2.5 did: the angles in degrees."""
    return np.tile(np.array([lengths[0], angles_deg[2], lengths[1], angles_deg[1], angles_deg[0], lengths[2]], np.float64), (F, 1))


def with_fixed(xyz, fixed):
    """Fixed atoms keep frame 0's coordinates: what a reader must return for them in every frame."""
    xyz = xyz.copy()
    xyz[:, fixed] = xyz[0, fixed]
    return xyz


def synthesised_cases():
    """name -> dict(bytes=..., xyz=the coordinates a reader must return [F', N, 3], note=...).  Deterministic."""
    rng = np.random.default_rng(SEED)
    c = {}

    def add(name, xyz, expect=None, **kw):
        c[name] = dict(bytes=synth_dcd(xyz, **kw), xyz=xyz if expect is None else expect)

    add("plain", coords(rng, 4, 9, True))
    add("plain_n1", coords(rng, 1, 1))
    add("cell_cos_right", coords(rng, 4, 9), cell=cos_cell((30, 40, 50), (90, 90, 90), 4))
    add("cell_cos_oblique", coords(rng, 5, 63), cell=cos_cell((30, 40, 50), (80, 100, 60), 5))
    add("cell_degrees", coords(rng, 4, 64), cell=deg_cell((30, 40, 50), (80, 100, 60), 4))
    add("big", coords(rng, 4, 65, True), cell=cos_cell((31, 41, 51), (90, 90, 90), 4), big=True, istart=100, nsavc=10, delta=0.5)
    add("rec64", coords(rng, 4, 63), cell=cos_cell((30, 40, 50), (90, 90, 90), 4), rec64=True)
    add("rec64_big", coords(rng, 4, 9), rec64=True, big=True)
    x = coords(rng, 4, 9)
    add("four", x, cell=cos_cell((30, 40, 50), (90, 90, 90), 4), fourth=rng.standard_normal((4, 9)).astype(np.float32))
    add("xplor", coords(rng, 4, 9), xplor=True, delta=0.25, istart=7, nsavc=3)
    x = with_fixed(coords(rng, 4, 9), [0])
    add("fixed_atom0", x, fixed=[0])
    x = with_fixed(coords(rng, 4, 9), [0, 1, 2, 3, 5, 6, 7, 8])
    add("fixed_all_but_one", x, fixed=[0, 1, 2, 3, 5, 6, 7, 8])
    third = list(range(0, 257, 3))
    x = with_fixed(coords(rng, 5, 257), third)
    add("fixed_third", x, fixed=third, cell=cos_cell((60, 60, 60), (90, 90, 90), 5))
    third = list(range(0, 65, 3))
    x = with_fixed(coords(rng, 4, 65), third)
    add("fixed_third_big", x, fixed=third, big=True)
    add("five_titles", coords(rng, 4, 9), titles=("one", "two", "three", "four", "five"))
    add("no_title", coords(rng, 1, 64), titles=())
    x = coords(rng, 4, 9)
    c["truncated"] = dict(bytes=synth_dcd(x, cell=cos_cell((30, 40, 50), (90, 90, 90), 4))[:-20], xyz=x[:3])
    return c


def refused_big_four():
    """The file this package refuses on purpose: opposite endian with a 4th dimension (the reference misreads it)."""
    rng = np.random.default_rng(SEED + 1)
    return synth_dcd(coords(rng, 4, 9), cell=cos_cell((30, 40, 50), (90, 90, 90), 4), fourth=rng.standard_normal((4, 9)).astype(np.float32),
                     big=True)


def written_cases():
    """name -> dict(xyz, lengths, angles, istart, nsavc, delta): what the reference's ``DCDTrajectoryFile.write`` is given to make the
    reference-written files (cells None: a file without unit cells)."""
    rng = np.random.default_rng(SEED + 2)
    c = {}

    def add(name, F, N, lengths=None, angles=None, special=False, **kw):
        L = None if lengths is None else (np.tile(np.asarray(lengths, np.float32), (F, 1)) * (1 + np.float32(0.01) * np.arange(F, dtype=np.float32))[:, None])
        A = None if angles is None else np.tile(np.asarray(angles, np.float32), (F, 1))
        c[name] = dict(xyz=coords(rng, F, N, special), lengths=L, angles=A, istart=kw.get("istart", 0), nsavc=kw.get("nsavc", 1),
                       delta=kw.get("delta", 1.0))

    add("w_n1_f1", 1, 1, (20, 20, 20), (90, 90, 90))
    add("w_n9_f4", 4, 9, (30, 40, 50), (90, 90, 90), special=True, istart=1000, nsavc=250, delta=0.0409)
    add("w_n63_f5", 5, 63, (30, 40, 50), (80, 100, 60))
    add("w_n64_f4_nocell", 4, 64)
    add("w_n65_f4_zero", 4, 65, (0, 0, 0), (0, 0, 0))
    add("w_n257_f5", 5, 257, (61.5, 62.25, 63.125), (90, 90, 90))
    add("w_n1000_f5", 5, 1000, (99.5, 98.25, 97.125), (90, 90, 90), special=True, istart=5, nsavc=2, delta=2.0)
    return c


def arg_sets(N, F):
    """The ``(stride, atom_indices, frame)`` arguments recorded per case: identity; stride 3 with a reversed permutation; stride 7 (> F)
    with every third atom; one frame with one atom."""
    return [(None, None, None), (3, np.arange(N)[::-1].copy(), None), (7, np.arange(0, N, 3), None), (None, np.array([N // 2]), min(3, F - 1))]


def arg_key(i):
    return "a%d" % i
