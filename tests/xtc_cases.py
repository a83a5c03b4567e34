"""tests/xtc_cases.py -- TEST INFRASTRUCTURE: seeded trajectories that drive the XTC decoders into their states, and the
emulated device decoder on a file.

The reference's writer (oracle/xtcref.py) compresses what these return.  What it makes of them is the point: every
generator targets a part of the format this package's own writer never produces -- runs of small atoms, the swap of the
first small atom with the full-precision one, changes of run length, +-1 steps of the small-number index (``smallidx``),
both ends of its table, per-axis bit fields, mixed-radix numbers of 64 and 65 bits.

A generator returns a ``Case``: ``coords`` float32 [F, N, 3] in nm, ``box`` float32 [F, 3, 3], ``precision`` (a scalar or
one per frame), written with ``write(case, path)``."""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", ["name", "coords", "box", "precision"])

XS_WIN_BITS = 1024 * 8          # csrc/xtc_gpu.h: XS_WIN bytes of a lane's window


def _box(F, L):
    b = np.zeros((F, 3, 3), np.float32)
    b[:, 0, 0] = b[:, 1, 1] = b[:, 2, 2] = np.float32(L)
    return b


def _case(name, x, L, precision=1000.0):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return Case(name, x, _box(x.shape[0], L), precision)


def water(rng, nmol=1000, F=2, L=None, precision=1000.0, origin=0.0, name="water"):
    """O-H-H triplets (O-H 0.1 nm, H-O-H ~104.5 deg) at liquid density: runs of two small atoms after each oxygen, the swap
    (O and H1 closer than the run's half-radix), steps of ``smallidx`` where a molecule lies unusually close to the next."""
    L = L or (nmol / 33.4) ** (1.0 / 3.0)
    xs = []
    for _ in range(F):
        o = rng.uniform(0, L, size=(nmol, 3))
        u = rng.normal(size=(nmol, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        v = rng.normal(size=(nmol, 3)); v -= (v * u).sum(1, keepdims=True) * u; v /= np.linalg.norm(v, axis=1, keepdims=True)
        th = np.deg2rad(104.5) / 2
        h1 = o + 0.09572 * (np.cos(th) * u + np.sin(th) * v)
        h2 = o + 0.09572 * (np.cos(th) * u - np.sin(th) * v)
        xs.append(np.stack([o, h1, h2], axis=1).reshape(-1, 3) + origin)
    return _case(name, np.stack(xs), L, precision)


def dense_chain(rng, N=800, F=2, spacing=0.02, precision=1000.0, origin=0.0, name="dense_chain"):
    """A random walk of steps of ``spacing`` nm (0.01-0.05): neighbours closer than the run's radix everywhere -- runs of the
    writer's maximum, 8 small atoms per group (``run < 8*3``)."""
    xs = []
    for _ in range(F):
        st = rng.normal(size=(N, 3)); st *= spacing / np.linalg.norm(st, axis=1, keepdims=True)
        xs.append(np.cumsum(st, axis=0) + origin)
    x = np.stack(xs)
    return _case(name, x, float(np.ptp(x)) + 1.0, precision)


def close_far(rng, N=600, F=2, precision=1000.0, name="close_far"):
    """Close pairs and far jumps in turn (a protein-like stream): the run length and ``smallidx`` change at nearly every
    group, so nearly every group carries a flag -- the one-group step of ``k_xtc_scan``."""
    xs = []
    for _ in range(F):
        p = np.empty((N, 3))
        p[0::2] = rng.uniform(0, 6.0, size=((N + 1) // 2, 3))
        d = rng.normal(size=(N // 2, 3)); d *= rng.uniform(0.05, 0.4, size=(N // 2, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
        p[1::2] = p[0:2 * (N // 2):2] + d
        xs.append(p)
    return _case(name, np.stack(xs), 6.0, precision)


def flag_free_then_edge(rng, N=3000, F=24, precision=1000.0, name="flag_free"):
    """Atoms on a jittered lattice far apart (no runs, no flag after the first groups: the speculative step takes XS_SPEC
    groups at a time over several XS_WIN windows), then close pairs placed one group further per frame around where the
    stream crosses a window edge -- some frame's flag falls right on it."""
    a = 0.6                                                           # lattice constant: no neighbour within a run's radix
    side = int(np.ceil(N ** (1 / 3)))
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3)[:N] * a
    xs = []
    for f in range(F):
        p = g + rng.uniform(-0.01, 0.01, size=g.shape)
        # a group of this stream is ~ triple_bits + 1 bits; put a close partner behind atoms near every window edge
        tb = int(np.ceil(np.log2(float(np.prod(np.ptp(g, axis=0) * precision + 1)))))
        for k in (1, 2, 3, 5):
            i = k * XS_WIN_BITS // (tb + 1) - F // 2 + f
            if 0 < i < N - 1:
                p[i + 1] = p[i] + rng.normal(size=3) * 0.004
        xs.append(p)
    return _case(name, np.stack(xs), side * a, precision)


def smallidx_ends(rng, N=240, precision=(1000.0, 1000.0, 1e5, 10.0, 1000.0), name="smallidx_ends"):
    """Frames whose smallest neighbour step is tiny or huge, in one file: duplicated and 1-quantum neighbours (``smallidx``
    at the table's low end, FIRSTIDX = 9), a dense chain at precision 1e5, a coarse one at precision 10, and far atoms with one
    close pair (the index climbs above 64 in groups without runs -- the top of the table)."""
    F = len(precision)
    x = np.zeros((F, N, 3))
    # frame 0: pairs of identical atoms and 1-quantum neighbours on a walk
    w = np.cumsum(rng.normal(0, 0.3, size=(N // 2, 3)), axis=0)
    x[0, 0::2] = w; x[0, 1::2] = w + rng.integers(0, 2, size=w.shape) * 1e-3
    # frame 1: a dense chain at ~2 quanta per step
    x[1] = np.cumsum(rng.choice([-0.002, 0.0, 0.002], size=(N, 3)), axis=0)
    # frame 2: precision 1e5, steps of 0.1 nm: ~1e4 quanta
    st = rng.normal(size=(N, 3)); st *= 0.1 / np.linalg.norm(st, axis=1, keepdims=True)
    x[2] = np.cumsum(st, axis=0)
    # frame 3: precision 10, steps of 1-3 nm
    x[3] = np.cumsum(rng.uniform(-3, 3, size=(N, 3)), axis=0)
    # frame 4: x alternating between 0 and 9 000 nm (no neighbour within even the table's top radix / 2), one pair 2 400 nm apart
    # on y -- the header index is 64 (the smallest step), each step of 2 400 nm raises it, no run ever comes: 65 and 66
    # without a small atom
    x[4, :, 0] = (np.arange(N) % 2) * 9000.0 + rng.uniform(0, 1, N)
    x[4, :, 1:] = rng.uniform(0, 1, (N, 2))
    x[4, N // 3 + 1] = x[4, N // 3] + np.array([0.0, 2400.0, 0.0])
    return Case(name, x.astype(np.float32), _box(F, 10.0), np.asarray(precision, np.float32))


def precisions(rng, N=300, name="precisions"):
    """Water at precisions 10, 100, 1000, 1e4 and 1e5, one per frame, with a negative origin."""
    prec = np.array([10.0, 100.0, 1000.0, 1e4, 1e5], np.float32)
    c = water(rng, nmol=N // 3, F=len(prec), origin=-37.5)
    return Case(name, c.coords, c.box, prec)


def wide(rng, span, N=90, F=2, precision=1000.0, name="wide"):
    """Water molecules scattered over a box of ``span`` nm per axis (a vector: one axis may exceed 0xffffff quanta -> per-axis
    bit fields; cubes of ~2 100-2 640 nm give 64-bit, ~2 650-3 300 nm 65-bit mixed-radix numbers)."""
    span = np.broadcast_to(np.asarray(span, np.float64), (3,))
    c = water(rng, nmol=N // 3, F=F, L=1.0)
    x = c.coords.astype(np.float64)
    x = x - x.min(axis=1, keepdims=True)
    # spread the molecules (not their atoms) over the span; pin two corners so the ranges are what is asked
    o = x[:, 0::3]
    shift = rng.uniform(0, 1, size=o.shape) * (span - 1.0)
    x = (x.reshape(F, -1, 3, 3) + shift[:, :, None, :]).reshape(F, -1, 3)
    x[:, 0] = 0.0; x[:, -1] = span
    return _case(name, x - span / 2, float(span.max()), precision)


def zigzag(rng=None, N=40, F=2, d=1000.0, name="zigzag"):
    """Atoms alternating between two points ``d`` nm apart per axis, precision 1000: ranges of ~1e6 quanta (triple_bits 60)
    but a smallest neighbour step of 3e6 -- ``smallidx`` 65 in the header and runs coded in 65 bits."""
    x = np.zeros((F, N, 3))
    x[:, 1::2] = d
    if rng is not None:
        x += rng.uniform(0, 1e-3, size=x.shape)
    return _case(name, x, 2 * d, 1000.0)


def few_atoms(rng, N, F=3, name=None):
    """1-11 atoms: plain floats up to 9, compressed from 10 (the raw/compressed boundary)."""
    x = rng.uniform(-2.0, 3.0, size=(F, N, 3))
    return _case(name or f"atoms{N}", x, 5.0, 1000.0)


def named_cases(seed=0, big=False):
    """The fixed cases: every state above at least once, seeded.  ``big``: sizes for the GPU tier (30 000 water atoms)."""
    r = lambda k: np.random.default_rng(seed * 1000 + k)
    out = [
        water(r(1), nmol=10000 if big else 1000, F=64 if big else 3),
        water(r(2), nmol=334, F=1, name="water_one_frame"),
        dense_chain(r(3), N=1200, F=3, spacing=0.01, name="chain_001"),
        dense_chain(r(4), N=1200, F=3, spacing=0.05, origin=-20.0, name="chain_005_neg"),
        close_far(r(5)),
        flag_free_then_edge(r(6)),
        smallidx_ends(r(7)),
        precisions(r(8)),
        wide(r(9), [20000.0, 3.0, 3.0], name="per_axis_x"),
        wide(r(10), 2300.0, name="triple64"),
        wide(r(11), 3000.0, name="triple65"),
        zigzag(),
    ]
    out += [few_atoms(r(20 + n), n) for n in (1, 2, 3, 9, 10, 11)]
    return out


def random_case(rng, i):
    """One small file of the sweep: a generator and its knobs drawn at random.  (The smallest neighbour step of a frame stays
    below the table's last entry, 2^24 quanta: beyond it the reference's writer puts an index of 73 into the header, which its
    own reader refuses -- the zig-zag frames of a mixture, which may be written at precision 1e5, are at most 50 nm wide.)"""
    kind = int(rng.integers(0, 7))
    F = int(rng.integers(1, 5))
    prec = float(rng.choice([10.0, 100.0, 1000.0, 1e4, 1e5]))
    name = f"sweep{i}"
    if kind == 0:
        return water(rng, nmol=int(rng.integers(4, 120)), F=F, precision=prec, origin=float(rng.uniform(-50, 50)), name=name)
    if kind == 1:
        return dense_chain(rng, N=int(rng.integers(10, 400)), F=F, spacing=float(rng.uniform(0.005, 0.06)), precision=prec,
                           origin=float(rng.uniform(-50, 50)), name=name)
    if kind == 2:
        return close_far(rng, N=int(rng.integers(10, 300)), F=F, precision=prec, name=name)
    if kind == 3:
        return few_atoms(rng, int(rng.integers(1, 14)), F=F, name=name)
    if kind == 4:
        return zigzag(rng, N=int(rng.integers(10, 60)), F=F, d=float(rng.choice([0.5, 30.0, 400.0, 1000.0])), name=name)
    if kind == 5:
        return wide(rng, rng.uniform(1, 4000, size=3) * (rng.random(3) < 0.5) + 2.0, N=3 * int(rng.integers(4, 40)), F=F, name=name)
    # a mixture: frames of different generators and precisions, one atom count
    N = 3 * int(rng.integers(4, 80))
    parts = [water(rng, nmol=N // 3, F=1).coords[0], dense_chain(rng, N=N, F=1, spacing=0.01).coords[0],
             close_far(rng, N=N, F=1).coords[0], zigzag(rng, N=N, F=1, d=float(rng.uniform(1, 50))).coords[0]]
    pick = rng.integers(0, len(parts), size=F)
    x = np.stack([parts[k] for k in pick])
    return Case(name, x, _box(F, 5.0), rng.choice([10.0, 100.0, 1000.0, 1e4, 1e5], size=F).astype(np.float32))


def write(case, path):
    from oracle.xtcref import ref_write_xtc
    ref_write_xtc(path, case.coords, case.box, precision=case.precision)
    return str(path)


# ------------------------------------------------------------------------------------------------
# the device decoder's two kernels, emulated on the host (tests/emu), on a file
# ------------------------------------------------------------------------------------------------
def device_decode_emulated(fn, sel=None, scale=1.0, groups=False):
    """The host half of the device decoder (headers, record bytes: libmkamd.so, no GPU involved) + the two kernels of
    csrc/xtc_gpu.h run by the host SIMT emulation (tests/emu): -> (xyz [n, natoms, 3], status [n], desc) and, with ``groups``,
    the walk's records and counts (``emu_build.xtc_decode``)."""
    from moleculekit_amd import _lib, xtc
    from tests import emu_build
    na, nf = xtc.get_xtc_natoms(fn), xtc.get_xtc_nframes(fn)
    sel = np.arange(nf, dtype=np.int64) if sel is None else np.asarray(sel, dtype=np.int64)
    desc, lo, hi, box, t, st = xtc.chunk_desc(fn, sel, na)
    raw = np.zeros(hi - lo + xtc.XTC_PAD, np.uint8)
    _lib._check(_lib.load().mkamd_xtc_copy_bytes(xtc._path(fn), lo, hi, raw.ctypes.data_as(ctypes.c_void_p), 1))
    assert np.array_equal(raw[:hi - lo], np.fromfile(fn, np.uint8, count=hi - lo, offset=lo))
    out = emu_build.xtc_decode(raw, desc, na, scale, groups=groups)
    return out[:2] + (desc,) + out[2:]


def reach(grp, ngrp, status, desc):
    """What the walk reached in the frames it decoded (status 0), from its group records: the most small atoms in a group, the
    lowest and highest ``smallidx`` of a group, the groups whose flag was set, and the runs whose bits cross a window refill."""
    from moleculekit_amd import xtc
    d = np.ascontiguousarray(desc).view(xtc.DESC_DTYPE).reshape(-1)
    r = {"max_small": 0, "idx_lo": None, "idx_hi": None, "flagged": 0, "run_across_refill": 0}
    for f in range(len(status)):
        n = int(ngrp[f])
        if status[f] != 0 or n == 0:
            continue
        pos = grp[f, :n, 0].astype(np.int64)
        what = grp[f, :n, 1].astype(np.int64)
        sidx, ns = (what >> 21) & 127, what >> 28
        r["max_small"] = max(r["max_small"], int(ns.max()))
        r["idx_lo"] = int(sidx.min()) if r["idx_lo"] is None else min(r["idx_lo"], int(sidx.min()))
        r["idx_hi"] = int(sidx.max()) if r["idx_hi"] is None else max(r["idx_hi"], int(sidx.max()))
        full = int(d["triple_bits"][f]) or int(d["field_bits"][f].sum())
        # a flagged group has 5 run bits behind its flag: the next group starts 5 bits later than behind an unflagged one
        r["flagged"] += int(np.count_nonzero(pos[1:] - (pos[:-1] + full + 1 + ns[:-1] * sidx[:-1]) == 5))
        # the windows the walk used: one starts at the word of the first group that did not fit the previous one
        wbit = (int(pos[0]) >> 5) << 5
        for k in range(n):
            if int(pos[k]) - wbit + full + 6 > XS_WIN_BITS:
                wbit = (int(pos[k]) >> 5) << 5
            if ns[k] and k + 1 < n and int(pos[k + 1]) > wbit + XS_WIN_BITS:
                r["run_across_refill"] += 1
    return r
