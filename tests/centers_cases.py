"""tests/centers_cases.py -- TEST INFRASTRUCTURE: the cases of the explicit-centre occupancy path (k_occupancy_centers behind
run_centers, csrc/pipeline.h) that the CPU tier (emulated kernel, tests/test_emu_centers.py) and the GPU tier
(tests/test_gpu_centers.py) share.

Builders only, seeded; neither the product nor the emulator is imported here.  A case is ``centers`` float64 [V, 3], ``coords``
float32 [N, 3], ``sigmas`` [N, C] (float64 unless said otherwise) and ``box`` (3 edges, or None).  The expected values are the
oracle's, computed by the tests.

The constants restate run_centers' launch rule: a workgroup owns 64 centres and is 4 waves wide, doubled (8, 16) while
``ceil(V / 64) * ceil(C / 8) * waves < 4096``.
"""
from __future__ import annotations

import functools
from collections import namedtuple
from fractions import Fraction

import numpy as np

Case = namedtuple("Case", "centers coords sigmas box")

CENTRES_PER_BLOCK = 64       # EXPL_CENTERS
CHANNEL_GROUP = 8            # CHG
FILL = 4096                  # waves the launch wants in flight before it stops widening the workgroup
MAX_CHANNELS = 65535 * CHANNEL_GROUP     # the grid's y limit: more channels are refused

SIGMA_POOL = (0.0, 1.1, 1.7, 2.0, 3.5)


def waves_for(V, C):
    """The workgroup width run_centers picks, restated."""
    wgs = -(-V // CENTRES_PER_BLOCK) * -(-C // CHANNEL_GROUP)
    waves = 4
    while waves < 16 and wgs * waves < FILL:
        waves *= 2
    return waves


THRESHOLDS = {1: [(32704, 16), (32705, 8), (65472, 8), (65473, 4)],       # the rule's thresholds, written out: (V, waves)
              2: [(16320, 16), (16321, 8), (32704, 8), (32705, 4)]}


def threshold_sizes(G):
    """Centre counts on each side of both thresholds of the rule for G channel groups -> [(V, waves)]:
    G = 1: 32 704 | 32 705 (16 | 8 waves) and 65 472 | 65 473 (8 | 4 waves); G = 2: half the blocks, 16 320 | 16 321 and
    32 704 | 32 705.  Both tiers take their inputs AND their expectations from here, so the literal table pins it."""
    out = []
    for waves in (16, 8):
        blocks = -(-FILL // (G * (waves // 2))) - 1          # the most blocks at which a workgroup of waves / 2 still doubles
        out += [(blocks * CENTRES_PER_BLOCK, waves), (blocks * CENTRES_PER_BLOCK + 1, waves // 2)]
    assert out == THRESHOLDS[G], (G, out)
    return out


# ---- every block size: one atom set, one long centre list, used whole and as prefixes ------------------------------------------
BLOCK_ATOMS = 1100           # five chunks of atoms at 4 waves, three at 8, two at 16 -- the last one ragged in each
BLOCK_ROWS = {3: 70016, 9: 35008}


def block_prefixes(C):
    """[(rows, waves)]: the whole list (4 waves), then the prefixes that run at 8 and at 16 waves."""
    half = 1 if C <= CHANNEL_GROUP else 2
    return [(BLOCK_ROWS[C], 4), (40000 // half, 8), (1000 // half, 16)]


@functools.lru_cache(maxsize=None)
def block_case(C):
    assert C in BLOCK_ROWS
    rng = np.random.default_rng(7000 + C)
    coords = rng.uniform(-9.0, 9.0, (BLOCK_ATOMS, 3)).astype(np.float32)
    centers = rng.uniform(-12.0, 12.0, (BLOCK_ROWS[C], 3))
    sigmas = rng.choice(SIGMA_POOL, (BLOCK_ATOMS, C))
    for rows, waves in block_prefixes(C):
        assert waves_for(rows, C) == waves, (rows, C)
    for a in (centers, coords, sigmas):
        a.setflags(write=False)
    return Case(centers, coords, sigmas, None)


# ---- sizes around the chunk, block and channel-group boundaries -------------------------------------------------------------
SHAPE_N = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
SHAPE_V = (1, 64, 65)
SHAPE_C = (1, 7, 8, 9, 16, 17, 24)


def shape_case(N, V, C):
    rng = np.random.default_rng([N, V, C])
    coords = rng.uniform(-6.0, 6.0, (N, 3)).astype(np.float32)
    centers = rng.uniform(-8.0, 8.0, (V, 3))
    return Case(centers, coords, rng.choice(SIGMA_POOL, (N, C)), None)


def shape_cases():
    for C in SHAPE_C:
        for N in SHAPE_N:
            for V in SHAPE_V:
                yield (N, V, C), shape_case(N, V, C)


# ---- the strict cut-off ------------------------------------------------------------------------------------------------------
def _exact_d2(centre):
    return sum(Fraction(float(x)) ** 2 for x in centre)


def _rounded_d2(centre):
    """d^2 from the origin the reference's way: every product and every sum rounded to double, left to right."""
    x, y, z = (float(v) for v in centre)
    return x * x + y * y + z * z


def cutoff_case():
    """One atom at the origin, sigmas (3.5, 4.0).  -> (case, where): rows 0 .. 2 sit ON the 5 A shell, (3, 4, 0), (0, 0, 5) and
    (5, 0, 0), where d^2 = 25 exactly however it is summed; then, for every non-zero coordinate of each of them, that row with
    the coordinate one double ulp nearer to the atom and one ulp farther.  `where` is "on" / "in" / "out" per row: d^2 summed
    with one rounding per operation (the reference's arithmetic) against 25 -- the tests hold the oracle to it too.

    Row (3 - 1 ulp, 4, 0) is the one that tells a contracted sum from the reference's: its exact d^2 is 3/4 ulp below 25, the
    square of its x rounds to 9 - 2^-49, and 16 + 9 - 2^-49 is a tie that rounds to 25: ON the shell, zero.  A kernel that
    rounds x*x + 16 once (a fused multiply-add) gets 25 - 2^-48 and answers 1.4e-2 and 6.6e-2 there."""
    on = np.array([[3.0, 4.0, 0.0], [0.0, 0.0, 5.0], [5.0, 0.0, 0.0]])
    rows = list(on)
    for base in on:
        for k in np.flatnonzero(base):
            for towards in (0.0, np.inf):
                row = base.copy()
                row[k] = np.nextafter(base[k], towards)
                rows.append(row)
    centers = np.array(rows)
    where = []
    for row in centers:
        d2 = _rounded_d2(row)
        where.append("in" if d2 < 25.0 else "on" if d2 == 25.0 else "out")
    assert where[:3] == ["on"] * 3 and all(_exact_d2(row) == 25 for row in on)
    assert where.count("in") == 3 and where.count("out") == 4
    tie = centers[3]                                  # (3 - 1 ulp, 4, 0)
    assert tie[0] == np.nextafter(3.0, 0.0) and tie[1] == 4.0 and where[3] == "on" and _exact_d2(tie) < 25
    coords = np.zeros((1, 3), np.float32)
    sigmas = np.array([[3.5, 4.0]])
    return Case(centers, coords, sigmas, None), where


# ---- sigmas that are no radii ------------------------------------------------------------------------------------------------
SPECIAL_SIGMAS = (0.0, -1.7, np.nan, np.inf, -np.inf, 1e-30, 1e-160, 1e30, 1e200, 2.0)


def special_case(dtype=np.float64):
    """9 channels of sigmas drawn from SPECIAL_SIGMAS (every one of them in every channel's first rows), as float64 or cast to
    float32 (1e-160 becomes 0, 1e200 +inf); the first 70 centres lie exactly ON atoms (d = 0), the rest are random."""
    rng = np.random.default_rng(7100)
    N, C, V = 150, 9, 200
    coords = rng.uniform(-5.0, 5.0, (N, 3)).astype(np.float32)
    sigmas = rng.choice(SPECIAL_SIGMAS, (N, C))
    for c in range(C):
        sigmas[:len(SPECIAL_SIGMAS), c] = np.roll(SPECIAL_SIGMAS, c)
    centers = rng.uniform(-7.0, 7.0, (V, 3))
    centers[:70] = coords[:70].astype(np.float64)
    with np.errstate(over="ignore", under="ignore"):
        sigmas = sigmas.astype(dtype)
    return Case(centers, coords, sigmas, None)


def nonfinite_case():
    """A NaN and an inf among the coordinates and among the centres: such pairs are never inside the cut-off."""
    rng = np.random.default_rng(7200)
    N, C, V = 130, 3, 100
    coords = rng.uniform(-5.0, 5.0, (N, 3)).astype(np.float32)
    coords[5] = [np.nan, 0.0, 1.0]
    coords[66] = [0.5, np.inf, -1.0]
    coords[129] = [-np.inf, np.nan, 3.0e38]
    centers = rng.uniform(-6.0, 6.0, (V, 3))
    centers[3] = [0.0, np.nan, 0.0]
    centers[64] = [np.inf, 1.0, 1.0]
    centers[99] = [-np.inf, np.inf, 0.0]
    return Case(centers, coords, rng.choice(SIGMA_POOL, (N, C)), None)


def far_case():
    """Everything 1e6 A from the origin (float32 coordinates are 1/16 A apart there): the differences are taken in double."""
    rng = np.random.default_rng(7300)
    N, C, V = 300, 8, 150
    coords = (1.0e6 + rng.uniform(-6.0, 6.0, (N, 3))).astype(np.float32)
    centers = 1.0e6 + rng.uniform(-7.0, 7.0, (V, 3))
    return Case(centers, coords, rng.choice(SIGMA_POOL, (N, C)), None)


def periodic_case():
    """A small box with the atoms up to 40 and the centres up to 20 box lengths away: many images."""
    rng = np.random.default_rng(7400)
    N, C, V = 700, 8, 400
    coords = rng.uniform(-200.0, 200.0, (N, 3)).astype(np.float32)
    centers = rng.uniform(-100.0, 100.0, (V, 3))
    return Case(centers, coords, rng.choice(SIGMA_POOL, (N, C)).astype(np.float32), np.array([10.5, 23.0, 11.25]))


def jitter_case():
    """A getCenters-like lattice moved off its points (no lattice: the pairwise route of calculate_occupancy) and a `results`
    array pre-filled with 0, 0.5, 2.0, -1.0 and NaN."""
    rng = np.random.default_rng(7500)
    n = 11
    g = np.arange(n) * 1.0 - 5.0
    centers = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + rng.normal(0.0, 1e-3, (n ** 3, 3))
    coords = rng.uniform(-6.0, 6.0, (260, 3)).astype(np.float32)
    sigmas = rng.choice(SIGMA_POOL, (260, 5))
    pre = rng.choice([0.0, 0.5, 2.0, -1.0, np.nan], (n ** 3, 5))
    return Case(np.ascontiguousarray(centers), coords, sigmas, None), pre


def in_place_max(values, old):
    """`value > old ? value : old` (occupancy_utils.pyx:61): a NaN in `old` stays."""
    with np.errstate(invalid="ignore"):
        return np.where(values > old, values, old)
