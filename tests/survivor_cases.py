"""tests/survivor_cases.py -- TEST INFRASTRUCTURE: the inputs of tests/test_emu_survivor_regs.py and tests/test_gpu_survivor_regs.py.

One batch per (grid, K).  Every item aims at ONE tile, the tile whose first x plane is voxel 8 (tile 1 at K = 8, tile 2 at K = 4, of the
16 x 16 x 8 and the 24 x 16 x 8 grid alike), y and z tile 0.  An item holds `n_in` atoms that survive that tile's cull and `n_far` atoms
of the same cell column that do not (x voxel 0.2 .. 2.4: more than 5.5 voxels below plane 8, yet in a cell the tile has to visit), so
the tile has n_in + n_far candidates and n_in survivors -- the emulated tier reads both numbers back from the kernel (MK_SURV_PROBE) and
tests/test_emu_survivor_regs.py asserts them, which is what lets the GPU tier use the same inputs without guessing a density.

The survivors sit in three bands of x, by the x-reach the tile gives them (ex = x relative to the tile's centre, y and z inside the
tile's square): ex <= -4.9 reaches the lower half of the planes only (xr 1), |ex| <= 4.3 all of them (xr 0), ex >= 4.9 the upper half
(xr 2).  Records are sorted by cell, so a 64-survivor chunk mixes the bands where a cell holds more than one of them.

Sigma rows, by kind (classes by radius; a class is COVERED when every atom that has it below channel 7 has it in channel 7 too):
  one    1.1  in one channel below 7                      (uncovered class: the hydrogens of the synthetic workloads)
  all8   1.1  in all eight channels                       (8 entries, fold on or off: the longest trip count of a lane)
  pair   1.7  in one channel below 7 and in channel 7     (covered: sort_ids clears nibble 7, the id word stays non-zero)
  only7  1.7  in channel 7 only                           (its channel 7 stays)
  all8c  1.52 in all eight channels                       (covered: 7 entries with the fold, 8 without)"""
import numpy as np

GRIDS = {"16x16x8": ([16, 16, 8], [-8.0, -8.0, -4.0]), "24x16x8": ([24, 16, 8], [-12.0, -8.0, -4.0])}
X0 = 8                                                   # first x plane of the tile the items aim at

MIXED = ["one", "pair", "only7", "all8", "one", "all8c", "only7", "pair"]
LEAN = ["one", "one", "only7", "one", "one", "pair", "one", "only7"]          # ~1.1 entries per atom: 520 atoms stay under 640 entries

EVEN, LOW, HIGH = (0.4, 0.3, 0.3), (0.04, 0.96, 0.0), (0.04, 0.0, 0.96)     # shares of the bands xr 0, 1, 2 among an item's survivors

# (n_in, n_far, kinds, band shares, what the target tile must report: candidates, survivors counted by the cull pass, took the list)
ITEMS = [
    (63, 194, MIXED, EVEN, (257, 63, 1)),          # runs.N = 4 * 64 + 1: the list side of the condition, one short chunk
    (63, 193, MIXED, EVEN, (256, 0, 0)),           # runs.N = 4 * 64: the two traversals (the cull pass never runs: no count)
    (64, 200, MIXED, EVEN, (264, 64, 1)),
    (65, 200, MIXED, EVEN, (265, 65, 1)),
    (128, 140, MIXED, EVEN, (268, 128, 1)),
    (129, 140, MIXED, EVEN, (269, 129, 1)),
    (479, 30, LEAN, EVEN, (509, 479, 1)),          # all eight survivor registers of the lower lanes, the bands mixed along the list
    (490, 30, LEAN, EVEN, (520, 490, 0)),          # over SURV_CAP = 480: the two traversals
    (0, 0, MIXED, EVEN, None),                     # an empty item
    (90, 180, None, EVEN, None),                   # an item absent from every channel (all sigmas 0)
    (479, 30, LEAN, LOW, (509, 479, 1)),           # xr 1 from the head of the list to its last register (the list is sorted by cell:
    (479, 30, LEAN, HIGH, (509, 479, 1)),          #   in a mixed item the low band comes first), and xr 2 from its first register on
]
MIXED_479 = 6                                      # the item whose target tile must mix x-reach values in every register


def sigma_rows(kinds, n):
    sig = np.zeros((n, 8), np.float32)
    for i in range(n):
        kind, c = kinds[i % len(kinds)], (i // len(kinds)) % 7
        if kind == "one":
            sig[i, c] = 1.1
        elif kind == "all8":
            sig[i, :] = 1.1
        elif kind == "pair":
            sig[i, c] = 1.7; sig[i, 7] = 1.7
        elif kind == "only7":
            sig[i, 7] = 1.7
        elif kind == "all8c":
            sig[i, :] = 1.52
    return sig


def batch(grid, K, seed=31):
    """-> xyz float32 [n, 3], offsets int64 [B + 1], sigmas float32 [n, 8], origins float64 [B, 3], nvoxels"""
    nv, origin = GRIDS[grid]
    rng = np.random.default_rng(seed)
    hx = 0.5 * (K - 1)
    centre = X0 + hx
    bands = [(-4.3, 4.3), (-hx - 4.6, -4.9), (4.9, hx + 4.6)]           # ex of xr 0, 1, 2
    xyz, sig, sizes = [], [], []
    for n_in, n_far, kinds, shares, _ in ITEMS:
        band = rng.choice(3, size=n_in, p=shares)
        lo, hi = np.array([bands[b][0] for b in band]), np.array([bands[b][1] for b in band])
        vx = np.concatenate([centre + rng.uniform(lo, hi), rng.uniform(0.2, 2.4, size=n_far)])
        v = np.stack([vx, rng.uniform(1.0, 6.0, size=n_in + n_far), rng.uniform(1.0, 6.0, size=n_in + n_far)], axis=1)
        order = rng.permutation(n_in + n_far)
        s = np.zeros((n_in + n_far, 8), np.float32) if kinds is None else sigma_rows(kinds, n_in + n_far)
        xyz.append((v + np.asarray(origin))[order]); sig.append(s[order]); sizes.append(n_in + n_far)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    B = len(sizes)
    return (np.concatenate(xyz).astype(np.float32), offs, np.ascontiguousarray(np.concatenate(sig)), np.tile(np.asarray(origin, np.float64), (B, 1)), nv)
