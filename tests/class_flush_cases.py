"""tests/class_flush_cases.py -- TEST INFRASTRUCTURE: the inputs of tests/test_emu_class_flush.py and tests/test_gpu_class_flush.py.

One batch per (grid, K): 16 x 16 x 8 at K = 8 and 8 x 16 x 16 at K = 4, voxel size 1, the origin a whole number, so voxel i's centre
sits at origin + i and whole-number coordinates are voxel centres.  One item per case of the class flush (round 11):
the cutoff applied to a class minimum as a masked minimum, a fast and an exact body under one scalar branch.

  at5      two lone atoms, 1.75 A (a class of their own, not in channel 7: 1.7 A stays covered for the items below).  A (channel 0) sits ON a voxel centre: every voxel at offset (+-3, +-4, 0), (+-4, +-3, 0), (0, +-3, +-4) ...
           is at d^2 = 25 exactly -- whole and half numbers, exact in float32 in the expanded form too -- and must stay OUT (the
           reference tests d^2 < 25): channel 0 is exactly 0.0f there.  B (channel 1) sits 1e-3 nearer: (3 - 1e-3, 4, 0) from a voxel
           centre, d^2 = 24.994, and must come IN: 1 - exp(-(1.75 / 4.9994)^12) = 3.4e-6, not zero.
  centre   an atom exactly on a voxel centre, in channels 3 and 7: d^2 rounds to +-1e-7 in the fast form, |d2| * w, occupancy 1.0f
  mixed    a fast class (1.7 A) and an exact class (w = 1 / sigma^2 above fast_w_max = 14 / c_max^2: 0.5 A, w = 4 against 1.14 at K = 8;
           0.35 A, w = 8.2 against 6.2 at K = 4) in the SAME channel (2), the fast ones in channel 7 as well (covered: folded)
  single   one atom in one channel: a one-entry group (an odd tail, no pair trip)
  half     a group whose entries all reach the LOWER half of the target tile's planes only (x-reach 1, as tests/survivor_cases.py
           places them): the upper planes' minima are still +inf when the group is flushed
  gap      atoms in channels 0, 1, 2 and 7; channels 3..6 hold nothing: an empty channel between full ones
  absent   an item absent from every channel (all sigmas 0)"""
import numpy as np

GRIDS = {8: ([16, 16, 8], [-8.0, -8.0, -4.0]), 4: ([8, 16, 16], [-4.0, -8.0, -8.0])}      # by K
EXACT_SIGMA = {8: 0.5, 4: 0.35}                         # w = 1 / sigma^2 above fast_w_max<K>
ITEMS = ["at5", "centre", "mixed", "single", "half", "gap", "absent"]
A_VOXEL = {8: (6, 6, 4), 4: (3, 6, 6)}                  # the voxel atom A of `at5` sits on
B_VOXEL = {8: (9, 8, 3), 4: (4, 8, 9)}                  # B is (3 - 1e-3, 4, 0) (K = 8) / (0, 4, 3 - 1e-3) (K = 4) away from this voxel's centre
CENTRE_VOXEL = {8: (5, 10, 5), 4: (5, 10, 5)}


def batch(K, seed=41):
    """-> xyz float32 [n, 3], offsets int64 [B + 1], sigmas float32 [n, 8], origins float64 [B, 3], nvoxels"""
    nv, origin = GRIDS[K]
    origin = np.asarray(origin, np.float64)
    rng = np.random.default_rng(seed)
    items = []

    def inside(n):
        return rng.uniform([0.5, 0.5, 0.5], np.asarray(nv) - 1.5, size=(n, 3))

    # at5
    a = np.asarray(A_VOXEL[K], np.float64)
    off = np.array([3.0 - 1e-3, 4.0, 0.0]) if K == 8 else np.array([0.0, 4.0, 3.0 - 1e-3])
    b = np.asarray(B_VOXEL[K], np.float64) + off
    s = np.zeros((2, 8), np.float32); s[0, 0] = 1.75; s[1, 1] = 1.75
    items.append((np.stack([a, b]), s))
    # centre
    s = np.zeros((1, 8), np.float32); s[0, 3] = 1.7; s[0, 7] = 1.7
    items.append((np.asarray([CENTRE_VOXEL[K]], np.float64), s))
    # mixed
    n = 40
    s = np.zeros((n, 8), np.float32)
    s[: n // 2, 2] = 1.7; s[: n // 2, 7] = 1.7
    s[n // 2:, 2] = EXACT_SIGMA[K]
    items.append((inside(n), s))
    # single
    s = np.zeros((1, 8), np.float32); s[0, 5] = 1.52
    items.append((inside(1), s))
    # half: ex = x - (centre of the tile whose first plane is voxel K) in (-hx - 4.6, -4.9), y and z inside the tile's square
    n = 12
    hx = 0.5 * (K - 1)
    v = np.stack([K + hx + rng.uniform(-hx - 4.6, -4.9, size=n), rng.uniform(1.0, 6.0, size=n), rng.uniform(1.0, 6.0, size=n)], axis=1)
    s = np.zeros((n, 8), np.float32); s[:, 1] = 1.55
    items.append((v, s))
    # gap
    n = 30
    s = np.zeros((n, 8), np.float32)
    s[:, 0] = 1.1; s[::2, 1] = 1.7; s[::3, 2] = 1.8; s[::2, 7] = 1.7
    items.append((inside(n), s))
    # absent
    items.append((inside(9), np.zeros((9, 8), np.float32)))

    assert len(items) == len(ITEMS)
    xyz = np.concatenate([v + origin for v, _ in items]).astype(np.float32)
    sig = np.ascontiguousarray(np.concatenate([s for _, s in items]))
    offs = np.concatenate([[0], np.cumsum([len(v) for v, _ in items])]).astype(np.int64)
    return xyz, offs, sig, np.tile(origin, (len(items), 1)), nv


def voxel_index(nv, v):
    return (v[0] * nv[1] + v[1]) * nv[2] + v[2]


def at_exactly_five(K):
    """flat indices of the voxels whose centre is at d^2 == 25 from atom A of `at5` (whole numbers: exact)"""
    nv, _ = GRIDS[K]
    g = np.stack(np.meshgrid(*[np.arange(n) for n in nv], indexing="ij"), axis=-1).reshape(-1, 3)
    d2 = ((g - np.asarray(A_VOXEL[K])) ** 2).sum(axis=1)
    return np.nonzero(d2 == 25)[0]


def check_values(out, K):
    """what every path's features of batch(K) must show, beyond agreeing with each other (out: numpy [B, V, 8])"""
    nv, _ = GRIDS[K]
    I = {name: i for i, name in enumerate(ITEMS)}
    ring = at_exactly_five(K)
    assert len(ring) >= 4
    assert not out[I["at5"]][ring, 0].any(), "a voxel at exactly 5 A took the atom in"
    assert out[I["at5"]][voxel_index(nv, A_VOXEL[K]), 0] == 1.0
    vb = out[I["at5"]][voxel_index(nv, B_VOXEL[K]), 1]
    assert 3e-6 < vb < 4e-6, vb                                      # 3.4e-6: in, by 1e-3 A
    c = voxel_index(nv, CENTRE_VOXEL[K])
    assert out[I["centre"]][c, 3] == 1.0 and out[I["centre"]][c, 7] == 1.0
    assert not out[I["centre"]][:, [0, 1, 2, 4, 5, 6]].any()
    mixed = out[I["mixed"]]
    assert mixed[:, 2].max() > 0.5 and mixed[:, 7].max() > 0.5 and (mixed[:, 2] >= mixed[:, 7]).all()
    assert out[I["single"]][:, 5].max() > 0.1 and not out[I["single"]][:, :5].any()
    assert out[I["half"]][:, 1].max() > 0.1
    gap = out[I["gap"]]
    assert not gap[:, 3:7].any() and gap[:, 0].max() > 0.5 and gap[:, 7].max() > 0.5
    assert not out[I["absent"]].any()
