"""tests/hbonds_restatement.py -- TEST INFRASTRUCTURE: a numpy float32 restatement of the reference's hydrogen-bond loop
(moleculekit interactions/hbonds/hbonds.pyx: `calculate`), as its generated C++ computes it.

Every float32 operation of the loop is one numpy float32 operation here, in the loop's order:
  thresholds   thr_d2 = float32(dist) * float32(dist); thr_ang = float32(float64(float32(angle)) / 57.29578)
  pair test    acceptor == donor heavy atom: skipped; then the selections, ALWAYS of the donor's heavy atom: intra sel1[a] != 0 and
               sel1[d] != 0; otherwise (sel1[a] == 1 and sel2[d] == 1) or (sel2[a] == 1 and sel1[d] == 1)
  wrapped vec  val = c[a] - c[d]; where |val| > box / 2 and box != 0: val - box * roundf(val / box), all float32; d2 a sum from 0
  distance     skipped where d2_a > thr_d2 (a NaN passes); ignore_hs: reported here as (heavy, -1, acceptor)
  angle        second vector c[heavy] - c[hydrogen], wrapped; skipped where d2_a == 0 or d2_b == 0; dot a sum from 0 of rounded products;
               ratio = float32(float64(dot) / float64(float32(sqrtf(d2_a) * sqrtf(d2_b)))), clamped to [-1, 1] (a NaN passes both clamps);
               reported where acosf(ratio) > thr_ang, a float32 comparison
`acosf` is the C library's float32 one, restated in tests/rings_restatement.py.  Vectorised over the frames and the acceptors; the lists
come out frame by frame, donors outer, acceptors inner.
"""
from __future__ import annotations

import numpy as np

from rings_restatement import _c_round, acosf

F32, F64 = np.float32, np.float64


def wrapped_vec(p1, p2, box):
    """p1 - p2 per axis, wrapped as the reference wraps it.  p1, p2 float32 [..., 3, F]; box float32 [3, F] -> (vec [..., 3, F], d2 [..., F])"""
    shape = np.broadcast_shapes(p1.shape, p2.shape)
    vec = np.zeros(shape, F32)
    d2 = np.zeros(shape[:-2] + shape[-1:], F32)
    with np.errstate(all="ignore"):
        for ax in range(3):
            val = (p1[..., ax, :] - p2[..., ax, :]).astype(F32)
            b = np.broadcast_to(box[ax], val.shape)
            half = (b / F32(2)).astype(F32)
            wrap = (np.abs(val) > half) & (b != 0)
            q = (val / b).astype(F32)
            w = (val - (b * _c_round(q)).astype(F32)).astype(F32)
            val = np.where(wrap, w, val)
            vec[..., ax, :] = val
            d2 = (d2 + (val * val).astype(F32)).astype(F32)
    return vec, d2


def thresholds(dist_threshold, angle_threshold):
    d = F32(dist_threshold)
    return F32(d * d), F32(F64(F32(angle_threshold)) / 57.29578)


def allowed_pairs(donors, acceptors, sel1, sel2, intra):
    """[nd, na] bool: the pairs the loop goes on to measure"""
    heavy = donors[:, 0].astype(np.int64)
    acc = acceptors.astype(np.int64)
    ok = heavy[:, None] != acc[None, :]
    if intra:
        return ok & (sel1[acc] != 0)[None, :] & (sel1[heavy] != 0)[:, None]
    a1, a2, d1, d2 = sel1[acc] == 1, sel2[acc] == 1, sel1[heavy] == 1, sel2[heavy] == 1
    return ok & ((a1[None, :] & d2[:, None]) | (a2[None, :] & d1[:, None]))


def calculate(donors, acceptors, coords, box, sel1, sel2, dist_threshold=2.5, angle_threshold=120, intra=False, ignore_hs=False, details=False):
    """The reference's `calculate`.  donors uint32 [nd, 2] ([nd, 1] with ignore_hs), acceptors uint32 [na], coords float32 [N, 3, F], box
    float32 [3, F] (None: zeros), sel1 / sel2 uint32 [N] -> (frame_offsets int64 [F + 1], triples int32 [n, 3]); with `details` also
    (tested [nd, na, F]: the pairs that reached the angle, angle64 [nd, na, F]: their float64 angles in degrees)."""
    coords = np.ascontiguousarray(coords, F32)
    F = coords.shape[2]
    box = np.zeros((3, F), F32) if box is None else np.ascontiguousarray(box, F32)
    donors = np.asarray(donors, np.uint32).reshape(len(donors), -1)
    acceptors = np.asarray(acceptors, np.uint32).reshape(-1)
    sel1 = np.asarray(sel1, np.uint32)
    sel2 = sel1 if sel2 is None else np.asarray(sel2, np.uint32)
    nd, na = len(donors), len(acceptors)
    thr_d2, thr_ang = thresholds(dist_threshold, angle_threshold)
    hit = np.zeros((nd, na, F), bool)
    tested = np.zeros((nd, na, F), bool)
    angle64 = np.full((nd, na, F), np.nan)
    if nd and na and F:
        allowed = allowed_pairs(donors, acceptors, sel1, sel2, intra)
        pa = coords[acceptors]                                         # [na, 3, F]
        with np.errstate(all="ignore"):
            for d in range(nd):
                heavy = donors[d, 0]
                ref = heavy if ignore_hs else donors[d, 1]
                va, d2a = wrapped_vec(pa, coords[ref][None], box)     # [na, 3, F], [na, F]
                near = allowed[d][:, None] & ~(d2a > thr_d2)
                if ignore_hs:
                    hit[d] = near
                    continue
                vb, d2b = wrapped_vec(coords[heavy][None], coords[ref][None], box)   # [1, 3, F], [1, F]
                go = near & ~((d2a == 0) | (d2b == 0))
                dot = np.zeros((na, F), F32)
                for ax in range(3):
                    dot = (dot + (va[:, ax] * vb[:, ax]).astype(F32)).astype(F32)
                den = (np.sqrt(d2a) * np.sqrt(d2b)).astype(F32)
                ratio = (dot.astype(F64) / den.astype(F64)).astype(F32)
                ratio = np.where(ratio > 1, F32(1), ratio)
                ratio = np.where(ratio < -1, F32(-1), ratio).astype(F32)
                hit[d] = go & (acosf(ratio).reshape(na, F) > thr_ang)
                tested[d] = go
                va64, vb64 = va.astype(F64), vb.astype(F64)
                c = (va64 * vb64).sum(axis=1) / np.sqrt((va64 * va64).sum(axis=1) * (vb64 * vb64).sum(axis=1))
                angle64[d] = np.degrees(np.arccos(np.clip(c, -1, 1)))
    offs = np.zeros(F + 1, np.int64)
    rows = []
    for f in range(F):
        i, j = np.nonzero(hit[:, :, f])
        offs[f + 1] = offs[f] + i.size
        hyd = np.full(i.size, -1, np.int64) if ignore_hs else donors[i, 1].astype(np.int64)
        rows.append(np.stack([donors[i, 0].astype(np.int64), hyd, acceptors[j].astype(np.int64)], axis=1))
    triples = (np.concatenate(rows) if rows else np.zeros((0, 3), np.int64)).reshape(-1, 3).astype(np.int32)
    return (offs, triples, tested, angle64) if details else (offs, triples)


def threshold_margin(angle_threshold, tested, angle64):
    """the smallest |angle - threshold| over the pairs that reached the angle (float64 degrees; inf: no such pair)"""
    a = angle64[tested & ~np.isnan(angle64)]
    return float(np.min(np.abs(a - F64(F32(angle_threshold))))) if a.size else np.inf
