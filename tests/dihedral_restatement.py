"""tests/dihedral_restatement.py -- TEST INFRASTRUCTURE: numpy restatement of the reference's dihedral projection
(dihedral.py:dihedralAngle, projections/metricdihedral.py:_calcDihedralAngles) and the "truth of the terms" the accuracy condition
of DESIGN.md section 11 is stated against.  The arithmetic is the reference's: float32 throughout the terms, numpy's cross and
axis-0 sums, `** 0.5` for the root, float32 arctan2; rad2deg as numpy does it on the float32 angle, stored into a float64 array;
sin / cos of `metric * pi / 180` in float64; astype(float32)."""
from __future__ import annotations

import numpy as np

F32 = np.float32


def _wrap(pos, box):
    hbox = box / 2
    under = pos < -hbox
    over = pos > hbox
    pos[under] += box[under]
    pos[over] -= box[over]
    return pos


def terms_one(pos, box=None):
    """pos float32 [4, 3, F] -> (p1, p2) float32 [F]"""
    r12 = pos[0] - pos[1]
    r23 = pos[1] - pos[2]
    r34 = pos[2] - pos[3]
    if box is not None and not np.all(box == 0):
        r12 = _wrap(r12, box)
        r23 = _wrap(r23, box)
        r34 = _wrap(r34, box)
    c1 = np.cross(r23, r34, axisa=0, axisb=0, axisc=0)
    c2 = np.cross(r12, r23, axisa=0, axisb=0, axisc=0)
    p1 = (r12 * c1).sum(axis=0)
    p1 *= (r23 * r23).sum(axis=0) ** 0.5
    p2 = (c1 * c2).sum(axis=0)
    assert p1.dtype == F32 and p2.dtype == F32
    return p1, p2


def terms(coords, quads, box=None):
    """coords float32 [N, 3, F], quads [D, 4] -> float32 [F, D, 2]"""
    coords = np.asarray(coords, F32)
    quads = np.asarray(quads, np.int64).reshape(-1, 4)
    out = np.empty((coords.shape[2], quads.shape[0], 2), F32)
    with np.errstate(all="ignore"):
        for i, q in enumerate(quads):
            out[:, i, 0], out[:, i, 1] = terms_one(coords[q, :, :], None if box is None else np.asarray(box, F32))
    return out


def project(t, sincos=True):
    """_calcDihedralAngles from the terms [F, D, 2]: float32 [F, 2 D] (sin, cos interleaved) or [F, D] degrees"""
    with np.errstate(all="ignore"):
        metric = np.zeros(t.shape[:2])
        for i in range(t.shape[1]):
            metric[:, i] = np.rad2deg(-np.arctan2(t[:, i, 0], t[:, i, 1]))
        if sincos:
            sc = np.zeros((metric.shape[0], metric.shape[1] * 2))
            sc[:, 0::2] = np.sin(metric * np.pi / 180.0)
            sc[:, 1::2] = np.cos(metric * np.pi / 180.0)
            metric = sc
        return metric.astype(F32)


def radians(t):
    """dihedralAngle's own return value: float32 [F, D]"""
    with np.errstate(all="ignore"):
        return -np.arctan2(t[..., 0], t[..., 1])


def truth(t):
    """the exact function of the float32 terms, in float64: (radians [F, D], degrees [F, D], sincos [F, 2 D])"""
    with np.errstate(all="ignore"):
        a = -np.arctan2(t[..., 0].astype(np.float64), t[..., 1].astype(np.float64))
        sc = np.empty((a.shape[0], 2 * a.shape[1]))
        sc[:, 0::2] = np.sin(a)
        sc[:, 1::2] = np.cos(a)
        return a, np.rad2deg(a), sc


def worst(got, want):
    """largest absolute difference over the positions where the truth is a number (NaN positions are compared separately)"""
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok].astype(np.float64) - want[ok]))) if ok.any() else 0.0
