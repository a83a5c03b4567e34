"""tests/rings_restatement.py -- TEST INFRASTRUCTURE: a numpy float32 restatement of the reference's three ring-interaction loops
(moleculekit interactions/pipi/pipi.pyx, cationpi/cationpi.pyx, sigmahole/sigmahole.pyx: `calculate`).

Every float32 operation of the loops is one numpy float32 operation here (numpy rounds each on its own), in the loops' order:
  centroid    a serial sum from 0 over the ring's atoms, divided by float32(count)
  normal      (a0 - a2) x (a1 - a2), products rounded, then the difference; norm = sqrt of the sum from 0 of the squares; divided
  wrapped d2  val = p1 - p2; where |val| > box / 2 and box != 0: val - box * round(val / box), all float32, C's round (half away
              from zero); d2 the sum from 0 of val * val
  angle       float64(acosf(dot)) * 57.29578, folded at 90 and compared in float64; a NaN fails every comparison
The modules are C++, where round / sqrt / acos of a float32 are the float32 overloads.  acosf is the C library's, which is not
correctly rounded in the library the golden data was made with (glibc 2.35): `acosf` below restates its algorithm (fdlibm's e_acosf.c,
"Developed at SunPro ... Permission to use, copy, modify, and distribute this software is freely granted") in numpy float32 operations.
Vectorised over the frames and the second partners; the lists come out frame by frame, r1 outer, r2 inner.
"""
from __future__ import annotations

import numpy as np

F32, F64 = np.float32, np.float64
PIPI, CATIONPI, SIGMAHOLE = 0, 1, 2


def _c_round(x):
    """C's roundf(): half away from zero (computed in float64, where |x| + 0.5 is exact)"""
    x = x.astype(F64)
    return (np.sign(x) * np.floor(np.abs(x) + 0.5)).astype(F32)


def _bits(v):
    return np.array([v], np.uint32).view(F32)[0]


_PI, _PIO2_HI, _PIO2_LO = _bits(0x40490fda), _bits(0x3fc90fda), _bits(0x33a22168)
_PS = [_bits(v) for v in (0x3e2aaaab, 0xbea6b090, 0x3e4e0aa8, 0xbd241146, 0x3a4f7f04, 0x3811ef08)]
_QS = [_bits(v) for v in (0xc019d139, 0x4001572d, 0xbf303361, 0x3d9dc62e)]


def acosf(x):
    """fdlibm's __ieee754_acosf on a float32 array: numpy rounds every float32 operation on its own, as the C code's are"""
    x = np.ascontiguousarray(x, F32)
    hx = x.view(np.int32)
    ix = hx & 0x7fffffff
    one, half, two = F32(1), F32(0.5), F32(2)

    def ratio(z):
        p = z * (_PS[0] + z * (_PS[1] + z * (_PS[2] + z * (_PS[3] + z * (_PS[4] + z * _PS[5])))))
        q = one + z * (_QS[0] + z * (_QS[1] + z * (_QS[2] + z * _QS[3])))
        return p / q

    with np.errstate(all="ignore"):
        small = _PIO2_HI - (x - (_PIO2_LO - x * ratio(x * x)))
        small = np.where(ix <= 0x23000000, _PIO2_HI + _PIO2_LO, small)
        z = (one + x) * half
        s = np.sqrt(z)
        neg = _PI - two * (s + (ratio(z) * s - _PIO2_LO))
        z = (one - x) * half
        s = np.sqrt(z)
        df = (s.view(np.int32) & np.int32(-4096)).view(F32)
        c = (z - df * df) / (s + df)
        pos = two * (df + (ratio(z) * s + c))
        out = np.where(ix < 0x3f000000, small, np.where(hx < 0, neg, pos))
        out = np.where(ix == 0x3f800000, np.where(hx > 0, F32(0), _PI + two * _PIO2_LO), out)
        out = np.where(ix > 0x3f800000, F32(np.nan), out)
    assert out.dtype == F32
    return out


def wrapped_dist2(p1, p2, box):
    """p1, p2 float32 [..., 3, F]; box float32 [3, F] -> float32 [..., F]"""
    d2 = np.zeros(np.broadcast_shapes(p1.shape, p2.shape)[:-2] + p1.shape[-1:], F32)
    with np.errstate(all="ignore"):
        for ax in range(3):
            val = (p1[..., ax, :] - p2[..., ax, :]).astype(F32)
            b = np.broadcast_to(box[ax], val.shape)
            half = (b / F32(2)).astype(F32)
            wrap = (np.abs(val) > half) & (b != 0)
            q = (val / b).astype(F32)
            w = (val - (b * _c_round(q)).astype(F32)).astype(F32)
            val = np.where(wrap, w, val)
            d2 = (d2 + (val * val).astype(F32)).astype(F32)
    return d2


def normalize(v):
    """v float32 [..., 3, F] -> v / |v| as the reference's _normalize"""
    with np.errstate(all="ignore"):
        n2 = np.zeros(v.shape[:-2] + v.shape[-1:], F32)
        for ax in range(3):
            n2 = (n2 + (v[..., ax, :] * v[..., ax, :]).astype(F32)).astype(F32)
        n = np.sqrt(n2).astype(F32)
        return (v / n[..., None, :]).astype(F32)


def ring_records(coords, ring_atoms, starts):
    """-> centroids, normals, first atoms: float32 [n_rings, 3, F] each"""
    F = coords.shape[2]
    n = len(starts) - 1
    mean, normal, first = (np.zeros((n, 3, F), F32) for _ in range(3))
    for r in range(n):
        s, e = int(starts[r]), int(starts[r + 1])
        acc = np.zeros((3, F), F32)
        for k in range(s, e):
            acc = (acc + coords[ring_atoms[k]]).astype(F32)
        mean[r] = (acc / F32(e - s)).astype(F32)
        a0, a1, a2 = (coords[ring_atoms[s + k]] for k in range(3))
        t1, t2 = (a0 - a2).astype(F32), (a1 - a2).astype(F32)
        c = np.empty((3, F), F32)
        c[0] = (t1[1] * t2[2]).astype(F32) - (t1[2] * t2[1]).astype(F32)
        c[1] = (t1[2] * t2[0]).astype(F32) - (t1[0] * t2[2]).astype(F32)
        c[2] = (t1[0] * t2[1]).astype(F32) - (t1[1] * t2[0]).astype(F32)
        normal[r] = normalize(c)
        first[r] = a0
    return mean, normal, first


def _dot(a, b):
    d = np.zeros(np.broadcast_shapes(a.shape, b.shape)[:-2] + a.shape[-1:], F32)
    with np.errstate(all="ignore"):
        for ax in range(3):
            d = (d + (a[..., ax, :] * b[..., ax, :]).astype(F32)).astype(F32)
    return d


def _angle(dot):
    with np.errstate(all="ignore"):
        ang = acosf(dot).astype(F64) * 57.29578
        return np.where(ang > 90, 180 - ang, ang)


def _lists(hit, second, dist2, angle):
    """hit [n1, n2, F] -> (frame_offsets, pairs, distang), frame by frame, r1 outer, r2 inner"""
    n1, n2, F = hit.shape
    offs = np.zeros(F + 1, np.int64)
    pairs, da = [], []
    for f in range(F):
        i, j = np.nonzero(hit[:, :, f])
        offs[f + 1] = offs[f] + i.size
        pairs.append(np.stack([i.astype(np.uint32), second[j]], axis=1))
        with np.errstate(all="ignore"):
            da.append(np.stack([np.sqrt(dist2[i, j, f].astype(F64)).astype(F32), angle[i, j, f].astype(F32)], axis=1))
    return offs, np.concatenate(pairs).reshape(-1, 2).astype(np.uint32), np.concatenate(da).reshape(-1, 2).astype(F32)


def calculate(kind, coords, box, ring_atoms, starts1, second, thr, details=False):
    """The reference's `calculate` of the given kind.  coords float32 [N, 3, F]; box float32 [3, F] (None: zeros); `second`: the second
    list's starts (pi-pi), cations [n] (cation-pi) or halides [n, 2] (sigma-hole); thr: (dist1, angle1 max, dist2, angle2 min) for
    pi-pi, (dist, angle min) for the others.  -> (frame_offsets int64 [F + 1], pairs uint32 [n, 2], distang float32 [n, 2]); with
    `details` also (tested, angle64): which (r1, r2, frame) passed the distance tests and their float64 angles."""
    coords = np.ascontiguousarray(coords, F32)
    F = coords.shape[2]
    box = np.zeros((3, F), F32) if box is None else np.ascontiguousarray(box, F32)
    ring_atoms, starts1, second = (np.asarray(a, np.uint32) for a in (ring_atoms, starts1, second))
    thr = [F32(t) for t in thr]
    mean1, normal1, first1 = ring_records(coords, ring_atoms, starts1)
    n1 = len(starts1) - 1
    if kind == PIPI:
        t1sq, a1, t2sq, a2 = F32(thr[0] * thr[0]), F64(thr[1]), F32(thr[2] * thr[2]), F64(thr[3])
        mean2, normal2, first2 = ring_records(coords, ring_atoms, second)
        n2 = len(second) - 1
        same = (starts1[:-1, None] == second[None, :-1]) & (starts1[1:, None] == second[None, 1:])
        early = wrapped_dist2(first1[:, None], first2[None], box) > F32(225)
        dist2 = wrapped_dist2(mean1[:, None], mean2[None], box)
        with np.errstate(all="ignore"):
            tested = ~same[:, :, None] & ~early & ~(dist2 > t2sq)
            angle = _angle(_dot(normal1[:, None], normal2[None]))
            hit = tested & (((dist2 < t1sq) & (angle <= a1)) | ((dist2 < t2sq) & (angle >= a2)))
        out = _lists(hit, np.arange(n2, dtype=np.uint32), dist2, angle)
    else:
        tsq, amin = F32(thr[0] * thr[0]), F64(thr[1])
        atoms = second if kind == CATIONPI else second[:, 0]
        pos = coords[atoms]                                            # [n2, 3, F]
        dist2 = wrapped_dist2(mean1[:, None], pos[None], box)
        if kind == CATIONPI:
            v = normalize((pos[None] - mean1[:, None]).astype(F32))   # not wrapped
        else:
            v = normalize((pos - coords[second[:, 1]]).astype(F32))[None]
        with np.errstate(all="ignore"):
            tested = ~(dist2 > tsq)
            angle = 90 - _angle(_dot(normal1[:, None], v))
            hit = tested & (angle >= amin)
        out = _lists(hit, atoms, dist2, angle)
    return out + (tested, angle) if details else out


def threshold_margin(kind, thr, tested, angle):
    """the smallest |angle - threshold| over the pairs that passed the distance tests (float64 degrees; inf: no such pair)"""
    a = angle[tested & ~np.isnan(angle)]
    if a.size == 0:
        return np.inf
    ts = [thr[1], thr[3]] if kind == PIPI else [thr[1]]
    return min(float(np.min(np.abs(a - F64(F32(t))))) for t in ts)
