"""tests/wrap_cell_restatement.py -- TEST INFRASTRUCTURE: numpy restatement of the reference's wrap of triclinic boxes
(moleculekit/wrapping/wrapping.pyx::wrap_triclinic_unitcell and wrap_compact_unitcell as Molecule.wrap calls them), every operation in
the reference's precision.  Written line by line from the reference's loops; the frames' recentring and the groups' running means are
vectorised over frames and axes, the decisions are scalar loops.  Pinned to the compiled reference's bits on the golden subset of
tests/wrap_cell_cases.py (tests/golden/wrap_cell_cases.npz, made by tests/golden/make_golden_wrap_cell.py).

    wrap_center = center                                               (no centre selection)
    per frame:
        wrap_center = running float32 mean of the centre selection (wrap_restatement.box_centre), from the unwrapped frame
        box_middle[j] = float32(double(box_middle[j]) + 0.5 * box[i][j])          i outer, j inner
        every atom:  x = (x - wrap_center) + box_middle                            float32
        per group:   grp_center = running float32 mean of the group's recentred atoms
      "triclinic":   shm01 = b10 / b11; shm02 = (b11 b20 - b21 b10) / (b11 b22); shm12 = b21 / b22          float64
                     shift_center = double(box_middle) - 0.5 * (b0 + b1 + b2);  [0] = shm01 [1] + shm02 [2]; [1] = shm12 [2]; [2] = 0
                     for m = 2, 1, 0:  shift = shift_center[m] (+ shm12 gc[2] | + (shm01 gc[1] + shm02 gc[2])), formed once
                                       while gc[m] - shift < 0:          gc[d] = float32(double(gc[d]) + box[m][d])  for d <= m
                                       while gc[m] - shift >= box[m][m]: gc[d] = float32(double(gc[d]) - box[m][d])
                                       x[atoms, m] -= (gc_init[m] - gc[m])                                    float32
      "rectangular" / "compact":  get_pbc(box) per frame (float64), pbc_dx(gc, box_middle) per group,
                     x[atoms] = float32(double((x - gc) + box_middle) + dx)

Two things are this project's, not the reference's (whose loops do not end there): every ``while`` loop stops after MAX_STEPS steps and
status[ST_CAP] is set; a frame whose box vectors are not finite, whose box[1][1] or box[2][2] is not positive or whose upper triangle is
not zero is copied through unchanged and status[ST_FRAME] is set.  More than 12 triclinic vectors: the frame is copied through,
status[ST_VECTORS] is set (the reference raises "Too many triclinic vectors!!").
"""
from __future__ import annotations

import numpy as np

from wrap_restatement import box_centre, from_frame_major, to_frame_major  # noqa: F401  (re-exported)

MAX_STEPS = 4096
ST_CAP, ST_FRAME, ST_VECTORS = 0, 1, 2
MODES = ("rectangular", "compact", "triclinic")
f32 = np.float32


def frame_bad(b):
    """b float64 [3, 3]"""
    return bool(not np.all(np.isfinite(b)) or not b[1, 1] > 0 or not b[2, 2] > 0 or b[0, 1] != 0 or b[0, 2] != 0 or b[1, 2] != 0)


def box_middle(b):
    bm = [f32(0), f32(0), f32(0)]
    for i in range(3):
        for j in range(3):
            bm[j] = f32(float(bm[j]) + 0.5 * float(b[i, j]))
    return bm


def _cmin(a, b):
    return a if a < b else b


def _cmax(a, b):
    return a if a > b else b


def _norm2(v):
    return v[0] * v[0] + v[1] * v[1] + v[2] * v[2]


def get_pbc(b):
    """the reference's get_pbc: (max_cutoff2, the triclinic vectors as a list of 3-lists, whether there were more than 12)"""
    b = [[float(b[i, j]) for j in range(3)] for i in range(3)]
    hbox = [b[i][i] * 0.5 for i in range(3)]
    min_hv2 = 0.25 * _cmin(_norm2(b[0]), _norm2(b[1]))
    min_hv2 = _cmin(min_hv2, 0.25 * _norm2(b[2]))
    min_ss = _cmin(b[0][0], _cmin(b[1][1] - abs(b[2][1]), b[2][2]))
    max_cutoff2 = _cmin(min_hv2, min_ss * min_ss)
    margin = 1.001
    vecs, too_many = [], False
    for k in (0, -1, 1):
        for j in (0, -1, 1):
            for i in (0, -1, 1):
                if not (j != 0 or k != 0):
                    continue
                d2old = d2new = 0.0
                trial, pos = [0.0] * 3, [0.0] * 3
                for d in range(3):
                    trial[d] = float(i) * b[0][d] + float(j) * b[1][d] + float(k) * b[2][d]
                    pos[d] = _cmin(hbox[d], -trial[d]) if trial[d] < 0 else _cmax(-hbox[d], -trial[d])
                    d2old += pos[d] * pos[d]
                    d2new += (pos[d] + trial[d]) * (pos[d] + trial[d])
                if margin * d2new < d2old:
                    use = True
                    for dd, shift in enumerate((i, j, k)):
                        if shift:
                            d2c = 0.0
                            for e in range(3):
                                t = pos[e] + trial[e] - float(shift) * b[dd][e]
                                d2c += t * t
                            if d2c <= margin * d2new:
                                use = False
                                break
                    if use:
                        if len(vecs) >= 12:
                            too_many = True
                            continue
                        vecs.append(list(trial))
    return max_cutoff2, vecs, too_many


def _loop(cond, step):
    """the capped ``while``: True when the cap was reached"""
    n = 0
    while cond():
        if n == MAX_STEPS:
            return True
        step()
        n += 1
    return False


def pbc_dx(gc, bm, b, hbox, vecs, max_cutoff2, mode):
    """(dx float64 [3], capped)"""
    dx = [float(f32(gc[i]) - f32(bm[i])) for i in range(3)]
    capped = False

    def move(i, sign, js):
        def step():
            for j in js:
                dx[j] = dx[j] + sign * float(b[i, j]) if sign > 0 else dx[j] - float(b[i, j])
        return step

    if mode == 0:
        for i in range(3):
            capped |= _loop(lambda: dx[i] > hbox[i], move(i, -1, (i,)))
            capped |= _loop(lambda: dx[i] <= -hbox[i], move(i, 1, (i,)))
    else:
        for i in (2, 1, 0):
            js = tuple(range(i, -1, -1))
            capped |= _loop(lambda: dx[i] > hbox[i], move(i, -1, js))
            capped |= _loop(lambda: dx[i] <= -hbox[i], move(i, 1, js))
            d2min = _norm2(dx)
            if d2min > max_cutoff2:
                start = list(dx)
                k = 0
                while d2min > max_cutoff2 and k < len(vecs):
                    trial = [start[j] + vecs[k][j] for j in range(3)]
                    d2 = _norm2(trial)
                    if d2 < d2min:
                        dx[:] = trial
                        d2min = d2
                    k += 1
    return dx, capped


def triclinic_deltas(gc, b, shm, sc):
    """(the float32 deltas gc_init[m] - gc[m], capped)"""
    g = [f32(gc[0]), f32(gc[1]), f32(gc[2])]
    init = list(g)
    shm01, shm02, shm12 = shm
    capped = False
    for m in (2, 1, 0):
        shift = sc[m]
        if m == 0:
            shift += shm01 * float(g[1]) + shm02 * float(g[2])
        elif m == 1:
            shift += shm12 * float(g[2])

        def add(sign, m=m):
            def step():
                for d in range(m + 1):
                    g[d] = f32(float(g[d]) + float(b[m, d])) if sign > 0 else f32(float(g[d]) - float(b[m, d]))
            return step

        capped |= _loop(lambda: float(g[m]) - shift < 0, add(1))
        capped |= _loop(lambda: float(g[m]) - shift >= float(b[m, m]), add(-1))
    with np.errstate(invalid="ignore"):
        return [f32(init[m] - g[m]) for m in range(3)], capped


def _group_means(xc, starts):
    """xc float32 [N, 3, F] -> float32 [G, 3, F], the running means"""
    G = len(starts) - 1
    c = np.zeros((G,) + xc.shape[1:], f32)
    sizes = np.diff(starts)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in np.unique(sizes):
            gs = np.flatnonzero(sizes == n)
            acc = np.zeros((gs.size,) + xc.shape[1:], f32)
            for k in range(int(n)):
                acc = acc + (xc[starts[gs] + k] - acc) / f32(k + 1)
            c[gs] = acc
    return c


def wrap_cell(coords, boxvectors, starts, mode, centersel=None, center=None):
    """coords float32 [N, 3, F] (a wrapped COPY is returned), boxvectors float64 [3, 3, F], starts [G + 1], mode a name of MODES or its
    index (0 rectangular, 1 compact, 2 triclinic) -> (the wrapped [N, 3, F], the status words int32 [3])"""
    mode = MODES.index(mode) if isinstance(mode, str) else int(mode)
    x = np.array(coords, f32)
    bv = np.asarray(boxvectors, np.float64)
    starts = np.asarray(starts, np.int64)
    N, _, F = x.shape
    status = np.zeros(3, np.int32)
    wc = box_centre(x, centersel, center)                                       # [3, F], from the unwrapped frame
    out = x.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(F):
            b = bv[:, :, f]
            if frame_bad(b):
                status[ST_FRAME] = 1
                continue
            bm = box_middle(b)
            bmv = np.array(bm, f32)
            xc = (x[:, :, f] - wc[None, :, f]) + bmv[None]                      # [N, 3] float32
            gcs = _group_means(xc[:, :, None], starts)[:, :, 0]                 # [G, 3]
            if mode == 2:
                b10, b11, b20, b21, b22 = (float(b[1, 0]), float(b[1, 1]), float(b[2, 0]), float(b[2, 1]), float(b[2, 2]))
                shm = (b10 / b11, (b11 * b20 - b21 * b10) / (b11 * b22), b21 / b22)
                sc = [0.0, 0.0, 0.0]
                for i in range(3):
                    for j in range(3):
                        sc[j] = sc[j] + float(b[i, j])
                sc = [float(bm[i]) - sc[i] * 0.5 for i in range(3)]
                sc[0] = shm[0] * sc[1] + shm[1] * sc[2]
                sc[1] = shm[2] * sc[2]
                sc[2] = 0.0
            else:
                hbox = [float(b[i, i]) * 0.5 for i in range(3)]
                max_cutoff2, vecs, too_many = get_pbc(b)
                if too_many:
                    status[ST_VECTORS] = 1
                    continue
            res = np.empty_like(xc)
            for g in range(len(starts) - 1):
                s, e = starts[g], starts[g + 1]
                gc = gcs[g]
                if mode == 2:
                    delta, capped = triclinic_deltas(gc, b, shm, sc)
                    res[s:e] = xc[s:e] - np.array(delta, f32)[None]
                else:
                    dx, capped = pbc_dx(gc, bm, b, hbox, vecs, max_cutoff2, mode)
                    res[s:e] = (((xc[s:e] - gc[None]) + bmv[None]).astype(np.float64) + np.array(dx)[None]).astype(f32)
                if capped:
                    status[ST_CAP] = 1
            out[:, :, f] = res
    return out, status


def wrap_cell_frames(xyz, boxvectors, starts, mode, centersel=None, center=None):
    """``wrap_cell`` on frame-major float32 [F, N, 3] -> (the wrapped [F, N, 3], status)"""
    r, status = wrap_cell(from_frame_major(xyz), boxvectors, starts, mode, centersel, center)
    return to_frame_major(r), status
