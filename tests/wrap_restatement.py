"""tests/wrap_restatement.py -- TEST INFRASTRUCTURE: numpy restatement of the reference's rectangular wrap
(moleculekit/wrapping/wrapping.pyx::wrap_box as Molecule.wrap calls it), every operation in the reference's precision.

It extends ``moments_restatement.wrap_box`` (bonds and a centre selection; used here unchanged, by import): ``wrap_box`` below takes the
groups as their starts -- what the reference's ``getBondedGroups`` hands to its loop -- and either a centre selection or a fixed centre.
Written line by line from the reference's loop; frames, and groups of one size, are vectorised, nothing else is:

    box_center = center                                             (no centre selection)
    per frame:
        box_center = 0; for n, atom in centersel: box_center += (x[atom] - box_center) / (n + 1)         float32, IEEE division
        half_box = box / 2
        per group:  grp_center = 0; for n, atom in group: grp_center += (x[atom] - grp_center) / (n + 1)
                    per axis:  diff = grp_center - box_center
                               if fabs(diff) > half_box:  translation = float32(double(box) * round(double(diff / box)))
                                                          x[atoms of the group] -= translation
The group centres come from coordinates that no earlier group has changed (groups are disjoint), the box centre from the frame before
any group moved.
"""
from __future__ import annotations

import numpy as np

from moments_restatement import _running_mean, bonded_groups, wrap_box as wrap_box_bonds  # noqa: F401  (re-exported)


def _round_half_away(q):
    """C's round() of float64 values"""
    return np.sign(q) * np.floor(np.abs(q) + 0.5)


def box_centre(x, centersel, center):
    """float32 [3, F]: the running mean of the centre selection's atoms (in the order given) or the centre given"""
    F = x.shape[2]
    if centersel is not None and len(centersel) > 0:
        return _running_mean(x[np.asarray(centersel, np.int64)])
    return np.repeat(np.asarray(center, np.float32).reshape(3, 1), F, axis=1)


def wrap_box(coords, box, starts, centersel=None, center=None, moved=None):
    """coords float32 [N, 3, F] (a wrapped COPY is returned), box float32 [3, F], starts [G + 1] (starts[G] = N), centersel atom
    indexes in order or None / empty: then ``center`` [3].  ``moved``: a list that receives bool [G, 3, F], which (group, axis, frame)
    moved."""
    x = np.array(coords, np.float32)
    box = np.asarray(box, np.float32)
    starts = np.asarray(starts, np.int64)
    centre = box_centre(x, centersel, center)                                   # [3, F], from the unwrapped frame
    half = box / np.float32(2)
    sizes = np.diff(starts)
    mv = np.zeros((sizes.size, 3, x.shape[2]), bool)
    for n in np.unique(sizes):
        gs = np.flatnonzero(sizes == n)
        idx = starts[gs][:, None] + np.arange(n)[None, :]                       # [g, n]
        xs = x[idx]                                                             # [g, n, 3, F]
        c = np.zeros((gs.size,) + x.shape[1:], np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(n):
                c = c + (xs[:, k] - c) / np.float32(k + 1)
            diff = c - centre[None]                                             # [g, 3, F] float32
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            q = (diff / box[None]).astype(np.float64)
            shift = (box.astype(np.float64)[None] * _round_half_away(q)).astype(np.float32)
            move = np.abs(diff) > half[None]
            x[idx] = np.where(move[:, None], xs - shift[:, None], xs)
        mv[gs] = move
    if moved is not None:
        moved.append(mv)
    return x


def to_frame_major(coords):
    """[N, 3, F] -> [F, N, 3]"""
    return np.ascontiguousarray(np.transpose(np.asarray(coords, np.float32), (2, 0, 1)))


def from_frame_major(xyz):
    """[F, N, 3] -> [N, 3, F]"""
    return np.ascontiguousarray(np.transpose(np.asarray(xyz, np.float32), (1, 2, 0)))


def wrap_frames(xyz, box, starts, centersel=None, center=None):
    """``wrap_box`` on frame-major float32 [F, N, 3] -> the wrapped [F, N, 3]"""
    return to_frame_major(wrap_box(from_frame_major(xyz), box, starts, centersel, center))
