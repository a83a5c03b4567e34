"""tests/bonds_restatement.py -- TEST INFRASTRUCTURE: a numpy restatement of the reference's bond guesser (moleculekit bondguesser.py:
`guess_bonds`, `bond_grid_search`; bondguesser_utils.pyx: the neighbour relations and the pair test), in this project's words
(DESIGN.md section 16).  One frame, a non-periodic grid.

  radii      the per-element table (moleculekit_amd/_bond_radii.py; capitalised keys, so "CL" misses it), else the default of the
             upper-cased first letter of the atom NAME, else 1.5; float32
  grid       grid_cutoff = max(radii) * 1.2 (numpy 2: the float32 scalar times a Python float stays float32), then float(); min and
             max per axis in float32, range = max - min in float32; boxes per axis floor(range / float32(pairdist)) + 1 as Python
             integers; pairdist a Python double, multiplied by cutoff_incr while the product of the counts exceeds max_boxes
  box        floor((x - min) / float32(pairdist)) per axis -- float32 subtraction, float32 division --, clipped to [0, count - 1],
             flattened z * nx * ny + y * nx + x
  pair test  not two hydrogens; d = x_i - x_j per axis; dist2 = (dx dx + dy dy) + dz dz, every operation a float32 one; rejected where
             dist2 > float32(pairdist)^2, where float64(dist2) < 0.001, where dist2 > cut * cut with
             cut = float32(0.6 * float64(r_i + r_j)) (the sum and the square float32).  Equality bonds
  order      occupied boxes by their lowest atom index; owners ascending; per owner the existing ones of the 14 neighbour boxes in
             RELATIONS' order; partners ascending, in the owner's own box only those above the owner.  Rows (i, j) as found
Vectorised over the partners of one (owner, neighbour box).
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from moleculekit_amd._bond_radii import BOND_RADII, FALLBACK, NAME_DEFAULTS  # noqa: E402

F32, F64 = np.float32, np.float64

# (dx, dy, dz) of the 14 neighbour boxes an owner looks into, in the reference's order
RELATIONS = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1),
             (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, -1, 0), (-1, 0, 1), (0, -1, 1),
             (1, 1, 1), (-1, 1, 1), (1, -1, 1), (-1, -1, 1))


def radii_of(element, name):
    out = []
    for el, nm in zip(element, name):
        if str(el) in BOND_RADII:
            out.append(BOND_RADII[str(el)])
        else:
            out.append(NAME_DEFAULTS.get(str(nm)[0].upper(), FALLBACK))
    return np.array(out, dtype=F32)


def default_cutoff(radii):
    return float(np.max(np.asarray(radii, F32)) * 1.2)


def grid_of(min_c, max_c, grid_cutoff, max_boxes=4e6, cutoff_incr=1.26):
    """(nx, ny, nz, pairdist)"""
    span = (np.asarray(max_c, F32) - np.asarray(min_c, F32)).astype(F32)
    pairdist = float(grid_cutoff)
    while True:
        counts = [int(v) + 1 for v in np.floor((span / F32(pairdist)).astype(F32)).astype(np.int64)]
        if counts[0] * counts[1] * counts[2] <= max_boxes:
            return counts[0], counts[1], counts[2], pairdist
        pairdist *= cutoff_incr


def boxes_of(coords, min_c, grid):
    nx, ny, nz, pairdist = grid
    q = np.floor(((coords - min_c).astype(F32) / F32(pairdist)).astype(F32)).astype(np.int64)
    q = np.minimum(np.maximum(q, 0), np.array([nx, ny, nz], np.int64) - 1)
    return q, q[:, 2] * (nx * ny) + q[:, 1] * nx + q[:, 0]


def dist2_of(coords, i, js):
    d = (coords[i][None, :] - coords[js]).astype(F32)
    sq = (d * d).astype(F32)
    return ((sq[:, 0] + sq[:, 1]).astype(F32) + sq[:, 2]).astype(F32)


def cut2_of(radii, i, js):
    cut = (0.6 * (radii[i] + radii[js]).astype(F32).astype(F64)).astype(F32)
    return (cut * cut).astype(F32)


def is_close(coords, radii, is_h, i, js, cutoff2):
    """bool per partner in js"""
    d2 = dist2_of(coords, i, js)
    ok = ~((is_h[i] != 0) & (is_h[js] != 0))
    ok &= ~(d2 > cutoff2)
    ok &= ~(d2.astype(F64) < 0.001)
    ok &= ~(d2 > cut2_of(radii, i, js))
    return ok


def search(coords, grid_cutoff, is_hydrogen, radii, max_boxes=4e6, cutoff_incr=1.26, details=False):
    """the reference's bond_grid_search -> uint32 [n, 2]; details: also a dict with the grid, the largest occupancy, the relation of
    every row, and the in-grid pairs the test rejected"""
    coords = np.ascontiguousarray(coords, F32)
    radii = np.ascontiguousarray(radii, F32)
    is_h = np.ascontiguousarray(is_hydrogen, np.uint32)
    if not np.isfinite(coords).all():
        raise ValueError("coordinates must be finite")
    if not (grid_cutoff > 0 and np.isfinite(grid_cutoff)):
        raise ValueError(f"grid_cutoff must be positive and finite, got {grid_cutoff!r}")
    min_c, max_c = coords.min(axis=0), coords.max(axis=0)
    grid = grid_of(min_c, max_c, grid_cutoff, max_boxes, cutoff_incr)
    nx, ny, nz, pairdist = grid
    cells, flat = boxes_of(coords, min_c, grid)
    cutoff2 = F32(F32(pairdist) * F32(pairdist))
    # the occupied boxes in the order of their lowest atom; every box's atoms ascending
    uniq, first = np.unique(flat, return_index=True)
    by_box = np.argsort(flat, kind="stable")
    members = {int(flat[g[0]]): g for g in np.split(by_box, np.flatnonzero(np.diff(flat[by_box])) + 1)}
    rows, rels, rejected = [], [], 0
    for b in uniq[np.argsort(first, kind="stable")]:
        own = members[int(b)]
        cx, cy, cz = (int(v) for v in cells[own[0]])
        for pos, i in enumerate(own):
            for k, (dx, dy, dz) in enumerate(RELATIONS):
                x, y, z = cx + dx, cy + dy, cz + dz
                if not (0 <= x < nx and 0 <= y < ny and 0 <= z < nz):
                    continue
                js = own[pos + 1:] if k == 0 else members.get(z * nx * ny + y * nx + x)
                if js is None or len(js) == 0:
                    continue
                ok = is_close(coords, radii, is_h, i, js, cutoff2)
                rejected += int((~ok).sum())
                for j in js[ok]:
                    rows.append((int(i), int(j)))
                    rels.append(k)
    pairs = np.array(rows, dtype=np.uint32).reshape(-1, 2)
    if not details:
        return pairs
    return pairs, {"grid": grid, "max_occ": int(max(len(m) for m in members.values())), "relations": np.array(rels, np.int64),
                   "rejected": rejected, "cutoff2": cutoff2}


def guess(coords, element, name):
    """the reference's guess_bonds on one frame's [N, 3] coordinates"""
    if len(coords) <= 1:
        return np.zeros((0, 2), np.uint32)
    element = np.asarray(element)
    radii = radii_of(element, name)
    return search(coords, default_cutoff(radii), (element == "H").astype(np.uint32), radii)
