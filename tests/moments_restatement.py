"""tests/moments_restatement.py -- TEST INFRASTRUCTURE: numpy float64 restatements of the reference's MetricCoordinate, MetricGyration,
MetricSphericalCoordinate and MetricFluctuation (moleculekit projections/metric*.py) AFTER the alignment: given float32 coordinates
(already aligned where an alignment is involved) they return the projections in float64, every intermediate in float64.  Frame-major
``xyz`` float32 ``[F, N, 3]`` throughout.  Plus the float64 Kabsch superposition the fixture tests align with."""
from __future__ import annotations

import numpy as np


def _w(weights, n):
    return np.ones(n, np.float64) if weights is None else np.asarray(weights, np.float32).astype(np.float64)


def center(xyz, groups, weights=None):
    """[F, 3 G], column c * G + g: sum w x_c / sum w (MetricCoordinate with groups; singleton groups: the coordinates themselves)"""
    x = np.asarray(xyz, np.float32).astype(np.float64)
    F, G = x.shape[0], len(groups)
    out = np.zeros((F, 3, G))
    k = 0
    for g, idx in enumerate(groups):
        idx = np.asarray(idx)
        w = _w(None if weights is None else np.asarray(weights)[k:k + idx.size], idx.size)
        k += idx.size
        out[:, :, g] = (x[:, idx, :] * w[None, :, None]).sum(axis=1) / w.sum()
    return out.reshape(F, 3 * G)


def gyration(xyz, groups, weights=None):
    """[F, G, 4]: sqrt(sum w q / sum w), q = |r|^2, r_y^2 + r_z^2, r_x^2 + r_z^2, r_x^2 + r_y^2, r = x - com (MetricGyration per group)"""
    x = np.asarray(xyz, np.float32).astype(np.float64)
    F, G = x.shape[0], len(groups)
    out = np.zeros((F, G, 4))
    k = 0
    for g, idx in enumerate(groups):
        idx = np.asarray(idx)
        w = _w(None if weights is None else np.asarray(weights)[k:k + idx.size], idx.size)
        k += idx.size
        c = x[:, idx, :]
        com = (c * w[None, :, None]).sum(axis=1) / w.sum()
        sq = (c - com[:, None, :]) ** 2
        q = np.stack([sq.sum(axis=2), sq[:, :, [1, 2]].sum(axis=2), sq[:, :, [0, 2]].sum(axis=2), sq[:, :, [0, 1]].sum(axis=2)], axis=2)
        out[:, g, :] = np.sqrt((q * w[None, :, None]).sum(axis=1) / w.sum())
    return out


def spherical(xyz, target, ref):
    """[F, 3]: r, theta, phi of centroid(target) - centroid(ref) (MetricSphericalCoordinate); |d| = 0 gives NaN for theta"""
    x = np.asarray(xyz, np.float32).astype(np.float64)
    d = x[:, np.asarray(target), :].mean(axis=1) - x[:, np.asarray(ref), :].mean(axis=1)
    r = np.sqrt((d * d).sum(axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        theta = np.arccos(d[:, 2] / r)
    return np.stack([r, theta, np.arctan2(d[:, 1], d[:, 0])], axis=1)


def fluctuation(xyz, atoms, ref=None, offsets=None):
    """[F, n]: sum_c (x_c - ref_c)^2 per listed atom, ref [n, 3] or the mean over the frames; with offsets [G + 1] (contiguous runs of
    positions in atoms) [F, G]: the mean over each run (MetricFluctuation, modes atom / residue)"""
    x = np.asarray(xyz, np.float32).astype(np.float64)[:, np.asarray(atoms), :]
    r = x.mean(axis=0) if ref is None else np.asarray(ref, np.float64)
    v = ((x - r[None]) ** 2).sum(axis=2)
    if offsets is None:
        return v
    o = np.asarray(offsets, np.int64)
    return np.stack([v[:, o[g]:o[g + 1]].mean(axis=1) for g in range(o.size - 1)], axis=1)


def apply_affine(xyz, affine):
    """float32(R x + t) per frame, evaluated in float64 in the operation order of csrc/mk_affine.h without fused multiply-adds: what the
    EMULATED kernels (built with -ffp-contract=off) compute.  (On the device the bits are align.apply_transforms'.)"""
    x = np.asarray(xyz, np.float32).astype(np.float64)
    A = np.asarray(affine, np.float64)
    out = np.empty(x.shape, np.float32)
    for r in range(3):
        a = A[:, None, 3 * r:3 * r + 3]
        out[:, :, r] = (a[:, :, 0] * x[:, :, 0] + a[:, :, 1] * x[:, :, 1] + a[:, :, 2] * x[:, :, 2] + A[:, None, 9 + r]).astype(np.float32)
    return out


def kabsch_align(xyz, sel, ref):
    """every frame of xyz float32 [F, N, 3] superposed with its atoms sel on ref [n, 3] (least squares, proper rotation) in float64;
    returns float32 [F, N, 3]"""
    x = np.asarray(xyz, np.float32).astype(np.float64)
    q = np.asarray(ref, np.float64)
    qc = q.mean(axis=0)
    out = np.empty(x.shape, np.float32)
    for f in range(x.shape[0]):
        p = x[f, sel]
        pc = p.mean(axis=0)
        U, _, Vt = np.linalg.svd((p - pc).T @ (q - qc))
        D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
        R = (U @ D @ Vt).T
        out[f] = ((x[f] - pc) @ R.T + qc).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------
# the reference's wrap_box (moleculekit/wrapping): a TEST HELPER only -- wrapping is not part of the package
# ------------------------------------------------------------------------------------------------
def bonded_groups(bonds, n_atoms):
    """start index of every bonded group, and n_atoms at the end (the reference's getBondedGroups): union-find over the bonds, then
    the first atom of every distinct root; groups are taken to be contiguous runs of atoms, as the reference takes them"""
    parent = np.arange(n_atoms)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    size = np.ones(n_atoms, np.int64)
    for a, b in np.asarray(bonds, np.int64).reshape(-1, 2):
        ra, rb = find(a), find(b)
        if ra == rb:
            continue
        if size[ra] < size[rb]:
            ra, rb = rb, ra
        parent[rb] = ra
        size[ra] += size[rb]
    roots = np.array([find(i) for i in range(n_atoms)])
    _, first = np.unique(roots, return_index=True)
    return np.r_[np.sort(first), n_atoms].astype(np.int64)


def _running_mean(x):
    """float32 running mean c += (x - c) / (n + 1) over axis 0 in order, vectorised over the other axes"""
    c = np.zeros(x.shape[1:], np.float32)
    for n in range(x.shape[0]):
        c = c + (x[n] - c) / np.float32(n + 1)
    return c


def wrap_box(coords, box, centersel, bonds):
    """the reference's rectangular wrap: coords float32 [N, 3, F] (a wrapped COPY is returned), box float32 [3, F], centersel atom
    indexes (in atom order), bonds [n_bonds, 2].  Per frame the box centre is the float32 running mean of the centersel atoms; every
    bonded group whose float32 running-mean centre is more than box / 2 from it along an axis is moved by box * round(diff / box)
    along that axis (the quotient in float32, the rounding half away from zero and the product in double, stored as float32)."""
    x = np.array(coords, np.float32)
    box = np.asarray(box, np.float32)
    centre = _running_mean(x[np.asarray(centersel)])                            # [3, F]
    half = box / np.float32(2)
    groups = bonded_groups(bonds, x.shape[0])
    for g in range(groups.size - 1):
        a, b = groups[g], groups[g + 1]
        diff = (x[a] if b - a == 1 else _running_mean(x[a:b])) - centre         # [3, F] float32
        with np.errstate(divide="ignore", invalid="ignore"):
            q = (diff / box).astype(np.float64)
        shift = (box.astype(np.float64) * (np.sign(q) * np.floor(np.abs(q) + 0.5))).astype(np.float32)
        move = np.abs(diff) > half
        x[a:b] = np.where(move[None], x[a:b] - shift[None], x[a:b])
    return x
