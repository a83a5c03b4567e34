"""``cdist``, ``pdist``, ``squareform`` with the signatures of moleculekit/distance.py:221-305 on top of the GPU ``distance_utils``,
for callers that do not have moleculekit installed.

Round 6: the drivers that sat here until round 5 -- ``pp_calcDistances`` / ``get_reduced_distances`` (projections/util.py:12-223) and
``calculate_contacts`` (distance.py:308-412) on duck-typed molecules -- are gone.  They restated the reference's own glue, and they
are not needed: the reference's drivers import ``moleculekit.distance_utils`` at call time, so ``moleculekit_amd.install()`` swaps the
eight compiled functions under them and MetricDistance, ``calculate_contacts``, ``cdist`` / ``pdist`` and ``_detectCollisions`` run on
the GPU unchanged (``moleculekit_amd/distance_utils.py::install``).  Whoever works below the Molecule level
calls ``moleculekit_amd.distance_utils`` directly -- the reference's Cython-level signatures."""
from __future__ import annotations

import numpy as np

from . import distance_utils as _du


def cdist(coords1, coords2):
    """(N, D) x (M, D) -> float32 (N, M) Euclidean distances (distance.py:221-252)."""
    coords1, coords2 = np.asarray(coords1), np.asarray(coords2)
    assert coords1.ndim == 2, "cdist only supports 2D arrays"
    assert coords2.ndim == 2, "cdist only supports 2D arrays"
    assert coords1.shape[1] == coords2.shape[1], "Second dimension of input arguments must match"
    results = np.zeros((coords1.shape[0], coords2.shape[0]), dtype=np.float32)
    _du.cdist(coords1.astype(np.float32), coords2.astype(np.float32), results)
    return results


def pdist(coords):
    """(N, D) -> condensed float32 upper-triangular distances (distance.py:255-282)."""
    coords = np.asarray(coords)
    assert coords.ndim == 2, "pdist only supports 2D arrays"
    n = coords.shape[0]
    results = np.zeros(int(n * (n - 1) / 2), dtype=np.float32)
    _du.pdist(coords.astype(np.float32), results)
    return results


def squareform(distances):
    """Condensed vector -> (N, N) symmetric matrix (distance.py:285-305)."""
    return np.array(_du.squareform(np.asarray(distances).astype(np.float32)))


def _clash_mask(mol, sel, natoms):
    """the reference's ``Molecule.atomselect`` for what ``find_clashes`` passes: None, a string (``mol.atomselect``), a boolean mask or
    an integer index array"""
    if sel is None or (isinstance(sel, str) and sel == "all"):
        return np.ones(natoms, dtype=bool)
    if isinstance(sel, str):
        return np.atleast_1d(np.asarray(mol.atomselect(sel), dtype=bool))
    sel = np.atleast_1d(np.asarray(sel))
    if sel.dtype == bool:
        if sel.shape != (natoms,):
            raise ValueError(f"a selection mask must have shape ({natoms},), got {sel.shape}")
        return sel
    if not np.issubdtype(sel.dtype, np.integer):
        raise ValueError(f"a selection must be a string, a boolean mask or an integer index array, got {sel.dtype}")
    if sel.size and (sel.min() < -natoms or sel.max() >= natoms):
        raise ValueError(f"selection index out of range for {natoms} atoms")
    mask = np.zeros(natoms, dtype=bool)
    mask[sel] = True
    return mask


def find_clashes(mol, sel1=None, sel2=None, overlap=0.6, exclude_bonded=True, exclude_14=True, guess_bonds=True, ctx=None):
    """``find_clashes`` of moleculekit/distance.py:9-218 on the GPU: the pairs of atoms closer than ``r_vdw_1 + r_vdw_2 - overlap``, without
    the 1-2 / 1-3 (``exclude_bonded``) and 1-4 (``exclude_14``) neighbours of ``mol.bonds`` stacked on the guessed bonds (``guess_bonds``).
    ``mol`` is duck-typed: ``element``, ``coords`` (``[N, 3, F]``), ``frame``, ``bonds``, ``numAtoms``, ``name``; ``atomselect`` only where a
    selection is a string.  Returns ``(pairs int64 [n, 2], distances float32 [n], overlaps float32 [n])`` sorted by overlap, largest
    first -- the reference's arrays; equal overlaps, whose order the reference leaves open, by ``(a, b)`` ascending.  With one selection
    (or two equal ones) the rows have ``a < b``; with two different ones they are ordered ``(a of sel1, b of sel2)`` and, as in the
    reference, neither filtered for ``a < b`` nor excluded where ``a > b`` (moleculekit_amd/clashes.py).  ``ValueError``: non-finite
    coordinates in a selection, a selection out of range, more than 4 096 atoms in one grid box."""
    from types import SimpleNamespace

    from . import _lib, bonds as _bonds, clashes as _cl

    natoms = int(mol.numAtoms)
    mask1 = _clash_mask(mol, sel1, natoms)
    mask2 = _clash_mask(mol, sel2, natoms) if sel2 is not None else mask1
    self_mode = sel2 is None or np.array_equal(mask1, mask2)
    empty = (np.empty((0, 2), dtype=np.int64), np.empty(0, dtype=np.float32), np.empty(0, dtype=np.float32))
    if not mask1.any() or not mask2.any():
        return empty
    coords = np.ascontiguousarray(np.asarray(mol.coords)[:, :, mol.frame], dtype=np.float32)
    if not np.isfinite(coords[mask1 | mask2]).all():
        raise ValueError("find_clashes received non-finite coordinates (NaN or inf) in its selections. Coordinates must be finite.")
    radii = _cl.clash_radii(mol.element)
    cutoff = _cl.clash_cutoff(radii.max(), overlap)
    ctx = ctx or _lib.default_context()
    ex_start = ex_partner = None
    if exclude_bonded or exclude_14:
        bonds = np.asarray(mol.bonds)
        bonds = bonds.reshape(-1, 2).astype(np.uint32) if len(bonds) else np.empty((0, 2), dtype=np.uint32)
        if guess_bonds:
            full = np.asarray(mol.coords)
            view = SimpleNamespace(numAtoms=natoms, frame=mol.frame, numFrames=full.shape[2], coords=full, element=mol.element, name=mol.name)
            bonds = np.vstack((bonds, _bonds.guess_bonds(view, ctx=ctx)))
        ex = _cl.clash_exclusions(bonds, natoms, exclude_bonded, exclude_14)
        ex_start, ex_partner = ex.start, ex.partner
    pairs, distances, overlaps, _ = ctx.find_clashes_host(coords, radii, np.ascontiguousarray(mask1, dtype=np.uint32),
                                                          None if self_mode else np.ascontiguousarray(mask2, dtype=np.uint32), ex_start,
                                                          ex_partner, float(overlap), cutoff)
    if len(pairs) == 0:
        return empty
    return pairs.astype(np.int64), distances, overlaps
