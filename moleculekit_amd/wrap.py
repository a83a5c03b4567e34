"""Periodic wrapping of trajectories on the MI355X (include/mkamd_distance.h "periodic wrap").

The reference's ``Molecule.wrap`` moves every bonded group of every frame by whole box lengths back to within half a box of a centre
-- the first step of every projection it offers (``mol.wrap(centersel)``, then ``mol.align(...)``) -- in a serial loop on the host.
Here the same arithmetic, to the bit, runs on the device (csrc/wrap_kernels.h): the centres are float32 running means in atom
order, so a group on the cell's boundary lands where the reference puts it.  The rectangular cell only; triclinic cells are refused
(or, once ``install()``-ed, handed back to the reference).

* ``bonded_groups(bonds, n_atoms)`` -- the starts of the bonded groups (the reference's ``getBondedGroups``), on the host.
* ``wrap_trajectory`` -- CUDA tensors, frame-major ``[F, N, 3]`` float32 and a ``[3, F]`` box; asynchronous; in place or not.
* ``wrap`` -- numpy arrays ``[N, 3, F]`` through the host entry point (``rows``: only the atoms that matter travel).
* ``wrap_molecule`` -- ``Molecule.wrap`` on a molecule-like object; ``install()`` / ``uninstall()`` swap ``Molecule.wrap`` of an
  installed moleculekit.

There is no CPU path: without the library or a device every entry point that computes raises.
"""
from __future__ import annotations

import logging

import numpy as np

from . import _lib
from .sasa import _coords, _mask

logger = logging.getLogger(__name__)

_F32, _U32 = np.float32, np.uint32
UNITCELLS = ("rectangular", "triclinic", "compact")


class NonContiguousGroups(ValueError):
    """a bonded component that is not one contiguous run of atoms"""


def _np(a):
    return np.asarray(a.cpu() if hasattr(a, "cpu") else a)


def bonded_groups(bonds, n_atoms):
    """The start index of every bonded group and ``n_atoms`` at the end, uint32 ``[G + 1]`` (the reference's ``getBondedGroups``):
    the connected components of the bond graph, which must each be one contiguous run of atoms -- the reference silently assumes
    that; here a component that is not raises ``ValueError``.  ``bonds``: integer ``[n_bonds, 2]`` (or ``None``: no bonds)."""
    n = int(n_atoms)
    if n < 0 or n >= 2 ** 30:
        raise ValueError(f"n_atoms must be in [0, 2^30), got {n_atoms}")
    b = np.zeros((0, 2), np.int64) if bonds is None else _np(bonds)
    if b.size and not np.issubdtype(b.dtype, np.integer):
        raise TypeError(f"bonds must be integer atom indices, got {b.dtype.name}")
    b = b.astype(np.int64).reshape(-1, 2)
    if b.size and (b.min() < 0 or b.max() >= n):
        raise IndexError(f"bonds: atom index out of range for {n} atoms")
    # union-find over all bonds at once: the larger root of every bond is hooked under the smaller, then every path is halved until
    # each atom points at its root; a root is its component's first atom
    parent = np.arange(n, dtype=np.int64)
    while b.size:
        ra, rb = parent[b[:, 0]], parent[b[:, 1]]
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        open_ = lo != hi
        if not open_.any():
            break
        np.minimum.at(parent, hi[open_], lo[open_])
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    if n and np.any(np.diff(parent) < 0):
        bad = int(np.flatnonzero(np.diff(parent) < 0)[0]) + 1
        raise NonContiguousGroups(f"the bonded group of atom {int(parent[bad])} is not one contiguous run of atoms (atom {bad} belongs to it, "
                                  f"atom {bad - 1} does not): wrapping needs every molecule's atoms in a row")
    return np.ascontiguousarray(np.r_[np.flatnonzero(parent == np.arange(n)), n], dtype=_U32)


def _starts(groups, N):
    """group starts [G + 1] -> uint32, checked: from 0, increasing, to N"""
    s = _np(groups)
    if s.size and not np.issubdtype(s.dtype, np.integer):
        raise TypeError(f"groups must be integer group starts, got {s.dtype.name}")
    s = s.astype(np.int64).reshape(-1)
    if N == 0 and s.size <= 1:
        return np.zeros(1, _U32)
    if s.size < 2 or s[0] != 0 or s[-1] != N or np.any(np.diff(s) <= 0):
        raise ValueError(f"groups: the starts must run from 0 to the number of atoms ({N}), increasing (bonded_groups)")
    return np.ascontiguousarray(s, dtype=_U32)


def _groups_or_bonds(g, N):
    a = _np(g) if g is not None else None
    if a is None or a.ndim == 2:
        return bonded_groups(a, N)
    return _starts(a, N)


def _centre_inputs(centersel, center, N):
    """(uint32 indices in the order given, or None; float32 [3] or None) -- a selection or a centre, never both"""
    sel = None
    if centersel is not None:
        a = _np(centersel)
        if a.dtype == bool:
            a = np.flatnonzero(_mask(a, N, "centersel"))
        elif a.size and not np.issubdtype(a.dtype, np.integer):
            raise TypeError("centersel: a boolean mask or an integer index array is required (this package has no selection language)")
        a = a.astype(np.int64).reshape(-1)
        a = np.where(a < 0, a + N, a)
        if a.size and (a.min() < 0 or a.max() >= N):
            raise IndexError(f"centersel: atom index out of range for {N} atoms")
        sel = np.ascontiguousarray(a, dtype=_U32) if a.size else None
    if sel is not None and center is not None:
        raise ValueError("give a centre selection or a centre, not both")
    if sel is None:
        if center is None:
            raise ValueError("a centre selection (of at least one atom) or a centre is required")
        c = np.ascontiguousarray(_np(center), dtype=_F32).reshape(-1)
        if c.shape != (3,):
            raise ValueError(f"center must be three numbers, got shape {c.shape}")
        return None, c
    return sel, None


def _large(starts, ctx):
    """the groups a wave handles instead of a lane: those of more atoms than the library's threshold (under the context's settings)"""
    small_max = int(_lib.load().mkamd_wrap_small_max(ctx._h))
    return np.ascontiguousarray(np.flatnonzero(np.diff(starts.astype(np.int64)) > small_max), dtype=_U32)


def wrap_trajectory(xyz, box, groups, *, centersel=None, center=None, out=None, stream=None, ctx=None):
    """Wrap every frame of a device-resident trajectory into its rectangular cell.  ``xyz``: CUDA float32 ``[F, N, 3]``; ``box``:
    float32 ``[3, F]`` (a CUDA tensor or an array); ``groups``: the group starts ``[G + 1]`` (``bonded_groups``).  The cell is centred
    on the float32 running mean of the atoms ``centersel`` (indices, used in the order given, or a mask) of each unwrapped frame, or
    on the three numbers ``center`` -- exactly one of the two.  ``out is xyz``: in place (groups that do not move are not written);
    ``out=None``: a new tensor; else the given tensor (contiguous, shaped like ``xyz``); ``xyz`` is then untouched.  Returns the
    wrapped tensor.  Asynchronous on ``stream`` (an integer ``hipStream_t``; default torch's current stream).  The bits are the
    reference's ``Molecule.wrap`` (``wrapping.wrap_box``)."""
    import torch

    from .moments import _device_inputs

    inplace = out is xyz
    if inplace and not (hasattr(xyz, "is_contiguous") and xyz.is_contiguous() and xyz.dim() == 3):
        raise ValueError("in place needs a contiguous [frames, atoms, 3] tensor")
    src, _, dev, ctx = _device_inputs(xyz, None, stream, ctx)
    F, N = int(src.shape[0]), int(src.shape[1])
    starts = _starts(groups, N)
    sel, cen = _centre_inputs(centersel, center, N)
    if hasattr(box, "is_cuda"):
        if box.dtype != torch.float32 or tuple(box.shape) != (3, F):
            raise ValueError(f"box must be float32 [3, {F}], got {box.dtype} {tuple(box.shape)}")
        d_box = box.to(dev).contiguous()
    else:
        b = np.asarray(box)
        if b.shape != (3, F):
            raise ValueError(f"box must have shape (3, {F}), got {b.shape}")
        d_box = torch.as_tensor(np.ascontiguousarray(b, dtype=_F32), device=dev)
    if inplace:
        res = src
    elif out is None:
        res = torch.empty_like(src)
    else:
        if not (hasattr(out, "is_cuda") and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == src.shape
                and out.device == src.device):
            raise ValueError("out must be a contiguous float32 CUDA tensor shaped like xyz, on its device")
        if out.data_ptr() == src.data_ptr():
            raise ValueError("out shares xyz's memory: pass out=xyz for an in-place wrap")
        res = out
    if F == 0 or N == 0:
        return res
    large = _large(starts, ctx)
    d_starts = torch.as_tensor(starts.view(np.int32), device=dev)
    d_large = torch.as_tensor(large.view(np.int32), device=dev) if large.size else None
    d_sel = torch.as_tensor(sel.view(np.int32), device=dev) if sel is not None else None
    if stream is not None and hasattr(box, "is_cuda"):
        torch.cuda.current_stream(dev).synchronize()           # (a conversion of box ran on torch's stream; the kernels go to a foreign one)
    _lib._check(_lib.load().mkamd_wrap_box_dev(ctx._h, src.data_ptr(), N, F, d_box.data_ptr(), d_starts.data_ptr(), int(starts.size) - 1,
                                               d_large.data_ptr() if d_large is not None else None, int(large.size),
                                               d_sel.data_ptr() if d_sel is not None else None, 0 if sel is None else int(sel.size),
                                               _lib._ptr(cen), res.data_ptr()))
    if stream is not None:
        ctx.synchronize()          # (the index tensors are torch's: their memory must not be reused before a foreign stream has read it)
    return res


def travel_rows(starts, named, centersel):
    """The atoms that must travel so that the atoms ``named`` come back wrapped: every atom of each group that holds a named atom,
    plus the centre selection's atoms.  Returns ``(rows uint32 ascending, starts of the groups among the rows uint32)``.  Wrapping is
    independent per group, so the named atoms get the bits that wrapping everything gives them (a centre atom whose group did not
    come along is wrapped with what is there of its group: it is not one of the named atoms)."""
    starts = np.asarray(starts, np.int64)
    N = int(starts[-1])
    named = np.unique(np.asarray(named, np.int64).reshape(-1))
    gid_named = np.unique(np.searchsorted(starts, named, side="right") - 1)
    take = np.zeros(N, bool)
    for a, b in zip(starts[gid_named], starts[gid_named + 1]):
        take[a:b] = True
    if centersel is not None and len(centersel):
        take[np.asarray(centersel, np.int64)] = True
    rows = np.flatnonzero(take)
    gid = np.searchsorted(starts, rows, side="right") - 1
    packed = np.r_[0, np.flatnonzero(np.diff(gid)) + 1, rows.size]
    return np.ascontiguousarray(rows, dtype=_U32), np.ascontiguousarray(packed, dtype=_U32)


def _box(box, F):
    b = np.asarray(box)
    if b.ndim == 1:
        b = b[:, None]
    if b.shape != (3, F):
        raise ValueError(f"box must have shape (3, {F}), got {b.shape}")
    return np.ascontiguousarray(b, dtype=_F32)


def wrap(coords, box, groups_or_bonds, centersel=None, center=None, rows=None, ctx=None):
    """``wrap_trajectory`` on host arrays in the reference's layout: ``coords`` float32 ``[N, 3, F]`` (``Molecule.coords``), ``box``
    ``[3, F]``; ``groups_or_bonds``: the group starts ``[G + 1]`` or a bond list ``[n_bonds, 2]`` (``None``: no bonds).  Returns a
    wrapped copy ``[N, 3, F]``.  With ``rows`` (indices or a mask: the atoms the caller needs) only those atoms' groups and the
    centre selection travel to the device, and the wrapped rows of exactly the atoms named come back, ``[len(rows), 3, F]`` in the
    order given -- the same bits as the rows of wrapping everything."""
    coords = _coords(coords)
    N, _, F = coords.shape
    box = _box(box, F)
    starts = _groups_or_bonds(groups_or_bonds, N)
    sel, cen = _centre_inputs(centersel, center, N)
    if rows is None:
        out = np.empty_like(coords)
        if N == 0 or F == 0:
            return out
        ctx = ctx or _lib.default_context()
        _lib._check(_lib.load().mkamd_wrap_box_host(ctx._h, _lib._ptr(coords), N, F, _lib._ptr(box), None, 0, _lib._ptr(starts), int(starts.size) - 1,
                                                    _lib._ptr(sel), 0 if sel is None else int(sel.size), _lib._ptr(cen), _lib._ptr(out)))
        return out
    r = _np(rows)
    if r.dtype == bool:
        named = np.flatnonzero(_mask(r, N, "rows"))
    else:
        _mask(r, N, "rows")                                     # (the checks: integers, in range)
        named = r.astype(np.int64).reshape(-1)
        named = np.where(named < 0, named + N, named)
    if named.size == 0 or F == 0:
        return np.empty((int(named.size), 3, F), _F32)
    travel, packed = travel_rows(starts, named, sel)
    out = np.empty((int(travel.size), 3, F), _F32)
    ctx = ctx or _lib.default_context()
    _lib._check(_lib.load().mkamd_wrap_box_host(ctx._h, _lib._ptr(coords), N, F, _lib._ptr(box), _lib._ptr(travel), int(travel.size),
                                                _lib._ptr(packed), int(packed.size) - 1, _lib._ptr(sel), 0 if sel is None else int(sel.size),
                                                _lib._ptr(cen), _lib._ptr(out)))
    return np.ascontiguousarray(out[np.searchsorted(travel, named)])


# ------------------------------------------------------------------------------------------------
# Molecule.wrap
# ------------------------------------------------------------------------------------------------
_ZERO_BOX = ("Zero box size detected in `Molecule.box`; skipping wrap. Read a topology / trajectory containing box information, "
             "or set `mol.box` and `mol.boxangles` manually before calling `wrap`.")
_FRAMES = ("Detected different number of simulation frames in `Molecule.box` and `Molecule.coords`. "
           "This could mean that you have not read correctly the box information from the simulation.")


def _select(mol, sel, N, guess_bonds):
    """the centre selection as indices: a mask or an index array; ``"all"``; any other string only through the molecule's own
    ``atomselect`` (an installed moleculekit's)"""
    if isinstance(sel, str):
        if sel == "all":
            return np.arange(N, dtype=_U32)
        if not hasattr(mol, "atomselect"):
            raise TypeError("wrapsel: a boolean mask or an integer index array is required (this package has no selection language)")
        return np.asarray(mol.atomselect(sel, indexes=True, guessBonds=guess_bonds)).astype(_U32)
    a = _np(sel)
    if a.dtype == bool:
        return np.flatnonzero(_mask(a, N, "wrapsel")).astype(_U32)
    _mask(a, N, "wrapsel")                                      # (the checks: integers, in range)
    a = a.astype(np.int64).reshape(-1)
    return np.where(a < 0, a + N, a).astype(_U32)


def wrap_molecule(mol, wrapsel="all", fileBonds=True, guessBonds=False, wrapcenter=None, unitcell="rectangular", ctx=None):
    """The reference's ``Molecule.wrap`` for rectangular cells, on the GPU: ``mol.coords`` (float32 ``[N, 3, F]``) is wrapped in place
    around the atoms ``wrapsel`` (a mask or an index array; ``"all"``) or around ``wrapcenter``, by the bonded groups of ``mol.bonds``
    (``fileBonds=False``: every atom on its own).  As the reference: ``ValueError`` for an unknown ``unitcell``, a warning and no
    change when the whole box is zero, ``RuntimeError`` when box and coordinates differ in their number of frames.  Unlike it:
    ``guessBonds=True`` and any ``boxangles`` other than 90 raise ``NotImplementedError`` -- the triclinic modes "rectangular",
    "triclinic" and "compact" are not on the device --, a bonded group that is not contiguous raises ``ValueError``."""
    unitcell = unitcell.lower()
    if unitcell not in UNITCELLS:
        raise ValueError(f"Invalid unit cell type: {unitcell}. Must be one of: rectangular, triclinic, compact")
    coords = np.asarray(mol.coords)
    N = int(coords.shape[0])
    bonds = np.asarray(mol.bonds).reshape(-1, 2) if getattr(mol, "bonds", None) is not None else np.zeros((0, 2), _U32)
    nbonds = int(bonds.shape[0])
    guess_sel = bool(guessBonds)
    if nbonds < N / 2:
        logger.warning(f"Wrapping detected {nbonds} bonds and {N} atoms. Ignore this message if you believe this is correct, otherwise make "
                       "sure you have loaded a topology containing all the bonds of the system before wrapping. The results may be "
                       "inaccurate. If you want to use guessed bonds use the guessBonds argument.")
        guess_sel = True
    centersel, center = None, None
    if wrapcenter is None:
        centersel = _select(mol, wrapsel, N, guess_sel)
        if centersel.size == 0:
            center = np.zeros(3, _F32)                          # (the reference's centre of an empty selection)
    else:
        center = np.array(wrapcenter, dtype=_F32)
    box = np.asarray(mol.box)
    if np.all(box == 0):
        logger.warning(_ZERO_BOX)
        return
    if box.shape[1] != coords.shape[2]:
        raise RuntimeError(_FRAMES)
    if guessBonds:
        raise NotImplementedError("guessBonds=True: this package does not guess bonds; pass a molecule whose bonds are read from a topology")
    angles = getattr(mol, "boxangles", None)
    if angles is not None and np.size(angles) and np.any(np.asarray(angles) != 90):
        raise NotImplementedError("the box is triclinic (boxangles != 90): the unit cells 'rectangular', 'triclinic' and 'compact' of a "
                                  "triclinic box are not wrapped on the device; use the reference's Molecule.wrap")
    groups = bonded_groups(bonds if fileBonds else None, N)
    mol.coords[...] = wrap(np.ascontiguousarray(coords, dtype=_F32), box, groups, centersel=centersel if center is None else None, center=center,
                           ctx=ctx)


def _molecule_wrap(self, wrapsel="all", fileBonds=True, guessBonds=False, wrapcenter=None, unitcell="rectangular"):
    """``Molecule.wrap`` once ``install()``-ed: the device for rectangular cells; the saved original for triclinic boxes, guessed bonds
    and bonded groups that are not contiguous"""
    import moleculekit.molecule as ref

    original = ref._mkamd_reference_wrap
    angles = getattr(self, "boxangles", None)
    triclinic = angles is not None and np.size(angles) and np.any(np.asarray(angles) != 90)
    if guessBonds or triclinic or not isinstance(unitcell, str) or unitcell.lower() not in UNITCELLS:
        return original(self, wrapsel, fileBonds, guessBonds, wrapcenter, unitcell)
    try:
        if fileBonds:
            bonded_groups(self.bonds, int(np.asarray(self.coords).shape[0]))
    except NonContiguousGroups:
        return original(self, wrapsel, fileBonds, guessBonds, wrapcenter, unitcell)
    return wrap_molecule(self, wrapsel, fileBonds, guessBonds, wrapcenter, unitcell)


def install():
    """Swap ``Molecule.wrap`` of an installed moleculekit for the GPU's: the reference's own projections (``mol.wrap(centersel)``,
    then ``mol.align(...)``) and everything else built on ``Molecule.wrap`` then wrap on the device.  Triclinic boxes,
    ``guessBonds=True`` and molecules whose bonded groups are not contiguous go to the saved original.  Returns the original;
    idempotent; ``uninstall()`` puts it back.  Independent of the other ``install()`` hooks."""
    import moleculekit.molecule as ref

    saved = getattr(ref, "_mkamd_reference_wrap", None)
    if saved is not None:
        return saved
    saved = ref.Molecule.wrap
    ref._mkamd_reference_wrap = saved
    ref.Molecule.wrap = _molecule_wrap
    return saved


def uninstall():
    """Undo ``install()``."""
    import moleculekit.molecule as ref

    saved = getattr(ref, "_mkamd_reference_wrap", None)
    if saved is not None:
        ref.Molecule.wrap = saved
        ref._mkamd_reference_wrap = None
