"""Periodic wrapping of trajectories on the MI355X (include/mkamd_distance.h "periodic wrap").

The reference's ``Molecule.wrap`` moves every bonded group of every frame by whole box lengths back to within half a box of a centre
-- the first step of every projection it offers (``mol.wrap(centersel)``, then ``mol.align(...)``) -- in a serial loop on the host.
Here the same arithmetic, to the bit, runs on the device (csrc/wrap_kernels.h): the centres are float32 running means in atom
order, so a group on the cell's boundary lands where the reference puts it.  Rectangular boxes take ``wrap_box``'s kernels; triclinic
boxes (a box angle other than 90) take the reference's three unit cells -- "rectangular", "compact", "triclinic" -- through
csrc/wrap_cell_kernels.h, opted into with ``wrap_molecule(..., triclinic_on_device=True)`` or ``install(triclinic=True)``.

* ``bonded_groups(bonds, n_atoms)`` -- the starts of the bonded groups (the reference's ``getBondedGroups``), on the host.
* ``wrap_trajectory`` -- CUDA tensors, frame-major ``[F, N, 3]`` float32 and a ``[3, F]`` box; asynchronous; in place or not.
* ``wrap`` -- numpy arrays ``[N, 3, F]`` through the host entry point (``rows``: only the atoms that matter travel).
* ``box_vectors`` -- box lengths and angles to the float64 box vectors ``[3, 3, F]`` (the reference's ``Molecule.boxvectors``).
* ``wrap_cell_trajectory`` / ``wrap_cell`` -- the same two forms for triclinic boxes: box vectors and a unit cell.  Where the reference's
  loops would not end (an infinite coordinate, a degenerate box) these stop after ``WRAP_CELL_MAX_STEPS`` steps and raise.
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
_F64 = np.float64
CELL_MODES = {"rectangular": 0, "compact": 1, "triclinic": 2}    # csrc/wrap_cell_kernels.h: WRAP_CELL_*
WRAP_CELL_MAX_STEPS = 4096                                        # ... WRAP_CELL_MAX_STEPS (mkamd_wrap_cell_max_steps)
_STATUS_ERRORS = (                                                # ... WRAP_CELL_ST_*, in the order they are reported
    (2, "Too many triclinic vectors!!"),
    (1, "wrap: a frame's box vectors are degenerate (non-finite, box[1][1] or box[2][2] not positive, or not lower triangular); the frame "
        "was copied through unchanged"),
    (0, f"wrap: a group did not come into the cell within {WRAP_CELL_MAX_STEPS} steps (an infinite coordinate, or a box length far below "
        "the coordinates); it was written with what was reached"),
)


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
# triclinic boxes
# ------------------------------------------------------------------------------------------------
def box_vectors(box, boxangles):
    """The box vectors of every frame, float64 ``[3, 3, F]`` (row i: vector i; lower triangular), from the box lengths ``[3, F]`` and the
    angles ``[3, F]`` (alpha, beta, gamma in degrees) -- the reference's ``Molecule.boxvectors``: float64 throughout, its order of
    operations, components within 1e-6 of zero set to 0.  All zeros when lengths and angles are all zero; ``AssertionError`` when an
    angle is 0."""
    b, ang = np.asarray(box), np.asarray(boxangles)
    if b.ndim == 1:
        b = b[:, None]
    if ang.ndim == 1:
        ang = ang[:, None]
    if b.ndim != 2 or b.shape[0] != 3 or ang.shape != b.shape:
        raise ValueError(f"box and boxangles must both have shape (3, frames), got {b.shape} and {ang.shape}")
    F = b.shape[1]
    if np.all(ang == 0) and np.all(b == 0):
        return np.zeros((3, 3, F), _F64)
    assert np.all(ang != 0), "Box angles should not be 0"
    a_len, b_len, c_len = (b[i].astype(_F64) for i in range(3))
    alpha, beta, gamma = (ang[i].astype(_F64) * np.pi / 180 for i in range(3))
    out = np.zeros((3, 3, F), _F64)
    out[0, 0] = a_len
    out[1, 0] = b_len * np.cos(gamma)
    out[1, 1] = b_len * np.sin(gamma)
    cx = c_len * np.cos(beta)
    cy = c_len * (np.cos(alpha) - np.cos(beta) * np.cos(gamma)) / np.sin(gamma)
    with np.errstate(invalid="ignore"):
        cz = np.sqrt(c_len * c_len - cx * cx - cy * cy)
    out[2, 0], out[2, 1], out[2, 2] = cx, cy, cz
    tol = 1e-6
    out[np.logical_and(out > -tol, out < tol)] = 0.0
    return out


def _check_boxvectors(bv):
    """what the library checks before it launches (csrc/wrap_cell_pipeline.h: wrap_cell_check_boxvectors), on a host array [3, 3, F]"""
    if not np.all(np.isfinite(bv)):
        raise ValueError("box vectors: a component is not finite")
    if not (np.all(bv[1, 1] > 0) and np.all(bv[2, 2] > 0)):
        raise ValueError("box vectors: box[1][1] and box[2][2] must be positive")
    if np.any(bv[0, 1] != 0) or np.any(bv[0, 2] != 0) or np.any(bv[1, 2] != 0):
        raise ValueError("box vectors: not lower triangular (box[0][1], box[0][2], box[1][2] must be 0)")


def _host_boxvectors(boxvectors, F):
    bv = np.asarray(boxvectors)
    if bv.ndim == 2:
        bv = bv[:, :, None]
    if bv.shape != (3, 3, F):
        raise ValueError(f"boxvectors must have shape (3, 3, {F}), got {bv.shape}")
    return np.array(bv, dtype=_F64, order="C")                 # (a copy: 72 B a frame, and the caller's array may be read-only)


def _cell_mode(unitcell):
    if not isinstance(unitcell, str) or unitcell.lower() not in CELL_MODES:
        raise ValueError(f"Invalid unit cell type: {unitcell}. Must be one of: rectangular, triclinic, compact")
    return CELL_MODES[unitcell.lower()]


def status_error(status):
    """the message of the first condition set in the three status words of a cell wrap, or None"""
    st = [int(v) for v in np.asarray(status).reshape(-1)[:3]]
    for word, text in _STATUS_ERRORS:
        if st[word]:
            return text
    return None


def wrap_cell_trajectory(xyz, boxvectors, groups, unitcell, *, centersel=None, center=None, out=None, stream=None, ctx=None, check=True):
    """Wrap every frame of a device-resident trajectory into a unit cell of its triclinic box.  ``xyz``: CUDA float32 ``[F, N, 3]``;
    ``boxvectors``: float64 ``[3, 3, F]`` (``box_vectors``; an array or a CUDA tensor); ``groups``, ``centersel`` / ``center``, ``out`` and
    ``stream`` as in ``wrap_trajectory``; ``unitcell``: "rectangular", "compact" or "triclinic" -- the reference's three modes of
    ``Molecule.wrap`` for a box whose angles are not all 90.  Every atom is written (each frame is recentred first), in place as well.
    The box vectors are checked before anything is launched (an array always; a CUDA tensor when ``check``): ``ValueError``.
    ``check=True``: the call synchronises, reads the status words and raises ``ValueError`` where the reference's loops would not have
    ended (a group that did not come into the cell within ``WRAP_CELL_MAX_STEPS`` steps), a frame was degenerate or had more than 12
    triclinic vectors; it returns the wrapped tensor.  ``check=False``: asynchronous; returns ``(tensor, status)`` with ``status`` a CUDA
    int32 tensor of three words (``status_error``).  The bits are the reference's ``wrap_triclinic_unitcell`` / ``wrap_compact_unitcell``."""
    import torch

    from .moments import _device_inputs

    mode = _cell_mode(unitcell)
    inplace = out is xyz
    if inplace and not (hasattr(xyz, "is_contiguous") and xyz.is_contiguous() and xyz.dim() == 3):
        raise ValueError("in place needs a contiguous [frames, atoms, 3] tensor")
    src, _, dev, ctx = _device_inputs(xyz, None, stream, ctx)
    F, N = int(src.shape[0]), int(src.shape[1])
    starts = _starts(groups, N)
    sel, cen = _centre_inputs(centersel, center, N)
    if hasattr(boxvectors, "is_cuda"):
        if boxvectors.dtype != torch.float64 or tuple(boxvectors.shape) != (3, 3, F):
            raise ValueError(f"boxvectors must be float64 [3, 3, {F}], got {boxvectors.dtype} {tuple(boxvectors.shape)}")
        if check:
            _check_boxvectors(boxvectors.detach().cpu().numpy())
        d_bv = boxvectors.to(dev).contiguous()
    else:
        bv = _host_boxvectors(boxvectors, F)
        _check_boxvectors(bv)
        d_bv = torch.as_tensor(bv, device=dev)
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
    status = torch.zeros(3, dtype=torch.int32, device=dev)
    if F == 0 or N == 0:
        return res if check else (res, status)
    large = _large(starts, ctx)
    d_starts = torch.as_tensor(starts.view(np.int32), device=dev)
    d_large = torch.as_tensor(large.view(np.int32), device=dev) if large.size else None
    d_sel = torch.as_tensor(sel.view(np.int32), device=dev) if sel is not None else None
    if stream is not None:
        torch.cuda.current_stream(dev).synchronize()           # (status and a conversion of the box vectors ran on torch's stream)
    _lib._check(_lib.load().mkamd_wrap_cell_dev(ctx._h, src.data_ptr(), N, F, d_bv.data_ptr(), d_starts.data_ptr(), int(starts.size) - 1,
                                                d_large.data_ptr() if d_large is not None else None, int(large.size),
                                                d_sel.data_ptr() if d_sel is not None else None, 0 if sel is None else int(sel.size),
                                                _lib._ptr(cen), mode, res.data_ptr(), status.data_ptr()))
    if stream is not None:
        ctx.synchronize()          # (the index tensors are torch's: their memory must not be reused before a foreign stream has read it)
    if not check:
        return res, status
    ctx.synchronize()
    message = status_error(status.cpu().numpy())
    if message:
        raise ValueError(message)
    return res


def wrap_cell(coords, boxvectors, groups_or_bonds, unitcell, centersel=None, center=None, rows=None, ctx=None):
    """``wrap_cell_trajectory`` on host arrays in the reference's layout: ``coords`` float32 ``[N, 3, F]``, ``boxvectors`` float64
    ``[3, 3, F]``; ``groups_or_bonds`` and ``rows`` as in ``wrap``.  Returns a wrapped copy (of the rows named, with ``rows``).  The box
    vectors are checked first; a status word set by the run raises ``ValueError`` with the condition's name."""
    mode = _cell_mode(unitcell)
    coords = _coords(coords)
    N, _, F = coords.shape
    bv = _host_boxvectors(boxvectors, F)
    _check_boxvectors(bv)
    starts = _groups_or_bonds(groups_or_bonds, N)
    sel, cen = _centre_inputs(centersel, center, N)

    def run(travel, n_travel, packed, out):
        h = (ctx or _lib.default_context())._h                  # (a status word set by the run comes back as MKAMD_EINVAL: ValueError)
        _lib._check(_lib.load().mkamd_wrap_cell_host(h, _lib._ptr(coords), N, F, _lib._ptr(bv), _lib._ptr(travel), n_travel, _lib._ptr(packed),
                                                     int(packed.size) - 1, _lib._ptr(sel), 0 if sel is None else int(sel.size),
                                                     _lib._ptr(cen), mode, _lib._ptr(out)))

    if rows is None:
        out = np.empty_like(coords)
        if N == 0 or F == 0:
            return out
        run(None, 0, starts, out)
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
    run(travel, int(travel.size), packed, out)
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


def _all_bonds(mol, file_bonds, fileBonds, ctx=None):
    """the reference's ``_getBonds(fileBonds, True)``: the file bonds, if wanted, on top of the bonds guessed on the device"""
    from . import bonds as _bonds

    guessed = _bonds.guess_bonds(mol, ctx=ctx)
    return np.vstack((file_bonds.astype(_U32), guessed)) if fileBonds else guessed


def wrap_molecule(mol, wrapsel="all", fileBonds=True, guessBonds=False, wrapcenter=None, unitcell="rectangular", ctx=None, *,
                  triclinic_on_device=False, guess_on_device=False):
    """The reference's ``Molecule.wrap`` on the GPU: ``mol.coords`` (float32 ``[N, 3, F]``) is wrapped in place around the atoms
    ``wrapsel`` (a mask or an index array; ``"all"``) or around ``wrapcenter``, by the bonded groups of ``mol.bonds``
    (``fileBonds=False``: every atom on its own).  As the reference: ``ValueError`` for an unknown ``unitcell``, a warning and no
    change when the whole box is zero, ``RuntimeError`` when box and coordinates differ in their number of frames.  Unlike it:
    ``guessBonds=True`` raises ``NotImplementedError`` unless ``guess_on_device=True`` -- then the groups are those of the reference's
    ``_getBonds(fileBonds, guessBonds)``: the file bonds (if ``fileBonds``) stacked on top of ``bonds.guess_bonds(mol)``, the bonds of
    frame ``mol.frame`` guessed on the device --, a bonded group that is not contiguous raises ``ValueError``, and a triclinic
    box (any ``boxangles`` other than 90 in any frame) raises ``NotImplementedError`` unless ``triclinic_on_device=True``: then, as in
    the reference, the whole call takes ``wrap_cell`` with ``box_vectors(mol.box, mol.boxangles)`` and ``unitcell`` ("rectangular",
    "triclinic" or "compact"); a box whose angles are all 90 takes ``wrap`` whatever ``unitcell`` says."""
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
    if guessBonds and not guess_on_device:
        raise NotImplementedError("guessBonds=True: this package does not guess bonds; pass a molecule whose bonds are read from a topology")
    angles = getattr(mol, "boxangles", None)
    triclinic = angles is not None and np.size(angles) and bool(np.any(np.asarray(angles) != 90))
    if triclinic and not triclinic_on_device:
        raise NotImplementedError("the box is triclinic (boxangles != 90): the unit cells 'rectangular', 'triclinic' and 'compact' of a "
                                  "triclinic box are not wrapped on the device; use the reference's Molecule.wrap")
    groups = bonded_groups(_all_bonds(mol, bonds, fileBonds, ctx) if guessBonds else (bonds if fileBonds else None), N)
    if triclinic:
        mol.coords[...] = wrap_cell(np.ascontiguousarray(coords, dtype=_F32), box_vectors(box, angles), groups, unitcell,
                                    centersel=centersel if center is None else None, center=center, ctx=ctx)
        return
    mol.coords[...] = wrap(np.ascontiguousarray(coords, dtype=_F32), box, groups, centersel=centersel if center is None else None, center=center,
                           ctx=ctx)


def _molecule_wrap(self, wrapsel="all", fileBonds=True, guessBonds=False, wrapcenter=None, unitcell="rectangular"):
    """``Molecule.wrap`` once ``install()``-ed: the device for rectangular boxes and, after ``install(triclinic=True)``, triclinic ones
    and, after ``install(guess=True)``, guessed bonds; the saved original for bonded groups that are not contiguous and (by default)
    guessed bonds and triclinic boxes"""
    import moleculekit.molecule as ref

    original = ref._mkamd_reference_wrap
    angles = getattr(self, "boxangles", None)
    on_device = bool(getattr(ref, "_mkamd_wrap_triclinic", False))
    triclinic = angles is not None and np.size(angles) and np.any(np.asarray(angles) != 90) and not on_device
    guess = bool(getattr(ref, "_mkamd_wrap_guess", False))
    if (guessBonds and not guess) or triclinic or not isinstance(unitcell, str) or unitcell.lower() not in UNITCELLS:
        return original(self, wrapsel, fileBonds, guessBonds, wrapcenter, unitcell)
    try:
        if guessBonds:
            return wrap_molecule(self, wrapsel, fileBonds, guessBonds, wrapcenter, unitcell, triclinic_on_device=on_device, guess_on_device=True)
        if fileBonds:
            bonded_groups(self.bonds, int(np.asarray(self.coords).shape[0]))
    except NonContiguousGroups:
        return original(self, wrapsel, fileBonds, guessBonds, wrapcenter, unitcell)
    return wrap_molecule(self, wrapsel, fileBonds, guessBonds, wrapcenter, unitcell, triclinic_on_device=on_device)


def install(triclinic=False, guess=False):
    """Swap ``Molecule.wrap`` of an installed moleculekit for the GPU's: the reference's own projections (``mol.wrap(centersel)``,
    then ``mol.align(...)``) and everything else built on ``Molecule.wrap`` then wrap on the device.  ``guessBonds=True`` and
    molecules whose bonded groups are not contiguous go to the saved original, and so do triclinic boxes unless ``triclinic=True``
    (the last call's value holds).  ``guess=True`` keeps ``guessBonds=True`` calls on the device too (``bonds.guess_bonds``); they fall
    back to the original only where the groups are not contiguous (the last call's value holds).  Returns the original; idempotent;
    ``uninstall()`` puts it back and clears the flags.  Independent of the other ``install()`` hooks."""
    import moleculekit.molecule as ref

    ref._mkamd_wrap_triclinic = bool(triclinic)
    ref._mkamd_wrap_guess = bool(guess)
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
    ref._mkamd_wrap_triclinic = False
    ref._mkamd_wrap_guess = False
    if saved is not None:
        ref.Molecule.wrap = saved
        ref._mkamd_reference_wrap = None
