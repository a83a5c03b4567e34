"""Bond guessing on the MI355X (include/mkamd_distance.h "bond guesser").

The reference's ``moleculekit.bondguesser.bond_grid_search`` bins the atoms of one frame into a grid in a Python loop and calls a
compiled pair loop once per occupied box.  Here the grid, the cell list and the pair test run on the device, and the list comes back
in the reference's ORDER: the same rows ``(i, j)``, row for row.  Every float32 operation is the reference's -- the box of an atom, the
squared distance, the two cut-offs -- so nothing is compared with a tolerance.

* ``bond_radii`` -- the radii of a molecule's atoms: the reference's per-element table, the defaults by atom name, 1.5.
* ``bond_grid`` -- the grid alone, on the host: boxes per axis and the box side after the reference's escalation loop.
* ``guess_bonds_tensor`` -- CUDA tensors in, an int32 ``[n, 2]`` CUDA tensor out.
* ``bond_grid_search`` / ``guess_bonds`` -- the reference's two functions: signatures, defaults, errors, uint32 ``[n, 2]``;
  ``install()`` / ``uninstall()`` swap them into an installed moleculekit, whose ``Molecule._guessBonds`` (and with it ``atomselect``,
  ``guessBonds()`` and ``wrap``) then guesses on the device.

One frame, a non-periodic grid, as in the reference.  A grid box may hold at most ``BOX_CAP`` atoms (the reference's escalation looks
at the NUMBER of boxes only, so coincident atoms pile up in one box): a frame that exceeds it raises ``ValueError`` naming the box.
There is no CPU path: without the library or a device every entry point raises.
"""
from __future__ import annotations

import logging

import numpy as np

from . import _lib
from ._bond_radii import BOND_RADII, FALLBACK, NAME_DEFAULTS

logger = logging.getLogger(__name__)

_F32, _U32 = np.float32, np.uint32
BOX_CAP = 4096                       # csrc/bond_kernels.h: BOND_BOX_CAP
AVOID_THREAD, AVOID_WAVE = 1, 2      # csrc/bond_pipeline.h: Context.set_bond_plan

_UNWRAPPED = ("It seems like you might be guessing bonds on an unwrapped simulation. "
              "This can consume large amounts of memory and possibly crash. If you already have "
              "all the bonds in Molecule pass `guessBonds=False` to the function or perform "
              "the bond guessing on a wrapped frame.")
_NONFINITE = "bond_grid_search received non-finite coordinates (NaN or inf). Coordinates must be finite."


def _bad_cutoff(grid_cutoff):
    return f"bond_grid_search requires a positive, finite grid_cutoff; got {grid_cutoff!r}."


def bond_radii(element, name):
    """float32 ``[N]``: per atom the table's radius of its element (``_bond_radii.BOND_RADII``; the keys are capitalised, so "CL" is
    not in it), else the default of the upper-cased first letter of its NAME (H, C, N, O, F, S), else 1.5."""
    out = np.empty(len(element), dtype=_F32)
    for i, el in enumerate(element):
        r = BOND_RADII.get(str(el))
        if r is None:
            r = NAME_DEFAULTS.get(str(name[i])[0].upper(), FALLBACK)
        out[i] = r
    return out


def bond_grid(min_c, max_c, grid_cutoff, max_boxes=4e6, cutoff_incr=1.26):
    """The reference's grid over the corners ``min_c`` / ``max_c`` (float32 ``[3]``): ``(nx, ny, nz, pairdist)``.  The boxes per
    axis are ``floor(range / pairdist) + 1`` with the range and the division in float32 and the counts Python integers; ``pairdist``
    starts at ``float(grid_cutoff)`` and is multiplied by ``cutoff_incr`` in double while the product of the counts exceeds
    ``max_boxes``."""
    if not (grid_cutoff > 0 and np.isfinite(grid_cutoff)):
        raise ValueError(_bad_cutoff(grid_cutoff))
    span = np.asarray(max_c, dtype=_F32) - np.asarray(min_c, dtype=_F32)
    pairdist = float(grid_cutoff)
    while True:
        with np.errstate(all="ignore"):
            quot = np.floor(span / _F32(pairdist))
        if np.all(np.isfinite(quot)) and np.all(quot < 4.0e18):
            nx, ny, nz = (int(q) + 1 for q in quot)
            if nx * ny * nz <= max_boxes:
                return nx, ny, nz, pairdist
        pairdist *= cutoff_incr
        if not np.isfinite(pairdist):
            raise ValueError(_bad_cutoff(grid_cutoff))


def _library_error(e, grid_cutoff):
    """the library's EINVAL messages as the reference's errors"""
    msg = str(e)
    if "non-finite coordinates" in msg:
        return ValueError(_NONFINITE)
    if "grid_cutoff" in msg:
        return ValueError(_bad_cutoff(grid_cutoff) + f" ({msg})")
    return ValueError(msg)


def _after(grid):
    if grid[0] * grid[1] * grid[2] > 1e6:
        logger.warning(_UNWRAPPED)


def guess_bonds_tensor(coords, radii, is_hydrogen, grid_cutoff=None, max_boxes=4e6, cutoff_incr=1.26, *, stream=None, ctx=None):
    """The bonds of device-resident atoms.  ``coords``: CUDA float32 ``[N, 3]``; ``radii``: CUDA float32 ``[N]``; ``is_hydrogen``: CUDA
    ``[N]`` of bool, uint8 or int32 (non-zero: a hydrogen; two hydrogens never bond).  ``grid_cutoff``: the first box side, default
    ``max(radii) * 1.2`` in float32 as the reference's ``guess_bonds`` takes it.  Returns the int32 CUDA ``[n, 2]`` rows ``(i, j)`` in
    the reference's order.  Runs on ``stream`` (an integer ``hipStream_t``; default torch's current stream) and returns when the list is
    complete: the grid, the occupancies and the size of the list reach the host on the way.  ``ValueError``: non-finite coordinates, a
    ``grid_cutoff`` that is not positive and finite, a box with more than ``BOX_CAP`` atoms."""
    import torch

    for nm, t in (("coords", coords), ("radii", radii), ("is_hydrogen", is_hydrogen)):
        if not (hasattr(t, "is_cuda") and t.is_cuda):
            raise TypeError(f"{nm}: a CUDA tensor is required (there is no CPU path)")
    if coords.dtype != torch.float32 or radii.dtype != torch.float32:
        raise ValueError(f"coords and radii must be float32, got {coords.dtype} and {radii.dtype}")
    if coords.dim() != 2 or coords.shape[1] != 3:
        raise ValueError(f"coords must be (natoms, 3), got shape {tuple(coords.shape)}")
    N = int(coords.shape[0])
    if tuple(radii.shape) != (N,) or tuple(is_hydrogen.shape) != (N,):
        raise ValueError(f"radii and is_hydrogen must have shape ({N},), got {tuple(radii.shape)} and {tuple(is_hydrogen.shape)}")
    if radii.device != coords.device or is_hydrogen.device != coords.device:
        raise ValueError("coords, radii and is_hydrogen live on different devices")
    dev = coords.device
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if ctx is not None and ctx.device != idx:
        raise ValueError(f"ctx lives on GPU {ctx.device} but the tensors are on cuda:{idx}")
    dev = torch.device("cuda", idx)
    empty = torch.empty((0, 2), dtype=torch.int32, device=dev)
    if grid_cutoff is None:
        if N == 0:
            return empty
        grid_cutoff = float(_F32(radii.max().item()) * 1.2)        # (float32 scalar times a Python float: float32)
    if not (grid_cutoff > 0 and np.isfinite(grid_cutoff)):
        raise ValueError(_bad_cutoff(grid_cutoff))
    if N == 0:
        return empty
    coords, radii = coords.contiguous(), radii.contiguous()
    flags = (is_hydrogen != 0).to(torch.int32).contiguous()
    ctx = ctx or _lib.default_context(idx)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream if stream is None else int(stream))
    try:
        try:
            p_pairs, n, grid = ctx.guess_bonds_dev(coords, radii, flags, N, float(grid_cutoff), float(max_boxes), float(cutoff_incr))
        except ValueError as e:                 # (MKAMD_EINVAL)
            raise _library_error(e, grid_cutoff) from None
        pairs = torch.empty((n, 2), dtype=torch.int32, device=dev)
        if n:                                   # the list is context-owned until the next bond call: a device-to-device copy keeps it
            _lib._check(_lib.load().mkamd_copy_dev(ctx._h, pairs.data_ptr(), p_pairs, n * 8))
        ctx.synchronize()
    finally:
        ctx.set_stream(None)
    _after(grid)
    return pairs


def bond_grid_search(coords, grid_cutoff, is_hydrogen, radii, max_boxes=4e6, cutoff_incr=1.26, ctx=None):
    """The reference's ``bond_grid_search`` on the GPU: host ``coords`` ``[N, 3]``, ``is_hydrogen`` ``[N]`` flags and ``radii`` ``[N]``
    -> uint32 ``[n, 2]``, its rows in its order.  ``ValueError`` for non-finite coordinates and for a ``grid_cutoff`` that is not
    positive and finite, with the reference's messages; also for a grid box of more than ``BOX_CAP`` atoms."""
    coords = np.asarray(coords)
    if not np.isfinite(coords).all():
        raise ValueError(_NONFINITE)
    if not (grid_cutoff > 0 and np.isfinite(grid_cutoff)):
        raise ValueError(_bad_cutoff(grid_cutoff))
    if coords.ndim != 2 or coords.shape[1] != 3:
        raise ValueError(f"coords must be (natoms, 3), got shape {coords.shape}")
    N = coords.shape[0]
    radii, is_hydrogen = np.asarray(radii), np.asarray(is_hydrogen)
    if radii.shape != (N,) or is_hydrogen.shape != (N,):
        raise ValueError(f"radii and is_hydrogen must have shape ({N},), got {radii.shape} and {is_hydrogen.shape}")
    if N == 0:
        return np.zeros((0, 2), dtype=_U32)
    pairs, grid = _host_call(np.ascontiguousarray(coords, dtype=_F32), np.ascontiguousarray(radii, dtype=_F32),
                             np.ascontiguousarray(is_hydrogen != 0, dtype=_U32), float(grid_cutoff), float(max_boxes), float(cutoff_incr), ctx)
    _after(grid)
    return pairs.astype(_U32).reshape(-1, 2)


def _host_call(coords, radii, flags, grid_cutoff, max_boxes, cutoff_incr, ctx=None):
    ctx = ctx or _lib.default_context()
    try:
        return ctx.guess_bonds_host(coords, radii, flags, grid_cutoff, max_boxes, cutoff_incr)
    except ValueError as e:                     # (MKAMD_EINVAL)
        raise _library_error(e, grid_cutoff) from None


def guess_bonds(mol, ctx=None):
    """The reference's ``guess_bonds`` on the GPU.  ``mol`` needs ``numAtoms``, ``frame``, ``numFrames``, ``coords`` (``[N, 3, F]``),
    ``element`` and ``name``.  The bonds of frame ``mol.frame`` as uint32 ``[n, 2]``; empty for a molecule of one atom or none;
    ``RuntimeError`` when ``mol.frame`` is out of range."""
    if mol.numAtoms <= 1:
        return np.zeros((0, 2), dtype=_U32)
    if mol.frame >= mol.numFrames:
        raise RuntimeError(f"Frame {mol.frame} (defined in mol.frame) is out of range. "
                           f"Must be less than the number of coordinate frames ({mol.numFrames}) in this molecule.")
    coords = np.asarray(mol.coords)[:, :, mol.frame].copy()
    element = np.asarray(mol.element)
    radii = bond_radii(element, mol.name)
    is_hydrogen = (element == "H").astype(_U32)
    grid_cutoff = np.max(radii) * 1.2          # (float32 scalar times a Python float: float32)
    return bond_grid_search(coords, grid_cutoff, is_hydrogen, radii, ctx=ctx)


# ------------------------------------------------------------------------------------------------
# moleculekit hook
# ------------------------------------------------------------------------------------------------
def install():
    """Swap ``guess_bonds`` and ``bond_grid_search`` of an installed ``moleculekit.bondguesser`` for the GPU's.  ``Molecule._guessBonds``
    imports ``guess_bonds`` from that module at call time, so ``atomselect``, ``guessBonds()`` and ``wrap`` of the reference then guess
    on the device.  Returns the originals ``(guess_bonds, bond_grid_search)``; idempotent; ``uninstall()`` puts them back.  Independent
    of the other ``install()`` hooks."""
    import moleculekit.bondguesser as ref

    saved = getattr(ref, "_mkamd_reference_bonds", None)
    if saved is not None:
        return saved
    saved = (ref.guess_bonds, ref.bond_grid_search)
    ref.guess_bonds = guess_bonds
    ref.bond_grid_search = bond_grid_search
    ref._mkamd_reference_bonds = saved
    return saved


def uninstall():
    """Undo ``install()``."""
    import moleculekit.bondguesser as ref

    saved = getattr(ref, "_mkamd_reference_bonds", None)
    if saved is not None:
        ref.guess_bonds, ref.bond_grid_search = saved
        ref._mkamd_reference_bonds = None
