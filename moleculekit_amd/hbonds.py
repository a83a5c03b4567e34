"""Hydrogen bonds of trajectory frames on the MI355X (include/mkamd_distance.h "hydrogen bonds").

The reference's ``moleculekit.interactions.interactions.hbonds_calculate`` runs one compiled loop, ``for frame: for donor: for acceptor:``
on one thread -- and ``waterbridge_calculate`` calls it ``order + 1`` times.  Here every pair the two selections allow is decided on the
device in every frame, and the hits are compacted into per-frame lists in the reference's order.  Every float32 operation is the
reference's (the wrapped vectors, the squared distances, the dot product, the ratio, the C library's float32 ``acos``), so the lists are
the reference's: the same triples in the same order.  The work is proportional to the ALLOWED pairs -- a donor row is held against the
acceptors of the selection its heavy atom is not in -- so a few selected atoms against all waters cost what they test.

* ``hbonds_trajectory`` -- CUDA tensors in the reference's ``[N, 3, F]`` layout -> host offsets and CUDA int32 triples.
* ``hbonds`` -- numpy arrays through the host entry point (only the donors' and acceptors' rows travel).
* ``hbonds_calculate`` -- the reference's function: signature, defaults, errors and the list of int64 ``(n, 3)`` arrays it returns;
  ``install()`` / ``uninstall()`` swap it into an installed moleculekit, whose own ``waterbridge_calculate`` then runs on the device.

Finding donors and acceptors stays with the reference (``get_donors_acceptors``, once per topology).  There is no CPU path: without the
library or a device every entry point raises.
"""
from __future__ import annotations

import numpy as np

from . import _lib

_F32, _U32 = np.float32, np.uint32


def _u32(a, name, n_atoms):
    a = np.asarray(a.cpu() if hasattr(a, "cpu") else a)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{name}: an integer array is required, got {a.dtype.name}")
    if a.size and (a.min() < 0 or a.max() >= n_atoms):
        raise IndexError(f"{name}: index out of range for {n_atoms} atoms")
    return np.ascontiguousarray(a, dtype=_U32)


def _flags(sel, name, n_atoms):
    """a selection as per-atom uint32 flags: a boolean mask or 0 / 1 flags of n_atoms entries"""
    sel = np.asarray(sel.cpu() if hasattr(sel, "cpu") else sel)
    if sel.shape != (n_atoms,) or not (sel.dtype == bool or np.issubdtype(sel.dtype, np.integer)):
        raise ValueError(f"{name} must be a boolean mask or 0/1 flags of {n_atoms} atoms, got {sel.dtype.name} {sel.shape}")
    return np.ascontiguousarray(sel, dtype=_U32)


def _arguments(n_atoms, donors, acceptors, sel1, sel2, dist_threshold, angle_threshold, ignore_hs):
    """the lists of a call, checked: (donors [n, 2] or [n, 1], acceptors [m], sel1, sel2 or None, intra)"""
    donors = _u32(donors, "donors", n_atoms)
    cols = 1 if ignore_hs else 2
    if donors.size == 0:
        donors = donors.reshape(0, cols)
    if donors.ndim != 2 or donors.shape[1] != cols:
        raise ValueError(f"donors must be ({'n, 1) rows of heavy atoms with ignore_hs' if ignore_hs else 'n, 2) rows of (heavy atom, hydrogen)'}, "
                         f"got shape {donors.shape}")
    acceptors = _u32(acceptors, "acceptors", n_atoms)
    if acceptors.ndim != 1:
        raise ValueError(f"acceptors must be a 1-D index array, got shape {acceptors.shape}")
    if np.isnan(float(dist_threshold)) or np.isnan(float(angle_threshold)):
        raise ValueError("thresholds must be numbers, not NaN")
    sel1 = _flags(sel1, "sel1", n_atoms)
    intra = sel2 is None
    return donors, acceptors, sel1, None if intra else _flags(sel2, "sel2", n_atoms), intra


def hbonds_trajectory(coords, box, donors, acceptors, sel1, sel2=None, dist_threshold=2.5, angle_threshold=120, ignore_hs=False, *, stream=None,
                      ctx=None):
    """Hydrogen bonds of a device-resident trajectory.  ``coords``: CUDA float32 ``[N, 3, F]`` (``Molecule.coords``), ``box`` CUDA float32
    ``[3, F]`` or None (every axis open; a zero axis of a box is open too).  ``donors`` ``[n, 2]`` rows of (heavy atom, hydrogen) --
    ``[n, 1]`` heavy atoms with ``ignore_hs`` --, ``acceptors`` ``[m]`` and the per-atom selections ``sel1`` / ``sel2`` (boolean masks
    or 0 / 1 flags; ``sel2`` None: bonds inside ``sel1``) are host arrays or tensors.  A bond is reported where the hydrogen (the heavy
    atom with ``ignore_hs``) is within ``dist_threshold`` of the acceptor and the heavy atom - hydrogen - acceptor angle is greater than
    ``angle_threshold`` degrees, between atoms of different selections.
    Returns ``(frame_offsets, triples)``: int64 host ``[F + 1]`` and int32 CUDA ``[n, 3]`` rows of (heavy atom, hydrogen or -1,
    acceptor); the bonds of frame ``f`` are rows ``frame_offsets[f]:frame_offsets[f + 1]``, in the reference's order.  Runs on
    ``stream`` (an integer ``hipStream_t``; default torch's current stream) and returns when the list is complete (its size has to
    reach the host)."""
    import torch

    for name, t in (("coords", coords),) + ((("box", box),) if box is not None else ()):
        if not (hasattr(t, "is_cuda") and t.is_cuda):
            raise TypeError(f"{name}: a CUDA tensor is required (there is no CPU path)")
        if t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32, got {t.dtype}")
    if coords.dim() == 2:
        coords = coords.unsqueeze(2)
    if coords.dim() != 3 or coords.shape[1] != 3:
        raise ValueError(f"coords must be (natoms, 3, nframes), got shape {tuple(coords.shape)}")
    coords = coords.contiguous()
    N, F = int(coords.shape[0]), int(coords.shape[2])
    dev = coords.device
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if box is not None:
        if tuple(box.shape) != (3, F):
            raise ValueError(f"box must have shape (3, {F}), got {tuple(box.shape)}")
        if box.device != coords.device:
            raise ValueError("coords and box live on different devices")
        box = box.contiguous()
    if ctx is not None and ctx.device != idx:
        raise ValueError(f"ctx lives on GPU {ctx.device} but the tensors are on cuda:{idx}")
    donors, acceptors, s1, s2, intra = _arguments(N, donors, acceptors, sel1, sel2, dist_threshold, angle_threshold, ignore_hs)
    ctx = ctx or _lib.default_context(idx)
    dev = torch.device("cuda", idx)
    if F == 0 or len(donors) == 0 or len(acceptors) == 0:
        return np.zeros(F + 1, np.int64), torch.empty((0, 3), dtype=torch.int32, device=dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream if stream is None else int(stream))
    try:
        # (the lists stay host arrays: the library sorts them into classes on the host and uploads one table)
        offs, p_triples, n = ctx.hbonds_dev(coords, N, F, box, donors, len(donors), acceptors, len(acceptors), s1, s2, dist_threshold,
                                            angle_threshold, intra, ignore_hs)
        triples = torch.empty((n, 3), dtype=torch.int32, device=dev)
        if n:                                   # the list is context-owned until the next hydrogen-bond call: a device-to-device copy keeps it
            _lib._check(_lib.load().mkamd_copy_dev(ctx._h, triples.data_ptr(), p_triples, n * 12))
        ctx.synchronize()                       # (the result is torch's: nothing of the call is pending when it returns)
    finally:
        ctx.set_stream(None)
    return offs, triples


def hbonds(coords, box, donors, acceptors, sel1, sel2=None, dist_threshold=2.5, angle_threshold=120, ignore_hs=False, *, ctx=None):
    """Hydrogen bonds of host arrays: ``coords`` float32 ``[N, 3, F]``, ``box`` float32 ``[3, F]`` (None: open); the other arguments as
    for ``hbonds_trajectory``.  Returns ``(frame_offsets int64 [F + 1], triples int32 [n, 3])``."""
    coords = np.asarray(coords)
    if coords.ndim == 2:
        coords = coords[:, :, None]
    if coords.ndim != 3 or coords.shape[1] != 3:
        raise ValueError(f"coords must be (natoms, 3, nframes), got shape {coords.shape}")
    coords = np.ascontiguousarray(coords, dtype=_F32)
    N, _, F = coords.shape
    if box is not None:
        box = np.asarray(box)
        if box.shape != (3, F):
            raise ValueError(f"box must have shape (3, {F}), got {box.shape}")
        box = np.ascontiguousarray(box, dtype=_F32)
    donors, acceptors, s1, s2, intra = _arguments(N, donors, acceptors, sel1, sel2, dist_threshold, angle_threshold, ignore_hs)
    if F == 0 or len(donors) == 0 or len(acceptors) == 0:
        return np.zeros(F + 1, np.int64), np.zeros((0, 3), np.int32)
    return _host_call(coords, box, donors, acceptors, s1, s2, dist_threshold, angle_threshold, intra, ignore_hs, ctx)


def _host_call(coords, box, donors, acceptors, sel1, sel2, dist_threshold, angle_threshold, intra, ignore_hs, ctx=None):
    ctx = ctx or _lib.default_context()
    return ctx.hbonds_host(coords, box, donors, acceptors, sel1, sel2, dist_threshold, angle_threshold, intra, ignore_hs)


# ------------------------------------------------------------------------------------------------
# the reference's function
# ------------------------------------------------------------------------------------------------
def hbonds_calculate(mol, donors, acceptors, sel1="all", sel2=None, dist_threshold: float = 2.5, angle_threshold: float = 120,
                     ignore_hs: bool = False):
    """The reference's ``hbonds_calculate`` on the GPU.  ``mol`` needs ``coords`` (``[N, 3, F]``), ``box`` (``[3, F]``), ``numFrames``,
    ``numAtoms`` and ``atomselect``.  ``donors``: ``(n, 2)`` rows of (heavy atom, hydrogen); ``acceptors``: atom indices; ``sel1`` /
    ``sel2``: atom selections (``sel2`` None: bonds inside ``sel1``).  Returns a list with one int64 ``(n_hbonds, 3)`` array per frame:
    heavy atom, hydrogen (-1 with ``ignore_hs``), acceptor."""
    if mol.box.shape[1] != mol.coords.shape[2]:
        raise RuntimeError("mol.box should have same number of frames as mol.coords")

    if len(donors) == 0 or len(acceptors) == 0:
        return [np.empty((0, 3), dtype=np.int64) for _ in range(mol.numFrames)]

    sel1 = mol.atomselect(sel1).astype(np.uint32).copy()
    if sel2 is None:
        sel2 = sel1.copy()
        intra = True
    else:
        sel2 = mol.atomselect(sel2).astype(np.uint32).copy()
        intra = False

    if len(sel1) != mol.numAtoms or len(sel2) != mol.numAtoms:
        raise RuntimeError("Selections must be boolean of size equal to number of atoms in the molecule")

    # as the reference: donors and acceptors outside both selections never pair
    donors, acceptors = np.asarray(donors), np.asarray(acceptors)
    sel_idx = np.where(sel1 | sel2)[0]
    donors = donors[np.all(np.isin(donors, sel_idx), axis=1)]
    acceptors = acceptors[np.isin(acceptors, sel_idx)]

    if ignore_hs:
        donors = np.unique(donors[:, 0])[:, None]

    offs, triples = hbonds(mol.coords, mol.box, donors, acceptors, sel1, None if intra else sel2, float(dist_threshold), float(angle_threshold),
                           bool(ignore_hs))
    triples = triples.astype(np.int64)
    return [triples[int(offs[f]):int(offs[f + 1])].reshape(-1, 3) if f + 1 < len(offs) else np.empty((0, 3), dtype=np.int64)
            for f in range(mol.numFrames)]


# ------------------------------------------------------------------------------------------------
# moleculekit hook
# ------------------------------------------------------------------------------------------------
def install():
    """Swap ``hbonds_calculate`` of an installed ``moleculekit.interactions.interactions`` for the GPU's.  The reference's own
    ``waterbridge_calculate`` calls that module global, so it then runs its hydrogen bonds on the device.  Returns the original;
    idempotent; ``uninstall()`` puts it back.  Independent of the other ``install()`` hooks."""
    import moleculekit.interactions.interactions as ref

    saved = getattr(ref, "_mkamd_reference_hbonds", None)
    if saved is not None:
        return saved
    saved = ref.hbonds_calculate
    ref.hbonds_calculate = hbonds_calculate
    ref._mkamd_reference_hbonds = saved
    return saved


def uninstall():
    """Undo ``install()``."""
    import moleculekit.interactions.interactions as ref

    saved = getattr(ref, "_mkamd_reference_hbonds", None)
    if saved is not None:
        ref.hbonds_calculate = saved
        ref._mkamd_reference_hbonds = None
