"""Proximity selections on the MI355X (include/mkamd_distance.h "proximity selections").

The reference's ``moleculekit.atomselect_utils.within_distance`` -- the loop behind every ``within X of ...`` and ``exwithin X of ...``
selection -- tests every atom against every source atom on one CPU thread, one frame a call.  Here one call answers all frames of a
resident trajectory: a lane per (frame, query) walks the frame's sources, stops at its first hit, and a wave leaves the loop when none
of its lanes still searches; one large frame runs over a cell list of the sources instead.  The pair test is the reference's float32
arithmetic, operation by operation, so the booleans equal the compiled reference's: nothing is compared with a tolerance.

* ``within_trajectory`` -- CUDA tensors in, a CUDA bool tensor ``[F, n1]`` out.
* ``within`` -- host arrays in the reference's ``[N, 3, F]`` layout; only the rows of the two selections travel.
* ``within_distance`` -- the reference's signature: applies its gate and ORs into ``results`` in place.
* ``within_molecule`` -- ``within`` / ``exwithin`` of a duck-typed molecule over frames.
* ``install()`` / ``uninstall()`` -- swap ``within_distance`` into an installed moleculekit.

Kept on purpose, because the reference does it: the comparison is strict (a pair at exactly the cutoff is not within); a cutoff of zero
selects nothing, not even an atom of both selections; the gate in front of the loop closes with NaN bounds and, with a NEGATIVE
cutoff, for atoms inside the shrunken source box -- so a negative cutoff is not its absolute value.  There is no CPU path: without the
library or a device every entry point raises.
"""
from __future__ import annotations

import numpy as np

from . import _lib

_F32, _U32 = np.float32, np.uint32
AVOID_PAIRS, AVOID_CELLS = 1, 2      # csrc/within_pipeline.h: Context.set_within_plan
PAIRS_KERNEL, CELLS_KERNEL = "mkamd::k_within_pairs", "mkamd::k_within_cells"


def _index_tensor(sel, N, torch, device, what):
    """a CUDA int32 index tensor (uint32 to the library) of a CUDA boolean mask or integer index tensor, every index in [0, N)"""
    if not (hasattr(sel, "is_cuda") and sel.is_cuda):
        raise TypeError(f"{what}: a CUDA tensor is required (there is no CPU path)")
    if sel.device != device:
        raise ValueError(f"{what} lives on another device than coords")
    if sel.dtype == torch.bool:
        if tuple(sel.shape) != (N,):
            raise ValueError(f"{what}: a mask must have shape ({N},), got {tuple(sel.shape)}")
        return torch.nonzero(sel).reshape(-1).to(torch.int32)
    if sel.dtype not in (torch.int32, torch.int64, torch.uint8, torch.int16):
        raise ValueError(f"{what}: a boolean mask or an integer index tensor is required, got {sel.dtype}")
    idx = sel.reshape(-1).to(torch.int64)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= N):
        raise ValueError(f"{what}: selection index out of range for {N} atoms")
    return idx.to(torch.int32).contiguous()


def within_trajectory(coords, sel1, sel2, cutoff, *, bounds=None, out=None, stream=None, ctx=None):
    """Which atoms of ``sel1`` have an atom of ``sel2`` closer than ``cutoff``, per frame.  ``coords``: CUDA float32 ``[F, N, 3]`` or
    ``[N, 3]``; ``sel1`` / ``sel2``: CUDA boolean masks ``[N]`` or integer index tensors (any order, duplicates allowed; the result follows
    ``sel1`` as given, a mask in ascending order).  ``bounds=None``: no gate; ``bounds=(min, max)`` with CUDA float32 tensors ``[F, 3]``
    (``[3]`` for one frame): the reference's gate with those floats.  ``out``: a CUDA bool or uint8 tensor ``[F, n1]`` to write into
    (every element is written).  Returns a CUDA bool tensor ``[F, n1]`` (``[n1]`` for ``[N, 3]`` coordinates).  Runs on ``stream`` (an
    integer ``hipStream_t``; default torch's current stream) and returns when the result is complete."""
    import torch

    if not (hasattr(coords, "is_cuda") and coords.is_cuda):
        raise TypeError("coords: a CUDA tensor is required (there is no CPU path)")
    if coords.dtype != torch.float32:
        raise ValueError(f"coords must be float32, got {coords.dtype}")
    single = coords.dim() == 2
    if coords.dim() not in (2, 3) or coords.shape[-1] != 3:
        raise ValueError(f"coords must be (nframes, natoms, 3) or (natoms, 3), got shape {tuple(coords.shape)}")
    xyz = (coords[None] if single else coords).contiguous()
    F, N = int(xyz.shape[0]), int(xyz.shape[1])
    dev = coords.device
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if ctx is not None and ctx.device != idx:
        raise ValueError(f"ctx lives on GPU {ctx.device} but the tensors are on cuda:{idx}")
    i1 = _index_tensor(sel1, N, torch, dev, "sel1")
    i2 = _index_tensor(sel2, N, torch, dev, "sel2")
    n1, n2 = int(i1.numel()), int(i2.numel())
    gate = None
    if bounds is not None:
        if len(bounds) != 2:
            raise ValueError("bounds: a pair (min, max) is required")
        for nm, b in zip(("bounds min", "bounds max"), bounds):
            if not (hasattr(b, "is_cuda") and b.is_cuda) or b.device != dev:
                raise TypeError(f"{nm}: a CUDA tensor on the device of coords is required")
            if b.dtype != torch.float32:
                raise ValueError(f"{nm} must be float32, got {b.dtype}")
            if tuple(b.shape) != (F, 3) and not (single and tuple(b.shape) == (3,)):
                raise ValueError(f"{nm}: shape ({F}, 3) is required, got {tuple(b.shape)}")
        gate = torch.stack([bounds[0].reshape(F, 3), bounds[1].reshape(F, 3)], dim=1).contiguous()      # [F, 2, 3]
    if out is None:
        res = torch.empty((F, n1), dtype=torch.uint8, device=dev)
    else:
        if not (hasattr(out, "is_cuda") and out.is_cuda) or out.device != dev:
            raise TypeError("out: a CUDA tensor on the device of coords is required")
        if out.dtype not in (torch.bool, torch.uint8) or tuple(out.shape) not in ((F, n1),) + (((n1,),) if single else ()) or not out.is_contiguous():
            raise ValueError(f"out: a contiguous bool or uint8 tensor of shape ({F}, {n1}) is required, got {out.dtype} {tuple(out.shape)}")
        res = out
    ctx = ctx or _lib.default_context(idx)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream if stream is None else int(stream))
    try:
        ctx.within_distance_dev(xyz, N, F, i1, n1, i2, n2, float(cutoff), gate, res)
    finally:
        ctx.set_stream(None)             # (drains the call's stream: the temporaries above may go)
    if out is not None:
        return out
    res = res.view(torch.bool)
    return res[0] if single else res


def _host_indices(sel, N, what):
    """uint32 indices of a boolean mask or an integer index array, every index in [0, N)"""
    sel = np.asarray(sel)
    if sel.dtype == bool:
        if sel.shape != (N,):
            raise ValueError(f"{what}: a mask must have shape ({N},), got {sel.shape}")
        return np.flatnonzero(sel).astype(_U32)
    if not np.issubdtype(sel.dtype, np.integer):
        raise ValueError(f"{what}: a boolean mask or an integer index array is required, got {sel.dtype}")
    idx = sel.reshape(-1).astype(np.int64)
    if idx.size and (idx.min() < 0 or idx.max() >= N):
        raise ValueError(f"{what}: selection index out of range for {N} atoms")
    return np.ascontiguousarray(idx.astype(_U32))


def _host_coords(coords):
    coords = np.asarray(coords)
    if coords.dtype != _F32:
        raise ValueError(f"coords must be float32, got {coords.dtype}")
    if coords.ndim == 2:
        coords = coords[:, :, None]
    if coords.ndim != 3 or coords.shape[1] != 3:
        raise ValueError(f"coords must be (natoms, 3, nframes) or (natoms, 3), got shape {coords.shape}")
    return coords


def within(coords, sel1, sel2, cutoff, frames=None, ctx=None, _gate=None):
    """Host arrays: ``coords`` float32 ``[N, 3, F]`` (the reference's layout; ``[N, 3]``: one frame), ``sel1`` / ``sel2`` boolean masks or
    integer index arrays, ``frames`` the frames to look at (default all).  Returns bool ``[n1, len(frames)]``.  No gate."""
    coords = _host_coords(coords)
    N = coords.shape[0]
    i1, i2 = _host_indices(sel1, N, "sel1"), _host_indices(sel2, N, "sel2")
    if frames is not None:
        frames = np.asarray(frames, dtype=np.int64).reshape(-1)
        if frames.size and (frames.min() < -coords.shape[2] or frames.max() >= coords.shape[2]):
            raise ValueError(f"frames: index out of range for {coords.shape[2]} frames")
        coords = coords[:, :, frames]
    coords = np.ascontiguousarray(coords)
    if _gate is not None:
        _gate = np.ascontiguousarray(_gate, dtype=_F32)
        if _gate.shape != (coords.shape[2], 2, 3):
            raise ValueError(f"bounds: shape ({coords.shape[2]}, 2, 3) is required, got {_gate.shape}")
    ctx = ctx or _lib.default_context()
    out = ctx.within_distance_host(coords, i1, i2, float(cutoff), _gate)
    return np.ascontiguousarray(out.T.astype(bool))


def within_distance(coords, cutoff, sel1, sel2, sel2_min_coords, sel2_max_coords, results, ctx=None):
    """The reference's ``atomselect_utils.within_distance``: ``coords`` float32 ``[N, 3]`` of one frame, ``sel1`` / ``sel2`` uint32 index
    arrays, the six floats of the gate, ``results`` a bool array ``[n1]`` that is ORed into IN PLACE.  Returns None."""
    coords = np.asarray(coords)
    if coords.ndim != 2 or coords.shape[1] != 3:
        raise ValueError(f"coords must be (natoms, 3), got shape {coords.shape}")
    for nm, s in (("sel1", sel1), ("sel2", sel2)):
        if np.asarray(s).dtype != _U32:
            raise ValueError(f"{nm} must be uint32 (the reference's buffer type), got {np.asarray(s).dtype}")
    if not isinstance(results, np.ndarray) or results.dtype != bool or results.shape != (len(sel1),):
        raise ValueError(f"results must be a bool array of shape ({len(sel1)},)")
    mn, mx = np.asarray(sel2_min_coords), np.asarray(sel2_max_coords)
    if mn.dtype != _F32 or mx.dtype != _F32 or mn.shape != (3,) or mx.shape != (3,):
        raise ValueError("sel2_min_coords and sel2_max_coords must be float32 arrays of shape (3,)")
    found = within(coords, sel1, sel2, cutoff, ctx=ctx, _gate=np.stack([mn, mx])[None])
    results |= found[:, 0]


def within_molecule(mol, source, cutoff, frames=None, exclusive=False, ctx=None):
    """``within cutoff of source`` (``exclusive``: ``exwithin``) of a duck-typed molecule (``coords`` float32 ``[N, 3, F]``, ``numAtoms``,
    ``frame``, ``atomselect``) for every atom, over ``frames`` (default: the molecule's current frame).  ``source``: whatever
    ``mol.atomselect`` takes (a boolean mask passes through).  Per frame the source's numpy min / max serve as the gate's bounds, as
    atomselect.py computes them.  Returns bool ``[numAtoms, len(frames)]``; an empty source gives all False."""
    src = np.asarray(source)
    if src.dtype != bool:
        src = np.asarray(mol.atomselect(source))
    coords = _host_coords(mol.coords)
    N = coords.shape[0]
    if src.shape != (N,):
        raise ValueError(f"source: a mask over the {N} atoms is required")
    frames = np.asarray([mol.frame] if frames is None else frames, dtype=np.int64).reshape(-1)
    out = np.zeros((N, len(frames)), dtype=bool)
    if not src.any() or not len(frames):
        return out
    sub = coords[:, :, frames]
    s = sub[src]                                                       # [n2, 3, f]
    gate = np.ascontiguousarray(np.stack([s.min(axis=0).T, s.max(axis=0).T], axis=1), dtype=_F32)         # [f, 2, 3]
    out = within(sub, np.arange(N, dtype=_U32), np.flatnonzero(src).astype(_U32), cutoff, ctx=ctx, _gate=gate)
    if exclusive:
        out[src] = False
    return out


# ------------------------------------------------------------------------------------------------
# moleculekit hook
# ------------------------------------------------------------------------------------------------
def install():
    """Swap ``within_distance`` of an installed moleculekit for the GPU's: in ``moleculekit.atomselect_utils`` and in
    ``moleculekit.atomselect.atomselect``, which imported the name and so holds its own reference.  Returns the original; idempotent;
    ``uninstall()`` puts it back.  Independent of the other ``install()`` hooks."""
    import moleculekit.atomselect.atomselect as user
    import moleculekit.atomselect_utils as ref

    saved = getattr(ref, "_mkamd_reference_within", None)
    if saved is not None:
        return saved
    saved = ref.within_distance
    ref._mkamd_reference_within = saved
    user._mkamd_reference_within = user.within_distance
    ref.within_distance = within_distance
    user.within_distance = within_distance
    return saved


def uninstall():
    """Undo ``install()``."""
    import moleculekit.atomselect.atomselect as user
    import moleculekit.atomselect_utils as ref

    saved = getattr(ref, "_mkamd_reference_within", None)
    if saved is not None:
        ref.within_distance = saved
        ref._mkamd_reference_within = None
    saved = getattr(user, "_mkamd_reference_within", None)
    if saved is not None:
        user.within_distance = saved
        user._mkamd_reference_within = None
