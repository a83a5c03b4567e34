"""Rigid superposition of trajectory frames on a reference structure on the MI355X (include/mkamd_distance.h "alignment").

* ``_pp_align`` -- drop-in for ``moleculekit.align._pp_align`` (what ``Molecule.align`` and ``MetricRmsd`` call), host arrays in
  the reference's layout, in place or on a copy; ``install()`` / ``uninstall()`` swap it into an installed moleculekit.
* ``kabsch_transforms`` / ``apply_transforms`` / ``align_trajectory`` / ``rmsd_trajectory`` -- the same on CUDA tensors in the
  frame-major layout of the XTC decoder and the voxelizer (``[F, N, 3]`` float32), asynchronous on torch's current stream.

Each frame's transform is the least-squares optimal PROPER rotation (Horn's quaternion, computed in double) as an affine float64
``[12]`` -- row-major R, then t = c_Q - R c_P -- the ``affine`` the voxelizer takes (``batch.voxelize_lattice_torch``), so a
voxelized aligned frame is bit for bit the frame voxelized with its affine.  There is no CPU path: without the library or a
device every entry point raises.
"""
from __future__ import annotations

import threading

import numpy as np

from . import _lib


def _req(name, a):
    if not isinstance(a, np.ndarray):
        raise TypeError(f"{name}: a numpy array is required")
    if a.dtype != np.float32:
        raise ValueError(f"Buffer dtype mismatch for {name}: expected float32, got {a.dtype.name}")
    if a.ndim != 3 or a.shape[1] != 3:
        raise ValueError(f"{name} must be (natoms, 3, nframes), got shape {a.shape}")
    return a


def _index(sel, n, name):
    """an index array or a boolean mask over n atoms -> uint32 indices (negative indices count from the end, as numpy's)"""
    a = np.asarray(sel)
    if a.dtype == bool:
        if a.ndim != 1 or a.shape[0] != n:
            raise IndexError(f"{name}: a boolean mask of {a.shape} over {n} atoms")
        return np.flatnonzero(a).astype(np.uint32)
    a = a.astype(np.int64).reshape(-1)
    a = np.where(a < 0, a + n, a)
    if a.size and (a.min() < 0 or a.max() >= n):
        raise IndexError(f"{name}: atom index out of range for {n} atoms")
    return np.ascontiguousarray(a, dtype=np.uint32)


def _frames(frames, F):
    fr = np.asarray(frames, dtype=np.int64).reshape(-1)
    fr = np.where(fr < 0, fr + F, fr)
    if fr.size and (fr.min() < 0 or fr.max() >= F):
        raise IndexError(f"frame index out of range for {F} frames")
    return np.ascontiguousarray(fr)


def _pp_align(coords, refcoords, sel, refsel, frames, refframe, matchingframes, inplace=False, ctx=None):
    """``moleculekit.align._pp_align`` on the GPU: superpose ``coords[sel, :, f]`` on ``refcoords[refsel, :, refframe]`` (or on
    frame ``f`` of ``refcoords`` with ``matchingframes``) for every ``f`` in ``frames`` and move all atoms of the frame with it.
    Same signature and semantics: in place (returns None) or on a copy (returned).  ``coords`` / ``refcoords`` must be float32
    ``[natoms, 3, nframes]`` (``Molecule.coords``); anything else raises -- nothing falls back to the CPU.  ``sel`` / ``refsel``:
    index arrays or boolean masks.

    Differences from the reference, by float32 rounding only: the rotation is computed in double (the reference: a float32 SVD),
    and when ``coords`` IS ``refcoords`` and ``inplace`` (``Molecule.align`` of a molecule on itself) the reference frame is taken
    as it was before the call -- the reference's loop reads it live, so frames after ``refframe`` see the reference frame already
    aligned on itself (identical up to rounding).  An empty selection gives NaN coordinates for the listed frames, as the
    reference's mean of nothing does."""
    coords = _req("coords", coords)
    refcoords = _req("refcoords", refcoords)
    N, _, F = coords.shape
    Nr, _, Fr = refcoords.shape
    s = _index(sel, N, "sel")
    rs = _index(refsel, Nr, "refsel")
    if s.size != rs.size:
        raise ValueError(f"sel picks {s.size} atoms and refsel {rs.size}")
    fr = _frames(frames, F)
    if matchingframes and Fr != F:
        raise ValueError("matchingframes needs a reference with as many frames as the trajectory")
    refframe = int(refframe)
    if not matchingframes and fr.size:
        if refframe < 0:
            refframe += Fr
        if not 0 <= refframe < Fr:
            raise IndexError(f"refframe {refframe} out of range for {Fr} frames")
    out = coords if inplace else coords.copy()
    work = out if out.flags.c_contiguous else np.ascontiguousarray(out)
    ref = np.ascontiguousarray(refcoords)      # (a copy when refcoords is a strided view; the library reads it before writing)
    if fr.size and N:
        ctx = ctx or _lib.default_context()
        _lib._check(_lib.load().mkamd_align_host(ctx._h, _lib._ptr(work), N, F, _lib._ptr(ref), Nr, Fr, _lib._ptr(s), _lib._ptr(rs),
                                                 int(s.size), _lib._ptr(fr), int(fr.size), refframe if not matchingframes else 0,
                                                 int(bool(matchingframes))))
    if work is not out:
        out[...] = work
    if not inplace:
        return out
    return None


# ------------------------------------------------------------------------------------------------
# device API: CUDA tensors, frame-major [F, N, 3] float32
# ------------------------------------------------------------------------------------------------
def _torch_ctx(t, ctx):
    import torch

    dev = t.device
    if dev.type != "cuda":
        raise RuntimeError("the alignment kernels need CUDA/HIP tensors (there is no CPU path)")
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if ctx is not None and ctx.device != idx:
        raise ValueError(f"ctx lives on GPU {ctx.device} but the tensors are on cuda:{idx}")
    ctx = ctx or _lib.default_context(idx)
    ctx.set_stream(torch.cuda.current_stream(torch.device("cuda", idx)).cuda_stream)
    return ctx, torch.device("cuda", idx)


def _xyz3(name, t):
    import torch

    if not (hasattr(t, "is_cuda") and t.is_cuda):
        raise TypeError(f"{name}: a CUDA tensor is required")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"{name} must be [frames, atoms, 3] (or [atoms, 3]), got {tuple(t.shape)}")
    return t.contiguous()


def _dev_sel(sel, n, name, dev):
    import torch

    s = sel if isinstance(sel, np.ndarray) or not hasattr(sel, "cpu") else sel.cpu().numpy()
    return torch.as_tensor(_index(s, n, name).view(np.int32), device=dev)


def _dev_frames(frames, F, dev):
    import torch

    if frames is None:
        return None, F
    fr = frames.cpu().numpy() if hasattr(frames, "cpu") else frames
    fr = _frames(fr, F)
    return torch.as_tensor(fr, device=dev), int(fr.size)


def _transforms(ctx, dev, xyz, ref, d_sel, d_refsel, n, d_fr, K, refframe, matchingframes, fit=True):
    import torch

    aff = torch.empty((K, 12), dtype=torch.float64, device=dev)
    rms = torch.empty(K, dtype=torch.float64, device=dev) if fit else None
    _lib._check(_lib.load().mkamd_align_transforms_dev(ctx._h, xyz.data_ptr(), int(xyz.shape[1]), int(xyz.shape[0]), ref.data_ptr(),
                                                       int(ref.shape[1]), int(ref.shape[0]), d_sel.data_ptr(), d_refsel.data_ptr(), int(n),
                                                       None if d_fr is None else d_fr.data_ptr(), int(K), int(refframe),
                                                       int(bool(matchingframes)), aff.data_ptr(), None if rms is None else rms.data_ptr()))
    return aff, rms


def _check_ref(ref, refframe, matchingframes, F):
    if matchingframes:
        if ref.shape[0] != F:
            raise ValueError("matchingframes needs a reference with as many frames as the trajectory")
        return 0
    refframe = int(refframe)
    if refframe < 0:
        refframe += int(ref.shape[0])
    if not 0 <= refframe < ref.shape[0]:
        raise IndexError(f"refframe out of range for {ref.shape[0]} reference frames")
    return refframe


def kabsch_transforms(xyz, ref, sel, refsel=None, frames=None, refframe=0, matchingframes=False, ctx=None):
    """Per listed frame of ``xyz`` (CUDA float32 ``[F, N, 3]``) the rigid transform that superposes ``xyz[f, sel]`` on
    ``ref[refframe, refsel]`` (``ref``: ``[Nr, 3]`` or ``[Fr, Nr, 3]``; with ``matchingframes`` on ``ref[f, refsel]``).
    Returns ``(affine, fit_rmsd)``: float64 ``[K, 12]`` (row-major R, then t; the voxelizer's ``affine``) and float32 ``[K]``
    (the RMSD of the fit), K = ``len(frames)`` (default: every frame, in order)."""
    xyz = _xyz3("xyz", xyz)
    ref = _xyz3("ref", ref)
    ctx, dev = _torch_ctx(xyz, ctx)
    refsel = sel if refsel is None else refsel
    d_sel = _dev_sel(sel, int(xyz.shape[1]), "sel", dev)
    d_refsel = _dev_sel(refsel, int(ref.shape[1]), "refsel", dev)
    if d_sel.numel() != d_refsel.numel():
        raise ValueError(f"sel picks {d_sel.numel()} atoms and refsel {d_refsel.numel()}")
    d_fr, K = _dev_frames(frames, int(xyz.shape[0]), dev)
    rf = _check_ref(ref, refframe, matchingframes, int(xyz.shape[0]))
    aff, rms = _transforms(ctx, dev, xyz, ref, d_sel, d_refsel, d_sel.numel(), d_fr, K, rf, matchingframes)
    return aff, rms.float()


def apply_transforms(xyz, affine, frames=None, out=None, ctx=None):
    """``out[f] = float32(R x + t)`` (in double, the voxelizer's operation order) for every atom of each listed frame ``f``
    (``frames[i]`` takes ``affine[i]``).  ``out``: a tensor like ``xyz`` (``xyz`` itself: in place); default a copy of ``xyz``
    (frames that are not listed keep their coordinates)."""
    import torch

    xyz = _xyz3("xyz", xyz)
    ctx, dev = _torch_ctx(xyz, ctx)
    d_fr, K = _dev_frames(frames, int(xyz.shape[0]), dev)
    if not (affine.dtype == torch.float64 and affine.is_contiguous() and tuple(affine.shape) == (K, 12) and affine.device == dev):
        raise ValueError(f"affine must be a contiguous float64 [{K}, 12] tensor on {dev}")
    if out is None:
        out = xyz.clone()
    elif not (out.dtype == torch.float32 and out.is_contiguous() and out.shape == xyz.shape and out.device == dev):
        raise ValueError("out must be a contiguous float32 tensor shaped like xyz")
    _lib._check(_lib.load().mkamd_align_apply_dev(ctx._h, xyz.data_ptr(), int(xyz.shape[1]), None if d_fr is None else d_fr.data_ptr(),
                                                  int(K), affine.data_ptr(), out.data_ptr()))
    return out


def align_trajectory(xyz, ref, sel, refsel=None, frames=None, refframe=0, matchingframes=False, inplace=False, ctx=None):
    """``Molecule.align`` on a device-resident trajectory: ``kabsch_transforms`` + ``apply_transforms``.  Returns the aligned
    ``[F, N, 3]`` tensor (``xyz`` itself with ``inplace``)."""
    xyz = _xyz3("xyz", xyz)
    aff, _ = kabsch_transforms(xyz, ref, sel, refsel, frames, refframe, matchingframes, ctx)
    return apply_transforms(xyz, aff, frames, out=xyz if inplace else None, ctx=ctx)


def rmsd_trajectory(xyz, ref, alnsel, refalnsel, rmsdsel=None, refrmsdsel=None, frames=None, refframe=0, ctx=None):
    """``MetricRmsd(refmol, ..., pbc=False).project(mol)`` on device arrays: per listed frame, align on (``alnsel``,
    ``refalnsel``) and return the RMSD over (``rmsdsel``, ``refrmsdsel``) -- defaults: the alignment selections -- as a
    float32 CUDA tensor ``[K]``.  The aligned coordinates are never written: the RMSD kernel applies each frame's transform
    on the fly (the same float32 values ``apply_transforms`` would store)."""
    import torch

    xyz = _xyz3("xyz", xyz)
    ref = _xyz3("ref", ref)
    ctx, dev = _torch_ctx(xyz, ctx)
    N, Nr = int(xyz.shape[1]), int(ref.shape[1])
    d_a, d_ra = _dev_sel(alnsel, N, "alnsel", dev), _dev_sel(refalnsel, Nr, "refalnsel", dev)
    d_r = d_a if rmsdsel is None else _dev_sel(rmsdsel, N, "rmsdsel", dev)
    d_rr = d_ra if refrmsdsel is None else _dev_sel(refrmsdsel, Nr, "refrmsdsel", dev)
    if d_a.numel() != d_ra.numel() or d_r.numel() != d_rr.numel():
        raise ValueError("the trajectory and reference selections pick different numbers of atoms")
    d_fr, K = _dev_frames(frames, int(xyz.shape[0]), dev)
    rf = _check_ref(ref, refframe, False, int(xyz.shape[0]))
    aff, _ = _transforms(ctx, dev, xyz, ref, d_a, d_ra, d_a.numel(), d_fr, K, rf, False, fit=False)
    out = torch.empty(K, dtype=torch.float32, device=dev)
    _lib._check(_lib.load().mkamd_align_rmsd_dev(ctx._h, xyz.data_ptr(), N, int(xyz.shape[0]), ref.data_ptr(), Nr, int(ref.shape[0]),
                                                 d_r.data_ptr(), d_rr.data_ptr(), int(d_r.numel()), None if d_fr is None else d_fr.data_ptr(),
                                                 int(K), rf, 0, aff.data_ptr(), out.data_ptr()))
    return out


# ------------------------------------------------------------------------------------------------
# streamed voxelization (batch.iterVoxelizeTrajectory / iterVoxelizeXTC with align=)
# ------------------------------------------------------------------------------------------------
_side = threading.local()


def _side_context(device):
    """a context of this thread for the transforms of the voxel streams: its stream is set to the stream that prepares a
    chunk, so that the voxelizer's context (and its pipelining) is left alone"""
    ctxs = getattr(_side, "ctxs", None)
    if ctxs is None:
        ctxs = _side.ctxs = {}
    if device not in ctxs:
        ctxs[device] = _lib.Context(device)
    return ctxs[device]


class StreamAligner:
    """``align = (ref_xyz [n, 3] Angstrom, sel)`` of the voxel streams, prepared once: the reference and the selection on the
    device; ``transforms(stream, xyz, out)`` writes each chunk frame's affine into ``out`` on ``stream``."""

    def __init__(self, align, natoms, dev):
        import torch

        if not (isinstance(align, (tuple, list)) and len(align) == 2):
            raise ValueError("align must be (ref_xyz [n, 3] in Angstrom, sel)")
        ref, sel = align
        ref = ref.detach().cpu().numpy() if hasattr(ref, "detach") else ref
        ref = np.ascontiguousarray(ref, dtype=np.float32)
        if ref.ndim != 2 or ref.shape[1] != 3:
            raise ValueError(f"align: ref_xyz must be [n, 3], got {ref.shape}")
        s = _index(sel, natoms, "align sel")
        if s.size != ref.shape[0]:
            raise ValueError(f"align: sel picks {s.size} atoms, ref_xyz has {ref.shape[0]}")
        self.n = int(s.size)
        self.ref = torch.as_tensor(ref, device=dev)
        self.sel = torch.as_tensor(s.view(np.int32), device=dev)
        self.refsel = torch.arange(self.n, dtype=torch.int32, device=dev)
        self.ctx = _side_context(dev.index)

    def transforms(self, stream, xyz, out):
        """xyz [n, N, 3] frame-major chunk, out float64 [n, 12]; enqueued on `stream` (an integer hipStream_t)"""
        self.ctx.set_stream(stream)
        _lib._check(_lib.load().mkamd_align_transforms_dev(self.ctx._h, xyz.data_ptr(), int(xyz.shape[1]), int(xyz.shape[0]),
                                                           self.ref.data_ptr(), self.n, 1, self.sel.data_ptr(), self.refsel.data_ptr(),
                                                           self.n, None, int(xyz.shape[0]), 0, 0, out.data_ptr(), None))


# ------------------------------------------------------------------------------------------------
# moleculekit hook
# ------------------------------------------------------------------------------------------------
def install():
    """Swap ``moleculekit.align._pp_align`` for this module's (``Molecule.align`` imports it at call time, so ``Molecule.align``,
    ``MetricRmsd`` and everything else built on it then align on the GPU).  Returns the original; idempotent; ``uninstall()``
    puts it back.  Independent of ``voxeldescriptors.install()``."""
    import moleculekit.align as ref

    saved = getattr(ref, "_mkamd_reference_pp_align", None)
    if saved is not None:
        return saved
    saved = ref._pp_align
    ref._pp_align = _pp_align
    ref._mkamd_reference_pp_align = saved
    return saved


def uninstall():
    """Undo ``install()``."""
    import moleculekit.align as ref

    saved = getattr(ref, "_mkamd_reference_pp_align", None)
    if saved is not None:
        ref._pp_align = saved
        ref._mkamd_reference_pp_align = None
