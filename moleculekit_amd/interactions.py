"""Ring interactions of trajectory frames on the MI355X (include/mkamd_distance.h "ring interactions").

The reference's ``moleculekit.interactions.interactions`` finds pi-pi stacking, cation-pi and sigma-hole contacts with three compiled
loops, ``for frame: for ring: for partner:`` on one thread.  Here a pre-pass computes every ring's centroid and plane normal once per
frame, a pair kernel decides every (ring, partner) of every frame and the hits are compacted into per-frame lists on the device, in the
reference's order.  Every float32 operation up to the squared distance and the dot product is the reference's, so the lists are the
reference's: the same pairs, the same float32 distances, angles within one float32 unit in the last place (the float64 ``acos`` of two
libraries differs in its last bits) -- and the same pairs silently dropped where the dot product of two unit normals comes out above 1.

* ``ring_interactions_trajectory`` -- CUDA tensors in the reference's ``[N, 3, F]`` layout -> host offsets, CUDA pairs and (distance, angle).
* ``pipi`` / ``cationpi`` / ``sigmahole`` -- numpy arrays through the host entry point (only the rings' and partners' rows travel).
* ``pipi_calculate`` / ``cationpi_calculate`` / ``sigmahole_calculate`` -- the reference's functions: signatures, defaults, errors and
  the nested Python lists they return; ``install()`` / ``uninstall()`` swap them into an installed moleculekit.

Ring detection stays with the reference (networkx / rdkit, once per topology).  There is no CPU path: without the library or a device
every entry point raises.
"""
from __future__ import annotations

import numpy as np

from . import _lib

_F32, _U32 = np.float32, np.uint32
PIPI, CATIONPI, SIGMAHOLE = 0, 1, 2
_KINDS = {"pipi": PIPI, "cationpi": CATIONPI, "sigmahole": SIGMAHOLE, PIPI: PIPI, CATIONPI: CATIONPI, SIGMAHOLE: SIGMAHOLE}
_NAMES = ("pipi_calculate", "cationpi_calculate", "sigmahole_calculate")


def _kind(kind):
    try:
        return _KINDS[kind]
    except (KeyError, TypeError):
        raise ValueError(f"kind must be 'pipi', 'cationpi' or 'sigmahole' (0, 1, 2), got {kind!r}") from None


def _u32(a, name, n_atoms=None):
    a = np.asarray(a.cpu() if hasattr(a, "cpu") else a)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{name}: an integer array is required, got {a.dtype.name}")
    if a.size and (a.min() < 0 or (n_atoms is not None and a.max() >= n_atoms)):
        raise IndexError(f"{name}: index out of range" + (f" for {n_atoms} atoms" if n_atoms is not None else ""))
    return np.ascontiguousarray(a, dtype=_U32)


def _lists(kind, n_atoms, ring_atoms, starts1, second):
    """the index lists of a call, checked: (ring_atoms, starts1, starts2 or None, partners or None, n2)"""
    ring_atoms = _u32(ring_atoms, "ring_atoms", n_atoms).reshape(-1)
    starts1 = _u32(starts1, "starts1").reshape(-1)
    second = _u32(second, "starts2" if kind == PIPI else "partners", None if kind == PIPI else n_atoms)

    def rings(starts, name):
        if starts.size < 1:
            raise ValueError(f"{name} must hold at least the offset 0 of an empty list")
        if starts.size > 1 and (np.any(np.diff(starts.astype(np.int64)) < 3) or int(starts[-1]) > ring_atoms.size):
            raise ValueError(f"{name}: every ring needs at least 3 atoms (the plane normal reads three) and must lie inside ring_atoms")
        return starts.size - 1

    rings(starts1, "starts1")
    if kind == PIPI:
        second = second.reshape(-1)
        return ring_atoms, starts1, second, None, rings(second, "starts2")
    if kind == CATIONPI:
        if second.ndim != 1:
            raise ValueError(f"cations must be a 1-D index array, got shape {second.shape}")
    elif second.ndim != 2 or second.shape[1] != 2:
        if second.size:
            raise ValueError(f"halides must be (n, 2) rows of (halogen, bonded atom), got shape {second.shape}")
        second = second.reshape(0, 2)
    return ring_atoms, starts1, None, second, int(second.shape[0])


def _thresholds(kind, thresholds):
    t = np.zeros(4, _F32)
    want = 4 if kind == PIPI else 2
    th = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if th.size != want:
        raise ValueError(f"thresholds: {want} numbers are required ({'dist1, angle1 max, dist2, angle2 min' if kind == PIPI else 'dist, angle min'})")
    if np.any(np.isnan(th)):
        raise ValueError("thresholds must be numbers, not NaN")
    t[:want] = th
    return t


def ring_interactions_trajectory(kind, coords, box, ring_atoms, starts1, second, thresholds, *, stream=None, ctx=None):
    """Ring interactions of a device-resident trajectory.  ``coords``: CUDA float32 ``[N, 3, F]`` (``Molecule.coords``), ``box`` CUDA
    float32 ``[3, F]`` or None (every axis open; a zero axis of a box is open too).  ``ring_atoms`` / ``starts1`` / ``second`` are the
    compiled reference's arguments (host arrays): the rings' atoms concatenated, the offsets of the first list's rings, and the second
    list's offsets (``kind`` ``"pipi"``), the cations ``[n]`` (``"cationpi"``) or the ``(halogen, bonded atom)`` rows ``[n, 2]``
    (``"sigmahole"``); ``thresholds``: ``(dist1, angle1 max, dist2, angle2 min)`` or ``(dist, angle min)``.
    Returns ``(frame_offsets, pairs, distang)``: int64 host ``[F + 1]``, int32 CUDA ``[n, 2]`` (ring index; ring index or atom index of
    the partner) and float32 CUDA ``[n, 2]`` (distance, angle in degrees); the pairs of frame ``f`` are rows
    ``frame_offsets[f]:frame_offsets[f + 1]``, in the reference's order.  Runs on ``stream`` (an integer ``hipStream_t``; default
    torch's current stream) and returns when the lists are complete (their size has to reach the host)."""
    import torch

    kind = _kind(kind)
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
    atoms, s1, s2, partners, n2 = _lists(kind, N, ring_atoms, starts1, second)
    thr = _thresholds(kind, thresholds)
    ctx = ctx or _lib.default_context(idx)
    dev = torch.device("cuda", idx)
    n1 = int(s1.size) - 1
    if F == 0 or n1 == 0 or n2 == 0:
        return (np.zeros(F + 1, np.int64), torch.empty((0, 2), dtype=torch.int32, device=dev), torch.empty((0, 2), dtype=torch.float32, device=dev))
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream if stream is None else int(stream))
    try:
        d_atoms, d_s1 = (torch.as_tensor(a.view(np.int32), device=dev) for a in (atoms, s1))
        d_s2 = torch.as_tensor(s2.view(np.int32), device=dev) if s2 is not None else None
        d_part = torch.as_tensor(np.ascontiguousarray(partners).view(np.int32), device=dev) if partners is not None else None
        offs, p_pairs, p_da, n = ctx.ring_interactions_dev(kind, coords, N, F, box, d_atoms, int(atoms.size), d_s1, n1, d_s2, d_part, n2, thr)
        pairs = torch.empty((n, 2), dtype=torch.int32, device=dev)
        distang = torch.empty((n, 2), dtype=torch.float32, device=dev)
        if n:                                   # the lists are context-owned until the next ring call: device-to-device copies keep them
            _lib._check(_lib.load().mkamd_copy_dev(ctx._h, pairs.data_ptr(), p_pairs, n * 8))
            _lib._check(_lib.load().mkamd_copy_dev(ctx._h, distang.data_ptr(), p_da, n * 8))
        ctx.synchronize()                       # (the index tensors and the results are torch's: nothing of the call is pending when it returns)
    finally:
        ctx.set_stream(None)
    return offs, pairs, distang


def _host_call(kind, coords, box, ring_atoms, starts1, second, thresholds, ctx=None):
    kind = _kind(kind)
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
    atoms, s1, s2, partners, n2 = _lists(kind, N, ring_atoms, starts1, second)
    thr = _thresholds(kind, thresholds)
    if F == 0 or s1.size < 2 or n2 == 0:
        return np.zeros(F + 1, np.int64), np.zeros((0, 2), _U32), np.zeros((0, 2), _F32)
    ctx = ctx or _lib.default_context()
    return ctx.ring_interactions_host(kind, coords, box, atoms, s1, s2, partners, n2, thr)


def _flatten(rings, name):
    rings = [np.asarray(r).reshape(-1) for r in rings]
    starts = np.insert(np.cumsum([len(r) for r in rings]), 0, 0)
    return np.hstack(rings), starts


def pipi(coords, box, rings1, rings2, dist_threshold1=4.4, angle_threshold1_max=30, dist_threshold2=5.5, angle_threshold2_min=60, ctx=None):
    """pi-pi interactions of host arrays: ``coords`` float32 ``[N, 3, F]``, ``box`` float32 ``[3, F]`` (None: open), ``rings1`` /
    ``rings2`` lists of atom-index arrays.  Returns ``(frame_offsets int64 [F + 1], pairs uint32 [n, 2], distang float32 [n, 2])``:
    indices into ``rings1`` and ``rings2``, centroid distance, angle between the planes."""
    if len(rings1) == 0 or len(rings2) == 0:
        F = np.asarray(coords).shape[2] if np.asarray(coords).ndim == 3 else 1
        return np.zeros(F + 1, np.int64), np.zeros((0, 2), _U32), np.zeros((0, 2), _F32)
    a1, s1 = _flatten(rings1, "rings1")
    a2, s2 = _flatten(rings2, "rings2")
    # as the reference's wrapper: the second list behind the first (a ring named in both lists pairs with itself)
    return _host_call(PIPI, coords, box, np.hstack((a1, a2)), s1, s2 + s1.max(),
                      (dist_threshold1, angle_threshold1_max, dist_threshold2, angle_threshold2_min), ctx)


def cationpi(coords, box, rings, cations, dist_threshold=5, angle_threshold_min=60, ctx=None):
    """cation-pi interactions of host arrays -> ``(frame_offsets, pairs, distang)``: ring index and the cation's ATOM index; distance
    from the ring's centroid, angle between the ring's plane and the centroid-cation vector."""
    if len(rings) == 0 or len(cations) == 0:
        F = np.asarray(coords).shape[2] if np.asarray(coords).ndim == 3 else 1
        return np.zeros(F + 1, np.int64), np.zeros((0, 2), _U32), np.zeros((0, 2), _F32)
    a, s = _flatten(rings, "rings")
    return _host_call(CATIONPI, coords, box, a, s, np.asarray(cations), (dist_threshold, angle_threshold_min), ctx)


def sigmahole(coords, box, rings, halides, dist_threshold=4.5, angle_threshold_min=60, ctx=None):
    """sigma-hole interactions of host arrays; ``halides``: ``(halogen, bonded atom)`` rows -> ``(frame_offsets, pairs, distang)``: ring
    index and the halogen's ATOM index; distance from the centroid, angle between the ring's plane and the bond's direction."""
    if len(rings) == 0 or len(halides) == 0:
        F = np.asarray(coords).shape[2] if np.asarray(coords).ndim == 3 else 1
        return np.zeros(F + 1, np.int64), np.zeros((0, 2), _U32), np.zeros((0, 2), _F32)
    a, s = _flatten(rings, "rings")
    return _host_call(SIGMAHOLE, coords, box, a, s, np.asarray(halides), (dist_threshold, angle_threshold_min), ctx)


# ------------------------------------------------------------------------------------------------
# the reference's functions
# ------------------------------------------------------------------------------------------------
def _frame_lists(num_frames, offs, pairs, distang):
    """what the reference builds from its C++ vectors: per frame a list of [i, j] (Python ints) and of [dist, angle] (Python floats)"""
    pl, dl = pairs.tolist(), distang.astype(np.float64).tolist()       # (a float32 widened: what a C++ float becomes in Python)
    idx, da = [], []
    for f in range(num_frames):
        lo, hi = (int(offs[f]), int(offs[f + 1])) if f + 1 < len(offs) else (0, 0)
        idx.append(pl[lo:hi])
        da.append(dl[lo:hi])
    return idx, da


def _check_angles(*angles):
    if any(a < 0 or a > 90 for a in angles):
        raise RuntimeError("Values for angles should be [0, 90] degrees")


def pipi_calculate(mol, rings1, rings2, dist_threshold1: float = 4.4, angle_threshold1_max: float = 30, dist_threshold2: float = 5.5,
                   angle_threshold2_min: float = 60, return_rings: bool = False):
    """The reference's ``pipi_calculate`` on the GPU.  ``mol`` needs ``coords`` (``[N, 3, F]``), ``box`` (``[3, F]``) and
    ``numFrames``.  Returns ``(pp_list, dist_ang_list)``: per frame a list of ``[i, j]`` (indices into ``rings1`` / ``rings2``; with
    ``return_rings`` the two rings' atom arrays) and of ``[distance, angle]``."""
    _check_angles(angle_threshold1_max, angle_threshold2_min)
    if len(rings1) == 0 or len(rings2) == 0:
        return [[] for _ in range(mol.numFrames)], [[] for _ in range(mol.numFrames)]
    offs, pairs, da = pipi(mol.coords, mol.box, rings1, rings2, dist_threshold1, angle_threshold1_max, dist_threshold2, angle_threshold2_min)
    idx, dist_ang_list = _frame_lists(mol.numFrames, offs, pairs, da)
    if return_rings:
        idx = [[[rings1[p[0]], rings2[p[1]]] for p in frame] for frame in idx]
    return idx, dist_ang_list


def cationpi_calculate(mol, rings, cations, dist_threshold: float = 5, angle_threshold_min: float = 60, return_rings: bool = False):
    """The reference's ``cationpi_calculate`` on the GPU -> ``(index_list, dist_ang_list)``: per frame ``[ring index, cation atom
    index]`` (with ``return_rings``: ``[ring atoms, cation atom index]``) and ``[distance, angle]``."""
    _check_angles(angle_threshold_min)
    if len(rings) == 0 or len(cations) == 0:
        return [[] for _ in range(mol.numFrames)], [[] for _ in range(mol.numFrames)]
    offs, pairs, da = cationpi(mol.coords, mol.box, rings, np.array(cations, dtype=_U32), dist_threshold, angle_threshold_min)
    idx, dist_ang_list = _frame_lists(mol.numFrames, offs, pairs, da)
    if return_rings:
        idx = [[[rings[p[0]], p[1]] for p in frame] for frame in idx]
    return idx, dist_ang_list


def sigmahole_calculate(mol, rings, halides, dist_threshold: float = 4.5, angle_threshold_min: float = 60, return_rings: bool = False):
    """The reference's ``sigmahole_calculate`` on the GPU -> ``(index_list, dist_ang_list)``: per frame ``[ring index, halogen atom
    index]`` (with ``return_rings``: ``[ring atoms, halogen atom index]``) and ``[distance, angle]``."""
    _check_angles(angle_threshold_min)
    if len(rings) == 0 or len(halides) == 0:
        return [[] for _ in range(mol.numFrames)], [[] for _ in range(mol.numFrames)]
    offs, pairs, da = sigmahole(mol.coords, mol.box, rings, np.array(halides, dtype=_U32), dist_threshold, angle_threshold_min)
    idx, dist_ang_list = _frame_lists(mol.numFrames, offs, pairs, da)
    if return_rings:
        idx = [[[rings[p[0]], p[1]] for p in frame] for frame in idx]
    return idx, dist_ang_list


# ------------------------------------------------------------------------------------------------
# moleculekit hook
# ------------------------------------------------------------------------------------------------
def install():
    """Swap ``pipi_calculate``, ``cationpi_calculate`` and ``sigmahole_calculate`` of an installed
    ``moleculekit.interactions.interactions`` for the GPU's.  Returns the originals (a dict by name); idempotent; ``uninstall()`` puts
    them back.  Independent of the other ``install()`` hooks."""
    import moleculekit.interactions.interactions as ref

    saved = getattr(ref, "_mkamd_reference_rings", None)
    if saved is not None:
        return saved
    saved = {name: getattr(ref, name) for name in _NAMES}
    for name in _NAMES:
        setattr(ref, name, globals()[name])
    ref._mkamd_reference_rings = saved
    return saved


def uninstall():
    """Undo ``install()``."""
    import moleculekit.interactions.interactions as ref

    saved = getattr(ref, "_mkamd_reference_rings", None)
    if saved is not None:
        for name in _NAMES:
            setattr(ref, name, saved[name])
        ref._mkamd_reference_rings = None
