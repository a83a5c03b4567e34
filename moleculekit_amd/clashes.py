"""Steric clashes on the MI355X (include/mkamd_distance.h "steric clashes").

The reference's ``moleculekit.distance.find_clashes`` builds a float64 kd-tree on the CPU, removes 1-2 / 1-3 / 1-4 neighbours with three
nested Python loops over sets and filters the pairs in a list comprehension.  Here the neighbour search runs over the bond guesser's
device cell list, the exclusions are a CSR table built once per topology with numpy, and the pair test -- the reference's float32
arithmetic, operation by operation -- runs in the pair kernels, so the three arrays come back equal to the reference's: nothing is
compared with a tolerance.  The reference's unstable sort leaves the order of EQUAL overlaps open; this package orders them by
``(a, b)`` ascending.

* ``clash_radii`` -- the van der Waals radii of a molecule's atoms as the reference takes them.
* ``clash_exclusions`` -- the exclusion table of a bond list; reusable across the frames and poses of one topology.
* ``find_clashes_tensor`` -- CUDA tensors in, three CUDA tensors out, in the final order.
* ``moleculekit_amd.distance.find_clashes`` -- the reference's function on a duck-typed molecule; ``install()`` / ``uninstall()`` swap
  it into an installed moleculekit.

Kept on purpose, because the reference does it: in cross mode (two different selections) there is no ``a < b`` filter, so selections
that overlap yield ``(a, b)``, ``(b, a)`` and ``(a, a)`` at distance 0, and a row with ``a > b`` is never excluded -- the exclusions are
stored as ``(min, max)`` and looked up as found.  A grid box may hold at most ``BOX_CAP`` atoms: a frame that exceeds it raises
``ValueError`` naming the box.  There is no CPU path: without the library or a device every entry point raises.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._vdw_radii import VDW_RADIUS

_F32, _U32, _I64 = np.float32, np.uint32, np.int64
BOX_CAP = 4096                       # csrc/bond_kernels.h: BOND_BOX_CAP
AVOID_THREAD, AVOID_WAVE = 1, 2      # csrc/clash_pipeline.h: Context.set_clash_plan
THREAD_KERNEL, WAVE_KERNEL = "mkamd::k_clash_pairs_thread", "mkamd::k_clash_pairs_wave"


def clash_radii(element):
    """float32 ``[N]``: per atom the table's van der Waals radius of its element; an element the table does not know takes carbon's
    entry, an entry without a radius takes 1.7."""
    return np.array([VDW_RADIUS.get(str(e), VDW_RADIUS["C"]) or 1.7 for e in element], dtype=_F32)


def clash_cutoff(max_radius, overlap):
    """the reference's kd-tree radius, in float64: twice the largest radius of ALL atoms minus ``overlap``"""
    return 2.0 * float(max_radius) - overlap


class ClashExclusions:
    """The exclusion table of one topology: a CSR over the atoms -- row ``a`` holds, ascending, the partners ``b >= a`` with which
    ``(a, b)`` is excluded.  ``start`` uint32 ``[natoms + 1]``, ``partner`` uint32.  Made by ``clash_exclusions``."""

    def __init__(self, start, partner, natoms):
        self.start, self.partner, self.natoms = start, partner, int(natoms)
        self._dev = {}

    def pairs(self):
        """int64 ``[n, 2]``: the excluded ``(min, max)`` rows, sorted"""
        lo = np.repeat(np.arange(self.natoms, dtype=_I64), np.diff(self.start.astype(_I64)))
        return np.stack([lo, self.partner.astype(_I64)], axis=1)

    def on_device(self, device):
        """(start, partner) as int32-viewed CUDA tensors on ``device``, uploaded once"""
        import torch

        key = str(device)
        if key not in self._dev:
            partner = self.partner if len(self.partner) else np.zeros(1, dtype=_U32)      # (an empty table still has an address)
            self._dev[key] = (torch.as_tensor(self.start.view(np.int32), device=device),
                              torch.as_tensor(np.ascontiguousarray(partner).view(np.int32), device=device))
        return self._dev[key]


def _expand(tail, start, deg, dst):
    """every neighbour of every path's last atom: (index of the path, the neighbour)"""
    cnt = deg[tail]
    rep = np.repeat(np.arange(len(tail), dtype=_I64), cnt)
    within = np.arange(int(cnt.sum()), dtype=_I64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return rep, dst[start[tail][rep] + within]


def clash_exclusions(bonds, natoms, exclude_bonded=True, exclude_14=True):
    """The pairs ``find_clashes`` does not report, from the bond list as given (duplicates and self-bonds allowed): 1-2 and 1-3
    neighbours where ``exclude_bonded``, 1-4 neighbours where ``exclude_14`` -- the reference's walks, ``b`` a neighbour of ``a``, ``c`` of
    ``b`` with ``c != a``, ``d`` of ``c`` with ``d != b`` and ``d != a`` -- as a ``ClashExclusions``.  Vectorised: the paths are expanded with
    ``numpy.repeat`` over a CSR of the neighbours, not walked in Python."""
    natoms = int(natoms)
    bonds = np.asarray(bonds).reshape(-1, 2).astype(_I64)
    if len(bonds) and (bonds.min() < 0 or bonds.max() >= natoms):
        raise ValueError(f"bonds: atom index out of range for {natoms} atoms")
    found = []
    if len(bonds) and (exclude_bonded or exclude_14):
        both = np.concatenate([bonds, bonds[:, ::-1]])
        key = np.unique(both[:, 0] * natoms + both[:, 1])           # the neighbour sets, both directions
        src, dst = key // natoms, key % natoms
        start = np.searchsorted(src, np.arange(natoms + 1, dtype=_I64))
        deg = np.diff(start)
        a, b = src, dst
        if exclude_bonded:
            found.append((a, b))
        rep, c = _expand(b, start, deg, dst)
        keep = c != a[rep]
        a, b, c = a[rep][keep], b[rep][keep], c[keep]
        if exclude_bonded:
            found.append((a, c))
        if exclude_14:
            rep, d = _expand(c, start, deg, dst)
            keep = (d != b[rep]) & (d != a[rep])
            found.append((a[rep][keep], d[keep]))
    if found:
        x, y = np.concatenate([f[0] for f in found]), np.concatenate([f[1] for f in found])
        key = np.unique(np.minimum(x, y) * natoms + np.maximum(x, y))
        lo, hi = key // natoms, key % natoms
    else:
        lo = hi = np.zeros(0, dtype=_I64)
    start = np.searchsorted(lo, np.arange(natoms + 1, dtype=_I64)).astype(_U32)
    return ClashExclusions(start, np.ascontiguousarray(hi.astype(_U32)), natoms)


def _selection_mask(sel, N, torch, device, what):
    """a CUDA boolean mask ``[N]`` of a CUDA boolean mask or integer index tensor"""
    if not (hasattr(sel, "is_cuda") and sel.is_cuda):
        raise TypeError(f"{what}: a CUDA tensor is required (there is no CPU path)")
    if sel.device != device:
        raise ValueError(f"{what} lives on another device than coords")
    if sel.dtype == torch.bool:
        if tuple(sel.shape) != (N,):
            raise ValueError(f"{what}: a mask must have shape ({N},), got {tuple(sel.shape)}")
        return sel
    if sel.dtype not in (torch.int32, torch.int64, torch.uint8, torch.int16):
        raise ValueError(f"{what}: a boolean mask or an integer index tensor is required, got {sel.dtype}")
    idx = sel.reshape(-1).to(torch.int64)
    if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= N):
        raise ValueError(f"{what}: selection index out of range for {N} atoms")
    mask = torch.zeros(N, dtype=torch.bool, device=device)
    mask[idx] = True
    return mask


def find_clashes_tensor(coords, radii, sel1, sel2=None, overlap=0.6, exclusions=None, max_radius=None, *, stream=None, ctx=None):
    """The clashes of device-resident atoms.  ``coords``: CUDA float32 ``[N, 3]``; ``radii``: CUDA float32 ``[N]``; ``sel1`` / ``sel2``:
    CUDA boolean masks ``[N]`` or integer index tensors (``sel2`` None, or a mask equal to ``sel1``'s: self mode, rows ``a < b``).
    ``exclusions``: a ``ClashExclusions`` over the ``N`` atoms, or None.  ``max_radius``: the largest radius of the molecule, default
    ``radii.max()``.  Returns CUDA tensors ``(pairs int64 [n, 2], distances float32 [n], overlaps float32 [n])`` sorted by overlap, largest
    first, equal overlaps by ``(a, b)``.  Runs on ``stream`` (an integer ``hipStream_t``; default torch's current stream) and returns when
    the lists are complete.  ``ValueError``: non-finite coordinates in a selection, a selection out of range, a box with more than
    ``BOX_CAP`` atoms."""
    import torch

    for nm, t in (("coords", coords), ("radii", radii)):
        if not (hasattr(t, "is_cuda") and t.is_cuda):
            raise TypeError(f"{nm}: a CUDA tensor is required (there is no CPU path)")
    if coords.dtype != torch.float32 or radii.dtype != torch.float32:
        raise ValueError(f"coords and radii must be float32, got {coords.dtype} and {radii.dtype}")
    if coords.dim() != 2 or coords.shape[1] != 3:
        raise ValueError(f"coords must be (natoms, 3), got shape {tuple(coords.shape)}")
    N = int(coords.shape[0])
    if tuple(radii.shape) != (N,) or radii.device != coords.device:
        raise ValueError(f"radii must have shape ({N},) on the device of coords, got {tuple(radii.shape)} on {radii.device}")
    if not np.isfinite(overlap):
        raise ValueError(f"overlap must be finite, got {overlap!r}")
    if exclusions is not None and exclusions.natoms != N:
        raise ValueError(f"exclusions were built for {exclusions.natoms} atoms, coords hold {N}")
    dev = coords.device
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if ctx is not None and ctx.device != idx:
        raise ValueError(f"ctx lives on GPU {ctx.device} but the tensors are on cuda:{idx}")
    mask1 = _selection_mask(sel1, N, torch, dev, "sel1")
    mask2 = None if sel2 is None else _selection_mask(sel2, N, torch, dev, "sel2")
    if mask2 is not None and torch.equal(mask1, mask2):
        mask2 = None                                                  # the reference's self mode
    dev = torch.device("cuda", idx)
    empty = (torch.empty((0, 2), dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.float32, device=dev),
             torch.empty(0, dtype=torch.float32, device=dev))
    if N == 0:
        return empty
    if max_radius is None:
        max_radius = radii.max().item()
    cutoff = clash_cutoff(max_radius, overlap)
    coords, radii = coords.contiguous(), radii.contiguous()
    s1 = mask1.to(torch.int32)
    s2 = None if mask2 is None else mask2.to(torch.int32)
    ex_start, ex_partner = (None, None) if exclusions is None else exclusions.on_device(dev)
    ctx = ctx or _lib.default_context(idx)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream if stream is None else int(stream))
    try:
        n, p_pairs, p_dist, p_over, _ = ctx.find_clashes_dev(coords, radii, s1, s2, N, ex_start, ex_partner, float(overlap), cutoff)
        if n == 0:
            ctx.synchronize()
            return empty
        pairs = torch.empty((n, 2), dtype=torch.int32, device=dev)
        dist = torch.empty(n, dtype=torch.float32, device=dev)
        over = torch.empty(n, dtype=torch.float32, device=dev)
        copy = _lib.load().mkamd_copy_dev                               # the lists are context-owned until the next clash call
        _lib._check(copy(ctx._h, pairs.data_ptr(), p_pairs, n * 8))
        _lib._check(copy(ctx._h, dist.data_ptr(), p_dist, n * 4))
        _lib._check(copy(ctx._h, over.data_ptr(), p_over, n * 4))
        ctx.synchronize()
    finally:
        ctx.set_stream(None)
    pairs = pairs.to(torch.int64)
    order = torch.sort(pairs[:, 0] * N + pairs[:, 1], stable=True).indices            # ties by (a, b) ...
    order = order[torch.sort(over[order], descending=True, stable=True).indices]      # ... under the largest overlap first
    return pairs[order], dist[order], over[order]


# ------------------------------------------------------------------------------------------------
# moleculekit hook
# ------------------------------------------------------------------------------------------------
def install():
    """Swap ``find_clashes`` of an installed ``moleculekit.distance`` for the GPU's.  Returns the original; idempotent; ``uninstall()``
    puts it back.  Independent of the other ``install()`` hooks."""
    import moleculekit.distance as ref

    from .distance import find_clashes

    saved = getattr(ref, "_mkamd_reference_clashes", None)
    if saved is not None:
        return saved
    saved = ref.find_clashes
    ref.find_clashes = find_clashes
    ref._mkamd_reference_clashes = saved
    return saved


def uninstall():
    """Undo ``install()``."""
    import moleculekit.distance as ref

    saved = getattr(ref, "_mkamd_reference_clashes", None)
    if saved is not None:
        ref.find_clashes = saved
        ref._mkamd_reference_clashes = None
