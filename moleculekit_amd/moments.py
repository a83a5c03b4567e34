"""Group moments of trajectory frames on the MI355X (include/mkamd_distance.h "group moments").

The reference's ``MetricCoordinate``, ``MetricGyration``, ``MetricFluctuation`` and ``MetricSphericalCoordinate`` all align every frame
to a reference and then reduce small sets of atoms to weighted first and second moments -- a centroid, a centre of mass, a radius
of gyration, a squared deviation from a reference position -- on the host, after ``Molecule.align`` has rewritten the whole
trajectory.  Here the alignment kernels produce each frame's affine and one kernel call gathers only the selected atoms, applies the
affine in registers (the bits ``align_trajectory`` would have stored), sums in double and writes a few numbers per frame and group:
the aligned trajectory is never materialised.

* ``group_moments_trajectory`` / ``fluctuation_trajectory`` -- CUDA tensors, frame-major ``[F, N, 3]`` float32, asynchronous.
* ``group_moments`` / ``fluctuation`` -- numpy arrays ``[N, 3, F]`` through the host entry points (only the rows of the atoms the
  groups and the alignment selection name travel).
* ``MetricCoordinate``, ``MetricGyration``, ``MetricFluctuation``, ``MetricSphericalCoordinate`` -- the reference's projections
  (``project`` / ``getMapping``); ``install()`` / ``uninstall()`` swap ``project`` of an installed moleculekit's four classes.

Periodic wrapping (the reference's ``mol.wrap(centersel)`` in front of the alignment) is on the device too (``moleculekit_amd.wrap``),
and opt-in here: by default ``pbc=True`` (the reference's default) with a box that is not all zeros still raises
``NotImplementedError``, as before; with ``wrap_on_device=True`` ``project`` first wraps -- only the centre selection and the bonded
groups (``mol.bonds``) of the atoms the projection and its alignment name travel -- and goes on with the wrapped atoms on the device.
Once ``wrap.install()`` has swapped ``Molecule.wrap``, the installed-mode projections below wrap on the device with no change here.
There is no CPU path: without the library or a device every entry point raises.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._masses import ATOMIC_MASSES
from .sasa import _Mapping, _coords, _mask, sequence_id

_F32, _F64, _U32 = np.float32, np.float64, np.uint32
MODES = {"center": 0, "gyration": 1, "spherical": 2}                # include/mkamd_distance.h: MKAMD_MOM_*


def _mode(out):
    if out not in MODES:
        raise ValueError(f"out must be one of {sorted(MODES)}, got {out!r}")
    return MODES[out]


def _shape(F, G, mode):
    return {0: (F, 3 * G), 1: (F, G, 4), 2: (F, 3)}[mode]


def _np(a):
    return np.asarray(a.cpu() if hasattr(a, "cpu") else a)


def _indices(a, n, name):
    a = _np(a)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{name} must be integer atom indices, got {a.dtype.name}")
    a = a.astype(np.int64).reshape(-1)
    a = np.where(a < 0, a + n, a)
    if a.size and (a.min() < 0 or a.max() >= n):
        raise IndexError(f"{name}: atom index out of range for {n} atoms")
    return np.ascontiguousarray(a, dtype=_U32)


def _csr(groups, n):
    """a LIST of index arrays, or the TUPLE ``(atoms, offsets)`` -> (atoms uint32 [n_sel], offsets uint32 [G + 1]); no group may be empty"""
    if isinstance(groups, tuple):                               # (a tuple is the CSR pair; a LIST holds one index array per group)
        if len(groups) != 2:
            raise ValueError("groups: a tuple must be (atoms, offsets)")
        atoms, offsets = _indices(groups[0], n, "groups"), _np(groups[1]).astype(np.int64).reshape(-1)
        if offsets.size < 1 or offsets[0] != 0 or offsets[-1] != atoms.size:
            raise ValueError("groups: offsets must run from 0 to the number of group atoms")
    else:
        parts = [_indices(g, n, "groups") for g in groups]
        atoms = np.concatenate(parts) if parts else np.zeros(0, _U32)
        offsets = np.zeros(len(parts) + 1, np.int64)
        offsets[1:] = np.cumsum([p.size for p in parts])
    if offsets.size > 1 and np.any(np.diff(offsets) <= 0):
        raise ValueError("groups: an empty group")
    if atoms.size >= 2 ** 30:
        raise ValueError("groups: too many atoms")
    return np.ascontiguousarray(atoms, dtype=_U32), np.ascontiguousarray(offsets, dtype=_U32)


def _weights(weights, n_sel):
    if weights is None:
        return None
    w = _np(weights)
    if w.shape != (n_sel,):
        raise ValueError(f"weights must have one entry per group atom ({n_sel}), got shape {w.shape}")
    return np.ascontiguousarray(w, dtype=_F32)


def _device_inputs(xyz, affine, stream, ctx):
    import torch

    if not (hasattr(xyz, "is_cuda") and xyz.is_cuda):
        raise TypeError("xyz: a CUDA tensor is required (there is no CPU path)")
    if xyz.dtype != torch.float32:
        raise ValueError(f"xyz must be float32, got {xyz.dtype}")
    if xyz.dim() == 2:
        xyz = xyz.unsqueeze(0)
    if xyz.dim() != 3 or xyz.shape[2] != 3:
        raise ValueError(f"xyz must be [frames, atoms, 3] (or [atoms, 3]), got {tuple(xyz.shape)}")
    xyz = xyz.contiguous()
    dev = xyz.device
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    dev = torch.device("cuda", idx)
    F = int(xyz.shape[0])
    if affine is not None:
        if not (hasattr(affine, "is_cuda") and affine.is_cuda and affine.dtype == torch.float64 and tuple(affine.shape) == (F, 12)
                and affine.device == xyz.device):
            raise ValueError(f"affine must be a float64 CUDA tensor [{F}, 12] on the device of xyz (align.kabsch_transforms)")
        affine = affine.contiguous()
    if ctx is not None and ctx.device != idx:
        raise ValueError(f"ctx lives on GPU {ctx.device} but the tensors are on cuda:{idx}")
    ctx = ctx or _lib.default_context(idx)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream if stream is None else int(stream))
    return xyz, affine, dev, ctx


def group_moments_trajectory(xyz, groups, *, weights=None, affine=None, out="center", stream=None, ctx=None):
    """Moments of groups of atoms in every frame of a device-resident trajectory.  ``xyz``: CUDA float32 ``[F, N, 3]``; ``groups``: a
    list of index arrays or the tuple ``(atoms, offsets)`` (CSR, no empty group); ``weights``: one per group atom (default 1); ``affine``:
    ``None`` or the float64 ``[F, 12]`` of ``align.kabsch_transforms`` -- every atom is then moved by its frame's transform first.
    ``out``: ``"center"`` -> float32 CUDA ``[F, 3 G]`` (column ``c * G + g``: the reference's X..., Y..., Z... order),
    ``"gyration"`` -> ``[F, G, 4]`` (total and about the x, y, z axes), ``"spherical"`` -> ``[F, 3]`` (r, theta, phi of
    centroid(group 0) - centroid(group 1); exactly two groups, no weights).  Asynchronous on ``stream`` (an integer ``hipStream_t``;
    default torch's current stream)."""
    import torch

    mode = _mode(out)
    xyz, affine, dev, ctx = _device_inputs(xyz, affine, stream, ctx)
    F, N = int(xyz.shape[0]), int(xyz.shape[1])
    atoms, offsets = _csr(groups, N)
    G = int(offsets.size) - 1
    w = _weights(weights, int(atoms.size))
    if mode == 2 and (G != 2 or w is not None):
        raise ValueError("out='spherical' takes exactly two unweighted groups (target, reference)")
    res = torch.empty(_shape(F, G, mode), dtype=torch.float32, device=dev)
    if F == 0 or G == 0:
        return res
    d_atoms = torch.as_tensor(atoms.view(np.int32), device=dev)
    d_offs = torch.as_tensor(offsets.view(np.int32), device=dev)
    d_w = torch.as_tensor(w, device=dev) if w is not None else None
    _lib._check(_lib.load().mkamd_group_moments_dev(ctx._h, xyz.data_ptr(), N, F, affine.data_ptr() if affine is not None else None,
                                                    d_atoms.data_ptr(), d_offs.data_ptr(), d_w.data_ptr() if d_w is not None else None, G,
                                                    int(atoms.size), int(np.diff(offsets.astype(np.int64)).max()), mode, res.data_ptr()))
    if stream is not None:
        ctx.synchronize()          # (the index tensors are torch's: their memory must not be reused before a foreign stream has read it)
    return res


def _fluct_groups(groups, n_sel):
    """``None`` or a list of arrays of POSITIONS in ``atoms`` that tile 0 .. n_sel - 1 in order (or their offsets) -> uint32 offsets"""
    if groups is None:
        return None
    g = _np(groups) if not isinstance(groups, (list, tuple)) else None
    if g is not None and g.ndim == 1:
        offsets = g.astype(np.int64)
    else:
        flat = np.concatenate([np.asarray(p).reshape(-1) for p in groups]) if len(groups) else np.zeros(0, np.int64)
        if not np.array_equal(flat, np.arange(n_sel)):
            raise ValueError("groups must list the positions 0 .. n_sel - 1 of atoms in order (contiguous groups)")
        offsets = np.zeros(len(groups) + 1, np.int64)
        offsets[1:] = np.cumsum([np.asarray(p).size for p in groups])
    if offsets.size < 1 or offsets[0] != 0 or offsets[-1] != n_sel or np.any(np.diff(offsets) <= 0):
        raise ValueError("groups: offsets must run from 0 to n_sel without an empty group")
    return np.ascontiguousarray(offsets, dtype=_U32)


def _ref(ref, n_sel):
    if ref is None:
        return None
    r = _np(ref)
    if r.shape != (n_sel, 3):
        raise ValueError(f"ref must have shape ({n_sel}, 3), got {r.shape}")
    return np.ascontiguousarray(r, dtype=_F64)


def fluctuation_trajectory(xyz, atoms, *, ref=None, groups=None, affine=None, stream=None, ctx=None):
    """Squared deviation of atoms from a reference position in every frame of a device-resident trajectory: float64 CUDA
    ``[F, n_sel]`` = sum_c (x_c - ref_c)^2 for the listed ``atoms``, or with ``groups`` (contiguous runs of positions in ``atoms``, or
    their offsets) ``[F, G]``: its mean over each group.  ``ref``: ``[n_sel, 3]`` (array or tensor, used as float64), default the mean
    over all frames of the (transformed) positions.  ``affine`` as in ``group_moments_trajectory``."""
    import torch

    xyz, affine, dev, ctx = _device_inputs(xyz, affine, stream, ctx)
    F, N = int(xyz.shape[0]), int(xyz.shape[1])
    a = _indices(atoms, N, "atoms")
    n_sel = int(a.size)
    offsets = _fluct_groups(groups, n_sel)
    G = 0 if offsets is None else int(offsets.size) - 1
    res = torch.empty((F, n_sel if offsets is None else G), dtype=torch.float64, device=dev)
    if F == 0 or n_sel == 0:
        return res
    d_atoms = torch.as_tensor(a.view(np.int32), device=dev)
    d_offs = torch.as_tensor(offsets.view(np.int32), device=dev) if offsets is not None else None
    if ref is not None and hasattr(ref, "is_cuda") and ref.is_cuda:
        if tuple(ref.shape) != (n_sel, 3):
            raise ValueError(f"ref must have shape ({n_sel}, 3), got {tuple(ref.shape)}")
        d_ref = ref.to(device=dev, dtype=torch.float64).contiguous()
        if stream is not None:
            torch.cuda.current_stream(dev).synchronize()       # (the conversion ran on torch's stream; the kernels go to a foreign one)
    else:
        r = _ref(ref, n_sel)
        d_ref = torch.as_tensor(r, device=dev) if r is not None else None
    _lib._check(_lib.load().mkamd_fluctuation_dev(ctx._h, xyz.data_ptr(), N, F, affine.data_ptr() if affine is not None else None,
                                                  d_atoms.data_ptr(), n_sel, d_offs.data_ptr() if d_offs is not None else None, G,
                                                  int(np.diff(offsets.astype(np.int64)).max()) if offsets is not None else 1,
                                                  d_ref.data_ptr() if d_ref is not None else None, res.data_ptr()))
    if stream is not None:
        ctx.synchronize()
    return res


def _align_inputs(align, N):
    """``None`` or ``(alnsel, alnref)``: the atoms of every frame (mask or indices) that are superposed on the positions ``alnref``
    float32 ``[n_aln, 3]``"""
    if align is None:
        return None, None
    sel, ref = align
    s = np.ascontiguousarray(np.flatnonzero(_mask(sel, N, "alnsel")) if _np(sel).dtype == bool else _indices(sel, N, "alnsel"), dtype=_U32)
    r = np.ascontiguousarray(_np(ref), dtype=_F32)
    if r.shape != (s.size, 3):
        raise ValueError(f"align: alnsel picks {s.size} atoms, alnref has shape {r.shape}")
    return s, r


def group_moments(coords, groups, *, weights=None, align=None, out="center", ctx=None):
    """``group_moments_trajectory`` on host arrays: ``coords`` float32 ``[N, 3, F]`` (``Molecule.coords``).  ``align``: ``None`` or
    ``(alnsel, alnref)`` -- every frame is first superposed with its atoms ``alnsel`` on the positions ``alnref`` ``[n_aln, 3]``.
    Returns float32 ``[F, 3 G]`` / ``[F, G, 4]`` / ``[F, 3]`` by ``out``."""
    mode = _mode(out)
    coords = _coords(coords)
    N, _, F = coords.shape
    atoms, offsets = _csr(groups, N)
    G = int(offsets.size) - 1
    w = _weights(weights, int(atoms.size))
    if mode == 2 and (G != 2 or w is not None):
        raise ValueError("out='spherical' takes exactly two unweighted groups (target, reference)")
    s, r = _align_inputs(align, N)
    res = np.zeros(_shape(F, G, mode), _F32)
    if F and G:
        ctx = ctx or _lib.default_context()
        _lib._check(_lib.load().mkamd_group_moments_host(ctx._h, _lib._ptr(coords), N, F, _lib._ptr(s), _lib._ptr(r), 0 if s is None else int(s.size),
                                                         _lib._ptr(atoms), _lib._ptr(offsets), _lib._ptr(w), G, mode, _lib._ptr(res)))
    return res


def fluctuation(coords, atoms, *, ref=None, groups=None, align=None, ctx=None):
    """``fluctuation_trajectory`` on host arrays: ``coords`` float32 ``[N, 3, F]``; ``align`` as in ``group_moments``.  Returns
    float64 ``[F, n_sel]`` or ``[F, G]``."""
    coords = _coords(coords)
    N, _, F = coords.shape
    a = _indices(atoms, N, "atoms")
    n_sel = int(a.size)
    offsets = _fluct_groups(groups, n_sel)
    G = 0 if offsets is None else int(offsets.size) - 1
    r = _ref(ref, n_sel)
    s, ar = _align_inputs(align, N)
    res = np.zeros((F, n_sel if offsets is None else G), _F64)
    if F and n_sel:
        ctx = ctx or _lib.default_context()
        _lib._check(_lib.load().mkamd_fluctuation_host(ctx._h, _lib._ptr(coords), N, F, _lib._ptr(s), _lib._ptr(ar), 0 if s is None else int(s.size),
                                                       _lib._ptr(a), n_sel, _lib._ptr(offsets), G, _lib._ptr(r), _lib._ptr(res)))
    return res


# ------------------------------------------------------------------------------------------------
# the projections
# ------------------------------------------------------------------------------------------------
def _natoms(mol):
    return int(np.asarray(mol.coords).shape[0])


def _sel(mol, sel, name, message):
    """a boolean mask or an index array (``"all"`` is understood) over the atoms of ``mol`` -> bool [N]; ``message``: the reference's
    error for a selection of no atoms"""
    n = _natoms(mol)
    if isinstance(sel, str):
        if sel != "all":
            raise TypeError(f"{name}: a boolean mask or an integer index array is required (this package has no selection language)")
        m = np.ones(n, bool)
    else:
        m = _mask(sel, n, name)
    if not m.any():
        raise RuntimeError(message)
    return m


def _needs_wrap(mol, pbc):
    """``pbc`` with a box that is there and not all zeros (a missing or all-zero box makes ``pbc=True`` the no-op it is in the reference)"""
    if not pbc:
        return False
    box = getattr(mol, "box", None)
    return not (box is None or np.size(box) == 0 or not np.any(np.asarray(box) != 0))


def _check_pbc(mol, pbc):
    """the pbc rule of the default (``wrap_on_device=False``): wrapping is not done unasked"""
    if _needs_wrap(mol, pbc):
        raise NotImplementedError("periodic wrapping is not done on the device: wrap the molecule first (Molecule.wrap) or pass pbc=False "
                                  "(or construct the projection with wrap_on_device=True)")


def _element_masses(mol, idx):
    return np.array([ATOMIC_MASSES[str(e)] for e in np.asarray(mol.element)[idx]], dtype=_F64)


def _frame0(mol, idx):
    """positions float32 [n, 3] of the atoms idx in frame 0 of mol"""
    c = np.asarray(mol.coords)
    if c.ndim == 2:
        c = c[:, :, None]
    return np.ascontiguousarray(c[idx, :, 0], dtype=_F32)


def _frame_table(cols):
    try:
        from pandas import DataFrame
    except ImportError:
        return _Mapping(cols)
    return DataFrame(cols)


class _Aligned:
    """what the four projections share: the pbc rule and the alignment of every frame on a reference, as ``(alnsel, alnref)``"""

    def _init_align(self, refmol, trajalnsel, refalnsel, centersel, pbc, wrap_on_device=False):
        self._wrap_on_device = bool(wrap_on_device)
        self._refmol = refmol
        self._trajalnsel = trajalnsel
        self._refalnsel = refalnsel if refalnsel is not None else trajalnsel
        self._centersel = centersel
        self._pbc = pbc
        if refmol is not None and trajalnsel is None:
            self._trajalnsel = "protein and name CA"            # the reference's default: a selection string, refused when it is needed
            self._refalnsel = refalnsel if refalnsel is not None else self._trajalnsel

    def _align(self, mol):
        """``None`` or ``(indices in mol, positions [n, 3])``: the reference's ``mol.align(trajalnsel[, refmol, refsel])`` (frame 0 of
        the reference molecule, or of ``mol`` itself)"""
        if self._trajalnsel is None:
            return None
        sel = np.flatnonzero(_sel(mol, self._trajalnsel, "trajalnsel", "Alignment selection resulted in 0 atoms."))
        if self._refmol is None:
            return sel, _frame0(mol, sel)
        refsel = np.flatnonzero(_sel(self._refmol, self._refalnsel, "refalnsel", "Alignment selection resulted in 0 atoms."))
        if refsel.size != sel.size:
            raise ValueError(f"trajalnsel picks {sel.size} atoms and refalnsel {refsel.size}")
        return sel, _frame0(self._refmol, refsel)

    def _wrapped(self, mol, named, ctx):
        """``None``: project ``mol.coords`` as they are (no wrapping is due).  Else ``_WrappedRows``: the trajectory wrapped on the
        device, cut down to the atoms that matter -- ``wrap_on_device=True``; without it the pbc rule raises."""
        if not _needs_wrap(mol, self._pbc):
            return None
        _check_pbc(mol, self._pbc and not self._wrap_on_device)
        align_idx = np.zeros(0, np.int64) if self._trajalnsel is None else \
            np.flatnonzero(_sel(mol, self._trajalnsel, "trajalnsel", "Alignment selection resulted in 0 atoms."))
        return _WrappedRows(mol, np.flatnonzero(_sel(mol, self._centersel, "centersel", "Center selection resulted in 0 atoms.")),
                            np.concatenate([np.asarray(named, np.int64).reshape(-1), align_idx]), ctx)

    def _affine(self, mol, w):
        """the frames' transforms on the wrapped rows ``w`` (``None``: no alignment); the reference aligns on frame 0 of the WRAPPED
        molecule where there is no refmol"""
        from . import align as _align_mod

        if self._trajalnsel is None:
            return None
        sel, ref = self._align(mol)
        rows = w.row_of(sel)
        import torch

        if self._refmol is None:
            ref = w.xyz[0].index_select(0, torch.as_tensor(rows.astype(np.int64), device=w.xyz.device)).cpu().numpy()
        d_ref = torch.as_tensor(np.ascontiguousarray(ref, dtype=_F32), device=w.xyz.device)
        return _align_mod.kabsch_transforms(w.xyz, d_ref, rows, refsel=np.arange(rows.size), ctx=w.ctx)[0]


class _WrappedRows:
    """A molecule's trajectory wrapped on the device (``wrap.wrap_trajectory``, in place on the upload), holding only the rows that
    matter: the centre selection and every atom of each bonded group with a named atom.  ``xyz``: CUDA float32 ``[F, M, 3]``;
    ``row_of(atoms)``: their rows in it."""

    def __init__(self, mol, centersel, named, ctx):
        import torch

        from . import wrap as _wrap

        coords = _coords(np.asarray(mol.coords))
        N, _, F = coords.shape
        box = np.asarray(mol.box)
        if box.shape[1] != F:
            raise RuntimeError(_wrap._FRAMES)
        angles = getattr(mol, "boxangles", None)
        if angles is not None and np.size(angles) and np.any(np.asarray(angles) != 90):
            raise NotImplementedError("the box is triclinic (boxangles != 90): the unit cells 'rectangular', 'triclinic' and 'compact' "
                                      "of a triclinic box are not wrapped on the device")
        starts = _wrap.bonded_groups(getattr(mol, "bonds", None), N)
        self.rows, packed = _wrap.travel_rows(starts, named, centersel)
        self.ctx = ctx or _lib.default_context()
        dev = torch.device("cuda", self.ctx.device)
        host = np.ascontiguousarray(np.transpose(coords[self.rows.astype(np.int64)], (2, 0, 1)))          # [F, M, 3]
        self.xyz = torch.as_tensor(host, device=dev)
        _wrap.wrap_trajectory(self.xyz, np.ascontiguousarray(box, dtype=_F32), packed, centersel=self.row_of(centersel), out=self.xyz,
                              ctx=self.ctx)

    def row_of(self, atoms):
        return np.ascontiguousarray(np.searchsorted(self.rows, np.asarray(atoms, np.int64)), dtype=_U32)

    def csr(self, groups):
        """a list of index arrays or the (atoms, offsets) pair, in rows"""
        if isinstance(groups, tuple):
            return (self.row_of(groups[0]), groups[1])
        return [self.row_of(g) for g in groups]


class MetricCoordinate(_Aligned):
    """The reference's ``moleculekit.projections.metriccoordinate.MetricCoordinate`` on the GPU: ``project(mol)`` -> float32
    ``[numFrames, 3 n]`` (all X, then all Y, then all Z) of the atoms of ``atomsel`` or, with ``groupsel`` ``"all"`` / ``"residue"``,
    of the centroid (``groupreduce="centroid"``) or centre of mass (``"com"``, element masses as float32) of each group;
    ``getMapping(mol)``.  Selections are boolean masks or integer index arrays (``"all"`` is understood).  ``pbc=True`` (the
    default) with a box that is not all zeros raises ``NotImplementedError`` unless ``wrap_on_device=True``: every frame is then wrapped
    on the device first, around ``centersel`` (a mask or indices) by the bonded groups of ``mol.bonds`` (``moleculekit_amd.wrap``)."""

    def __init__(self, atomsel, refmol=None, trajalnsel=None, refalnsel=None, centersel="protein", groupsel=None, groupreduce="com", pbc=True,
                 wrap_on_device=False):
        if atomsel is None:
            raise ValueError("Atom selection cannot be None")
        self._atomsel = atomsel
        self._groupsel = groupsel
        self._groupreduce = groupreduce
        self._init_align(refmol, trajalnsel, refalnsel, centersel, pbc, wrap_on_device)

    def _groups(self, mol):
        """(atom indexes [n], list of groups of atom indexes or None)"""
        idx = np.flatnonzero(_sel(mol, self._atomsel, "atomsel", "Atom selection resulted in 0 atoms."))
        if self._groupsel is None:
            return idx, None
        if self._groupsel == "all":
            return idx, [idx]
        if self._groupsel == "residue":                          # by the VALUE of resid among the selected atoms, as the reference
            resids = np.asarray(mol.resid)[idx]
            return idx, [idx[resids == uq] for uq in np.unique(resids)]
        raise RuntimeError("Invalid groupsel option. Can only be 'all' or 'residue'")

    def project(self, mol, ctx=None):
        _check_pbc(mol, self._pbc and not self._wrap_on_device)
        idx, groups = self._groups(mol)
        weights = None
        if groups is None:
            groups = (idx, np.arange(idx.size + 1))
        elif self._groupreduce == "com":
            weights = np.concatenate([_element_masses(mol, g).astype(_F32) for g in groups])
        elif self._groupreduce != "centroid":
            raise RuntimeError("Invalid groupreduce option. Can onlye be 'centroid' or 'com'")
        w = self._wrapped(mol, idx, ctx)
        if w is None:
            return group_moments(mol.coords, groups, weights=weights, align=self._align(mol), out="center", ctx=ctx)
        return group_moments_trajectory(w.xyz, w.csr(groups), weights=weights, affine=self._affine(mol, w), out="center", ctx=w.ctx).cpu().numpy()

    def getMapping(self, mol):
        idx, groups = self._groups(mol)
        types_, indexes, description = [], [], []
        for xyz in ("X", "Y", "Z"):
            if groups is None:
                for i in idx:
                    types_.append("coordinate")
                    indexes.append(i)
                    description.append(f"{xyz} coordinate of {mol.resname[i]} {mol.resid[i]} {mol.name[i]}")
            else:
                for group in groups:
                    types_.append("coordinate")
                    indexes.append(group)
                    description.append(f"{xyz} {self._groupreduce} coordinate of group")
        return _frame_table({"type": types_, "atomIndexes": indexes, "description": description})


class MetricGyration(_Aligned):
    """The reference's ``MetricGyration`` on the GPU: ``project(mol)`` -> float32 ``[numFrames, 4]``: the mass-weighted radius of
    gyration of ``atomsel`` and its components about the x, y and z axes.  ``mol.masses``, or element masses where any mass is 0."""

    def __init__(self, atomsel, refmol=None, trajalnsel=None, refalnsel=None, centersel="protein", pbc=True, wrap_on_device=False):
        if atomsel is None:
            raise ValueError("Atom selection cannot be None")
        self._atomsel = atomsel
        self._init_align(refmol, trajalnsel, refalnsel, centersel, pbc, wrap_on_device)

    def _masses(self, mol, idx):
        masses = np.asarray(mol.masses)[idx]
        if np.any(masses == 0):
            masses = _element_masses(mol, idx)
            if np.sum(masses) == 0:
                raise RuntimeError("The molecule selection has 0 total mass. Please read atom masses from a prmtop or psf file.")
        return masses

    def project(self, mol, ctx=None):
        _check_pbc(mol, self._pbc and not self._wrap_on_device)
        idx = np.flatnonzero(_sel(mol, self._atomsel, "atomsel", "Atom selection resulted in 0 atoms."))
        w = self._wrapped(mol, idx, ctx)
        if w is None:
            res = group_moments(mol.coords, [idx], weights=self._masses(mol, idx), align=self._align(mol), out="gyration", ctx=ctx)
        else:
            res = group_moments_trajectory(w.xyz, w.csr([idx]), weights=self._masses(mol, idx), affine=self._affine(mol, w), out="gyration",
                                           ctx=w.ctx).cpu().numpy()
        return res[:, 0, :]

    def getMapping(self, mol):
        idx = np.flatnonzero(_sel(mol, self._atomsel, "atomsel", "Atom selection resulted in 0 atoms."))
        return _frame_table({"type": ["rog"] * 4, "atomIndexes": [idx] * 4,
                             "description": ["Radius of gyration", "x component", "y component", "z component"]})


class MetricFluctuation(MetricCoordinate):
    """The reference's ``MetricFluctuation`` on the GPU: ``project(mol)`` -> float64 ``[numFrames, n]`` -- the squared distance of
    every atom of ``atomsel`` from its mean position over the (aligned) trajectory or, with a ``refmol``, from its position in the
    ``refmol`` aligned on itself -- or with ``mode="residue"`` ``[numFrames, R]``: the mean over the atoms of each residue
    (``sequenceID(mol.resid)`` over the whole molecule).  The default ``trajalnsel`` is the reference's selection STRING, which this
    package cannot evaluate: pass a mask or indices (``project`` raises ``TypeError`` otherwise)."""

    def __init__(self, atomsel, refmol=None, trajalnsel="protein and name CA", refalnsel=None, centersel="protein", pbc=True, mode="atom",
                 wrap_on_device=False):
        super().__init__(atomsel, refmol=refmol, trajalnsel=trajalnsel, refalnsel=refalnsel, centersel=centersel, pbc=pbc,
                         wrap_on_device=wrap_on_device)
        self._mode = mode

    def _residues(self, mol, idx):
        if self._mode == "atom":
            return None
        if self._mode != "residue":
            raise RuntimeError(f"Invalid mode {self._mode} given. Choose between `atom` and `residue`")
        return sequence_id((np.asarray(mol.resid),))[idx]

    def project(self, mol, ctx=None):
        _check_pbc(mol, self._pbc and not self._wrap_on_device)
        idx = np.flatnonzero(_sel(mol, self._atomsel, "atomsel", "Atom selection resulted in 0 atoms."))
        res_of = self._residues(mol, idx)
        ref = None
        if self._refmol is not None:
            # the refmol through the same pipeline, aligned onto itself with refalnsel: float32 positions, as the reference's
            refbox = getattr(self._refmol, "box", None)
            wrapref = self._pbc and not (refbox is None or np.size(refbox) == 0 or np.all(np.asarray(refbox) == 0))
            rc = MetricCoordinate(self._atomsel, refmol=self._refmol, trajalnsel=self._refalnsel, refalnsel=self._refalnsel,
                                  centersel=self._centersel, pbc=wrapref, wrap_on_device=self._wrap_on_device).project(self._refmol, ctx=ctx)
            if rc.shape[0] != 1 or rc.shape[1] != 3 * idx.size:
                raise ValueError(f"refmol must have one frame and the atoms of atomsel; its projection has shape {rc.shape}")
            ref = rc.reshape(3, idx.size).T.astype(_F64)
        groups = None
        if res_of is not None:
            order = np.argsort(res_of, kind="stable")             # the atoms of a residue contiguous, residues ascending
            idx, res_of = idx[order], res_of[order]
            ref = ref[order] if ref is not None else None
            groups = np.r_[0, np.flatnonzero(np.diff(res_of)) + 1, idx.size]
        w = self._wrapped(mol, idx, ctx)
        if w is None:
            return fluctuation(mol.coords, idx, ref=ref, groups=groups, align=self._align(mol), ctx=ctx)
        return fluctuation_trajectory(w.xyz, w.row_of(idx), ref=ref, groups=groups, affine=self._affine(mol, w), ctx=w.ctx).cpu().numpy()

    def getMapping(self, mol):
        idx = np.flatnonzero(_sel(mol, self._atomsel, "atomsel", "Atom selection resulted in 0 atoms."))
        res_of = self._residues(mol, idx)
        types_, indexes, description = [], [], []
        if res_of is None:
            for i in idx:
                types_.append("fluctuation")
                indexes.append(i)
                description.append(f"Fluctuation of {mol.resname[i]} {mol.resid[i]} {mol.name[i]}")
        else:
            for r in np.unique(res_of):
                i = idx[np.flatnonzero(res_of == r)[0]]
                types_.append("fluctuation")
                indexes.append(i)
                description.append(f"Mean fluctuation of {mol.resname[i]} {mol.resid[i]}")
        return _frame_table({"type": types_, "atomIndexes": indexes, "description": description})


class MetricSphericalCoordinate(_Aligned):
    """The reference's ``MetricSphericalCoordinate`` on the GPU: ``project(mol)`` -> float32 ``[numFrames, 3]``: r, theta, phi of the
    vector from the centroid of ``refcom`` to the centroid of ``targetcom`` after aligning every frame on ``refmol``."""

    def __init__(self, refmol, targetcom, refcom, trajalnsel="protein and name CA", refalnsel=None, centersel="protein", pbc=True,
                 wrap_on_device=False):
        self._targetcom = targetcom
        self._refcom = refcom
        self._init_align(refmol, trajalnsel, refalnsel, centersel, pbc, wrap_on_device)

    def _coms(self, mol):
        return (np.flatnonzero(_sel(mol, self._targetcom, "targetcom", "Atom selection for `targetcom` resulted in 0 atoms.")),
                np.flatnonzero(_sel(mol, self._refcom, "refcom", "Atom selection for `refcom` resulted in 0 atoms.")))

    def project(self, mol, ctx=None):
        _check_pbc(mol, self._pbc and not self._wrap_on_device)
        target, ref = self._coms(mol)
        w = self._wrapped(mol, np.concatenate([target, ref]), ctx)
        if w is None:
            return group_moments(mol.coords, [target, ref], align=self._align(mol), out="spherical", ctx=ctx)
        return group_moments_trajectory(w.xyz, w.csr([target, ref]), affine=self._affine(mol, w), out="spherical", ctx=w.ctx).cpu().numpy()

    def getMapping(self, mol):
        target, ref = self._coms(mol)
        return _frame_table({"type": ["r", "theta", "phi"], "atomIndexes": [[target, ref]] * 3, "description": ["r", "theta", "phi"]})


# ------------------------------------------------------------------------------------------------
# moleculekit hook
# ------------------------------------------------------------------------------------------------
def _ref_prepare(self, mol, centersel):
    """the reference's own preamble of ``project``: a copy, wrapped by its ``Molecule.wrap`` where ``_pbc`` (on the device once
    ``wrap.install()`` has swapped that method)"""
    mol = mol.copy()
    if self._pbc:
        mol.wrap(centersel)
    return mol


def _ref_align(self, mol, orig):
    """``(indices, positions)`` of the reference object's alignment, selections from its own ``_getMolProp``"""
    trajalnsel = self._getMolProp(orig, "trajalnsel")
    if trajalnsel is None:
        return None
    sel = np.flatnonzero(trajalnsel)
    if self._refmol is None:
        return sel, _frame0(mol, sel)
    # the reference keeps refmol.atomselect(refalnsel), a MASK over the refmol's atoms, in its cache (whatever form refalnsel was given in)
    return sel, _frame0(self._refmol, _mask_indices(self._getMolProp(orig, "refalnsel")))


def _mask_indices(sel):
    """a boolean mask -> the indices it marks; an integer index array -> itself"""
    a = np.asarray(sel)
    return np.flatnonzero(a) if a.dtype == bool else a.astype(np.int64).reshape(-1)


def _reference_coordinate(self, mol):
    orig = mol
    mol = _ref_prepare(self, mol, self._getMolProp(mol, "centersel") if self._pbc else None)
    idx = np.flatnonzero(self._getMolProp(orig, "atomsel"))
    weights = None
    if self._groupsel is None:
        groups = (idx, np.arange(idx.size + 1))
    else:
        if self._groupsel == "all":
            groups = [idx]
        elif self._groupsel == "residue":
            resids = mol.resid[idx]
            groups = [idx[resids == uq] for uq in np.unique(resids)]
        else:
            raise RuntimeError("Invalid groupsel option. Can only be 'all' or 'residue'")
        if self._groupreduce == "com":
            from moleculekit.periodictable import periodictable

            weights = np.array([periodictable[el].mass for el in mol.element[np.concatenate(groups)]], dtype=_F32)
        elif self._groupreduce != "centroid":
            raise RuntimeError("Invalid groupreduce option. Can onlye be 'centroid' or 'com'")
    return group_moments(mol.coords, groups, weights=weights, align=_ref_align(self, mol, orig), out="center")


def _reference_gyration(self, mol):
    orig = mol
    mol = _ref_prepare(self, mol, self._getMolProp(mol, "centersel") if self._pbc else None)
    idx = np.flatnonzero(self._getMolProp(orig, "atomsel"))
    masses = self._getMolProp(orig, "masses")
    return group_moments(mol.coords, [idx], weights=masses, align=_ref_align(self, mol, orig), out="gyration")[:, 0, :]


def _reference_spherical(self, mol):
    orig = mol
    mol = _ref_prepare(self, mol, self._centersel)
    sel = np.flatnonzero(self._getMolProp(orig, "trajalnsel"))
    align = (sel, _frame0(self._refmol, _mask_indices(self._refalnsel)))      # (a mask: the constructor stores refmol.atomselect(refalnsel))
    groups = [np.flatnonzero(self._getMolProp(orig, "targetcom")), np.flatnonzero(self._getMolProp(orig, "refcom"))]
    return group_moments(mol.coords, groups, align=align, out="spherical")


def _reference_fluctuation(self, mol):
    from moleculekit.util import sequenceID

    orig = mol
    mol = _ref_prepare(self, mol, self._getMolProp(mol, "centersel") if self._pbc else None)
    idx = np.flatnonzero(self._getMolProp(orig, "atomsel"))
    if self._mode not in ("atom", "residue"):
        raise RuntimeError(f"Invalid mode {self._mode} given. Choose between `atom` and `residue`")
    ref = None
    if self._refmol is not None:
        import moleculekit.projections.metriccoordinate as mc

        refbox = self._refmol.box
        wrapref = self._pbc and not (refbox is None or len(refbox) == 0 or np.all(refbox == 0))
        rc = mc.MetricCoordinate(atomsel=self._atomsel, refmol=self._refmol, trajalnsel=self._refalnsel, refalnsel=self._refalnsel,
                                 centersel=self._centersel, pbc=wrapref).project(self._refmol)
        if rc.shape[0] != 1:
            raise ValueError("refmol must have one frame")
        ref = rc.reshape(3, idx.size).T.astype(_F64)
    groups = None
    if self._mode == "residue":
        res_of = sequenceID(mol.resid)[idx]
        order = np.argsort(res_of, kind="stable")
        idx, res_of = idx[order], res_of[order]
        ref = ref[order] if ref is not None else None
        groups = np.r_[0, np.flatnonzero(np.diff(res_of)) + 1, idx.size]
    return fluctuation(mol.coords, idx, ref=ref, groups=groups, align=_ref_align(self, mol, orig))


def _targets():
    import moleculekit.projections.metriccoordinate as mc
    import moleculekit.projections.metricfluctuation as mf
    import moleculekit.projections.metricgyration as mg
    import moleculekit.projections.metricsphericalcoordinate as ms

    return ((mc, mc.MetricCoordinate, _reference_coordinate), (mg, mg.MetricGyration, _reference_gyration),
            (mf, mf.MetricFluctuation, _reference_fluctuation), (ms, ms.MetricSphericalCoordinate, _reference_spherical))


def install():
    """Swap ``project`` of an installed moleculekit's ``MetricCoordinate``, ``MetricGyration``, ``MetricFluctuation`` and
    ``MetricSphericalCoordinate`` for the GPU's: wrapping is the molecule's own ``Molecule.wrap`` (the reference's on the host; the device's once ``wrap.install()`` has swapped it), selections come
    from the object's own ``_getMolProp``, alignment and moments run on the device.  Returns the originals; idempotent;
    ``uninstall()`` puts them back.  Independent of the other ``install()`` hooks."""
    saved = []
    for module, cls, ours in _targets():
        kept = getattr(module, "_mkamd_reference_project", None)
        if kept is None:
            kept = cls.project
            cls.project = ours
            module._mkamd_reference_project = kept
        saved.append(kept)
    return tuple(saved)


def uninstall():
    """Undo ``install()``."""
    for module, cls, _ in _targets():
        kept = getattr(module, "_mkamd_reference_project", None)
        if kept is not None:
            cls.project = kept
            module._mkamd_reference_project = None
