"""Solvent-accessible surface area of trajectory frames on the MI355X (include/mkamd_distance.h "surface area").

The Shrake-Rupley surface the reference's ``MetricSasa`` gets from mdtraj: per atom ``n_points`` sphere points at the atom's radius
plus the probe's, the ones no neighbour buries counted, ``area = 4 pi / n * R^2 * count``.  The kernels repeat the reference's float32
arithmetic operation by operation, in its nanometres, so the counts -- and the areas -- are the reference's.

* ``sasa_trajectory`` -- CUDA tensors, frame-major ``[F, N, 3]`` float32 in Angstrom (the XTC decoder's and ``align_trajectory``'s layout).
* ``sasa`` -- numpy arrays in the reference's ``[N, 3, F]`` layout, through the host entry point (only the kept atoms' rows travel).
* ``MetricSasa`` -- the reference's projection (``project`` / ``getMapping``) with masks or index arrays for selections;
  ``install()`` / ``uninstall()`` swap ``project`` of an installed moleculekit's ``MetricSasa``.

There is no CPU path: without the library or a device every entry point raises.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._sasa_radii import ATOMIC_RADII

_F32 = np.float32


def _mask(sel, n, name):
    """a boolean mask or an index array over n atoms -> bool [n]"""
    a = np.asarray(sel.cpu() if hasattr(sel, "cpu") else sel)
    if a.dtype == bool:
        if a.ndim != 1 or a.shape[0] != n:
            raise IndexError(f"{name}: a boolean mask of {a.shape} over {n} atoms")
        return a.copy()
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{name}: a boolean mask or an integer index array is required (this package has no selection language)")
    a = a.astype(np.int64).reshape(-1)
    a = np.where(a < 0, a + n, a)
    if a.size and (a.min() < 0 or a.max() >= n):
        raise IndexError(f"{name}: atom index out of range for {n} atoms")
    m = np.zeros(n, bool)
    m[a] = True
    return m


def _mapping(atom_mapping, n):
    if atom_mapping is None:
        return np.arange(n, dtype=np.int32)
    m = np.asarray(atom_mapping.cpu() if hasattr(atom_mapping, "cpu") else atom_mapping)
    if m.shape != (n,) or not np.issubdtype(m.dtype, np.integer):
        raise ValueError(f"atom_mapping must be an integer array of {n} entries, got {m.dtype.name} {m.shape}")
    if n and (m.min() < 0 or np.any(np.diff(m) < 0)):
        raise ValueError("atom_mapping must be non-negative and non-decreasing (the atoms of an output column contiguous)")
    return np.ascontiguousarray(m, dtype=np.int32)


def _radii(radii, n, scale_div):
    r = np.asarray(radii.cpu() if hasattr(radii, "cpu") else radii)
    if r.shape != (n,):
        raise ValueError(f"radii must have one entry per atom ({n}), got shape {r.shape}")
    r = np.ascontiguousarray(r, dtype=_F32)
    return r / _F32(scale_div) if scale_div != 1 else r


def _points(n_points):
    n = int(n_points)
    if n < 1:
        raise ValueError("n_points must be at least 1")
    return n


def sasa_trajectory(xyz, radii, *, n_points=960, atom_mapping=None, sel=None, out=None, stream=None, ctx=None):
    """Surface area per frame of a device-resident trajectory.  ``xyz``: CUDA float32 ``[F, N, 3]`` (or ``[N, 3]``) in Angstrom;
    ``radii`` ``[N]`` in Angstrom, probe included (array or tensor).  ``sel`` (mask or indices, default all): the atoms whose area
    is computed -- every atom shields.  ``atom_mapping`` int ``[N]``, non-decreasing (default ``arange(N)``): the output column an
    atom's area is added to (a residue index gives per-residue areas, summed in atom order).  Returns float32 CUDA ``[F, n_out]``
    in square Angstrom (``out``, when given, is overwritten with it); columns without a selected atom are 0.  Runs on ``stream``
    (an integer ``hipStream_t``; default torch's current stream) and returns after the kernels have finished.  Coincident atoms
    (closer than 1e-4 Angstrom) raise ``ValueError``."""
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
    F, N = int(xyz.shape[0]), int(xyz.shape[1])
    n_points = _points(n_points)
    dev = xyz.device
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if ctx is not None and ctx.device != idx:
        raise ValueError(f"ctx lives on GPU {ctx.device} but the tensors are on cuda:{idx}")
    ctx = ctx or _lib.default_context(idx)
    dev = torch.device("cuda", idx)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream if stream is None else int(stream))
    mapping = _mapping(atom_mapping, N)
    mask = (np.ones(N, bool) if sel is None else _mask(sel, N, "sel")).astype(np.int32)
    r = _radii(radii, N, 10)
    n_out = int(mapping.max()) + 1 if N else 0
    if out is not None and not (out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (F, n_out) and out.device == dev):
        raise ValueError(f"out must be a contiguous float32 [{F}, {n_out}] tensor on {dev}")
    work = torch.zeros((F, n_out), dtype=torch.float32, device=dev)
    if N and F:
        d_r, d_map, d_mask = (torch.as_tensor(a, device=dev) for a in (r, mapping, mask))
        _lib._check(_lib.load().mkamd_sasa_dev(ctx._h, xyz.data_ptr(), N, F, d_r.data_ptr(), n_points, d_map.data_ptr(), d_mask.data_ptr(),
                                               10.0, work.data_ptr(), n_out))
    work *= 100
    if out is None:
        return work
    out.copy_(work)
    return out


def _host_call(coords, keep, radii_nm, n_points, mapping, mask, out_nm, ctx):
    """out_nm [F, n_out] float32 (filled by the caller, square nanometres) += the areas; coords float32 [N, 3, F] Angstrom"""
    N, _, F = coords.shape
    n = N if keep is None else int(keep.size)
    if n and F:
        ctx = ctx or _lib.default_context()
        _lib._check(_lib.load().mkamd_sasa_host(ctx._h, _lib._ptr(coords), N, F, _lib._ptr(keep), n, _lib._ptr(radii_nm), int(n_points),
                                                _lib._ptr(mapping), _lib._ptr(mask), 10.0, _lib._ptr(out_nm), int(out_nm.shape[1])))
    return out_nm


def _coords(coords):
    if not isinstance(coords, np.ndarray):
        raise TypeError("coords: a numpy array is required")
    if coords.dtype != np.float32:
        raise ValueError(f"Buffer dtype mismatch for coords: expected float32, got {coords.dtype.name}")
    if coords.ndim == 2:
        coords = coords[:, :, None]
    if coords.ndim != 3 or coords.shape[1] != 3:
        raise ValueError(f"coords must be (natoms, 3, nframes), got shape {coords.shape}")
    return np.ascontiguousarray(coords)


def sasa(coords, radii, *, n_points=960, atom_mapping=None, sel=None, keep=None, ctx=None):
    """``sasa_trajectory`` on host arrays in the reference's layout: ``coords`` float32 ``[N, 3, F]`` in Angstrom (``Molecule.coords``).
    ``keep`` (mask or indices, default all): the atoms that make up the system -- the others neither shield nor travel to the
    device; ``radii`` (Angstrom, probe included), ``atom_mapping`` and ``sel`` have one entry per KEPT atom, in atom order.
    Returns float32 ``[F, n_out]`` in square Angstrom."""
    coords = _coords(coords)
    N, _, F = coords.shape
    n_points = _points(n_points)
    kept = None if keep is None else np.ascontiguousarray(np.flatnonzero(_mask(keep, N, "keep")), dtype=np.uint32)
    n = N if kept is None else int(kept.size)
    mapping = _mapping(atom_mapping, n)
    mask = (np.ones(n, bool) if sel is None else _mask(sel, n, "sel")).astype(np.int32)
    out = np.zeros((F, int(mapping.max()) + 1 if n else 0), _F32)
    return _host_call(coords, kept, _radii(radii, n, 10), n_points, mapping, mask, out, ctx) * 100


def sequence_id(fields):
    """``moleculekit.util.sequenceID`` of a tuple of per-atom arrays: a counter that steps wherever any field changes"""
    fields = [np.asarray(f) for f in fields]
    n = len(fields[0])
    if n == 0:
        return np.zeros(0, np.int64)
    step = np.zeros(n, bool)
    for f in fields:
        step[1:] |= f[1:] != f[:-1]
    return np.cumsum(step)


def _project(mol, sel, filtersel, probe_nm, n_points, mode, ctx=None):
    """the reference's MetricSasa.project with boolean masks ``sel`` / ``filtersel`` over the atoms of ``mol``"""
    props = _mol_props(mol, sel, filtersel, probe_nm, mode)
    atom_mapping = props["atom_mapping"]
    tokeep = np.unique(atom_mapping[props["tokeep"]])
    nframes = int(mol.numFrames)
    coords = _coords(mol.coords)
    out = np.full((nframes, int(atom_mapping.max()) + 1), -1, dtype=_F32)
    out[:, tokeep] = 0
    keep = np.ascontiguousarray(np.flatnonzero(filtersel), dtype=np.uint32)
    _host_call(coords, keep, props["radii"], _points(n_points), _mapping(atom_mapping, keep.size),
               np.ascontiguousarray(sel[filtersel], dtype=np.int32), out, ctx)
    out = out[:, tokeep] * 100                     # square nm -> square Angstrom
    assert not np.any(out == -1), "Some atoms are not excluded"
    return out


def _mol_props(mol, sel, filtersel, probe_nm, mode):
    selidx, filterselidx = np.where(sel)[0], np.where(filtersel)[0]
    if len(np.setdiff1d(selidx, filterselidx)) != 0:
        raise RuntimeError("Some atoms selected by `sel` are not selected by `filtersel` and thus would not be calculated. "
                           "Make sure `sel` is a subset of `filtersel`.")
    res = {}
    filterselmod = filtersel.copy().astype(int)
    filterselmod[filterselmod == 0] = -1
    filterselmod[filtersel] = np.arange(np.count_nonzero(filtersel))
    res["tokeep"] = filterselmod[sel]
    vdw = [ATOMIC_RADII[str(e)] for e in np.asarray(mol.element)[filtersel]]       # KeyError: an element without a radius
    res["radii"] = np.array(vdw, _F32) + _F32(probe_nm)
    if mode == "atom":
        res["atom_mapping"] = np.arange(np.sum(filtersel), dtype=np.int32)
    elif mode == "residue":
        res["atom_mapping"] = sequence_id((np.asarray(mol.resid)[filtersel], np.asarray(mol.chain)[filtersel],
                                           np.asarray(mol.segid)[filtersel])).astype(np.int32)
    else:
        raise ValueError(f'mode must be one of "residue", "atom". "{mode}" supplied')
    return res


class _Mapping(dict):
    """what getMapping returns where pandas is not installed: the DataFrame's columns by key or attribute"""
    __getattr__ = dict.__getitem__


class MetricSasa:
    """The reference's ``moleculekit.projections.metricsasa.MetricSasa`` on the GPU: same constructor, ``project(mol)`` ->
    float32 ``[numFrames, n_selected_atoms or n_selected_residues]`` in square Angstrom, ``getMapping(mol)``.  ``sel`` / ``filtersel``
    are boolean masks or integer index arrays over the molecule's atoms (``"all"`` is understood; other selection strings are
    not -- this package has no selection language).  ``mol`` needs ``coords`` (float32 ``[N, 3, F]``), ``element``, ``resid``,
    ``chain``, ``segid``, ``resname``, ``name`` and ``numFrames``."""

    def __init__(self, sel, filtersel="all", probeRadius=1.4, numSpherePoints=960, mode="atom"):
        self._probeRadius = probeRadius / 10  # nanometres
        self._numSpherePoints = numSpherePoints
        self._mode = mode
        self._sel = sel
        self._filtersel = filtersel

    def _masks(self, mol):
        n = int(np.asarray(mol.coords).shape[0])

        def one(s, name):
            if isinstance(s, str):
                if s == "all":
                    return np.ones(n, bool)
                raise TypeError(f"{name}: a boolean mask or an integer index array is required (this package has no selection language)")
            return _mask(s, n, name)

        return one(self._sel, "sel"), one(self._filtersel, "filtersel")

    def project(self, mol, ctx=None):
        sel, filtersel = self._masks(mol)
        return _project(mol, sel, filtersel, self._probeRadius, self._numSpherePoints, self._mode, ctx)

    def getMapping(self, mol):
        sel, filtersel = self._masks(mol)
        props = _mol_props(mol, sel, filtersel, self._probeRadius, self._mode)
        if self._mode == "atom":
            atomidx = np.where(sel)[0]
        else:
            _, firstidx = np.unique(props["atom_mapping"][props["tokeep"]], return_index=True)
            atomidx = np.where(sel)[0][firstidx]
        cols = {"type": ["SASA"] * len(atomidx), "atomIndexes": [int(i) for i in atomidx],
                "description": [f"SASA of {mol.resname[i]} {mol.resid[i]} {mol.name[i]}" for i in atomidx]}
        try:
            from pandas import DataFrame
        except ImportError:
            return _Mapping(cols)
        return DataFrame(cols)


# ------------------------------------------------------------------------------------------------
# moleculekit hook
# ------------------------------------------------------------------------------------------------
def _reference_project(self, mol):
    """``MetricSasa.project`` of an installed moleculekit, on the GPU: the object's own selections (``mol.atomselect``)"""
    sel = np.asarray(mol.atomselect(self._sel), dtype=bool)
    filtersel = np.asarray(mol.atomselect(self._filtersel), dtype=bool)
    return _project(mol, sel, filtersel, self._probeRadius, self._numSpherePoints, self._mode)


def install():
    """Swap ``moleculekit.projections.metricsasa.MetricSasa.project`` for the GPU's.  Returns the original; idempotent;
    ``uninstall()`` puts it back.  Independent of the other ``install()`` hooks."""
    import moleculekit.projections.metricsasa as ref

    saved = getattr(ref, "_mkamd_reference_project", None)
    if saved is not None:
        return saved
    saved = ref.MetricSasa.project
    ref.MetricSasa.project = _reference_project
    ref._mkamd_reference_project = saved
    return saved


def uninstall():
    """Undo ``install()``."""
    import moleculekit.projections.metricsasa as ref

    saved = getattr(ref, "_mkamd_reference_project", None)
    if saved is not None:
        ref.MetricSasa.project = saved
        ref._mkamd_reference_project = None
