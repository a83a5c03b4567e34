"""Secondary structure of trajectory frames on the MI355X (include/mkamd_distance.h "secondary structure").

The reference's ``MetricSecondaryStructure`` hands every frame to mdtraj's DSSP, one frame at a time on one CPU thread, and raises
``ImportError`` without mdtraj.  Here Kabsch and Sander's rules (stated in DESIGN.md section 19) run on the device for all frames of a
call: backbone hydrogen-bond energies in float32, the two best acceptors of every donor, n-turns, helices, bends, bridges and ladders
with bulge merging.  No box is used, as in the reference.

* ``dssp_trajectory`` -- CUDA tensor in the reference's ``[N, 3, F]`` layout -> uint8 CUDA tensor ``[F, R]``, asynchronous.
* ``dssp`` -- numpy arrays through the host entry point (only the rows of the 4 R backbone atoms travel).
* ``backbone_arrays`` -- the four per-residue arrays of a molecule: CA, (N, C, O), proline flags, chain numbers.
* ``MetricSecondaryStructure`` -- the reference's projection (``project`` / ``getMapping``); ``install()`` / ``uninstall()`` swap
  ``project`` of an installed moleculekit's ``MetricSecondaryStructure``.

Codes (the reference's integers): full H 3, B 4, E 5, G 6, I 7, T 8, S 9, ' ' 10; simplified helix (H, G, I) 2, strand (E, B) 1,
coil 0.  There is no CPU path: without the library or a device every entry point raises.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .dihedral import _field
from .sasa import _Mapping, _coords, _mask, sequence_id

_U32, _I32 = np.uint32, np.int32
FULL_CODES = {"H": 3, "B": 4, "E": 5, "G": 6, "I": 7, "T": 8, "S": 9, " ": 10}
SIMPLE_CODES = {"C": 0, "E": 1, "H": 2}
_LETTERS = np.array([""] * 11, dtype="U2")
for _k, _v in FULL_CODES.items():
    _LETTERS[_v] = _k
for _k, _v in SIMPLE_CODES.items():
    _LETTERS[_v] = _k
AVOID_FRAMES, AVOID_ATOMS, SMALL_CHUNKS = 1, 2, 4       # csrc/dssp_pipeline.h: Context.set_dssp_plan


def letters(codes):
    """integer codes (full or simplified) -> the reference's ``U2`` letter array"""
    return _LETTERS[np.asarray(codes)]


def _residue_arrays(ca, nco, proline, chains, n):
    """the four per-residue arrays (numpy or tensors) checked against n atoms -> uint32 [R], uint32 [R, 3], int32 [R], int32 [R]"""
    def host(a):
        return np.asarray(a.cpu() if hasattr(a, "cpu") else a)

    ca, nco, proline, chains = host(ca), host(nco), host(proline), host(chains)
    for name, a in (("ca", ca), ("nco", nco), ("chains", chains)):
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"{name} must be integers, got {a.dtype.name}")
    if proline.size and not (np.issubdtype(proline.dtype, np.integer) or proline.dtype == bool):
        raise TypeError(f"proline must be integers or booleans, got {proline.dtype.name}")
    ca = ca.reshape(-1).astype(np.int64)
    R = int(ca.shape[0])
    if nco.size != 3 * R or (nco.ndim != 2 and R > 0) or (nco.ndim == 2 and nco.shape[1] != 3):
        raise ValueError(f"nco must have shape ({R}, 3), got {nco.shape}")
    nco = nco.reshape(R, 3).astype(np.int64)
    if proline.shape != (R,) or chains.shape != (R,):
        raise ValueError(f"proline and chains must have one entry per residue ({R}), got {proline.shape} and {chains.shape}")
    for name, a in (("ca", ca), ("nco", nco)):
        if a.size and (a.min() < 0 or a.max() >= n):
            raise IndexError(f"{name}: atom index out of range for {n} atoms")
    return (np.ascontiguousarray(ca, dtype=_U32), np.ascontiguousarray(nco, dtype=_U32), np.ascontiguousarray(proline != 0, dtype=_I32),
            np.ascontiguousarray(chains, dtype=_I32))


def dssp_trajectory(coords, ca, nco, proline, chains, *, simplified=True, stream=None, ctx=None):
    """Secondary structure of a device-resident trajectory.  ``coords``: CUDA float32 ``[N, 3, F]`` (``Molecule.coords``, in
    Angstrom); ``ca`` ``[R]``, ``nco`` ``[R, 3]``: the atom indices of every residue's CA and of its N, C, O; ``proline`` ``[R]``:
    true where the residue donates no hydrogen bond; ``chains`` ``[R]``: integers, equal in neighbouring residues of one chain
    (``backbone_arrays`` builds all four).  Returns a uint8 CUDA tensor ``[F, R]`` of the reference's integer codes, simplified
    (helix 2, strand 1, coil 0) or full.  Asynchronous on ``stream`` (an integer ``hipStream_t``; default torch's current stream)."""
    import torch

    if not (hasattr(coords, "is_cuda") and coords.is_cuda):
        raise TypeError("coords: a CUDA tensor is required (there is no CPU path)")
    if coords.dtype != torch.float32:
        raise ValueError(f"coords must be float32, got {coords.dtype}")
    if coords.dim() == 2:
        coords = coords.unsqueeze(2)
    if coords.dim() != 3 or coords.shape[1] != 3:
        raise ValueError(f"coords must be (natoms, 3, nframes), got shape {tuple(coords.shape)}")
    coords = coords.contiguous()
    N, F = int(coords.shape[0]), int(coords.shape[2])
    dev = coords.device
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if ctx is not None and ctx.device != idx:
        raise ValueError(f"ctx lives on GPU {ctx.device} but the tensors are on cuda:{idx}")
    ca, nco, proline, chains = _residue_arrays(ca, nco, proline, chains, N)
    R = int(ca.shape[0])
    ctx = ctx or _lib.default_context(idx)
    dev = torch.device("cuda", idx)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream if stream is None else int(stream))
    res = torch.empty((F, R), dtype=torch.uint8, device=dev)
    if F == 0 or R == 0:
        return res
    d = [torch.as_tensor(a.view(np.int32), device=dev) for a in (ca, nco, proline, chains)]
    _lib._check(_lib.load().mkamd_dssp_dev(ctx._h, coords.data_ptr(), N, F, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(),
                                           d[3].data_ptr(), R, int(bool(simplified)), res.data_ptr()))
    if stream is not None:
        ctx.synchronize()          # (the index tensors are torch's: their memory must not be reused before a foreign stream has read it)
    return res


def dssp(coords, ca, nco, proline, chains, *, simplified=True, ctx=None):
    """``dssp_trajectory`` on host arrays: ``coords`` float32 ``[N, 3, F]``.  Returns uint8 ``[F, R]``."""
    coords = _coords(coords)
    N, _, F = coords.shape
    ca, nco, proline, chains = _residue_arrays(ca, nco, proline, chains, N)
    R = int(ca.shape[0])
    res = np.zeros((F, R), np.uint8)
    if F and R:
        ctx = ctx or _lib.default_context()
        _lib._check(_lib.load().mkamd_dssp_host(ctx._h, _lib._ptr(coords), N, F, _lib._ptr(ca), _lib._ptr(nco), _lib._ptr(proline),
                                                _lib._ptr(chains), R, int(bool(simplified)), _lib._ptr(res)))
    return res


# ------------------------------------------------------------------------------------------------
# topology: the backbone atoms of every residue
# ------------------------------------------------------------------------------------------------
def _selected(mol, sel):
    n = int(np.asarray(mol.name).shape[0])
    if isinstance(sel, str):
        if sel != "all":
            raise TypeError("sel: a boolean mask or an integer index array is required (this package has no selection language)")
        return n, np.arange(n)
    return n, np.flatnonzero(_mask(sel, n, "sel"))


def backbone_arrays(mol, sel="all"):
    """``(ca int32 [R], nco int32 [R, 3], proline int32 [R], chain_ids int32 [R])`` of the atoms ``sel`` (mask or indexes) selects in
    a molecule with ``name``, ``resname``, ``resid``, ``chain``, ``segid`` and, where it has insertion codes, ``insertion``: what
    the reference's ``MetricSecondaryStructure._calculateMolProp`` builds after filtering by ``sel``, with the atom indices counted
    in ``mol`` itself (so that its coordinates serve as they are; with ``sel="all"`` the two numberings agree).  A residue starts
    where resid, insertion, chain or segid changes.  A residue without a CA, or with a CA and without N, C or O, is a
    ``ValueError`` (the reference ends in an assertion or a failed integer conversion there)."""
    n, idx = _selected(mol, sel)
    f = {k: _field(mol, k, n)[idx] for k in ("name", "resname", "resid", "insertion", "chain", "segid")}
    res = sequence_id((f["resid"], f["insertion"], f["chain"], f["segid"]))
    R = int(res[-1]) + 1 if res.size else 0
    name = f["name"].astype(str)
    at_ca = np.flatnonzero(name == "CA")
    if at_ca.size != R or not np.array_equal(res[at_ca], np.arange(R)):
        counts = np.bincount(res[at_ca], minlength=R)
        bad = int(np.flatnonzero(counts != 1)[0])
        k = int(np.flatnonzero(res == bad)[0])
        raise ValueError(f"residue {f['resname'][k]} {f['resid'][k]}{f['insertion'][k]} of the selection has {int(counts[bad])} CA atoms; "
                         "select protein residues only")
    nco = np.full((R, 3), -1, np.int64)
    for col, nm in enumerate(("N", "C", "O")):
        at = np.flatnonzero(name == nm)
        nco[res[at], col] = idx[at]
    if R and nco.min() < 0:
        bad = int(np.flatnonzero((nco < 0).any(axis=1))[0])
        k = int(at_ca[bad])
        raise ValueError(f"residue {f['resname'][k]} {f['resid'][k]}{f['insertion'][k]} has a CA but lacks a backbone N, C or O")
    proline = (f["resname"][at_ca].astype(str) == "PRO").astype(_I32)
    _, chain_ids = np.unique(f["chain"][at_ca].astype(str), return_inverse=True) if R else (None, np.zeros(0, np.int64))
    return idx[at_ca].astype(_I32), nco.astype(_I32), proline, np.asarray(chain_ids).reshape(-1).astype(_I32)


# ------------------------------------------------------------------------------------------------
# the projection
# ------------------------------------------------------------------------------------------------
def _format(codes, integer):
    """uint8 codes -> what the reference's project returns: int32, or its U2 letters"""
    return codes.astype(_I32) if integer else letters(codes)


class MetricSecondaryStructure:
    """The reference's ``moleculekit.projections.metricsecondarystructure.MetricSecondaryStructure`` on the GPU: ``project(mol)`` ->
    int32 ``[numFrames, R]`` of the simplified (default) or full codes, or with ``integer=False`` the reference's ``U2`` letter
    arrays; ``getMapping(mol)``.  ``sel``: a boolean mask or an integer index array over the molecule's atoms that selects the
    protein (``"all"`` is understood; other selection strings are not -- this package has no selection language).  ``mol`` needs
    ``coords`` (float32 ``[N, 3, F]``), ``name``, ``resname``, ``resid``, ``chain``, ``segid`` and, where it has insertion codes,
    ``insertion``."""

    def __init__(self, sel="all", simplified=True, integer=True):
        self.sel = sel
        self.simplified = simplified
        self.integer = integer

    def project(self, mol, ctx=None):
        ca, nco, proline, chains = backbone_arrays(mol, self.sel)
        codes = dssp(mol.coords, ca, nco, proline, chains, simplified=self.simplified, ctx=ctx)
        return _format(codes, self.integer)

    def getMapping(self, mol):
        ca = backbone_arrays(mol, self.sel)[0]
        n = int(np.asarray(mol.name).shape[0])
        ins = _field(mol, "insertion", n)
        cols = {"type": ["secondary structure"] * len(ca), "atomIndexes": [int(i) for i in ca],
                "description": ["Secondary structure of residue {} {}{}".format(mol.resname[i], mol.resid[i], ins[i]) for i in ca]}
        try:
            from pandas import DataFrame
        except ImportError:
            return _Mapping(cols)
        return DataFrame(cols)


# ------------------------------------------------------------------------------------------------
# moleculekit hook
# ------------------------------------------------------------------------------------------------
def _reference_project(self, mol):
    """``MetricSecondaryStructure.project`` of an installed moleculekit, on the GPU: the per-residue arrays and the filtering are
    the object's own"""
    mol = mol.copy()
    props = self._getMolProp(mol, "all")
    mol.filter(self.sel, _logger=False)
    coords = np.ascontiguousarray(np.atleast_3d(mol.coords), dtype=np.float32)
    codes = dssp(coords, props["ca_indices"], props["nco_indices"], props["proline_indices"], props["chain_ids"], simplified=self.simplified)
    return _format(codes, self.integer)


def install():
    """Swap ``moleculekit.projections.metricsecondarystructure.MetricSecondaryStructure.project`` for the GPU's.  Returns the
    original; idempotent; ``uninstall()`` puts it back.  Independent of the other ``install()`` hooks."""
    import moleculekit.projections.metricsecondarystructure as ref

    saved = getattr(ref, "_mkamd_reference_project", None)
    if saved is not None:
        return saved
    saved = ref.MetricSecondaryStructure.project
    ref.MetricSecondaryStructure.project = _reference_project
    ref._mkamd_reference_project = saved
    return saved


def uninstall():
    """Undo ``install()``."""
    import moleculekit.projections.metricsecondarystructure as ref

    saved = getattr(ref, "_mkamd_reference_project", None)
    if saved is not None:
        ref.MetricSecondaryStructure.project = saved
        ref._mkamd_reference_project = None
