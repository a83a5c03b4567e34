"""Shell densities of trajectory frames on the MI355X (include/mkamd_distance.h "shell counts").

The reference's ``MetricShell`` projects the density of interchangeable atoms (water oxygens, ions) in concentric shells around
chosen atoms: it builds the whole ``[frames, n1 * n2]`` float32 distance matrix with ``MetricDistance`` and histograms it on the host.
Here the histogram is fused into the pair kernel -- the matrix never exists -- and the projection is EQUAL to the reference's, not
merely close: the pair arithmetic is the distance row's (bit for bit), a count is an integer, and the shell edges are turned into
thresholds on the squared distance that decide every pair as the reference's comparison of the rounded root does.

* ``shell_thresholds`` -- shell edges (and ``truncate``) -> float32 thresholds on the squared distance.
* ``shell_counts_trajectory`` -- CUDA tensors in the reference's ``[N, 3, F]`` layout -> int32 CUDA ``[F, n1, S]``.
* ``shell_counts`` -- numpy arrays through the host entry point (only the selected atoms' rows travel).
* ``MetricShell`` -- the reference's projection (``project`` / ``getMapping``) with masks or index arrays for selections;
  ``install()`` / ``uninstall()`` swap ``project`` of an installed moleculekit's ``MetricShell``.

There is no CPU path: without the library or a device every entry point raises.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from .sasa import _Mapping, _coords, _mask

_F32, _U32 = np.float32, np.uint32
MAX_SHELLS = 32


def shell_thresholds(edges, truncate=None):
    """float32 ``[n_edges]``: for every shell edge ``e`` the largest float32 ``T`` with ``float32(sqrt(T)) <= e``.

    The reference asks ``d <= e`` of ``d = float32(sqrt(d2))`` (in float64 when ``e`` is one: the same as ``d <=`` the largest
    float32 at or below ``e``).  The correctly rounded root is monotone -- ``x <= y`` implies ``fl(sqrt(x)) <= fl(sqrt(y))`` -- so the
    set of float32 ``d2`` that pass is everything up to one last value ``T``, and ``d2 <= T`` is the same test without a root.  ``T`` is
    found by ``nextafter`` steps around ``e * e`` against numpy's float32 ``sqrt`` (correctly rounded, as IEEE 754 requires).
    With ``truncate`` every distance above ``float32(truncate)`` BECOMES it (the reference's quirk), so it passes every edge at or
    above that value: those thresholds are ``+inf`` (which even an infinite distance passes; a NaN passes nothing)."""
    e = np.asarray(edges)
    if e.ndim != 1 or e.size < 2:
        raise ValueError(f"edges must be a 1-D array of at least two shell edges, got shape {e.shape}")
    if not (np.issubdtype(e.dtype, np.integer) or np.issubdtype(e.dtype, np.floating)):
        raise TypeError(f"edges must be numbers, got {e.dtype.name}")
    e = e.astype(np.float64)
    if not np.all(np.isfinite(e)) or e[0] < 0 or np.any(np.diff(e) < 0):
        raise ValueError("edges must be finite, non-negative and non-decreasing")
    tr = None if truncate is None else _F32(truncate)
    out = np.empty(e.size, _F32)
    inf = _F32(np.inf)
    for s, edge in enumerate(e):
        if tr is not None and edge >= float(tr):
            out[s] = inf
            continue
        e32 = _F32(edge)
        if float(e32) > edge:                                   # the largest float32 at or below a float64 edge
            e32 = np.nextafter(e32, -inf)
        x = e32 * e32
        if not np.isfinite(x):
            x = np.finfo(_F32).max
        while np.sqrt(x) > e32:
            x = np.nextafter(x, -inf)
        while True:
            up = np.nextafter(x, inf)
            if not np.isfinite(up) or np.sqrt(up) > e32:
                break
            x = up
        out[s] = x
    return out


def shell_edges(numshells, shellwidth):
    """the reference's ``np.arange(shellwidth * (numshells + 1), step=shellwidth)`` and its shell volumes (float64)"""
    numshells = int(numshells)
    if not 1 <= numshells <= MAX_SHELLS:
        raise ValueError(f"numshells must be between 1 and {MAX_SHELLS}, got {numshells}")
    if not shellwidth > 0:
        raise ValueError(f"shellwidth must be positive, got {shellwidth}")
    edges = np.arange(shellwidth * (numshells + 1), step=shellwidth)
    if edges.size != numshells + 1:
        raise ValueError(f"shellwidth {shellwidth!r} x {numshells} shells does not give {numshells + 1} edges in np.arange")
    vol = 4 / 3 * np.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
    return edges, vol


def _index(sel, n, name):
    """a boolean mask or an index array over n atoms -> uint32 indices IN THE GIVEN ORDER (a mask: ascending)"""
    a = np.asarray(sel.cpu() if hasattr(sel, "cpu") else sel)
    if a.dtype == bool:
        return np.ascontiguousarray(np.flatnonzero(_mask(a, n, name)), dtype=_U32)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise TypeError(f"{name}: a boolean mask or an integer index array is required (this package has no selection language)")
    a = a.astype(np.int64).reshape(-1)
    a = np.where(a < 0, a + n, a)
    if a.size and (a.min() < 0 or a.max() >= n):
        raise IndexError(f"{name}: atom index out of range for {n} atoms")
    return np.ascontiguousarray(a, dtype=_U32)


def _chains(chains, n):
    c = np.asarray(chains.cpu() if hasattr(chains, "cpu") else chains)
    if c.shape != (n,) or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"chains must be an integer array of {n} entries (one per atom), got {c.dtype.name} {c.shape}")
    return np.ascontiguousarray(c, dtype=_U32)


def _call_args(n, sel1, sel2, chains, edges, symmetric, truncate):
    s1, s2 = _index(sel1, n, "sel1"), _index(sel2, n, "sel2")
    if symmetric and not np.array_equal(s1, s2):
        raise ValueError("symmetric: sel1 and sel2 must be the same selection")
    thr = shell_thresholds(edges, truncate)
    if thr.size - 1 > MAX_SHELLS:
        raise ValueError(f"numshells must be between 1 and {MAX_SHELLS}, got {thr.size - 1}")
    return s1, s2, _chains(chains, n), thr


def shell_counts_trajectory(coords, box, sel1, sel2, chains, edges, *, symmetric=False, pbc=True, truncate=None, out=None, stream=None,
                            ctx=None):
    """Shell counts of a device-resident trajectory.  ``coords``: CUDA float32 ``[N, 3, F]`` (``Molecule.coords``), ``box`` CUDA float32
    ``[3, F]``; ``sel1`` (the centres) / ``sel2`` masks or index arrays, ``chains`` one integer per atom (the minimum image is applied
    where ``pbc`` and the chains of a pair differ), ``edges`` the ``S + 1`` shell edges.  Returns int32 CUDA ``[F, n1, S]``:
    ``counts[f, i, s]`` atoms of ``sel2`` lie at ``edges[s] < d <= edges[s + 1]`` from ``sel1[i]`` (``sel1`` order is the output order);
    ``symmetric`` (both selections the same) leaves the atom itself out.  ``truncate``: the reference's -- distances above it count
    as it.  Asynchronous on ``stream`` (an integer ``hipStream_t``; default torch's current stream)."""
    import torch

    for name, t in (("coords", coords), ("box", box)):
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
    if tuple(box.shape) != (3, F):
        raise ValueError(f"box must have shape (3, {F}), got {tuple(box.shape)}")
    box = box.contiguous()
    dev = coords.device
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if box.device != coords.device:
        raise ValueError("coords and box live on different devices")
    if ctx is not None and ctx.device != idx:
        raise ValueError(f"ctx lives on GPU {ctx.device} but the tensors are on cuda:{idx}")
    s1, s2, ch, thr = _call_args(N, sel1, sel2, chains, edges, symmetric, truncate)
    ctx = ctx or _lib.default_context(idx)
    dev = torch.device("cuda", idx)
    S = thr.size - 1
    shape = (F, int(s1.size), S)
    if out is not None and not (out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == shape and out.device == dev):
        raise ValueError(f"out must be a contiguous int32 {list(shape)} tensor on {dev}")
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream if stream is None else int(stream))
    if out is None:
        out = torch.empty(shape, dtype=torch.int32, device=dev)
    d1, d2, dch = (torch.as_tensor(a.view(np.int32), device=dev) for a in (s1, s2, ch))
    _lib._check(_lib.load().mkamd_shell_counts_dev(ctx._h, coords.data_ptr(), N, F, box.data_ptr(), d1.data_ptr(), int(s1.size), d2.data_ptr(),
                                                   int(s2.size), dch.data_ptr(), int(bool(symmetric)), int(bool(pbc)), _lib._ptr(thr), int(thr.size),
                                                   out.data_ptr()))
    if stream is not None:
        ctx.synchronize()          # (the index tensors are torch's: their memory must not be reused before a foreign stream has read them)
    return out


def shell_counts(coords, box, sel1, sel2, chains, edges, *, symmetric=False, pbc=True, truncate=None, ctx=None):
    """``shell_counts_trajectory`` on host arrays: ``coords`` float32 ``[N, 3, F]``, ``box`` float32 ``[3, F]`` (anything else
    without ``pbc``: zeros stand in).  Returns int32 ``[F, n1, S]``."""
    coords = _coords(coords)
    N, _, F = coords.shape
    box = np.asarray(box)
    if box.shape != (3, F):
        if pbc:
            raise ValueError(f"box must have shape (3, {F}) for periodic distances, got {box.shape}")
        box = np.zeros((3, F), _F32)
    box = np.ascontiguousarray(box, dtype=_F32)
    s1, s2, ch, thr = _call_args(N, sel1, sel2, chains, edges, symmetric, truncate)
    out = np.zeros((F, int(s1.size), int(thr.size) - 1), np.int32)
    if F and s1.size:
        ctx = ctx or _lib.default_context()
        _lib._check(_lib.load().mkamd_shell_counts_host(ctx._h, _lib._ptr(coords), N, F, _lib._ptr(box), _lib._ptr(s1), int(s1.size), _lib._ptr(s2),
                                                        int(s2.size), _lib._ptr(ch), int(bool(symmetric)), int(bool(pbc)), _lib._ptr(thr),
                                                        int(thr.size), _lib._ptr(out)))
    return out


# ------------------------------------------------------------------------------------------------
# the projection
# ------------------------------------------------------------------------------------------------
def _project(mol, sel1, sel2, periodic, numshells, shellwidth, truncate, symmetrical, ctx=None):
    """the reference's MetricShell.project with boolean masks over the atoms of ``mol`` (projections/util.py:pp_calcDistances for
    the box and the chains, metricshell.py:_shells for the densities)"""
    coords = _coords(mol.coords)
    N, _, F = coords.shape
    box = getattr(mol, "box", None)
    if periodic is not None:
        if box is None or np.sum(box) == 0:
            raise RuntimeError("No periodic box dimensions given in the molecule/trajectory. "
                               "If you want to calculate distance without wrapping, set the periodic option to None")
    else:
        box = np.zeros((3, F), dtype=_F32)
    box = np.asarray(box)
    if box.shape[1] != F:
        raise RuntimeError("Different number of frames in mol.coords and mol.box. "
                           "Please ensure they both have the same number of frames")
    if periodic is None:
        chains = np.zeros(N, dtype=_U32)
    elif periodic == "chains":
        chains = np.unique(np.asarray(mol.chain), return_inverse=True)[1].astype(_U32)
    elif periodic == "selections":
        chains = np.ones(N, dtype=_U32)
        chains[sel2] = 2
    else:
        raise RuntimeError(f"Invalid periodic option {periodic}")
    edges, vol = shell_edges(numshells, shellwidth)
    counts = shell_counts(coords, box, sel1, sel2, chains, edges, symmetric=bool(symmetrical), pbc=periodic is not None, truncate=truncate,
                          ctx=ctx)
    return (counts / vol).reshape(F, -1)


class MetricShell:
    """The reference's ``moleculekit.projections.metricshell.MetricShell`` on the GPU: same constructor, ``project(mol)`` -> float64
    ``[numFrames, n_centres * numshells]`` (centre-major, centres in ascending atom index: atoms of ``sel2`` per cubic Angstrom of
    each shell), ``getMapping(mol)``.  ``sel1`` / ``sel2`` are boolean masks or integer index arrays over the molecule's atoms
    (``"all"`` is understood; other selection strings are not -- this package has no selection language).  ``periodic``: ``None``,
    ``"chains"`` or ``"selections"`` as in MetricDistance.  ``mol`` needs ``coords`` (float32 ``[N, 3, F]``), ``box`` (``[3, F]``) for
    the periodic modes, ``chain`` for ``"chains"``, and ``resname`` / ``resid`` / ``name`` for ``getMapping``."""

    def __init__(self, sel1, sel2, periodic, numshells=4, shellwidth=3, pbc=None, gap=None, truncate=None):
        if pbc is not None:
            raise DeprecationWarning("The `pbc` option is deprecated please use the `periodic` option as described in MetricDistance.")
        if periodic is not None and periodic not in ("chains", "selections"):
            raise RuntimeError(f"Invalid periodic option {periodic}")
        shell_edges(numshells, shellwidth)
        self.sel1, self.sel2 = sel1, sel2
        self.periodic = periodic
        self.numshells = numshells
        self.shellwidth = shellwidth
        self.truncate = truncate

    def _masks(self, mol):
        n = int(np.asarray(mol.coords).shape[0])

        def one(s, name):
            if isinstance(s, str):
                if s == "all":
                    return np.ones(n, bool)
                raise TypeError(f"{name}: a boolean mask or an integer index array is required (this package has no selection language)")
            return _mask(s, n, name)

        m1, m2 = one(self.sel1, "sel1"), one(self.sel2, "sel2")
        return m1, m2, bool(np.array_equal(m1, m2))

    def project(self, mol, ctx=None):
        m1, m2, symmetrical = self._masks(mol)
        return _project(mol, m1, m2, self.periodic, self.numshells, self.shellwidth, self.truncate, symmetrical, ctx)

    def getMapping(self, mol):
        m1, _, _ = self._masks(mol)
        types, indexes, description = [], [], []
        for i in np.flatnonzero(m1):
            for n in range(self.numshells):
                types.append("shell")
                indexes.append(int(i))
                description.append("Density of sel2 atoms in shell {}-{} A centered on atom {} {} {}".format(
                    n * self.shellwidth, (n + 1) * self.shellwidth, mol.resname[i], mol.resid[i], mol.name[i]))
        cols = {"type": types, "atomIndexes": indexes, "description": description}
        try:
            from pandas import DataFrame
        except ImportError:
            return _Mapping(cols)
        return DataFrame(cols)


# ------------------------------------------------------------------------------------------------
# moleculekit hook
# ------------------------------------------------------------------------------------------------
def _reference_project(self, mol):
    """``MetricShell.project`` of an installed moleculekit, on the GPU: the selections and options of the object's own MetricDistance
    (``mol.atomselect``), the symmetry it decided itself"""
    md = self.metricdistance
    sel1 = np.asarray(mol.atomselect(md.sel1), dtype=bool)
    sel2 = np.asarray(mol.atomselect(md.sel2), dtype=bool)
    return _project(mol, sel1, sel2, md.periodic, self.numshells, self.shellwidth, md.truncate, self.symmetrical)


def install():
    """Swap ``moleculekit.projections.metricshell.MetricShell.project`` for the GPU's.  Returns the original; idempotent;
    ``uninstall()`` puts it back.  Independent of the other ``install()`` hooks."""
    import moleculekit.projections.metricshell as ref

    saved = getattr(ref, "_mkamd_reference_project", None)
    if saved is not None:
        return saved
    saved = ref.MetricShell.project
    ref.MetricShell.project = _reference_project
    ref._mkamd_reference_project = saved
    return saved


def uninstall():
    """Undo ``install()``."""
    import moleculekit.projections.metricshell as ref

    saved = getattr(ref, "_mkamd_reference_project", None)
    if saved is not None:
        ref.MetricShell.project = saved
        ref._mkamd_reference_project = None
