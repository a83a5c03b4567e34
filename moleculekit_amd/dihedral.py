"""Dihedral angles of trajectory frames on the MI355X (include/mkamd_distance.h "dihedral angles").

The reference's ``MetricDihedral`` projects the sine and cosine (or the degrees) of backbone and side-chain torsions of every frame;
it computes them on the host, one dihedral at a time (``projections/metricdihedral.py:_calcDihedralAngles`` ->
``dihedral.py:dihedralAngle``).  Here one kernel call does all dihedrals of all frames.  The two float32 terms that go into the
reference's ``atan2`` are reproduced to the bit; everything after them is done in float64 and rounded once, so it is at least as
close to the exact function of those terms as the reference's own float32 angle.

* ``dihedral_trajectory`` -- CUDA tensors in the reference's ``[N, 3, F]`` layout -> float32 CUDA tensor, asynchronous.
* ``dihedrals`` -- numpy arrays through the host entry point (only the rows of the atoms the quads name travel).
* ``Dihedral`` -- the reference's description of a dihedral by four atoms, ``phi`` ... ``chi5``, ``proteinDihedrals``,
  ``dihedralsToIndexes``; selections are boolean masks or index arrays.
* ``MetricDihedral`` -- the reference's projection (``project`` / ``getMapping``); ``install()`` / ``uninstall()`` swap
  ``_calcDihedralAngles`` of an installed moleculekit's ``MetricDihedral``.

There is no CPU path: without the library or a device every entry point raises.
"""
from __future__ import annotations

import types

import numpy as np

from . import _lib
from .sasa import _Mapping, _coords, _mask

_F32, _U32 = np.float32, np.uint32
MODES = {"terms": 0, "radians": 1, "degrees": 2, "sincos": 3}       # include/mkamd_distance.h: MKAMD_DIH_*


def _mode(out):
    if out not in MODES:
        raise ValueError(f"out must be one of {sorted(MODES)}, got {out!r}")
    return MODES[out]


def _shape(F, D, mode):
    return {0: (F, D, 2), 1: (F, D), 2: (F, D), 3: (F, 2 * D)}[mode]


def _quads(quads, n):
    """[D, 4] atom indices (numpy or tensor, any integer type; negative counts from the end) -> uint32, checked against n atoms"""
    q = np.asarray(quads.cpu() if hasattr(quads, "cpu") else quads)
    if q.size == 0:
        return np.zeros((0, 4), _U32)
    if not np.issubdtype(q.dtype, np.integer):
        raise TypeError(f"quads must be integer atom indices, got {q.dtype.name}")
    if q.ndim == 1 and q.size == 4:
        q = q.reshape(1, 4)
    if q.ndim != 2 or q.shape[1] != 4:
        raise ValueError(f"quads must have shape (n_dihedrals, 4), got {q.shape}")
    q = q.astype(np.int64)
    q = np.where(q < 0, q + n, q)
    if q.min() < 0 or q.max() >= n:
        raise IndexError(f"quads: atom index out of range for {n} atoms")
    return np.ascontiguousarray(q, dtype=_U32)


def dihedral_trajectory(coords, quads, *, box=None, out="sincos", stream=None, ctx=None):
    """Dihedral angles of a device-resident trajectory.  ``coords``: CUDA float32 ``[N, 3, F]`` (``Molecule.coords``); ``quads``
    ``[D, 4]`` atom indices (numpy or tensor); ``box`` ``None`` or CUDA float32 ``[3, F]`` -- then every component of the three bond
    vectors is wrapped once as the reference's ``_wrapBondedDistance`` does (a box of zeros changes nothing).  ``out``: ``"sincos"``
    -> float32 CUDA ``[F, 2 D]`` (sin, cos interleaved: the reference's projection), ``"degrees"`` / ``"radians"`` -> ``[F, D]``,
    ``"terms"`` -> ``[F, D, 2]``, the two float32 arguments ``(p1, p2)`` of the reference's ``-atan2(p1, p2)``, its bits.
    Asynchronous on ``stream`` (an integer ``hipStream_t``; default torch's current stream)."""
    import torch

    mode = _mode(out)
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
    q = _quads(quads, N)
    D = int(q.shape[0])
    ctx = ctx or _lib.default_context(idx)
    dev = torch.device("cuda", idx)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream if stream is None else int(stream))
    res = torch.empty(_shape(F, D, mode), dtype=torch.float32, device=dev)
    if F == 0 or D == 0:
        return res
    dq = torch.as_tensor(q.view(np.int32), device=dev)
    _lib._check(_lib.load().mkamd_dihedrals_dev(ctx._h, coords.data_ptr(), N, F, box.data_ptr() if box is not None else None, F,
                                                dq.data_ptr(), D, mode, res.data_ptr()))
    if stream is not None:
        ctx.synchronize()          # (the index tensor is torch's: its memory must not be reused before a foreign stream has read it)
    return res


def dihedrals(coords, quads, *, box=None, out="sincos", ctx=None):
    """``dihedral_trajectory`` on host arrays: ``coords`` float32 ``[N, 3, F]``, ``quads`` ``[D, 4]``, ``box`` ``None`` or float32
    ``[3, F]``.  Returns float32 ``[F, 2 D]`` / ``[F, D]`` / ``[F, D, 2]`` by ``out``."""
    mode = _mode(out)
    coords = _coords(coords)
    N, _, F = coords.shape
    if box is not None:
        box = np.asarray(box)
        if box.shape != (3, F):
            raise ValueError(f"box must have shape (3, {F}), got {box.shape}")
        box = np.ascontiguousarray(box, dtype=_F32)
    q = _quads(quads, N)
    D = int(q.shape[0])
    res = np.zeros(_shape(F, D, mode), _F32)
    if F and D:
        ctx = ctx or _lib.default_context()
        _lib._check(_lib.load().mkamd_dihedrals_host(ctx._h, _lib._ptr(coords), N, F, _lib._ptr(box) if box is not None else None, F,
                                                     _lib._ptr(q), D, mode, _lib._ptr(res)))
    return res


# ------------------------------------------------------------------------------------------------
# topology: which four atoms make which dihedral
# ------------------------------------------------------------------------------------------------
# Side-chain torsions by residue (the IUPAC-IUB definitions as tabulated in the Garlic manual, "dihedrals": the table the reference
# cites).  chi[k][resname] = the four atom names of chi(k + 1); a residue without an entry has no such angle.
_STD1 = ("N", "CA", "CB", "CG")
_STD2 = ("CA", "CB", "CG", "CD")
_RING2 = ("CA", "CB", "CG", "CD1")
_CHI = (
    dict({r: _STD1 for r in ("ARG", "ASN", "ASP", "GLN", "GLU", "HIS", "LEU", "LYS", "MET", "PHE", "PRO", "TRP", "TYR")},
         CYS=("N", "CA", "CB", "SG"), ILE=("N", "CA", "CB", "CG1"), SER=("N", "CA", "CB", "OG"), THR=("N", "CA", "CB", "OG1"),
         VAL=("N", "CA", "CB", "CG1")),
    dict({r: _STD2 for r in ("ARG", "GLN", "GLU", "LYS", "PRO")}, **{r: _RING2 for r in ("LEU", "PHE", "TRP", "TYR")},
         ASN=("CA", "CB", "CG", "OD1"), ASP=("CA", "CB", "CG", "OD1"), HIS=("CA", "CB", "CG", "ND1"), ILE=("CA", "CB", "CG1", "CD1"),
         MET=("CA", "CB", "CG", "SD")),
    dict(ARG=("CB", "CG", "CD", "NE"), GLN=("CB", "CG", "CD", "OE1"), GLU=("CB", "CG", "CD", "OE1"), LYS=("CB", "CG", "CD", "CE"),
         MET=("CB", "CG", "SD", "CE")),
    dict(ARG=("CG", "CD", "NE", "CZ"), LYS=("CG", "CD", "CE", "NZ")),
    dict(ARG=("CD", "NE", "CZ", "NH1")),
)
_ILE_CD = {"amber": "CD1", "charmm": "CD"}            # the one name the two force fields' conventions differ in (ILE chi2)
_KNOWN = frozenset(("ARG", "ASN", "ASP", "CYS", "GLN", "GLU", "HIS", "ILE", "LEU", "LYS", "MET", "PHE", "PRO", "SER", "THR", "TRP", "TYR",
                    "VAL", "GLY", "ALA"))
_KEYS = ("name", "resid", "insertion", "chain", "segid")


class AtomNotFoundException(Exception):
    pass


def _field(mol, name, n):
    a = getattr(mol, name, None)
    if a is None:
        if name == "insertion":
            return np.full(n, "", dtype="<U1")
        raise AttributeError(f"mol.{name} is required")
    a = np.asarray(a)
    if a.shape != (n,):
        raise ValueError(f"mol.{name} must have one entry per atom ({n}), got shape {a.shape}")
    return a


def _topology(mol, sel=None):
    """the naming fields of ``mol`` (restricted to ``sel``) as a namespace of arrays"""
    n = int(np.asarray(mol.name).shape[0])
    f = {k: _field(mol, k, n) for k in _KEYS + ("resname",)}
    if sel is not None and not (isinstance(sel, str) and sel == "all"):
        if isinstance(sel, str):
            raise TypeError("sel: a boolean mask or an integer index array is required (this package has no selection language)")
        m = _mask(sel, n, "sel")
        f = {k: v[m] for k, v in f.items()}
    return types.SimpleNamespace(**f)


class Dihedral:
    """Four atoms that define a dihedral angle, each a dictionary with the keys ``name``, ``resid``, ``insertion``, ``chain`` and
    ``segid`` (the reference's ``moleculekit.projections.metricdihedral.Dihedral``), and a label ``dihedraltype``.

    >>> d = Dihedral.phi(mol, 5, 6, segid="P0")
    >>> d = Dihedral({"name": "N", "resid": 5}, {"name": "CA", "resid": 5}, {"name": "C", "resid": 5}, {"name": "N", "resid": 6})
    """

    def __init__(self, atom1, atom2, atom3, atom4, dihedraltype=None, check_valid=True):
        atoms = [atom1, atom2, atom3, atom4]
        if check_valid:
            defaults = {"name": "", "resid": 0, "segid": "", "insertion": "", "chain": ""}
            for a in atoms:
                for k in a:
                    if k not in _KEYS:
                        raise RuntimeError(f'Dictionary key can\'t be "{k}". Valid keys are: {_KEYS}')
                for k, v in defaults.items():
                    a.setdefault(k, v)
        self.atoms = atoms
        self.dihedraltype = dihedraltype

    def __str__(self):
        head = f'"{self.dihedraltype}" dihedral angle including atoms:\n' if self.dihedraltype is not None else ""
        rows = "".join("{}\t{}\t{}\t\t{}\t{}\n".format(a["name"], a["resid"], a["insertion"], a["chain"], a["segid"]) for a in self.atoms)
        return head + "name\tresid\tinsertion\tchain\tsegid\n" + rows

    __repr__ = __str__

    # -- atoms of a molecule ------------------------------------------------------------------
    @staticmethod
    def dihedralsToIndexes(mol, dihedrals, sel="all"):
        """the atom indexes (in ``mol``) of one Dihedral or a list of them: a list of four-element lists.  Every atom must match
        exactly one atom of ``sel`` by (name, resid, insertion, chain, segid), else ``RuntimeError``."""
        n = int(np.asarray(mol.name).shape[0])
        f = [_field(mol, k, n) for k in _KEYS]
        if isinstance(sel, str):
            if sel != "all":
                raise TypeError("sel: a boolean mask or an integer index array is required (this package has no selection language)")
            chosen = np.arange(n)
        else:
            chosen = np.flatnonzero(_mask(sel, n, "sel"))
        lookup = {}
        for i in chosen:
            key = (str(f[0][i]), int(f[1][i]), str(f[2][i]), str(f[3][i]), str(f[4][i]))
            lookup.setdefault(key, []).append(int(i))
        if isinstance(dihedrals, Dihedral):
            dihedrals = [dihedrals]
        indexes = []
        for d in dihedrals:
            quad = []
            for a in d.atoms:
                hits = lookup.get((str(a["name"]), int(a["resid"]), str(a["insertion"]), str(a["chain"]), str(a["segid"])), ())
                if len(hits) != 1:
                    raise RuntimeError(f"Expected one atom from atomselection {a}. Got {len(hits)} instead.")
                quad.append(hits[0])
            indexes.append(quad)
        return indexes

    @staticmethod
    def _residue(top, resid, insertion=None, chain=None, segid=None):
        m = top.resid == resid
        what = f'Resid "{resid}"'
        for label, given, arr in (("Insertion", insertion, top.insertion), ("Chain", chain, top.chain), ("Segid", segid, top.segid)):
            if given is not None:
                m = m & (arr == given)
                what += f' {label} "{given}"'
        idx = np.flatnonzero(m)
        if idx.size == 0:
            raise RuntimeError(f"No residues found with description ({what})")
        if idx[-1] - idx[0] + 1 != idx.size:
            raise RuntimeError(f"Residue with ({what}) has non-continuous indexes ({idx})")
        found = {}
        for label, arr in (("insertion", top.insertion), ("chain", top.chain), ("segid", top.segid)):
            u = np.unique(arr[idx])
            if u.size > 1:
                raise RuntimeError(f"Residue with ({what}) exists with multiple {label}s ({u}). Define {label} to disambiguate.")
            found[label] = u[0]
        names = np.unique(top.resname[idx])
        if names.size > 1:
            raise RuntimeError(f"Multiple resnames ({names}) found in ({what})")
        return dict(found, resid=resid, resname=str(names[0]), names=set(map(str, top.name[idx])))

    @staticmethod
    def _atom(res, name):
        if name not in res["names"]:
            raise AtomNotFoundException(f'No atoms found in residue {res["resname"]} {res["resid"]} with name "{name}".')
        return {"name": name, "resid": res["resid"], "insertion": res["insertion"], "chain": res["chain"], "segid": res["segid"]}

    @staticmethod
    def _top(mol):
        return mol if isinstance(mol, types.SimpleNamespace) and hasattr(mol, "_mkamd_top") else _mark(_topology(mol))

    @staticmethod
    def _backbone(mol, spec, res1, res2, segid, chain, insertion1, insertion2, label):
        """spec: (which residue, atom name, required) x 4 -- a missing optional atom (a capped terminal) means no dihedral"""
        top = Dihedral._top(mol)
        r = (Dihedral._residue(top, res1, insertion1, chain, segid), Dihedral._residue(top, res2, insertion2, chain, segid))
        atoms = []
        for which, name, required in spec:
            try:
                atoms.append(Dihedral._atom(r[which], name))
            except AtomNotFoundException:
                if required:
                    raise
                return None
        return Dihedral(*atoms, dihedraltype=label, check_valid=False)

    @staticmethod
    def phi(mol, res1, res2, segid=None, chain=None, insertion1=None, insertion2=None, ff="amber"):
        """C of ``res1`` and N, CA, C of ``res2`` (``None`` where ``res2`` is a cap without them)"""
        return Dihedral._backbone(mol, ((0, "C", True), (1, "N", False), (1, "CA", False), (1, "C", False)), res1, res2, segid, chain,
                                  insertion1, insertion2, "phi")

    @staticmethod
    def psi(mol, res1, res2, segid=None, chain=None, insertion1=None, insertion2=None, ff="amber"):
        """N, CA, C of ``res1`` (``None`` where it is a cap without them) and N of ``res2``"""
        return Dihedral._backbone(mol, ((0, "N", False), (0, "CA", False), (0, "C", False), (1, "N", True)), res1, res2, segid, chain,
                                  insertion1, insertion2, "psi")

    @staticmethod
    def omega(mol, res1, res2, segid=None, chain=None, insertion1=None, insertion2=None, ff="amber"):
        """CA, C of ``res1`` and N, CA of ``res2`` (``None`` where a cap lacks one)"""
        return Dihedral._backbone(mol, ((0, "CA", False), (0, "C", False), (1, "N", False), (1, "CA", False)), res1, res2, segid, chain,
                                  insertion1, insertion2, "omega")

    @staticmethod
    def _chi(k, mol, res, segid, chain, insertion, ff):
        ff = str(ff).lower()
        if ff not in _ILE_CD:
            raise ValueError(f'ff must be "amber" or "charmm", got {ff!r}')
        r = Dihedral._residue(Dihedral._top(mol), res, insertion, chain, segid)
        if r["resname"] not in _KNOWN:
            raise RuntimeError(f"Residue {r['resname']} not in list of known residues {sorted(_KNOWN)}. Rename your residues to match these.")
        names = _CHI[k - 1].get(r["resname"])
        if names is None:
            return None
        if k == 2 and r["resname"] == "ILE":
            names = names[:3] + (_ILE_CD[ff],)
        return Dihedral(*(Dihedral._atom(r, nm) for nm in names), dihedraltype=f"chi{k}", check_valid=False)

    @staticmethod
    def chi1(mol, res, segid=None, chain=None, insertion=None, ff="amber"):
        return Dihedral._chi(1, mol, res, segid, chain, insertion, ff)

    @staticmethod
    def chi2(mol, res, segid=None, chain=None, insertion=None, ff="amber"):
        return Dihedral._chi(2, mol, res, segid, chain, insertion, ff)

    @staticmethod
    def chi3(mol, res, segid=None, chain=None, insertion=None, ff="amber"):
        return Dihedral._chi(3, mol, res, segid, chain, insertion, ff)

    @staticmethod
    def chi4(mol, res, segid=None, chain=None, insertion=None, ff="amber"):
        return Dihedral._chi(4, mol, res, segid, chain, insertion, ff)

    @staticmethod
    def chi5(mol, res, segid=None, chain=None, insertion=None, ff="amber"):
        return Dihedral._chi(5, mol, res, segid, chain, insertion, ff)

    @staticmethod
    def proteinDihedrals(mol, sel="all", dih=("psi", "phi"), ff="amber"):
        """The dihedrals of the kinds named in ``dih`` for every residue of the atoms ``sel`` (mask or indexes) selects, as a list of
        Dihedral objects.  A new residue starts where resid, insertion, chain or segid changes, a new segment where chain or segid
        does; phi needs a previous residue in the segment, psi and omega a next one.  Per residue the order is phi, psi, omega,
        chi1 ... chi5, whatever the order in ``dih``."""
        top = _mark(_topology(mol, sel))
        segments, residues, prev = [], [], None
        for key in zip(top.resid, top.insertion, top.chain, top.segid):
            if prev is not None and key[2:] != prev[2:]:
                segments.append(residues)
                residues = []
            if key != prev:
                residues.append(key)
                prev = key
        if residues:
            segments.append(residues)
        found = []
        for residues in segments:
            for k, (resid, ins, chain, segid) in enumerate(residues):
                if "phi" in dih and k > 0:
                    found.append(Dihedral.phi(top, residues[k - 1][0], resid, segid, chain, residues[k - 1][1], ins, ff))
                if k + 1 < len(residues):
                    if "psi" in dih:
                        found.append(Dihedral.psi(top, resid, residues[k + 1][0], segid, chain, ins, residues[k + 1][1], ff))
                    if "omega" in dih:
                        found.append(Dihedral.omega(top, resid, residues[k + 1][0], segid, chain, ins, residues[k + 1][1], ff))
                for c in range(1, 6):
                    if f"chi{c}" in dih:
                        found.append(Dihedral._chi(c, top, resid, segid, chain, ins, ff))
        return [d for d in found if d is not None]


def _mark(top):
    top._mkamd_top = True
    return top


# ------------------------------------------------------------------------------------------------
# the projection
# ------------------------------------------------------------------------------------------------
class MetricDihedral:
    """The reference's ``moleculekit.projections.metricdihedral.MetricDihedral`` on the GPU: ``project(mol)`` -> float32
    ``[numFrames, 2 D]`` (sine and cosine of every dihedral, interleaved) or, with ``sincos=False``, ``[numFrames, D]`` in degrees;
    ``getMapping(mol)``.  ``dih``: a list of Dihedral objects (default: the phi and psi angles of ``protsel``); ``protsel``: a
    boolean mask or an integer index array over the molecule's atoms (``"all"`` is understood; other selection strings are not --
    this package has no selection language).  ``mol`` needs ``coords`` (float32 ``[N, 3, F]``), ``name``, ``resname``, ``resid``,
    ``chain``, ``segid`` and, where it has insertion codes, ``insertion``."""

    def __init__(self, dih=None, sincos=True, protsel="all"):
        if dih is not None and not isinstance(dih[0], Dihedral):
            raise RuntimeError("Manually passing dihedrals to MetricDihedral requires use of the Dihedral class.")
        self._protsel = protsel
        self._sincos = sincos
        self._dihedrals = dih

    def _indexes(self, mol):
        dih = Dihedral.proteinDihedrals(mol, self._protsel) if self._dihedrals is None else list(self._dihedrals)
        return Dihedral.dihedralsToIndexes(mol, dih, self._protsel)

    def project(self, mol, ctx=None):
        return dihedrals(mol.coords, np.asarray(self._indexes(mol), dtype=np.int64).reshape(-1, 4),
                         out="sincos" if self._sincos else "degrees", ctx=ctx)

    def getMapping(self, mol):
        types_, indexes, description = [], [], []
        for quad in self._indexes(mol):
            what = "".join("({} {} {} {} {}) ".format(mol.resname[a], mol.resid[a], mol.name[a], mol.segid[a], mol.chain[a]) for a in quad)
            for text in (("Sine of angle of ", "Cosine of angle of ") if self._sincos else ("Angle of ",)):
                types_.append("dihedral")
                indexes.append(quad)
                description.append(text + what)
        cols = {"type": types_, "atomIndexes": indexes, "description": description}
        try:
            from pandas import DataFrame
        except ImportError:
            return _Mapping(cols)
        return DataFrame(cols)


# ------------------------------------------------------------------------------------------------
# moleculekit hook
# ------------------------------------------------------------------------------------------------
def _reference_calc(self, mol, dihedrals_, sincos=True):
    """``MetricDihedral._calcDihedralAngles`` of an installed moleculekit, on the GPU: the atom indexes are the object's own"""
    return dihedrals(mol.coords, np.asarray(dihedrals_, dtype=np.int64).reshape(-1, 4), out="sincos" if sincos else "degrees")


def install():
    """Swap ``moleculekit.projections.metricdihedral.MetricDihedral._calcDihedralAngles`` for the GPU's.  Returns the original;
    idempotent; ``uninstall()`` puts it back.  Independent of the other ``install()`` hooks."""
    import moleculekit.projections.metricdihedral as ref

    saved = getattr(ref, "_mkamd_reference_calc", None)
    if saved is not None:
        return saved
    saved = ref.MetricDihedral._calcDihedralAngles
    ref.MetricDihedral._calcDihedralAngles = _reference_calc
    ref._mkamd_reference_calc = saved
    return saved


def uninstall():
    """Undo ``install()``."""
    import moleculekit.projections.metricdihedral as ref

    saved = getattr(ref, "_mkamd_reference_calc", None)
    if saved is not None:
        ref.MetricDihedral._calcDihedralAngles = saved
        ref._mkamd_reference_calc = None
