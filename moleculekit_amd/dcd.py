"""DCD trajectories (CHARMM / NAMD / X-PLOR / OpenMM) read and written with the frames decoded and encoded ON THE GPU
(include/mkamd_xtc.h "DCD"; csrc/dcd_reader.h, csrc/dcd_kernels.h).

Mirrors the reference's low-level module ``moleculekit.dcd`` (fileformats/dcd/dcd.pyx: ``load_dcd``, ``DCDTrajectoryFile.read`` /
``.write``) and ``readers.DCDread`` / ``writers.DCDwrite``.  Coordinates are float32 bit patterns carried unchanged -- the same bits as
the reference's ``load_dcd``, the same file bytes as its writer (but for the creation-time remark of the header).  Units are the
file's: Angstrom and degrees.

A DCD frame is three planes of floats at offsets the header fixes, so the host only parses the header, checks the selected frames'
record markers and copies their bytes; the device gathers, byte-swaps and transposes into the frame-major items ``[n, n_sel, 3]`` every
other entry point of this package takes (``read_dcd_frames_dev``), and the reverse for writing (``encode_dcd_dev`` / ``write_dcd_dev``).
``load_dcd`` is the host loop (``mkamd_dcd_read``): what the CPU tier and ``decode="host"`` use.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _lib
from .xtc import Trajectory, _path

DESC_BYTES = 32                 # sizeof(mkamd::dcd::FrameDesc)
HEADER_BYTES = 276              # the writer's file header
DESC_DTYPE = np.dtype([("x_off", "<u8"), ("y_off", "<u8"), ("z_off", "<u8"), ("count", "<u4"), ("flags", "<u4")])
assert DESC_DTYPE.itemsize == DESC_BYTES
FLAG_SWAP, FLAG_REC64, FLAG_CHARMM, FLAG_EXTRA, FLAG_4DIMS = 1, 2, 4, 8, 16
_FS_PER_DELTA = 0.04888821      # AKMA time unit in ps (readers.DCDread / writers.DCDwrite)


def info(filename) -> dict:
    """The header: ``n_atoms``, ``n_frames`` (from the file's size; a frame cut off at the end is not counted), ``istart``, ``nsavc``,
    ``delta``, ``n_fixed`` and ``flags`` (``FLAG_*``).  Raises ``ValueError`` for a file the parser refuses."""
    na, nf = ctypes.c_int64(0), ctypes.c_int64(0)
    istart, nsavc, nfixed, flags, delta = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_double(0)
    _lib._check(_lib.load().mkamd_dcd_info(_path(filename), ctypes.byref(na), ctypes.byref(nf), ctypes.byref(istart), ctypes.byref(nsavc),
                                           ctypes.byref(delta), ctypes.byref(nfixed), ctypes.byref(flags)))
    return dict(n_atoms=na.value, n_frames=nf.value, istart=istart.value, nsavc=nsavc.value, delta=delta.value, n_fixed=nfixed.value,
                flags=flags.value)


def read_header(filename):
    """``DCDTrajectoryFile.read_header()``: ``(istart, nsavc, delta)``."""
    h = info(filename)
    return h["istart"], h["nsavc"], h["delta"]


def _atoms(atom_indices, natoms):
    """``cast_indices`` plus the range check of ``DCDTrajectoryFile.read``: None, or unique integers in ``[0, natoms)`` as int32."""
    if atom_indices is None:
        return None
    if isinstance(atom_indices, slice):
        return np.arange(natoms, dtype=np.int32)[atom_indices].copy()
    if len(atom_indices) != len(set(np.asarray(atom_indices).reshape(-1).tolist())):
        raise ValueError("indices must be unique.")
    out = np.asarray(atom_indices)
    if not issubclass(out.dtype.type, np.integer):
        raise ValueError("indices must be of an integer type. %s is not an integer type" % out.dtype)
    out = out.reshape(-1)
    if len(out) and (out.min() < 0 or out.max() >= natoms):
        raise ValueError("atom_indices must lie in [0, n_atoms)")
    return np.ascontiguousarray(out, dtype=np.int32)


def _frame_list(nframes, stride, frame):
    if frame is not None:
        frame = int(frame)
        if frame < 0:
            raise IOError("Invalid argument")
        return np.arange(frame, min(frame + 1, nframes), dtype=np.int64)      # (seeking past the end reads nothing, like the reference)
    stride = 1 if stride is None else int(stride)
    if stride < 1:
        raise ValueError("stride must be >= 1")
    return np.arange(0, nframes, stride, dtype=np.int64)


def _cells(cell):
    """What ``DCDTrajectoryFile.read`` returns for the unit cells ``[n, 6]``: ``(lengths [n, 3], angles [n, 3])``, or ``(None, None)``
    when every length is below 1e-10 (a file without cells reads as lengths 0, angles 90)."""
    lengths, angles = np.ascontiguousarray(cell[:, :3]), np.ascontiguousarray(cell[:, 3:])
    if np.all(lengths < 1e-10):
        return None, None
    return lengths, angles


def load_dcd(filename, stride=None, atom_indices=None, frame=None):
    """``moleculekit.dcd.load_dcd`` on the host: ``(xyz float32 [n, n_sel, 3], cell_lengths float32 [n, 3] | None, cell_angles
    float32 [n, 3] | None)``.  ``frame`` overrides ``stride``; a stride past the end gives one frame."""
    if not isinstance(filename, (str, os.PathLike)):
        raise TypeError("filename must be of type path-like for load_dcd. you supplied %s" % type(filename))
    h = info(filename)
    atoms = _atoms(atom_indices, h["n_atoms"])
    fr = _frame_list(h["n_frames"], stride, frame)
    n, nsel = len(fr), h["n_atoms"] if atoms is None else len(atoms)
    xyz = np.zeros((n, nsel, 3), dtype=np.float32)
    cell = np.zeros((n, 6), dtype=np.float32)
    _lib._check(_lib.load().mkamd_dcd_read(_path(filename), _lib._ptr(fr), n, _lib._ptr(atoms), nsel, _lib._ptr(xyz), _lib._ptr(cell)))
    return (xyz,) + _cells(cell)


def chunk_desc(filename, frames):
    """Host half of the device decoder for ``frames`` (any order): ``(desc uint8 [n, 32], byte_lo, byte_hi, cell float32 [n, 6])``.  The
    selected frames' record markers are checked against the atom count, the descriptors against the file's size."""
    sel = np.ascontiguousarray(frames, dtype=np.int64).reshape(-1)
    n = len(sel)
    desc = np.empty((n, DESC_BYTES), dtype=np.uint8)
    cell = np.empty((n, 6), dtype=np.float32)
    lo, hi = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib._check(_lib.load().mkamd_dcd_chunk_desc(_path(filename), _lib._ptr(sel), n, _lib._ptr(desc), ctypes.byref(lo), ctypes.byref(hi),
                                                 _lib._ptr(cell)))
    return desc, int(lo.value), int(hi.value), cell


def source_table(filename, atoms, natoms):
    """``(sel, src)`` int32 ``[n_sel]``: the atom selection as indices into a full frame's planes, and composed with the fixed-atom map for
    the frames that store free atoms only (``src < 0``: atom ``-1 - src`` of frame 0)."""
    nsel = natoms if atoms is None else len(atoms)
    sel, src = np.empty(nsel, dtype=np.int32), np.empty(nsel, dtype=np.int32)
    _lib._check(_lib.load().mkamd_dcd_source_table(_path(filename), _lib._ptr(atoms), nsel, _lib._ptr(sel), _lib._ptr(src)))
    return sel, src


class DeviceReader:
    """A DCD file opened for decoding on one GPU: the header, the source tables on the device and -- for a file with fixed atoms --
    frame 0 decoded once and kept resident.  A chunk of frames is ``stage`` (host: descriptors, bytes into pinned memory), the upload
    of those bytes by the caller, then ``launch`` (the decode kernel on a stream)."""

    def __init__(self, filename, atom_indices=None, ctx=None):
        import torch

        self.filename, self.path = filename, _path(filename)
        self.ctx = ctx or _lib.default_context()
        self.dev = torch.device("cuda", self.ctx.device)
        self.header = info(filename)
        self.natoms, self.nframes = self.header["n_atoms"], self.header["n_frames"]
        atoms = _atoms(atom_indices, self.natoms)
        sel, src = source_table(filename, atoms, self.natoms)
        self.nsel = len(sel)
        with torch.cuda.device(self.dev):
            self.d_sel, self.d_src = torch.as_tensor(sel, device=self.dev), torch.as_tensor(src, device=self.dev)
            self.frame0 = None
            if self.header["n_fixed"]:
                ident = torch.arange(self.natoms, dtype=torch.int32, device=self.dev)
                f0 = torch.empty((1, self.natoms, 3), dtype=torch.float32, device=self.dev)
                raw, nb, desc, _ = self.stage(np.zeros(1, np.int64))
                st = torch.empty(1, dtype=torch.int32, device=self.dev)
                self.launch(raw[:nb].to(self.dev), torch.as_tensor(desc, device=self.dev), 1, f0, st, 1.0, sel=ident, src=ident, nsel=self.natoms)
                if int(st.item()):
                    raise RuntimeError(f"device DCD decoder: frame 0 of {filename} is not inside the bytes it was given")
                self.frame0 = f0

    def stage(self, idx, pinned=None):
        """The bytes of the span between the lowest and the highest frame of ``idx`` in pinned memory (``pinned`` when it is large
        enough, else a new buffer), their descriptors and unit cells: ``(buffer, n_bytes, desc, cell)``."""
        import torch

        desc, lo, hi, cell = chunk_desc(self.filename, idx)
        if pinned is None or pinned.numel() < hi - lo:
            pinned = torch.empty(hi - lo, dtype=torch.uint8, pin_memory=True)
        _lib._check(_lib.load().mkamd_xtc_copy_bytes(self.path, lo, hi, pinned.data_ptr(), 0))
        return pinned, hi - lo, desc, cell

    def launch(self, d_raw, d_desc, n, xyz, d_st, scale, sel=None, src=None, nsel=None, stream=None):
        import torch

        s = stream if stream is not None else torch.cuda.current_stream(self.dev).cuda_stream
        _lib._check(_lib.load().mkamd_dcd_decode_dev(self.ctx._h, s or None, d_raw.data_ptr(), d_raw.numel(), d_desc.data_ptr(), n,
                                                     (self.d_sel if sel is None else sel).data_ptr(), (self.d_src if src is None else src).data_ptr(),
                                                     self.nsel if nsel is None else nsel, None if self.frame0 is None else self.frame0.data_ptr(),
                                                     self.natoms, float(scale), xyz.data_ptr(), d_st.data_ptr()))


def read_dcd_frames_dev(filename, frames=None, atom_indices=None, scale: float = 1.0, ctx=None):
    """The listed frames (any order, repeats allowed; None = all) with the coordinates decoded ON THE GPU: ``(xyz, cell_lengths,
    cell_angles)`` with ``xyz`` a float32 CUDA tensor ``[n, n_sel, 3]`` (frame-major, the layout ``read_xtc_frames_dev`` returns) whose
    values are bit for bit ``load_dcd``'s (times ``scale``, multiplied as float32 only when it is not 1) and the cells as ``load_dcd``
    returns them.  One chunk: the span of the file between the lowest and the highest listed frame is uploaded.  Synchronous; the
    streaming form is ``batch.iterVoxelizeDCD``.  Raises on a nonzero status, naming the frame."""
    import torch

    rd = DeviceReader(filename, atom_indices, ctx)
    sel = np.arange(rd.nframes, dtype=np.int64) if frames is None else np.ascontiguousarray(frames, dtype=np.int64).reshape(-1)
    n = len(sel)
    xyz = torch.empty((n, rd.nsel, 3), dtype=torch.float32, device=rd.dev)
    if n == 0:
        return xyz, None, None
    raw, nb, desc, cell = rd.stage(sel)
    with torch.cuda.device(rd.dev):
        d_raw = raw[:nb].to(rd.dev, non_blocking=True)
        d_desc = torch.as_tensor(desc, device=rd.dev)
        d_st = torch.empty(n, dtype=torch.int32, device=rd.dev)
        rd.launch(d_raw, d_desc, n, xyz, d_st, scale)
        st = d_st.cpu().numpy()
    if st.any():
        raise RuntimeError(f"device DCD decoder: frame {int(sel[int(np.flatnonzero(st)[0])])} of {filename} reaches outside the uploaded bytes")
    return (xyz,) + _cells(cell)


def DCDread(filename, frame=None, stride=None, atom_indices=None) -> Trajectory:
    """``readers.DCDread``: coordinates ``[N, 3, F]``, box and boxangles ``[3, F]`` (or None), ``step`` from ISTART / NSAVC and ``time`` in
    fs from DELTA.  The reference numbers the steps of the frames it returned and then strides them AGAIN when a stride is given; kept."""
    xyz, lengths, angles = load_dcd(filename, stride=stride, atom_indices=atom_indices, frame=frame)
    istart, nsavc, delta = read_header(filename)
    delta = np.round(delta * _FS_PER_DELTA, decimals=8)
    steps = np.arange(istart, (nsavc * xyz.shape[0]) + istart, nsavc)
    if stride is not None:
        steps = steps[::stride]
    # (step / time with the dtypes the reference's Trajectory record gives them; box and boxangles stay None for a file without cells)
    return Trajectory(coords=np.transpose(xyz, (1, 2, 0)), box=None if lengths is None else lengths.T,
                      boxangles=None if angles is None else angles.T, step=np.array(steps, dtype=np.uint64),
                      time=np.array(steps * delta * 1000, dtype=np.float64))


# ------------------------------------------------------------------------------------------------
# writing: the reference writer's bytes
# ------------------------------------------------------------------------------------------------
def cell_records(cell_lengths, cell_angles, nframes):
    """The six doubles of every frame's unit-cell record ``[F, 6]`` from float32 lengths and angles ``[F, 3]``: A, cos(gamma), B,
    cos(beta), cos(alpha), C with the cosines as ``sin(pi/2 / 90 * (90 - angle))`` (an angle of 0 is written as 1, of 90 as 0)."""
    if (cell_lengths is None) != (cell_angles is None):
        raise ValueError("cell_lengths and cell_angles must be given together")
    if cell_lengths is None:
        return None
    lengths = np.ascontiguousarray(np.asarray(cell_lengths), dtype=np.float32)
    angles = np.ascontiguousarray(np.asarray(cell_angles), dtype=np.float32)
    if lengths.shape != (nframes, 3) or angles.shape != (nframes, 3):
        raise ValueError("cell_lengths and cell_angles must be (nframes, 3)")
    out = np.empty((nframes, 6), dtype=np.float64)
    _lib._check(_lib.load().mkamd_dcd_cell_record(_lib._ptr(lengths), _lib._ptr(angles), nframes, _lib._ptr(out)))
    return out


def file_header(natoms, nframes, istart=0, nsavc=1, delta=1.0, with_cell=True) -> bytes:
    """The writer's 276-byte header: NSET = ``nframes`` at byte 8, ``istart + nframes * nsavc`` at byte 20."""
    for name, v in (("istart", istart), ("nsavc", nsavc)):
        if not -2 ** 31 <= int(v) < 2 ** 31:
            raise OverflowError(f"{name} does not fit the DCD header's int")
    out = np.zeros(HEADER_BYTES, dtype=np.uint8)
    _lib._check(_lib.load().mkamd_dcd_header(int(natoms), int(nframes), int(istart), int(nsavc), float(delta), int(bool(with_cell)), _lib._ptr(out)))
    return out.tobytes()


def encode_dcd_dev(xyz, cell_lengths, cell_angles, ctx=None):
    """The frame images of ``xyz`` (float32 CUDA tensor ``[F, N, 3]``) as the reference's writer lays them out, one after the other, as
    a uint8 CUDA tensor: per frame the 48-byte cell record between its markers (unless both cell arguments are None), then the x, y
    and z planes between theirs."""
    import torch

    ctx = ctx or _lib.default_context()
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda or xyz.ndim != 3 or xyz.shape[2] != 3:
        raise ValueError("xyz must be a CUDA tensor of shape (nframes, natoms, 3)")
    F, N = int(xyz.shape[0]), int(xyz.shape[1])
    if N == 0:
        raise ValueError("a DCD file holds at least one atom")
    cell = cell_records(cell_lengths, cell_angles, F)
    lib, dev = _lib.load(), xyz.device
    with torch.cuda.device(dev):
        x = xyz.to(torch.float32).contiguous()
        bound = int(lib.mkamd_dcd_encode_bound(F, N, int(cell is not None)))
        image = torch.empty(bound, dtype=torch.uint8, device=dev)
        d_cell = None if cell is None or F == 0 else torch.as_tensor(cell, device=dev)
        s = torch.cuda.current_stream(dev)
        _lib._check(lib.mkamd_dcd_encode_dev(ctx._h, s.cuda_stream or None, x.data_ptr(), None if d_cell is None else d_cell.data_ptr(), F, N,
                                             image.data_ptr(), bound))
        s.synchronize()                                           # (x and d_cell may be temporaries)
    return image


def default_chunk(natoms: int) -> int:
    """Frames ``write_dcd_dev`` encodes per call unless told otherwise: an image of about 1 GiB."""
    return max(1, (1 << 30) // (12 * int(natoms) + 80))


def write_dcd_dev(filename, xyz, cell_lengths, cell_angles, istart=0, nsavc=1, delta=1.0, chunk=None, ctx=None):
    """Write frames resident on the GPU as a DCD file with the reference writer's bytes (all but the creation-time remark, bytes
    180..259 of the header).  Chunks of ``chunk`` frames are encoded on the device and copied out through pinned memory into a temporary
    file next to the target, which is renamed over the target at the end."""
    import torch

    if not isinstance(xyz, torch.Tensor) or xyz.ndim != 3 or xyz.shape[2] != 3:
        raise ValueError("xyz must be a CUDA tensor of shape (nframes, natoms, 3)")
    F, N = int(xyz.shape[0]), int(xyz.shape[1])
    fn = os.fspath(filename)
    fn = fn.decode("UTF-8") if isinstance(fn, bytes) else fn
    chunk = default_chunk(N) if chunk is None else max(1, int(chunk))
    if (cell_lengths is None) != (cell_angles is None):
        raise ValueError("cell_lengths and cell_angles must be given together")
    with_cell = cell_lengths is not None
    if with_cell:
        cell_lengths, cell_angles = (np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v) for v in (cell_lengths, cell_angles))
        if cell_lengths.shape != (F, 3) or cell_angles.shape != (F, 3):
            raise ValueError("cell_lengths and cell_angles must be (nframes, 3)")
    head = file_header(N, F, istart, nsavc, delta, with_cell)
    tmp = "%s.tmp.%d" % (fn, os.getpid())
    try:
        with open(tmp, "wb") as fh:
            fh.write(head)
            for lo in range(0, F, chunk):
                hi = min(F, lo + chunk)
                image = encode_dcd_dev(xyz[lo:hi], cell_lengths[lo:hi] if with_cell else None, cell_angles[lo:hi] if with_cell else None, ctx)
                host = torch.empty(image.numel(), dtype=torch.uint8, pin_memory=True)
                host.copy_(image, non_blocking=True)
                torch.cuda.current_stream(image.device).synchronize()
                fh.write(memoryview(host.numpy()))
        os.replace(tmp, fn)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _dcdwrite_arrays(mol):
    """What ``writers.DCDwrite`` hands to its writer, from a duck-typed molecule: ``(coords [N, 3, F], cell_lengths [F, 3], cell_angles
    [F, 3], istart, nsavc, delta)``.  All-zero boxes / angles are written as zeros; ``istart``, ``nsavc`` and ``delta`` come from ``step``
    and ``fstep`` (ns), steps that do not fit an int32 are renumbered, and anything that fails gives 0 / 1 / 1.0."""
    coords = np.asarray(mol.coords)
    n_frames = coords.shape[2]
    box = np.asarray(mol.box).T if not np.all(np.asarray(mol.box) == 0) else np.zeros((n_frames, 3), dtype=np.float32)
    boxangles = np.asarray(mol.boxangles).T if not np.all(np.asarray(mol.boxangles) == 0) else np.zeros((n_frames, 3), dtype=np.float32)
    try:
        istart = int(mol.step[0])
        nsavc = int(mol.step[1] - mol.step[0])
        fstep = mol.fstep * 1000                                  # ns -> ps
        delta = fstep / nsavc / _FS_PER_DELTA
        if mol.step[0] != mol.step[0].astype(np.int32):
            istart //= nsavc
            delta *= nsavc
            nsavc = 1
        if istart != np.array(istart).astype(np.int32):           # still too large: start from 1
            istart = 1
    except Exception:
        istart, nsavc, delta = 0, 1, 1.0
    return coords, box, boxangles, istart, nsavc, delta


def DCDwrite(mol, filename, ctx=None):
    """``writers.DCDwrite`` with the frame images formed on the GPU: the same file but for the creation-time remark."""
    import torch

    ctx = ctx or _lib.default_context()
    coords, box, boxangles, istart, nsavc, delta = _dcdwrite_arrays(mol)
    dev = torch.device("cuda", ctx.device)
    xyz = torch.as_tensor(np.ascontiguousarray(np.asarray(coords, dtype=np.float32).transpose(2, 0, 1))).to(dev)
    write_dcd_dev(filename, xyz, box, boxangles, istart=istart, nsavc=nsavc, delta=delta, ctx=ctx)


def install():
    """Make an installed moleculekit read and write DCD files through this module: swaps ``moleculekit.readers.DCDread`` and the
    ``"dcd"`` entry of ``_TRAJECTORY_READERS``, ``moleculekit.writers.DCDwrite`` and the ``"dcd"`` entry of ``_WRITERS``.  Returns the
    original ``(reader, writer)``; ``uninstall()`` puts everything back."""
    import moleculekit.readers as rd
    import moleculekit.writers as wr

    if getattr(rd, "_DCDread_reference", None) is not None:             # already installed
        return rd._DCDread_reference, wr._DCDwrite_reference

    def read_hook(filename, frame=None, topoloc=None, stride=None, atom_indices=None):
        t = DCDread(filename, frame=frame, stride=stride, atom_indices=atom_indices)
        traj = rd.Trajectory(coords=t.coords, box=t.box, boxangles=t.boxangles, step=t.step, time=t.time)
        return rd.MolFactory.construct(None, traj, filename, frame)

    write_hook = lambda mol, filename, **kw: DCDwrite(mol, filename, **kw)   # noqa: E731
    rd._DCDread_reference, rd._TRAJECTORY_READERS_dcd_reference = rd.DCDread, rd._TRAJECTORY_READERS.get("dcd")
    wr._DCDwrite_reference, wr._WRITERS_dcd_reference = wr.DCDwrite, wr._WRITERS.get("dcd")
    rd.DCDread = rd._TRAJECTORY_READERS["dcd"] = read_hook
    wr.DCDwrite = wr._WRITERS["dcd"] = write_hook
    return rd._DCDread_reference, wr._DCDwrite_reference


def uninstall():
    """Undo ``install()``."""
    import moleculekit.readers as rd
    import moleculekit.writers as wr

    if getattr(rd, "_DCDread_reference", None) is None:
        return
    for mod, name, table, key in ((rd, "DCDread", rd._TRAJECTORY_READERS, "_TRAJECTORY_READERS_dcd_reference"),
                                  (wr, "DCDwrite", wr._WRITERS, "_WRITERS_dcd_reference")):
        setattr(mod, name, getattr(mod, "_%s_reference" % name))
        if getattr(mod, key) is not None:
            table["dcd"] = getattr(mod, key)
        else:
            table.pop("dcd", None)
        setattr(mod, "_%s_reference" % name, None)
        setattr(mod, key, None)
