"""XTC trajectory reading on top of libmkamd.so's host-side decoder.

Mirrors the reference's low-level module ``moleculekit.xtc`` (fileformats/xtc/xtc.pyx: ``get_xtc_natoms``,
``get_xtc_nframes``, ``read_xtc`` :34-53, ``read_xtc_frames`` :57-81 -- same arrays, same float32 bits, units as in the
file: nm / ps) and ``readers.XTCread`` (readers.py:1830-1866: the conversion to Angstrom / fs and from box vectors to
lengths and angles, unitcell.py:128-221).  Frames are decoded in parallel on host threads.  ``XTCread`` returns a
plain ``Trajectory`` record (coords float32 [N,3,F] in A, box [3,F], boxangles, step, time) -- the arrays
``batch.iterVoxelizeTrajectory`` / ``voxelizeTrajectory`` take; building a ``Molecule`` around it is outside this package.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import numpy as np

from . import _lib

Trajectory = namedtuple("Trajectory", ["coords", "box", "boxangles", "step", "time"])


def _path(filename) -> bytes:
    return filename if isinstance(filename, bytes) else str(filename).encode("UTF-8")


def _info(filename):
    na, nf = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib._check(_lib.load().mkamd_xtc_info(_path(filename), ctypes.byref(na), ctypes.byref(nf)))
    return na.value, nf.value


def get_xtc_natoms(filename) -> int:
    return _info(filename)[0]


def get_xtc_nframes(filename) -> int:
    return _info(filename)[1]


def _read(filename, frames, nthreads):
    natoms, nframes = _info(filename)
    if frames is None:
        sel, n = None, nframes
    else:
        sel = np.ascontiguousarray(frames, dtype=np.int64).reshape(-1)
        n = len(sel)
    coords = np.zeros((natoms, 3, n), dtype=np.float32)
    box = np.zeros((3, 3, n), dtype=np.float32)
    time = np.zeros(n, dtype=np.float32)
    step = np.zeros(n, dtype=np.int32)
    _lib._check(_lib.load().mkamd_xtc_read(_path(filename), _lib._ptr(sel), n, natoms, _lib._ptr(coords), _lib._ptr(box),
                                           _lib._ptr(time), _lib._ptr(step), int(nthreads)))
    return coords, box, time, step


def read_xtc(filename, nthreads: int = 0):
    """All frames: ``(coords f32 [N,3,F] nm, boxvectors f32 [3,3,F] nm, time f32 [F] ps, step i32 [F])``."""
    return _read(filename, None, nthreads)


def read_xtc_frames(filename, frames, nthreads: int = 0):
    """The listed frames (any order), same return layout as ``read_xtc``."""
    return _read(filename, frames, nthreads)


def box_vectors_to_lengths_and_angles(a, b, c):
    """Box lengths and angles (degrees) from box vectors, per frame (unitcell.py:128-221); all-zero vectors give
    zero lengths and 90 degree angles."""
    a, b, c = (np.asarray(v) for v in (a, b, c))
    if np.all(a == 0) or np.all(b == 0) or np.all(c == 0):
        nf = a.shape[:-1]
        return np.zeros(nf), np.zeros(nf), np.zeros(nf), np.full(nf, 90.0), np.full(nf, 90.0), np.full(nf, 90.0)
    la, lb, lc = (np.sqrt(np.sum(v * v, axis=-1)) for v in (a, b, c))
    ang = lambda u, v, lu, lv: np.arccos(np.einsum("...i, ...i", u, v) / (lu * lv)) * 180.0 / np.pi
    return la, lb, lc, ang(b, c, lb, lc), ang(c, a, lc, la), ang(a, b, la, lb)


def XTCread(filename, frame=None, nthreads: int = 0) -> Trajectory:
    """``readers.XTCread`` (readers.py:1830-1866): coordinates and box in Angstrom (x10), time in fs (x1e3); step
    and time replaced by 0..F-1 / zeros when the file holds none (all-zero sums), like the reference."""
    if frame is None:
        coords, boxvectors, time, step = read_xtc(filename, nthreads)
    else:
        coords, boxvectors, time, step = read_xtc_frames(filename, np.atleast_1d(frame), nthreads)
    if coords.shape[2] == 0:
        raise RuntimeError(f"Malformed XTC file. No frames read from: {filename}")
    if coords.shape[0] == 0:
        raise RuntimeError(f"Malformed XTC file. No atoms read from: {filename}")
    time = time.astype(np.float64)
    coords *= 10.0
    boxvectors *= 10.0
    time *= 1e3
    nframes = coords.shape[2]
    if np.sum(step) == 0:
        step = np.arange(nframes, dtype=np.uint64)
    if np.sum(time) == 0:
        time = np.zeros(nframes, dtype=np.float64)
    bx, by, bz, alpha, beta, gamma = box_vectors_to_lengths_and_angles(boxvectors[0].T, boxvectors[1].T, boxvectors[2].T)
    return Trajectory(coords=coords, box=np.stack([bx, by, bz], axis=0), boxangles=np.stack([alpha, beta, gamma], axis=0),
                      step=step, time=time)


# ------------------------------------------------------------------------------------------------
# decoding on the device (round 4; include/mkamd_xtc.h, csrc/xtc_gpu.h): a GPU lane decodes a frame
# ------------------------------------------------------------------------------------------------
DESC_BYTES = 64        # sizeof(mkamd::XtcFrameDesc)
XTC_PAD = 1024         # bytes the device copy of a chunk's records extends past them (MKAMD_XTC_PAD, include/mkamd_xtc.h)


DESC_DTYPE = np.dtype([("data_off", "<u8"), ("nbytes", "<u4"), ("smallidx", "<i4"), ("lo", "<i4", 3), ("range", "<u4", 3),
                       ("inv_precision", "<f4"), ("triple_bits", "<i4"), ("field_bits", "<i4", 3), ("raw", "<i4")])
assert DESC_DTYPE.itemsize == DESC_BYTES


def device_decodable(desc, natoms) -> bool:
    """What the headers tell about ``status 2`` of the device decoder (include/mkamd_xtc.h): no frame of ``desc`` (from
    ``chunk_desc``) packs a coordinate into more than 64 bits, has >= 2^21 atoms or a stream of >= 512 MB, or may code a run
    of small atoms in more than 64 bits.  The last is not a matter of the ranges: the writer picks the header's small-number
    index from the smallest step between neighbouring atoms (xdrfile.cpp, the ``mindiff`` loop) -- atoms 1 000 nm apart in a
    file of 1e6 quanta per axis give 65 -- and within a frame the index never exceeds its initial value + 8.  Whether a run
    actually comes at an index above 64 only the stream tells, so a compressed frame (> 9 atoms) whose header index + 8 exceeds
    64 is refused: True means the device decodes every frame (status 0); False, that the host decoder should."""
    d = np.ascontiguousarray(desc).view(DESC_DTYPE).reshape(-1)
    runs_fit = natoms <= 9 or bool(np.all(d["smallidx"] + 8 <= 64))
    return bool(natoms < (1 << 21) and runs_fit and np.all(d["triple_bits"] <= 64) and np.all(d["nbytes"] < (1 << 29) - 4))


def chunk_desc(filename, frames, natoms):
    """Host half of the device decoder for the frames ``frames`` (int64 array): ``(desc uint8 [n, 64], byte_lo, byte_hi,
    boxvectors f32 [3,3,n] nm, time f32 [n] ps, step i32 [n])`` -- record headers only, no coordinate is decoded."""
    sel = np.ascontiguousarray(frames, dtype=np.int64).reshape(-1)
    n = len(sel)
    desc = np.empty((n, DESC_BYTES), dtype=np.uint8)
    box = np.empty((3, 3, n), dtype=np.float32)
    time = np.empty(n, dtype=np.float32)
    step = np.empty(n, dtype=np.int32)
    lo, hi = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib._check(_lib.load().mkamd_xtc_chunk_desc(_path(filename), _lib._ptr(sel), n, int(natoms), _lib._ptr(desc), ctypes.byref(lo),
                                                 ctypes.byref(hi), _lib._ptr(box), _lib._ptr(time), _lib._ptr(step)))
    return desc, int(lo.value), int(hi.value), box, time, step


def byte_range(filename, frames, natoms):
    """``(byte_lo, byte_hi)`` of the records of ``frames`` from the frame index alone (no record is read)."""
    sel = np.ascontiguousarray(frames, dtype=np.int64).reshape(-1)
    lo, hi = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib._check(_lib.load().mkamd_xtc_byte_range(_path(filename), _lib._ptr(sel), len(sel), int(natoms), ctypes.byref(lo), ctypes.byref(hi)))
    return int(lo.value), int(hi.value)


def chunk_desc_mem(filename, frames, natoms, bytes_ptr, bytes_lo, bytes_hi):
    """``chunk_desc`` from a host COPY of the file's bytes ``[bytes_lo, bytes_hi)`` at address ``bytes_ptr`` (the pinned staging buffer
    ``mkamd_xtc_copy_bytes`` has just filled): the same tuple, without touching the file's pages once more."""
    sel = np.ascontiguousarray(frames, dtype=np.int64).reshape(-1)
    n = len(sel)
    desc = np.empty((n, DESC_BYTES), dtype=np.uint8)
    box = np.empty((3, 3, n), dtype=np.float32)
    time = np.empty(n, dtype=np.float32)
    step = np.empty(n, dtype=np.int32)
    lo, hi = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib._check(_lib.load().mkamd_xtc_chunk_desc_mem(_path(filename), _lib._ptr(sel), n, int(natoms), ctypes.c_void_p(int(bytes_ptr)), int(bytes_lo),
                                                     int(bytes_hi), _lib._ptr(desc), ctypes.byref(lo), ctypes.byref(hi), _lib._ptr(box), _lib._ptr(time),
                                                     _lib._ptr(step)))
    return desc, int(lo.value), int(hi.value), box, time, step


def read_xtc_frames_dev(filename, frames=None, scale: float = 1.0, ctx=None):
    """``read_xtc_frames`` with the coordinates decoded ON THE GPU: returns ``(xyz, boxvectors, time, step)`` with ``xyz`` a
    float32 CUDA tensor ``[n, natoms, 3]`` (frame-major: the voxelizer's packed items; ``scale`` 10 gives Angstrom) whose
    values are bit for bit ``read_xtc_frames(...)[0] * scale`` transposed.  Synchronous (tests, one-off reads); the streaming
    form is ``batch.iterVoxelizeXTC`` (``decode="auto"`` / ``"gpu"``).  Raises for a stream the device decoder refuses (ranges
    whose mixed-radix number exceeds 64 bits, >= 2^21 atoms: use the host decoder)."""
    import torch

    ctx = ctx or _lib.default_context()
    natoms, nframes = _info(filename)
    sel = np.arange(nframes, dtype=np.int64) if frames is None else np.ascontiguousarray(frames, dtype=np.int64).reshape(-1)
    dev = torch.device("cuda", ctx.device)
    n = len(sel)
    xyz = torch.empty((n, natoms, 3), dtype=torch.float32, device=dev)
    if n == 0:
        return xyz, np.zeros((3, 3, 0), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32)
    desc, lo, hi, box, time, step = chunk_desc(filename, sel, natoms)
    raw = torch.zeros(hi - lo + XTC_PAD, dtype=torch.uint8).pin_memory()          # (the kernel reads ahead of what it uses)
    _lib._check(_lib.load().mkamd_xtc_copy_bytes(_path(filename), lo, hi, raw.data_ptr(), 0))
    with torch.cuda.device(dev):
        d_raw = raw.to(dev, non_blocking=True)
        d_desc = torch.as_tensor(desc, device=dev)
        d_st = torch.empty(n, dtype=torch.int32, device=dev)
        work = torch.empty(int(_lib.load().mkamd_xtc_decode_work_bytes(n, natoms)), dtype=torch.uint8, device=dev)
        s = torch.cuda.current_stream(dev)
        _lib._check(_lib.load().mkamd_xtc_decode_dev(ctx._h, s.cuda_stream or None, d_raw.data_ptr(), d_desc.data_ptr(), n, natoms,
                                                     float(scale), xyz.data_ptr(), d_st.data_ptr(), work.data_ptr(), work.numel()))
        st = d_st.cpu().numpy()
    if st.any():
        bad = int(np.flatnonzero(st)[0])
        raise RuntimeError(f"device XTC decoder: frame {int(sel[bad])} " + ("is corrupt" if st[bad] == 1 else
                           "is outside what the device decoder takes (numbers of more than 64 bits -- a coordinate range beyond ~2 million "
                           "quanta per axis --, >= 2^21 atoms or >= 512 MB per frame): use the host decoder"))
    return xyz, box, time, step


# ------------------------------------------------------------------------------------------------
# writing (round 4): enough of an encoder to produce valid trajectories for tests and benchmarks
# ------------------------------------------------------------------------------------------------
_MAGIC = 1995
_FIRSTIDX = 9          # index of the first usable entry of the format's table of "magic" sizes (xdrfile.cpp:545)


def _pack_bits(*fields):
    """Per atom the bit fields ``(values uint64 [N], nbits)`` one after the other, most significant bit first; the atoms
    concatenated -> uint8 bytes, zero-padded to a whole byte."""
    cols = []
    for values, nbits in fields:
        shifts = np.arange(nbits - 1, -1, -1, dtype=np.uint64)
        cols.append(((values[:, None] >> shifts[None, :]) & np.uint64(1)).astype(np.uint8))
    return np.packbits(np.concatenate(cols, axis=1).reshape(-1))


def write_xtc(filename, coords, box, time, step, precision: float = 1000.0):
    """``moleculekit.xtc.write_xtc`` (fileformats/xtc/xtc.pyx:86-97): coords float32 [N,3,F] in nm, box vectors float32
    [3,3,F] in nm, time float32 [F] (ps), step [F].  Appends nothing, overwrites ``filename``.

    The coordinate block is the format's compressed form (xdrfile.cpp: xdrfile_compress_coord_float) in its simplest legal
    shape: every atom is written as one "large" coordinate -- the three integers ``round(x * precision) - min`` folded into
    one mixed-radix number of ``bits(prod(range))`` bits, least-significant byte first -- followed by a 0 flag bit ("run
    length unchanged": it starts at 0, so no atom is ever coded as a small difference to its predecessor).  The
    reference's writer finds runs of near neighbours (water molecules) and codes them in fewer bits; a decoder reads both
    alike, and this one costs ~5 bytes per atom of a 67 A box instead of ~4.  Up to nine atoms are stored as plain floats,
    like the reference does."""
    import struct

    coords = np.ascontiguousarray(coords, dtype=np.float32)
    if coords.ndim != 3 or coords.shape[1] != 3:
        raise ValueError("coords must be (natoms, 3, nframes)")
    N, _, F = coords.shape
    box = np.ascontiguousarray(box, dtype=np.float32).reshape(3, 3, -1)
    if box.shape[2] != F:
        raise ValueError("box must hold one set of box vectors per frame: (3, 3, nframes)")
    time = np.ascontiguousarray(time, dtype=np.float32).reshape(-1)
    step = np.ascontiguousarray(step).astype(np.int64).reshape(-1)
    if len(time) != F or len(step) != F:
        raise ValueError("time and step must have one entry per frame")
    prec = np.float32(precision)
    with open(_path(filename), "wb") as fh:
        for f in range(F):
            fh.write(struct.pack(">iii", _MAGIC, N, int(step[f]) & 0x7fffffff))
            fh.write(struct.pack(">f", float(time[f])))
            fh.write(box[:, :, f].astype(">f4").tobytes())               # row-major box vectors
            fh.write(struct.pack(">i", N))
            x = coords[:, :, f]
            if N <= 9:
                fh.write(x.astype(">f4").tobytes())
                continue
            # xdrfile.cpp:606-624: lf = x * precision; (int)(lf + 0.5) for lf >= 0, (int)(lf - 0.5) below (float arithmetic)
            lf = x * prec
            if not np.all(np.abs(lf) < 2.0e9):
                raise ValueError("coordinate too large for the XTC integer range at this precision")
            ints = np.where(lf >= 0, lf + np.float32(0.5), lf - np.float32(0.5)).astype(np.int64)
            lo, hi = ints.min(0), ints.max(0)
            size = (hi - lo + 1).astype(np.int64)
            rel = (ints - lo).astype(np.uint64)
            head = struct.pack(">f", float(prec)) + struct.pack(">iii", *[int(v) for v in lo]) + struct.pack(">iii", *[int(v) for v in hi])
            if np.any(size > 0xffffff):
                # per-axis fields (xdrfile.cpp:634-640: bitsize = 0)
                nb = [int(int(s).bit_length()) for s in size]
                payload = _pack_bits((rel[:, 0], nb[0]), (rel[:, 1], nb[1]), (rel[:, 2], nb[2]), (np.zeros(N, np.uint64), 1))
            else:
                prod = int(size[0]) * int(size[1]) * int(size[2])
                nbits = prod.bit_length()                                # sizeofints(3, sizeint), xdrfile.cpp:425-457
                if nbits <= 63:
                    V = (rel[:, 0] * np.uint64(size[1]) + rel[:, 1]) * np.uint64(size[2]) + rel[:, 2]
                else:                                                    # three ranges of up to 24 bits: up to 72 bits -- Python integers
                    V = (rel[:, 0].astype(object) * int(size[1]) + rel[:, 1].astype(object)) * int(size[2]) + rel[:, 2].astype(object)
                # the number goes out least-significant BYTE first, its top (nbits mod 8, or 8) bits last (sendints, :489-543)
                nfull, top = (nbits - 1) // 8, nbits - 8 * ((nbits - 1) // 8)
                if nbits <= 63:
                    fields = [((V >> np.uint64(8 * b)) & np.uint64(0xff), 8) for b in range(nfull)]
                    fields.append(((V >> np.uint64(8 * nfull)) & np.uint64((1 << top) - 1), top))
                else:
                    byte = lambda sh, mask: np.array([(int(v) >> sh) & mask for v in V], dtype=np.uint64)
                    fields = [(byte(8 * b, 0xff), 8) for b in range(nfull)]
                    fields.append((byte(8 * nfull, (1 << top) - 1), top))
                fields.append((np.zeros(N, np.uint64), 1))               # ... then the flag bit: 0
                payload = _pack_bits(*fields)
            fh.write(head + struct.pack(">i", _FIRSTIDX))                # smallidx: any valid index (never used: no small atoms)
            fh.write(struct.pack(">i", len(payload)))
            fh.write(payload.tobytes() + b"\0" * ((4 - len(payload) % 4) % 4))


# ------------------------------------------------------------------------------------------------
# writing ON THE DEVICE (include/mkamd_xtc.h, csrc/xtc_encode.h): the reference writer's compressed bytes
# ------------------------------------------------------------------------------------------------
_REFUSED = ("is outside what the device writer takes: a coordinate that is not finite or leaves the int range at this precision, a "
            "coordinate range of >= 2^31 quanta, a full coordinate of more than 64 bits (ranges beyond ~2 million quanta per axis), a "
            "smallest neighbour step so large that the small-number index of the header exceeds 56, or >= 2^21 atoms")


def _to_dev(v, dtype, dev, shape=None):
    import torch
    if isinstance(v, torch.Tensor):
        t = v.to(device=dev, dtype=dtype)
        return (t.expand(shape) if t.ndim == 0 else t.reshape(shape)).contiguous()
    a = np.asarray(v, dtype={torch.float32: np.float32, torch.int32: np.int32}[dtype])
    a = np.array(np.broadcast_to(a, shape) if a.ndim == 0 else a.reshape(shape))       # (a writable copy: torch asks for one)
    return torch.as_tensor(a).to(dev)


def _step_i32(step):
    """Steps as the 32 bits an XTC record holds (the reference hands them over as unsigned)."""
    import torch
    if isinstance(step, torch.Tensor):
        return step
    return (np.asarray(step).astype(np.int64) & 0xffffffff).astype(np.uint32).view(np.int32)


def encode_xtc_dev(xyz, box, time, step, precision=1000.0, scale: float = 1.0, ctx=None):
    """The XTC file image of frames resident on the GPU, byte for byte what the reference's writer makes of them.

    ``xyz`` float32 CUDA tensor ``[F, N, 3]`` (frame-major, as ``read_xtc_frames_dev`` returns it), ``box`` the box vectors
    ``[3, 3, F]`` in nm, ``time`` ``[F]`` in ps, ``step`` ``[F]`` (arrays or tensors, as that reader returns them), ``precision`` a
    scalar or one value per frame; every coordinate is multiplied by ``scale`` first, rounded to float32 once (1 for nm, the float32
    0.1 for Angstrom).  Returns ``(image, offsets, status)``: a uint8 CUDA tensor trimmed to the records' total size, the records'
    byte offsets (int64 numpy ``[F + 1]``) and per frame 0 or 2 (int32 numpy ``[F]``); a frame of status 2 is outside what the device
    path takes and has no bytes in the image -- nothing falls back to another encoder."""
    import torch

    ctx = ctx or _lib.default_context()
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda or xyz.ndim != 3 or xyz.shape[2] != 3:
        raise ValueError("xyz must be a CUDA tensor of shape (nframes, natoms, 3)")
    dev = xyz.device
    F, N = int(xyz.shape[0]), int(xyz.shape[1])
    lib = _lib.load()
    with torch.cuda.device(dev):
        x = xyz.to(torch.float32).contiguous()
        b = box if isinstance(box, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(box, np.float32))
        if tuple(b.shape) != (3, 3, F):
            raise ValueError("box must hold one set of box vectors per frame: (3, 3, nframes)")
        d_box = b.to(device=dev, dtype=torch.float32).permute(2, 0, 1).contiguous()
        d_time = _to_dev(time, torch.float32, dev, (F,))
        d_step = _to_dev(_step_i32(step), torch.int32, dev, (F,))
        d_prec = _to_dev(precision, torch.float32, dev, (F,))
        bound = int(lib.mkamd_xtc_encode_bound(F, N))
        image = torch.empty(max(bound, 4), dtype=torch.uint8, device=dev)
        d_off = torch.zeros(F + 1, dtype=torch.int64, device=dev)
        d_st = torch.zeros(F, dtype=torch.int32, device=dev)
        work = torch.empty(max(int(lib.mkamd_xtc_encode_work_bytes(F, N)), 8), dtype=torch.uint8, device=dev)
        s = torch.cuda.current_stream(dev)
        _lib._check(lib.mkamd_xtc_encode_dev(ctx._h, s.cuda_stream or None, x.data_ptr(), float(np.float32(scale)), d_prec.data_ptr(),
                                             d_box.data_ptr(), d_time.data_ptr(), d_step.data_ptr(), F, N, image.data_ptr(), bound,
                                             d_off.data_ptr(), d_st.data_ptr(), work.data_ptr(), work.numel()))
        offsets = d_off.cpu().numpy()
        status = d_st.cpu().numpy()
    return image[:int(offsets[-1])], offsets, status


def _index_side_file(filename):
    """The frame-index side file an installed moleculekit keeps beside a trajectory (``<dir>/.<name>``); this package's own reader
    keeps its index in memory, keyed by the file's identity, and needs no invalidation."""
    import os
    d, name = os.path.split(os.fspath(filename))
    return os.path.join(d, "." + name)


def default_chunk(natoms: int) -> int:
    """Frames ``write_xtc_dev`` encodes per call unless told otherwise: work buffer and image (24 + 13 bytes per atom) of about
    4 GiB.  A call's time is the longest frame's walk whatever the number of frames, so fewer, larger chunks are faster."""
    return max(1, (4 << 30) // (40 * int(natoms) + 256))


def write_xtc_dev(filename, xyz, box, time, step, precision=1000.0, scale: float = 1.0, append: bool = False, chunk=None, ctx=None):
    """Write frames resident on the GPU as an XTC file with the reference writer's bytes (arguments as ``encode_xtc_dev``).

    Chunks of ``chunk`` frames are encoded on the device and copied out through pinned memory into a temporary file next to the
    target; on success it is renamed over the target, or its bytes are appended with ``append=True``.  If a frame is outside what the
    device path takes, ``RuntimeError`` names the first one and the target is left as it was."""
    import os
    import torch

    if not isinstance(xyz, torch.Tensor) or xyz.ndim != 3:
        raise ValueError("xyz must be a CUDA tensor of shape (nframes, natoms, 3)")
    F, N = int(xyz.shape[0]), int(xyz.shape[1])
    fn = os.fspath(filename)
    fn = fn.decode("UTF-8") if isinstance(fn, bytes) else fn
    chunk = default_chunk(N) if chunk is None else max(1, int(chunk))
    b = box if isinstance(box, torch.Tensor) else np.ascontiguousarray(box, np.float32)
    per = lambda v, lo, hi: v if getattr(v, "ndim", 0) == 0 else v[lo:hi]   # noqa: E731
    tmp = "%s.tmp.%d" % (fn, os.getpid())
    try:
        with open(tmp, "wb") as fh:
            for lo in range(0, F, chunk):
                hi = min(F, lo + chunk)
                image, _, status = encode_xtc_dev(xyz[lo:hi], b[:, :, lo:hi], per(time, lo, hi), per(step, lo, hi), per(precision, lo, hi),
                                                  scale, ctx)
                if status.any():
                    raise RuntimeError(f"device XTC writer: frame {lo + int(np.flatnonzero(status)[0])} {_REFUSED}")
                if image.numel():
                    host = torch.empty(image.numel(), dtype=torch.uint8, pin_memory=True)
                    host.copy_(image, non_blocking=True)
                    torch.cuda.current_stream(image.device).synchronize()
                    fh.write(memoryview(host.numpy()))
        side = _index_side_file(fn)
        if os.path.isfile(side):
            os.remove(side)
        if append and os.path.exists(fn):
            with open(fn, "ab") as out, open(tmp, "rb") as src:
                while True:
                    buf = src.read(1 << 24)
                    if not buf:
                        break
                    out.write(buf)
        else:
            os.replace(tmp, fn)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _xtcwrite_arrays(mol):
    """What ``writers.XTCwrite`` (writers.py:271-311) hands to its writer, from a duck-typed molecule: ``(coords float32 [N, 3, F] in
    Angstrom, box vectors float32 [3, 3, F] in nm, time float32 [F] in ps, step uint32 [F])``.  Box vectors default to zeros and one
    frame's are repeated for every frame; steps that do not fit 32 bits are renumbered from 1; times (fs) that float32 cannot hold are
    rebuilt from ``fstep`` and the step stride, starting from the first frame (``_format_large_time``)."""
    coords = np.asarray(mol.coords)
    nframes = int(getattr(mol, "numFrames", coords.shape[2]))
    box = np.zeros((3, 3, nframes), dtype=np.float32)
    if hasattr(mol, "box") and getattr(mol, "boxvectors", None) is not None:
        box = np.asarray(mol.boxvectors)
    if np.size(box, 2) != nframes:
        box = np.tile(box, (1, 1, nframes))
    step = np.asarray(getattr(mol, "step", np.zeros(nframes, dtype=np.int64)))
    time = np.asarray(getattr(mol, "time", np.zeros(nframes)))
    trajfreq = step[0] if len(step) == 1 else step[1] - step[0]
    if step[-1] != step[-1].astype(np.uint32):
        out_step = np.arange(1, nframes + 1, dtype=np.uint32)
    else:
        out_step = step.astype(np.uint32)
    out_time = time / 1e3                                            # fs -> ps
    if out_time[-1] != out_time[-1].astype(np.float32):
        if trajfreq == 0:
            raise AssertionError("The trajectory step should not be 0")
        timestep = (mol.fstep / trajfreq) / 1e-6
        out_time = (time - ((step[0] - trajfreq) * timestep)) / 1e3
    return coords, np.ascontiguousarray(box.astype(np.float32) * 0.1), np.ascontiguousarray(out_time.astype(np.float32)), np.ascontiguousarray(out_step)


def XTCwrite(mol, filename, ctx=None):
    """``writers.XTCwrite`` with the compression on the GPU: the same file, byte for byte.  Precision 1000; coordinates go to nm as
    float32 ``* 0.1`` on the device; an existing file is replaced.  Only the coordinates, box vectors, times and steps travel to the
    device."""
    import torch

    ctx = ctx or _lib.default_context()
    coords, box, time, step = _xtcwrite_arrays(mol)
    dev = torch.device("cuda", ctx.device)
    xyz = torch.as_tensor(np.ascontiguousarray(np.asarray(coords, dtype=np.float32).transpose(2, 0, 1))).to(dev)
    write_xtc_dev(filename, xyz, box, time, step, precision=1000.0, scale=float(np.float32(0.1)), ctx=ctx)


def install():
    """Make an installed moleculekit write XTC files through the GPU: swaps ``moleculekit.writers.XTCwrite`` and the ``"xtc"`` entry of
    ``moleculekit.writers._WRITERS``.  Returns the original function; ``uninstall()`` puts both back."""
    import moleculekit.writers as ref

    if getattr(ref, "_XTCwrite_reference", None) is not None:           # already installed
        return ref._XTCwrite_reference
    original = ref.XTCwrite
    hook = lambda mol, filename, **kw: XTCwrite(mol, filename, **kw)   # noqa: E731
    ref._XTCwrite_reference = original
    ref._WRITERS_xtc_reference = ref._WRITERS.get("xtc")
    ref.XTCwrite = hook
    ref._WRITERS["xtc"] = hook
    return original


def uninstall():
    """Undo ``install()``."""
    import moleculekit.writers as ref

    original = getattr(ref, "_XTCwrite_reference", None)
    if original is None:
        return
    ref.XTCwrite = original
    if ref._WRITERS_xtc_reference is not None:
        ref._WRITERS["xtc"] = ref._WRITERS_xtc_reference
    else:
        ref._WRITERS.pop("xtc", None)
    ref._XTCwrite_reference = None
    ref._WRITERS_xtc_reference = None
