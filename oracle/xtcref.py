"""oracle/xtcref.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

ctypes front-end for ``oracle/_ref/libxtcref.so``, the reference's own XTC codec compiled from the reference tree by
``oracle.build_ref_xtc()``: its writer compresses trajectories the way real files are written (runs of small atoms, the
water swap, the adaptive small-number table) and its reader is what the package's two XTC decoders are pinned against.
Only the library's exported C symbols are used: ``xdrfile_open``, ``xdrfile_close``, ``write_xtc``, ``read_xtc``.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import oracle

_lib = None
_EXDR_ENDOFFILE = 11      # xdrfile.h: the enum's 12th entry


def available() -> bool:
    """The library exists, or can be built from the reference tree."""
    try:
        return oracle.build_ref_xtc() is not None
    except Exception:
        return False


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        path = oracle.build_ref_xtc()
        if path is None:
            raise RuntimeError("oracle/_ref/libxtcref.so is absent and the reference tree is not there to build it from")
        L = ctypes.CDLL(path)
        L.xdrfile_open.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        L.xdrfile_open.restype = ctypes.c_void_p
        L.xdrfile_close.argtypes = [ctypes.c_void_p]
        L.xdrfile_close.restype = ctypes.c_int
        L.write_xtc.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float]
        L.write_xtc.restype = ctypes.c_int
        L.read_xtc.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float), ctypes.c_void_p,
                               ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        L.read_xtc.restype = ctypes.c_int
        _lib = L
    return _lib


def _per_frame(v, F, dtype, default):
    if v is None:
        return default
    a = np.asarray(v, dtype=dtype)
    return np.broadcast_to(a, (F,)) if a.ndim == 0 else a.reshape(F)


def ref_write_xtc(path, coords, box=None, time=None, step=None, precision=1000.0):
    """Write ``coords`` float32 [F, N, 3] (nm) with the reference's ``write_xtc``, one call per frame.  ``box`` [F, 3, 3] or
    [3, 3] (box vectors, rows; zeros when None), ``time`` / ``step`` per frame (0..F-1 when None), ``precision`` a scalar or one
    per frame."""
    coords = np.ascontiguousarray(coords, dtype=np.float32)
    if coords.ndim != 3 or coords.shape[2] != 3:
        raise ValueError("coords must be (nframes, natoms, 3)")
    F, N = coords.shape[:2]
    box = np.zeros((F, 3, 3), np.float32) if box is None else np.ascontiguousarray(np.broadcast_to(np.asarray(box, np.float32), (F, 3, 3)))
    time = _per_frame(time, F, np.float32, np.arange(F, dtype=np.float32))
    step = _per_frame(step, F, np.int64, np.arange(F, dtype=np.int64))
    prec = _per_frame(precision, F, np.float32, None)
    L = lib()
    xd = L.xdrfile_open(os.fsencode(str(path)), b"w")
    if not xd:
        raise OSError(f"xdrfile_open failed for {path}")
    try:
        for f in range(F):
            x = np.ascontiguousarray(coords[f])
            b = np.ascontiguousarray(box[f])
            rc = L.write_xtc(xd, N, int(step[f]), float(time[f]), b.ctypes.data, x.ctypes.data, float(prec[f]))
            if rc != 0:
                raise RuntimeError(f"reference write_xtc failed on frame {f} (code {rc})")
    finally:
        L.xdrfile_close(xd)


def ref_read_xtc(path, natoms):
    """Every frame through the reference's ``read_xtc``: ``(coords f32 [F, N, 3], box f32 [F, 3, 3], time f32 [F], step i32 [F],
    precision f32 [F])``."""
    L = lib()
    xd = L.xdrfile_open(os.fsencode(str(path)), b"r")
    if not xd:
        raise OSError(f"xdrfile_open failed for {path}")
    cs, bs, ts, ss, ps = [], [], [], [], []
    try:
        while True:
            x = np.zeros((natoms, 3), np.float32)
            b = np.zeros((3, 3), np.float32)
            st, t, p = ctypes.c_int(0), ctypes.c_float(0), ctypes.c_float(0)
            rc = L.read_xtc(xd, int(natoms), ctypes.byref(st), ctypes.byref(t), b.ctypes.data, x.ctypes.data, ctypes.byref(p))
            if rc == _EXDR_ENDOFFILE:
                break
            if rc != 0:
                raise RuntimeError(f"reference read_xtc failed on frame {len(cs)} (code {rc})")
            cs.append(x); bs.append(b); ts.append(t.value); ss.append(st.value); ps.append(p.value)
    finally:
        L.xdrfile_close(xd)
    return (np.stack(cs) if cs else np.zeros((0, natoms, 3), np.float32), np.stack(bs) if bs else np.zeros((0, 3, 3), np.float32),
            np.array(ts, np.float32), np.array(ss, np.int32), np.array(ps, np.float32))
