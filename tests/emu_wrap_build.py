"""tests/emu_wrap_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_wrap.so.

The periodic-wrap kernels (moleculekit_amd/csrc/wrap_kernels.h) and their launch plan (wrap_pipeline.h) compiled for the HOST on the
SIMT emulation of tests/emu/emu_device.h, with -ffp-contract=off, so that the CPU-only tier checks them bit for bit against the numpy
restatement of the reference (tests/wrap_restatement.py).  Never imported by the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_wrap.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None
AVOID_LANES, AVOID_WAVES = 1, 2           # wrap_pipeline.h: WRAP_AVOID_*
LL = ctypes.c_longlong


def build(force=False):
    srcs = [os.path.join(_EMU, "emu_wrap.cpp"), os.path.join(_EMU, "emu_device.h")] + \
           [os.path.join(_CSRC, h) for h in ("wrap_kernels.h", "wrap_pipeline.h", "pipeline.h", "kernels.h")]
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(
            ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
             "-Wno-unused-variable", "-Wno-unknown-pragmas", "-ffp-contract=off",
             os.path.join(_EMU, "emu_wrap.cpp"), "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        L.emu_wrap_last_error.restype = ctypes.c_char_p
        L.emu_wrap_last_kernel.restype = ctypes.c_char_p
        L.emu_wrap_check_starts.restype = ctypes.c_char_p
        L.emu_wrap_small_max.restype = ctypes.c_longlong
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def small_max(avoid=0):
    """the largest group the lane-per-group kernel takes under ``avoid``"""
    return int(lib().emu_wrap_small_max(ctypes.c_int(avoid)))


def chunk():
    """atoms per LDS chunk of the wave kernels"""
    return int(lib().emu_wrap_chunk())


def check_starts(starts, n_atoms):
    """the text of wrap_check_starts, or None"""
    s = np.ascontiguousarray(starts, np.uint32)
    r = lib().emu_wrap_check_starts(_p(s), LL(s.size - 1), LL(n_atoms))
    return r.decode() if r else None


def wrap_box(xyz, box, starts, centersel=None, center=None, avoid=0, inplace=False):
    """xyz float32 [F, N, 3], box float32 [3, F], starts [G + 1] -> the wrapped float32 [F, N, 3].  ``inplace``: ``xyz`` itself (which
    must then be a contiguous float32 array) is wrapped and returned; otherwise it is left as it is."""
    if inplace:
        assert isinstance(xyz, np.ndarray) and xyz.dtype == np.float32 and xyz.flags["C_CONTIGUOUS"]
        out = xyz
    else:
        xyz = np.ascontiguousarray(xyz, np.float32)
        out = np.full(xyz.shape, -7.0, np.float32)
    box = np.ascontiguousarray(box, np.float32)
    starts = np.ascontiguousarray(starts, np.uint32)
    sel = None if centersel is None else np.ascontiguousarray(centersel, np.uint32)
    cen = None if center is None else np.ascontiguousarray(center, np.float32)
    F, N = xyz.shape[0], xyz.shape[1]
    st = lib().emu_wrap_box(_p(xyz), LL(N), LL(F), _p(box), _p(starts), LL(starts.size - 1), _p(sel), LL(0 if sel is None else sel.size),
                            _p(cen), _p(out), ctypes.c_int(avoid))
    if st:
        raise ValueError(f"emulated wrap call failed ({st}): {lib().emu_wrap_last_error().decode()}")
    return out


def last_kernel():
    return lib().emu_wrap_last_kernel().decode()
