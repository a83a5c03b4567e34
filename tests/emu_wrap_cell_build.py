"""tests/emu_wrap_cell_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_wrap_cell.so.

The triclinic periodic-wrap kernels (moleculekit_amd/csrc/wrap_cell_kernels.h) and their launch plan (wrap_cell_pipeline.h) compiled for
the HOST on the SIMT emulation of tests/emu/emu_device.h, with -ffp-contract=off, so that the CPU-only tier checks them bit for bit
against the numpy restatement of the reference (tests/wrap_cell_restatement.py).  Never imported by the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_wrap_cell.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None
AVOID_LANES, AVOID_WAVES = 1, 2           # wrap_pipeline.h: WRAP_AVOID_*
MODES = {"rectangular": 0, "compact": 1, "triclinic": 2}
ST_CAP, ST_FRAME, ST_VECTORS = 0, 1, 2    # wrap_cell_kernels.h: WRAP_CELL_ST_*
LL = ctypes.c_longlong


def build(force=False):
    srcs = [os.path.join(_EMU, "emu_wrap_cell.cpp"), os.path.join(_EMU, "emu_device.h")] + \
           [os.path.join(_CSRC, h) for h in ("wrap_cell_kernels.h", "wrap_cell_pipeline.h", "wrap_kernels.h", "wrap_pipeline.h", "pipeline.h",
                                             "kernels.h")]
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(
            ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
             "-Wno-unused-variable", "-Wno-unknown-pragmas", "-ffp-contract=off",
             os.path.join(_EMU, "emu_wrap_cell.cpp"), "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        for name in ("emu_wrap_cell_last_error", "emu_wrap_cell_last_kernel", "emu_wrap_cell_check_boxvectors", "emu_wrap_cell_status_error"):
            getattr(L, name).restype = ctypes.c_char_p
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def max_steps():
    """WRAP_CELL_MAX_STEPS"""
    return int(lib().emu_wrap_cell_max_steps())


def check_boxvectors(bv):
    """the text of wrap_cell_check_boxvectors ([3, 3, F] float64), or None"""
    b = np.ascontiguousarray(bv, np.float64)
    r = lib().emu_wrap_cell_check_boxvectors(_p(b), LL(b.shape[2]))
    return r.decode() if r else None


def status_error(status):
    """the text of wrap_cell_status_error, or None"""
    s = np.ascontiguousarray(status, np.int32)
    r = lib().emu_wrap_cell_status_error(_p(s))
    return r.decode() if r else None


def wrap_cell(xyz, boxvectors, starts, mode, centersel=None, center=None, avoid=0, inplace=False):
    """xyz float32 [F, N, 3], boxvectors float64 [3, 3, F], starts [G + 1], mode a name of MODES -> (the wrapped float32 [F, N, 3], the
    status words int32 [3]).  The launch plan alone: nothing checks the box vectors first.  ``inplace``: ``xyz`` itself (which must then
    be a contiguous float32 array) is wrapped and returned; otherwise it is left as it is."""
    if inplace:
        assert isinstance(xyz, np.ndarray) and xyz.dtype == np.float32 and xyz.flags["C_CONTIGUOUS"]
        out = xyz
    else:
        xyz = np.ascontiguousarray(xyz, np.float32)
        out = np.full(xyz.shape, -7.0, np.float32)
    bv = np.ascontiguousarray(boxvectors, np.float64)
    starts = np.ascontiguousarray(starts, np.uint32)
    sel = None if centersel is None else np.ascontiguousarray(centersel, np.uint32)
    cen = None if center is None else np.ascontiguousarray(center, np.float32)
    status = np.full(3, -1, np.int32)
    F, N = xyz.shape[0], xyz.shape[1]
    assert bv.shape == (3, 3, F)
    st = lib().emu_wrap_cell(_p(xyz), LL(N), LL(F), _p(bv), _p(starts), LL(starts.size - 1), _p(sel), LL(0 if sel is None else sel.size),
                             _p(cen), ctypes.c_int(MODES[mode] if isinstance(mode, str) else mode), _p(out), _p(status), ctypes.c_int(avoid))
    if st:
        raise ValueError(f"emulated wrap call failed ({st}): {lib().emu_wrap_cell_last_error().decode()}")
    return out, status


def last_kernel():
    return lib().emu_wrap_cell_last_kernel().decode()
