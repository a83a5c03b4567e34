"""tests/emu_dihedral_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_dihedral.so.

The dihedral kernels (moleculekit_amd/csrc/dihedral_kernels.h) and their launch plan (dihedral_pipeline.h) compiled for the HOST on
the SIMT emulation of tests/emu/emu_device.h, with -ffp-contract=off, so that the CPU-only tier checks their terms and angles against
the numpy restatement of the reference (tests/dihedral_restatement.py).  Never imported by the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_dihedral.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None
AVOID_FRAMES, AVOID_ATOMS = 1, 2          # dihedral_pipeline.h: DIH_AVOID_*
MODES = {"terms": 0, "radians": 1, "degrees": 2, "sincos": 3}


def build(force=False):
    srcs = [os.path.join(_EMU, "emu_dihedral.cpp"), os.path.join(_EMU, "emu_device.h")] + \
           [os.path.join(_CSRC, h) for h in ("dihedral_kernels.h", "dihedral_pipeline.h", "dist_kernels.h", "pipeline.h", "kernels.h")]
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(
            ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
             "-Wno-unused-variable", "-Wno-unknown-pragmas", "-ffp-contract=off",
             os.path.join(_EMU, "emu_dihedral.cpp"), "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        L.emu_dihedral_last_error.restype = ctypes.c_char_p
        L.emu_dihedral_last_kernel.restype = ctypes.c_char_p
        L.emu_dihedral_last_workspace.restype = ctypes.c_longlong
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def dihedrals(coords, quads, box=None, out="sincos", avoid=0):
    """coords float32 [N, 3, F], quads [D, 4], box None or float32 [3, F] -> float32 [F, D, 2] / [F, D] / [F, 2 D] by mode"""
    coords = np.ascontiguousarray(coords, np.float32)
    quads = np.ascontiguousarray(quads, np.uint32).reshape(-1, 4)
    if box is not None:
        box = np.ascontiguousarray(box, np.float32)
    F, D = coords.shape[2], quads.shape[0]
    mode = MODES[out] if isinstance(out, str) else int(out)
    shape = {0: (F, D, 2), 1: (F, D), 2: (F, D), 3: (F, 2 * D)}.get(mode, (F, D))
    res = np.full(shape, -7.0, np.float32)
    LL = ctypes.c_longlong
    st = lib().emu_dihedrals(_p(coords), LL(F), _p(box), _p(quads), LL(D), ctypes.c_int(mode), _p(res), ctypes.c_int(avoid))
    if st:
        raise ValueError(f"emulated dihedral call failed ({st}): {lib().emu_dihedral_last_error().decode()}")
    return res


def last_kernel():
    return lib().emu_dihedral_last_kernel().decode()


def last_workspace():
    return int(lib().emu_dihedral_last_workspace())
