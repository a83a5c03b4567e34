"""tests/emu_dssp_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_dssp.so.

The secondary-structure kernels (moleculekit_amd/csrc/dssp_kernels.h) and their launch plan (dssp_pipeline.h) compiled for the HOST on
the SIMT emulation of tests/emu/emu_device.h, with -ffp-contract=off, so that the CPU-only tier checks their slots and codes against
the numpy restatement of the rules (tests/dssp_restatement.py).  Never imported by the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_dssp.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None
AVOID_FRAMES, AVOID_ATOMS, SMALL_CHUNKS = 1, 2, 4          # dssp_pipeline.h: DSSP_*


def build(force=False):
    srcs = [os.path.join(_EMU, "emu_dssp.cpp"), os.path.join(_EMU, "emu_device.h")] + \
           [os.path.join(_CSRC, h) for h in ("dssp_kernels.h", "dssp_pipeline.h", "dist_kernels.h", "pipeline.h", "kernels.h")]
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(
            ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
             "-Wno-unused-variable", "-Wno-unknown-pragmas", "-ffp-contract=off",
             os.path.join(_EMU, "emu_dssp.cpp"), "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        L.emu_dssp_last_error.restype = ctypes.c_char_p
        L.emu_dssp_last_kernel.restype = ctypes.c_char_p
        L.emu_dssp_last_workspace.restype = ctypes.c_longlong
        L.emu_dssp_last_chunks.restype = ctypes.c_longlong
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def dssp(coords, ca, nco, proline, chain, simplified=False, avoid=0):
    """coords float32 [N, 3, F] -> (slot acceptors int32 [F, R, 2], slot energies float32 [F, R, 2], codes uint8 [F, R])"""
    coords = np.ascontiguousarray(coords, np.float32)
    ca = np.ascontiguousarray(ca, np.uint32)
    nco = np.ascontiguousarray(nco, np.uint32).reshape(-1, 3)
    proline = np.ascontiguousarray(proline, np.int32)
    chain = np.ascontiguousarray(chain, np.int32)
    F, R = coords.shape[2], ca.shape[0]
    out = np.full((F, R), 255, np.uint8)
    sa = np.full((F, R, 2), -7, np.int32)
    se = np.full((F, R, 2), -7.0, np.float32)
    LL = ctypes.c_longlong
    st = lib().emu_dssp(_p(coords), LL(F), _p(ca), _p(nco), _p(proline), _p(chain), LL(R), ctypes.c_int(int(bool(simplified))), _p(out),
                        _p(sa), _p(se), ctypes.c_int(avoid))
    if st:
        raise ValueError(f"emulated dssp call failed ({st}): {lib().emu_dssp_last_error().decode()}")
    return sa, se, out


def last_kernel():
    return lib().emu_dssp_last_kernel().decode()


def last_workspace():
    return int(lib().emu_dssp_last_workspace())


def last_chunks():
    return int(lib().emu_dssp_last_chunks())
