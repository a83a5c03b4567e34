"""tests/emu_sasa_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_sasa.so.

The surface-area kernels (moleculekit_amd/csrc/sasa_kernels.h) and their launch plan (sasa_pipeline.h) compiled for the HOST on the
SIMT emulation of tests/emu/emu_device.h, with -ffp-contract=off, so that the CPU-only tier checks them bit for bit against the
float32 restatement (tests/sasa_restatement.py).  Never imported by the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_sasa.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_EMU, "emu_sasa.cpp"), os.path.join(_EMU, "emu_device.h"), os.path.join(_CSRC, "sasa_kernels.h"),
            os.path.join(_CSRC, "sasa_pipeline.h"), os.path.join(_CSRC, "pipeline.h"), os.path.join(_CSRC, "kernels.h")]
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(
            ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
             "-Wno-unused-variable", "-Wno-unknown-pragmas", "-ffp-contract=off",
             os.path.join(_EMU, "emu_sasa.cpp"), "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        L.emu_sasa_last_error.restype = ctypes.c_char_p
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def sasa(xyz, radii, n_points=960, mapping=None, sel=None, out=None, coord_div=1.0):
    """xyz float32 [F, N, 3], radii float32 [N] -> out float32 [F, n_out] (areas ADDED to `out`; default zeros)"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    radii = np.ascontiguousarray(radii, np.float32)
    F, N = xyz.shape[:2]
    mapping = np.arange(N, dtype=np.int32) if mapping is None else np.ascontiguousarray(mapping, np.int32)
    mask = np.ones(N, np.int32) if sel is None else np.ascontiguousarray(np.asarray(sel).astype(bool), np.int32)
    if out is None:
        out = np.zeros((F, int(mapping.max()) + 1 if N else 0), np.float32)
    assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape[0] == F
    st = lib().emu_sasa(_p(xyz), ctypes.c_longlong(N), ctypes.c_longlong(F), _p(radii), ctypes.c_int(int(n_points)), _p(mapping), _p(mask),
                        ctypes.c_float(coord_div), _p(out), ctypes.c_longlong(out.shape[1]))
    if st:
        raise ValueError(f"emulated surface-area call failed ({st}): {lib().emu_sasa_last_error().decode()}")
    return out


def sphere_points(n):
    out = np.zeros((n, 3), np.float32)
    lib().emu_sasa_sphere_points(ctypes.c_int(n), _p(out))
    return out


def max_neighbours():
    return int(lib().emu_sasa_max_neighbours())
