"""tests/emu_dcd_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_dcd.so, and the build of the
stand-alone sanitized driver tests/emu/dcd_damage_main.

The device DCD kernels (moleculekit_amd/csrc/dcd_kernels.h) and their launch plans compiled for the HOST on the SIMT emulation of
tests/emu/emu_device.h, so that the CPU-only tier checks their output against the reference's.  Never imported by the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_dcd.so")
_MAIN = os.path.join(_EMU, "dcd_damage_main")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None
_SRCS = [os.path.join(_EMU, "emu_dcd.cpp"), os.path.join(_EMU, "emu_device.h"), os.path.join(_CSRC, "dcd_kernels.h"),
         os.path.join(_CSRC, "dcd_reader.h"), os.path.join(_CSRC, "xtc_reader.h")]
_WARN = ["-Wall", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-unknown-pragmas"]
POISON = 0xCD


def _stale(target, srcs):
    return (not os.path.exists(target)) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in srcs)


def build(force=False):
    if force or _stale(_LIB, _SRCS):
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-pthread"] + _WARN + ["-ffp-contract=off", _SRCS[0], "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def build_main(force=False):
    """The stand-alone damaged-file driver (its own main), with AddressSanitizer and UBSan; run as a child process, nothing is preloaded."""
    src = os.path.join(_EMU, "dcd_damage_main.cpp")
    if force or _stale(_MAIN, _SRCS[3:] + [src]):
        tmp = "%s.%d.tmp" % (_MAIN, os.getpid())
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-fno-omit-frame-pointer"] + _WARN + [src, "-o", tmp])
        os.replace(tmp, _MAIN)
    return _MAIN


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        vp, ll = ctypes.c_void_p, ctypes.c_longlong
        L.emu_dcd_decode.argtypes = [vp, ctypes.c_uint64, vp, ll, vp, vp, ll, vp, ll, ctypes.c_float, vp, vp]
        L.emu_dcd_encode_bound.restype = ctypes.c_uint64
        L.emu_dcd_encode_bound.argtypes = [ll, ll, ctypes.c_int]
        L.emu_dcd_encode.argtypes = [vp, vp, ll, ll, vp, ctypes.c_uint64]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _aligned_bytes(n, fill=POISON):
    """uint8 [n] at a 4-byte aligned address."""
    return np.full(n // 4 + 1, fill * 0x01010101, np.uint32).view(np.uint8)[:n]


def decode(raw, desc, sel, src, natoms, frame0=None, scale=1.0, n_bytes=None):
    """raw: the byte range (uint8), desc uint8 [n, 32], sel / src int32 [n_sel] -> (xyz float32 [n, n_sel, 3], poisoned before the call;
    status int32 [n])."""
    n, nsel = len(desc), len(sel)
    buf = _aligned_bytes(len(raw))
    buf[:] = raw
    xyz = np.full((n, nsel, 3), POISON * 0x01010101, np.uint32).view(np.float32)
    status = np.full(n, -7, np.int32)
    d = np.ascontiguousarray(desc)
    st = lib().emu_dcd_decode(_p(buf), len(raw) if n_bytes is None else n_bytes, _p(d), n, _p(np.ascontiguousarray(sel, np.int32)),
                              _p(np.ascontiguousarray(src, np.int32)), nsel, _p(frame0), natoms, ctypes.c_float(scale), _p(xyz), _p(status))
    if st:
        raise ValueError(f"emulated decode call failed ({st})")
    return xyz, status


def encode(xyz, cell=None):
    """xyz float32 [F, N, 3], cell float64 [F, 6] or None -> the image (uint8, exactly the promised size, poisoned before the call)."""
    x = np.ascontiguousarray(xyz, np.float32)
    F, N = x.shape[:2]
    bound = int(lib().emu_dcd_encode_bound(F, N, int(cell is not None)))
    image = _aligned_bytes(bound)
    c = None if cell is None else np.ascontiguousarray(cell, np.float64)
    st = lib().emu_dcd_encode(_p(x), _p(c), F, N, _p(image), bound)
    if st:
        raise ValueError(f"emulated encode call failed ({st})")
    return image
