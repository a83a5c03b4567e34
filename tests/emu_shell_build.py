"""tests/emu_shell_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_shell.so.

The shell-count kernels (moleculekit_amd/csrc/shell_kernels.h) and their launch plan (shell_pipeline.h) compiled for the HOST on the
SIMT emulation of tests/emu/emu_device.h, with -ffp-contract=off, so that the CPU-only tier checks their counts against the numpy
restatement of the reference's histogram (tests/shell_restatement.py).  Never imported by the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_shell.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None
AVOID_FRAMES, AVOID_ATOMS = 1, 2          # shell_pipeline.h: SHELL_AVOID_*


def build(force=False):
    srcs = [os.path.join(_EMU, "emu_shell.cpp"), os.path.join(_EMU, "emu_device.h")] + \
           [os.path.join(_CSRC, h) for h in ("shell_kernels.h", "shell_pipeline.h", "dist_kernels.h", "pipeline.h", "kernels.h")]
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(
            ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
             "-Wno-unused-variable", "-Wno-unknown-pragmas", "-ffp-contract=off",
             os.path.join(_EMU, "emu_shell.cpp"), "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        L.emu_shell_last_error.restype = ctypes.c_char_p
        L.emu_shell_last_kernel.restype = ctypes.c_char_p
        L.emu_shell_last_workspace.restype = ctypes.c_longlong
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def shell_counts(coords, box, sel1, sel2, chains, thresholds, symmetric=False, pbc=True, avoid=0):
    """coords float32 [N, 3, F], box float32 [3, F], thresholds float32 [n_edges] on d2 -> int32 [F, n1, n_edges - 1]"""
    coords = np.ascontiguousarray(coords, np.float32)
    box = np.ascontiguousarray(box, np.float32)
    sel1, sel2, chains = (np.ascontiguousarray(a, np.uint32) for a in (sel1, sel2, chains))
    thresholds = np.ascontiguousarray(thresholds, np.float32)
    F = coords.shape[2]
    out = np.full((F, len(sel1), max(len(thresholds) - 1, 0)), -7, np.int32)          # (the call clears it)
    LL = ctypes.c_longlong
    st = lib().emu_shell_counts(_p(coords), LL(F), _p(box), _p(sel1), LL(len(sel1)), _p(sel2), LL(len(sel2)), _p(chains),
                                ctypes.c_int(int(symmetric)), ctypes.c_int(int(pbc)), _p(thresholds), LL(len(thresholds)), _p(out),
                                ctypes.c_int(avoid))
    if st:
        raise ValueError(f"emulated shell-count call failed ({st}): {lib().emu_shell_last_error().decode()}")
    return out


def last_kernel():
    return lib().emu_shell_last_kernel().decode()


def last_workspace():
    return int(lib().emu_shell_last_workspace())
