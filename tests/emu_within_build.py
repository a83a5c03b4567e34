"""tests/emu_within_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_within.so.

The proximity-selection kernels (moleculekit_amd/csrc/within_kernels.h), the bond guesser's cell-list kernels under them and their
launch plan (within_pipeline.h) compiled for the HOST on the SIMT emulation of tests/emu/emu_device.h, with -ffp-contract=off, so that
the CPU-only tier checks their bytes against the compiled reference's (tests/golden/within_cases.npz).  Never imported by the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_within.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None
AVOID_PAIRS, AVOID_CELLS = 1, 2           # within_pipeline.h: WITHIN_AVOID_*
PAIRS_KERNEL, CELLS_KERNEL = "mkamd::k_within_pairs", "mkamd::k_within_cells"


def build(force=False):
    srcs = [os.path.join(_EMU, "emu_within.cpp"), os.path.join(_EMU, "emu_device.h")] + \
           [os.path.join(_CSRC, h) for h in ("within_kernels.h", "within_pipeline.h", "clash_kernels.h", "clash_pipeline.h", "bond_kernels.h",
                                             "bond_pipeline.h", "pipeline.h", "kernels.h")]
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(
            ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
             "-Wno-unused-variable", "-Wno-unknown-pragmas", "-ffp-contract=off",
             os.path.join(_EMU, "emu_within.cpp"), "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        for f in (L.emu_within_last_error, L.emu_within_last_kernel, L.emu_within_left):
            f.restype = ctypes.c_char_p
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def within(coords, sel1, sel2, cutoff, gate=None, avoid=0, no_cull=False):
    """float32 [F, N, 3], uint32 index arrays, the cutoff (rounded to float32 here as a C float argument is), gate float32 [F, 2, 3] or
    None -> (bool [F, n1], info); ValueError with the library's message where the call ends with a status.  The output array goes in
    poisoned, so an element the kernels do not write fails the comparison."""
    coords = np.ascontiguousarray(coords, np.float32)
    F, N = coords.shape[0], coords.shape[1]
    s1, s2 = np.ascontiguousarray(sel1, np.uint32), np.ascontiguousarray(sel2, np.uint32)
    g = None if gate is None else np.ascontiguousarray(gate, np.float32)
    assert g is None or g.shape == (F, 2, 3)
    out = np.full((F, len(s1)), 0xCD, np.uint8)
    info = np.zeros(8, np.float64)
    L = ctypes.c_longlong
    st = lib().emu_within(_p(coords), L(N), L(F), _p(s1) if len(s1) else None, L(len(s1)), _p(s2) if len(s2) else None, L(len(s2)),
                          ctypes.c_float(cutoff), _p(g), ctypes.c_int(avoid), ctypes.c_int(int(no_cull)), _p(out), _p(info))
    if st:
        raise ValueError(f"emulated within call failed ({st}): {lib().emu_within_last_error().decode()}")
    assert ((out == 0) | (out == 1)).all(), "an output byte the kernels did not write"
    return out.astype(bool), info


def last_kernel():
    return lib().emu_within_last_kernel().decode()


def left():
    return lib().emu_within_left().decode()
