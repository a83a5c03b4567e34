"""tests/emu_hbonds_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_hbonds.so.

The hydrogen-bond kernels (moleculekit_amd/csrc/hbond_kernels.h) and their launch plan (hbond_pipeline.h) compiled for the HOST on the
SIMT emulation of tests/emu/emu_device.h, with -ffp-contract=off, so that the CPU-only tier checks their lists against the numpy
restatement of the reference's loop (tests/hbonds_restatement.py).  Never imported by the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_hbonds.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None
AVOID_FRAMES, AVOID_PAIRS = 1, 2          # hbond_pipeline.h: HB_AVOID_*
BUDGET = 256 << 20


def build(force=False):
    srcs = [os.path.join(_EMU, "emu_hbonds.cpp"), os.path.join(_EMU, "emu_device.h")] + \
           [os.path.join(_CSRC, h) for h in ("hbond_kernels.h", "hbond_pipeline.h", "ring_kernels.h", "dist_kernels.h", "pipeline.h", "kernels.h")]
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(
            ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
             "-Wno-unused-variable", "-Wno-unknown-pragmas", "-ffp-contract=off",
             os.path.join(_EMU, "emu_hbonds.cpp"), "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        L.emu_hbonds_last_error.restype = ctypes.c_char_p
        L.emu_hbonds_last_kernel.restype = ctypes.c_char_p
        L.emu_hbonds_last_workspace.restype = ctypes.c_longlong
        L.emu_hbonds_last_chunks.restype = ctypes.c_longlong
        L.emu_hbonds_triples.restype = ctypes.c_void_p
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def hbonds(donors, acceptors, coords, box, sel1, sel2, dist_threshold=2.5, angle_threshold=120, intra=False, ignore_hs=False, avoid=0,
           chunk_frames=0, budget=BUDGET, device_sink=False, names=None):
    """the arguments of the reference's `calculate` (box may be None) -> (frame_offsets int64 [F + 1], triples int32 [n, 3])"""
    coords = np.ascontiguousarray(coords, np.float32)
    N, _, F = coords.shape
    box = None if box is None else np.ascontiguousarray(box, np.float32)
    donors = np.ascontiguousarray(donors, np.uint32)
    donors = donors.reshape(len(donors), 1 if ignore_hs else 2)
    acceptors, sel1 = (np.ascontiguousarray(a, np.uint32) for a in (acceptors, sel1))
    sel2 = None if sel2 is None else np.ascontiguousarray(sel2, np.uint32)
    names = None if names is None else np.ascontiguousarray(names, np.uint32)
    offs = np.full(F + 1, -7, np.int64)
    LL, I = ctypes.c_longlong, ctypes.c_int
    st = lib().emu_hbonds(_p(coords), LL(N), LL(F), _p(box), _p(donors), LL(len(donors)), _p(acceptors), LL(len(acceptors)), _p(sel1), _p(sel2),
                          _p(names), ctypes.c_float(dist_threshold), ctypes.c_float(angle_threshold), I(int(intra)), I(int(ignore_hs)), LL(budget),
                          LL(chunk_frames), I(avoid), I(int(device_sink)), _p(offs))
    if st:
        raise ValueError(f"emulated hydrogen-bond call failed ({st}): {lib().emu_hbonds_last_error().decode()}")
    n = int(offs[-1])
    if n == 0:
        return offs, np.zeros((0, 3), np.int32)
    return offs, np.frombuffer((ctypes.c_int32 * (3 * n)).from_address(lib().emu_hbonds_triples()), np.int32).reshape(n, 3).copy()


def last_kernel():
    return lib().emu_hbonds_last_kernel().decode()


def last_workspace():
    return int(lib().emu_hbonds_last_workspace())


def last_chunks():
    return int(lib().emu_hbonds_last_chunks())
