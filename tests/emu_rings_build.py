"""tests/emu_rings_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_rings.so.

The ring-interaction kernels (moleculekit_amd/csrc/ring_kernels.h) and their launch plan (ring_pipeline.h) compiled for the HOST on the
SIMT emulation of tests/emu/emu_device.h, with -ffp-contract=off, so that the CPU-only tier checks their lists against the numpy
restatement of the reference's loops (tests/rings_restatement.py).  Never imported by the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_rings.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None
AVOID_FRAMES, AVOID_PAIRS = 1, 2          # ring_pipeline.h: RING_AVOID_*
PIPI, CATIONPI, SIGMAHOLE = 0, 1, 2
BUDGET = 256 << 20


def build(force=False):
    srcs = [os.path.join(_EMU, "emu_rings.cpp"), os.path.join(_EMU, "emu_device.h")] + \
           [os.path.join(_CSRC, h) for h in ("ring_kernels.h", "ring_pipeline.h", "dist_kernels.h", "pipeline.h", "kernels.h")]
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(
            ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
             "-Wno-unused-variable", "-Wno-unknown-pragmas", "-ffp-contract=off",
             os.path.join(_EMU, "emu_rings.cpp"), "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        L.emu_rings_last_error.restype = ctypes.c_char_p
        L.emu_rings_last_kernel.restype = ctypes.c_char_p
        L.emu_rings_last_workspace.restype = ctypes.c_longlong
        L.emu_rings_last_chunks.restype = ctypes.c_longlong
        L.emu_rings_pairs.restype = ctypes.c_void_p
        L.emu_rings_distang.restype = ctypes.c_void_p
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def rings(kind, coords, box, ring_atoms, starts1, second, thr, avoid=0, chunk_frames=0, budget=BUDGET, device_sink=False):
    """coords float32 [N, 3, F], box float32 [3, F] or None; `second`: starts2 (pi-pi), cations [n] or halides [n, 2]; thr: four
    floats (ring_pipeline.h: RingArgs.thr) -> (frame_offsets int64 [F + 1], pairs uint32 [n, 2], distang float32 [n, 2])"""
    coords = np.ascontiguousarray(coords, np.float32)
    F = coords.shape[2]
    box = None if box is None else np.ascontiguousarray(box, np.float32)
    ring_atoms, starts1, second = (np.ascontiguousarray(a, np.uint32) for a in (ring_atoms, starts1, second))
    n2 = len(second) - 1 if kind == PIPI else len(second)
    thr4 = np.zeros(4, np.float32)
    thr4[:len(thr)] = thr
    offs = np.full(F + 1, -7, np.int64)
    LL = ctypes.c_longlong
    st = lib().emu_rings(ctypes.c_int(kind), _p(coords), LL(F), _p(box), _p(ring_atoms), LL(len(ring_atoms)), _p(starts1), LL(len(starts1) - 1),
                         _p(second) if kind == PIPI else None, None if kind == PIPI else _p(second), LL(n2), _p(thr4), LL(budget),
                         LL(chunk_frames), ctypes.c_int(avoid), ctypes.c_int(int(device_sink)), _p(offs))
    if st:
        raise ValueError(f"emulated ring-interaction call failed ({st}): {lib().emu_rings_last_error().decode()}")
    n = int(offs[-1])
    if n == 0:
        return offs, np.zeros((0, 2), np.uint32), np.zeros((0, 2), np.float32)
    pairs = np.frombuffer((ctypes.c_uint32 * (2 * n)).from_address(lib().emu_rings_pairs()), np.uint32).reshape(n, 2).copy()
    da = np.frombuffer((ctypes.c_float * (2 * n)).from_address(lib().emu_rings_distang()), np.float32).reshape(n, 2).copy()
    return offs, pairs, da


def last_kernel():
    return lib().emu_rings_last_kernel().decode()


def last_workspace():
    return int(lib().emu_rings_last_workspace())


def last_chunks():
    return int(lib().emu_rings_last_chunks())
