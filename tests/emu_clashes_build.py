"""tests/emu_clashes_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_clashes.so.

The steric-clash kernels (moleculekit_amd/csrc/clash_kernels.h), the bond guesser's cell-list kernels under them and their launch plan
(clash_pipeline.h) compiled for the HOST on the SIMT emulation of tests/emu/emu_device.h, with -ffp-contract=off, so that the CPU-only
tier checks their lists against the compiled reference's (tests/golden/clash_cases.npz).  Never imported by the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_clashes.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None
AVOID_THREAD, AVOID_WAVE = 1, 2           # clash_pipeline.h: CLASH_AVOID_*
THREAD_KERNEL, WAVE_KERNEL = "mkamd::k_clash_pairs_thread", "mkamd::k_clash_pairs_wave"


def build(force=False):
    srcs = [os.path.join(_EMU, "emu_clashes.cpp"), os.path.join(_EMU, "emu_device.h")] + \
           [os.path.join(_CSRC, h) for h in ("clash_kernels.h", "clash_pipeline.h", "bond_kernels.h", "bond_pipeline.h", "pipeline.h", "kernels.h")]
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(
            ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
             "-Wno-unused-variable", "-Wno-unknown-pragmas", "-ffp-contract=off",
             os.path.join(_EMU, "emu_clashes.cpp"), "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        L.emu_clashes_last_error.restype = ctypes.c_char_p
        L.emu_clashes_last_kernel.restype = ctypes.c_char_p
        for f in (L.emu_clashes_pairs, L.emu_clashes_dist, L.emu_clashes_over):
            f.restype = ctypes.c_void_p
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def find_clashes(coords, radii, mask1, mask2, ex_start, ex_partner, overlap, cutoff, max_boxes=4e6, avoid=0):
    """float32 [N, 3], float32 [N], masks [N] (``mask2`` None: self mode), the exclusion CSR or None twice ->
    (pairs int64 [n, 2], distances float32 [n], overlaps float32 [n], info) in the PAIR KERNELS' order; ValueError with the library's
    message where the call ends with a status"""
    coords = np.ascontiguousarray(coords, np.float32)
    radii = np.ascontiguousarray(radii, np.float32)
    s1 = np.ascontiguousarray(mask1, np.uint32)
    s2 = None if mask2 is None else np.ascontiguousarray(mask2, np.uint32)
    es = None if ex_start is None else np.ascontiguousarray(ex_start, np.uint32)
    ep = None if ex_partner is None else np.ascontiguousarray(ex_partner, np.uint32)
    if ep is not None and ep.size == 0:
        ep = np.zeros(1, np.uint32)       # (a pointer that is not NULL)
    npairs = ctypes.c_longlong(-1)
    info = np.zeros(8, np.float64)
    D = ctypes.c_double
    st = lib().emu_find_clashes(_p(coords), _p(radii), _p(s1), _p(s2), ctypes.c_longlong(len(coords)), ctypes.c_int(int(s2 is None)), _p(es), _p(ep),
                                D(float(overlap)), D(float(cutoff)), D(float(max_boxes)), ctypes.c_int(avoid), ctypes.byref(npairs), _p(info))
    if st:
        raise ValueError(f"emulated clash call failed ({st}): {lib().emu_clashes_last_error().decode()}")
    k = int(npairs.value)
    if k == 0:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.float32), np.zeros(0, np.float32), info
    pairs = np.frombuffer((ctypes.c_int32 * (2 * k)).from_address(lib().emu_clashes_pairs()), np.int32).reshape(k, 2).astype(np.int64)
    dist = np.frombuffer((ctypes.c_float * k).from_address(lib().emu_clashes_dist()), np.float32).copy()
    over = np.frombuffer((ctypes.c_float * k).from_address(lib().emu_clashes_over()), np.float32).copy()
    return pairs, dist, over, info


def clash_grid(min_c, max_c, cutoff, max_boxes=4e6):
    """the library's box side -> (nx, ny, nz, side)"""
    mn, mx = np.ascontiguousarray(min_c, np.float32), np.ascontiguousarray(max_c, np.float32)
    info = np.zeros(4, np.float64)
    D = ctypes.c_double
    st = lib().emu_clash_grid(_p(mn), _p(mx), D(float(cutoff)), D(float(max_boxes)), _p(info))
    if st:
        raise ValueError(lib().emu_clashes_last_error().decode())
    return int(info[0]), int(info[1]), int(info[2]), float(info[3])


def last_kernel():
    return lib().emu_clashes_last_kernel().decode()
