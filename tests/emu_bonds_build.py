"""tests/emu_bonds_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_bonds.so.

The bond-guesser kernels (moleculekit_amd/csrc/bond_kernels.h) and their launch plan (bond_pipeline.h) compiled for the HOST on the SIMT
emulation of tests/emu/emu_device.h, with -ffp-contract=off, so that the CPU-only tier checks their lists against the numpy
restatement of the reference's search (tests/bonds_restatement.py).  Never imported by the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_bonds.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None
AVOID_THREAD, AVOID_WAVE = 1, 2           # bond_pipeline.h: BOND_AVOID_*
THREAD_KERNEL, WAVE_KERNEL = "mkamd::k_bond_pairs_thread", "mkamd::k_bond_pairs_wave"


class CrowdedBox(ValueError):
    """the emulated call ended with a status"""


def build(force=False):
    srcs = [os.path.join(_EMU, "emu_bonds.cpp"), os.path.join(_EMU, "emu_device.h")] + \
           [os.path.join(_CSRC, h) for h in ("bond_kernels.h", "bond_pipeline.h", "pipeline.h", "kernels.h")]
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(
            ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
             "-Wno-unused-variable", "-Wno-unknown-pragmas", "-ffp-contract=off",
             os.path.join(_EMU, "emu_bonds.cpp"), "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        L.emu_bonds_last_error.restype = ctypes.c_char_p
        L.emu_bonds_last_kernel.restype = ctypes.c_char_p
        L.emu_bonds_last_workspace.restype = ctypes.c_longlong
        L.emu_bonds_pairs.restype = ctypes.c_void_p
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def guess_bonds(coords, grid_cutoff, is_hydrogen, radii, max_boxes=4e6, cutoff_incr=1.26, avoid=0):
    """the arguments of the reference's bond_grid_search -> (pairs uint32 [n, 2], (nx, ny, nz, pairdist), largest occupancy);
    ValueError with the library's message where the call ends with a status"""
    coords = np.ascontiguousarray(coords, np.float32)
    radii = np.ascontiguousarray(radii, np.float32)
    is_h = np.ascontiguousarray(is_hydrogen, np.uint32)
    n = len(coords)
    npairs = ctypes.c_longlong(-1)
    info = np.zeros(5, np.float64)
    D = ctypes.c_double
    st = lib().emu_guess_bonds(_p(coords), _p(radii), _p(is_h), ctypes.c_longlong(n), D(float(grid_cutoff)), D(float(max_boxes)), D(float(cutoff_incr)),
                               ctypes.c_int(avoid), ctypes.byref(npairs), _p(info))
    if st:
        raise CrowdedBox(f"emulated bond call failed ({st}): {lib().emu_bonds_last_error().decode()}")
    k = int(npairs.value)
    grid = (int(info[0]), int(info[1]), int(info[2]), float(info[3]))
    if k == 0:
        return np.zeros((0, 2), np.uint32), grid, int(info[4])
    pairs = np.frombuffer((ctypes.c_int32 * (2 * k)).from_address(lib().emu_bonds_pairs()), np.int32).reshape(k, 2).astype(np.uint32)
    return pairs, grid, int(info[4])


def bond_grid(min_c, max_c, grid_cutoff, max_boxes=4e6, cutoff_incr=1.26):
    """the library's escalation loop -> (nx, ny, nz, pairdist)"""
    mn, mx = np.ascontiguousarray(min_c, np.float32), np.ascontiguousarray(max_c, np.float32)
    info = np.zeros(4, np.float64)
    D = ctypes.c_double
    st = lib().emu_bond_grid(_p(mn), _p(mx), D(float(grid_cutoff)), D(float(max_boxes)), D(float(cutoff_incr)), _p(info))
    if st:
        raise ValueError(lib().emu_bonds_last_error().decode())
    return int(info[0]), int(info[1]), int(info[2]), float(info[3])


def last_kernel():
    return lib().emu_bonds_last_kernel().decode()


def last_workspace():
    return int(lib().emu_bonds_last_workspace())
