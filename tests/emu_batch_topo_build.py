"""tests/emu_batch_topo_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_batch.so, the host
emulation of the product's kernels (tests/emu_build.py) with the entry points of the BATCH topology handle (tests/emu/emu_batch_topo.cpp)."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_batch.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None


def lib():
    global _lib
    if _lib is None:
        srcs = [os.path.join(_EMU, f) for f in ("emu_batch_topo.cpp", "emu_capi.cpp", "emu_device.h")] + \
               [os.path.join(_CSRC, f) for f in ("kernels.h", "pipeline.h", "dist_kernels.h", "dist_pipeline.h", "xtc_gpu.h", "host_pack.h")]
        if not os.path.exists(_LIB) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs):
            tmp = "%s.%d.tmp" % (_LIB, os.getpid())
            subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
                                   "-Wno-unknown-pragmas", "-ffp-contract=off", srcs[0], "-o", tmp, "-ldl"])
            os.replace(tmp, _LIB)
        _lib = ctypes.CDLL(_LIB)
        _lib.emu_last_error.restype = ctypes.c_char_p
        _lib.emu_trace_text.restype = ctypes.c_char_p
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def voxelize_range(coords, batch_offsets, sigmas, origins, nvox, lo=0, hi=None, call_offsets=None, box=None, max_images=1, tile_k=0, affine=None,
                   prepass_mode=0, tile_team=0, tile_items=0, direct=0, exact_redo=0):
    """items [lo, hi) of the batch through a handle built over ALL of `sigmas` -> (features [hi - lo, V, C], device error flag, wide
    atoms in the handle).  `call_offsets`: what the call passes instead of the handle's own (rebased) offsets."""
    batch_offsets = np.ascontiguousarray(batch_offsets, np.int64)
    n_items = len(batch_offsets) - 1
    hi = n_items if hi is None else hi
    a0, a1 = int(batch_offsets[lo]), int(batch_offsets[hi])
    sig64 = sigmas.dtype == np.float64
    sigmas = np.ascontiguousarray(sigmas, np.float64 if sig64 else np.float32)
    xyz = np.ascontiguousarray(np.asarray(coords, np.float32).reshape(-1, 3)[a0:a1])
    offs = np.ascontiguousarray(batch_offsets[lo:hi + 1] - a0 if call_offsets is None else call_offsets, np.int64)
    org = np.ascontiguousarray(np.asarray(origins, np.float64).reshape(-1, 3)[lo:hi])
    nvox = np.ascontiguousarray(nvox, np.int32)
    B, C = hi - lo, sigmas.shape[1]
    out = np.empty((B, int(np.prod(nvox)), C), np.float32)
    bx = None if box is None else np.ascontiguousarray(np.asarray(box, np.float32).reshape(-1, 3)[lo:hi])
    aff = None if affine is None else np.ascontiguousarray(np.asarray(affine, np.float64)[lo:hi])
    err, wide = ctypes.c_int(0), ctypes.c_int(0)
    st = lib().emu_voxelize_lattice_batch_topo(
        ctypes.c_int(n_items), _p(batch_offsets), _p(sigmas), ctypes.c_int(int(sig64)), ctypes.c_int(C), ctypes.c_int(lo), ctypes.c_int(B),
        _p(xyz), _p(offs), _p(org), _p(nvox), ctypes.c_double(1.0), _p(bx), ctypes.c_int(max_images), ctypes.c_int(tile_k), _p(aff),
        ctypes.c_int(prepass_mode), ctypes.c_int(tile_team), ctypes.c_int(tile_items), ctypes.c_int(direct), ctypes.c_int(exact_redo), _p(out),
        ctypes.byref(err), ctypes.byref(wide))
    if st != 0:
        raise RuntimeError(f"emu status {st}: {lib().emu_last_error().decode()}")
    return out, err.value, wide.value


def trace(n_items=30, item_atoms=5000, first_item=0, B=None, C=8, nvox=(24, 24, 24), pbc=0, max_images=1, prepass_mode=-1, tile_team=-1,
          tile_items=-1, direct=-1, exact_redo=0, wide_every=0, pipelining=0, calls=1):
    """(status, launch sequence) of a batch-handle call: run_lattice's host side on the recording backend"""
    B = n_items - first_item if B is None else B
    nv = np.ascontiguousarray(nvox, np.int32)
    st = lib().emu_trace_lattice_batch(ctypes.c_int(n_items), ctypes.c_longlong(item_atoms), ctypes.c_int(first_item), ctypes.c_int(B), ctypes.c_int(C),
                                       _p(nv), ctypes.c_int(pbc), ctypes.c_int(max_images), ctypes.c_int(prepass_mode), ctypes.c_int(tile_team),
                                       ctypes.c_int(tile_items), ctypes.c_int(direct), ctypes.c_int(exact_redo), ctypes.c_int(wide_every),
                                       ctypes.c_int(pipelining), ctypes.c_int(calls))
    return st, lib().emu_trace_text().decode()
