"""tests/emu_cover_fold_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_cover[_mut].so, the host
emulation of the product's kernels (tests/emu_build.py) with the entry point of the cover fold (tests/emu/emu_cover_fold.cpp).  The
`mutant` library is the same source with -DMK_DIAG=128: channel 7 leaves the covered atoms out and nobody folds them back in."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_libs = {}


def lib(mutant=False):
    if mutant not in _libs:
        path = os.path.join(_EMU, "libmkamd_emu_cover_mut.so" if mutant else "libmkamd_emu_cover.so")
        srcs = [os.path.join(_EMU, f) for f in ("emu_cover_fold.cpp", "emu_capi.cpp", "emu_device.h")] + \
               [os.path.join(_CSRC, f) for f in ("kernels.h", "pipeline.h", "mk_diagnostics.h", "dist_kernels.h", "dist_pipeline.h", "xtc_gpu.h", "host_pack.h")]
        if not os.path.exists(path) or any(os.path.getmtime(s) > os.path.getmtime(path) for s in srcs):
            tmp = "%s.%d.tmp" % (path, os.getpid())
            knobs = ["-DMKAMD_DIAGNOSTICS_BUILD", "-DMK_DIAG=128"] if mutant else []
            subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
                                   "-Wno-unknown-pragmas", "-ffp-contract=off", *knobs, srcs[0], "-o", tmp, "-ldl"])
            os.replace(tmp, path)
        L = ctypes.CDLL(path)
        L.emu_last_error.restype = ctypes.c_char_p
        _libs[mutant] = L
    return _libs[mutant]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def voxelize(coords, offsets, sigmas, origins, nvox, lo=0, hi=None, frame_atoms=0, box=None, max_images=1, tile_k=0, tile_team=0, lds_tier=-1,
             cover_fold=0, mutant=False, run=True):
    """Batch handle (default; `offsets` the batch's, `sigmas` of all its atoms): its items [lo, hi).  Frame handle (`frame_atoms` > 0,
    `sigmas` [frame_atoms, C]): every item of `offsets` is one set of coordinates of that molecule.
    -> dict(out [B, V, C], err, masks [G], table uint32[16], feedback uint32[7]); run=False: the handle alone (no `out`)."""
    offsets = np.ascontiguousarray(offsets, np.int64)
    n_items = len(offsets) - 1
    hi = n_items if hi is None else hi
    a0, a1 = int(offsets[lo]), int(offsets[hi])
    sig64 = sigmas.dtype == np.float64
    sigmas = np.ascontiguousarray(sigmas, np.float64 if sig64 else np.float32)
    C = sigmas.shape[1]
    xyz = np.ascontiguousarray(np.asarray(coords, np.float32).reshape(-1, 3)[a0:a1])
    offs = np.ascontiguousarray(offsets[lo:hi + 1] - a0, np.int64)
    org = np.ascontiguousarray(np.asarray(origins, np.float64).reshape(-1, 3)[lo:hi])
    nvox = np.ascontiguousarray(nvox, np.int32)
    B = hi - lo
    out = np.empty((B, int(np.prod(nvox)), C), np.float32) if run else None
    bx = None if box is None else np.ascontiguousarray(np.asarray(box, np.float32).reshape(-1, 3)[lo:hi])
    err = ctypes.c_int(0)
    G = (C + 7) // 8
    masks, table, fb = np.zeros(G, np.uint32), np.zeros(16, np.uint32), np.zeros(7, np.uint32)
    L = lib(mutant)
    st = L.emu_cover_fold_voxelize(
        ctypes.c_int(n_items), _p(None if frame_atoms else offsets), ctypes.c_longlong(frame_atoms), _p(sigmas), ctypes.c_int(int(sig64)), ctypes.c_int(C),
        ctypes.c_int(lo), ctypes.c_int(B), _p(xyz), _p(offs), _p(org), _p(nvox), ctypes.c_double(1.0), _p(bx), ctypes.c_int(max_images),
        ctypes.c_int(tile_k), ctypes.c_int(tile_team), ctypes.c_int(lds_tier), ctypes.c_int(cover_fold), _p(out), ctypes.byref(err), _p(masks),
        _p(table), _p(fb))
    if st != 0:
        raise RuntimeError(f"emu status {st}: {L.emu_last_error().decode()}")
    return dict(out=out, err=err.value, masks=masks, table=table, feedback=fb)


def class_bit(table, sigma, voxelsize=1.0):
    """bit of the class of `sigma` in a cover mask: class id = 1 + its position in the handle's table of w = voxelsize^2 / sigma^2 bits"""
    w = np.float32(np.float64(voxelsize) ** 2 / np.float64(sigma) ** 2)
    hit = np.nonzero(np.asarray(table[:15], np.uint32) == w.view(np.uint32))[0]
    assert len(hit) == 1, (sigma, hit)
    return 1 << (int(hit[0]) + 1)
