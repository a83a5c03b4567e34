"""tests/emu_moments_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_moments.so.

The group-moment kernels (moleculekit_amd/csrc/moments_kernels.h) and their launch plans (moments_pipeline.h) compiled for the HOST on
the SIMT emulation of tests/emu/emu_device.h, with -ffp-contract=off, so that the CPU-only tier checks them against the numpy
restatement of the reference (tests/moments_restatement.py).  Never imported by the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_moments.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None
AVOID_OWNED, AVOID_SEGMENTED = 1, 2       # moments_pipeline.h: MOM_AVOID_*
MODES = {"center": 0, "gyration": 1, "spherical": 2}
LL = ctypes.c_longlong


def build(force=False):
    srcs = [os.path.join(_EMU, "emu_moments.cpp"), os.path.join(_EMU, "emu_device.h")] + \
           [os.path.join(_CSRC, h) for h in ("moments_kernels.h", "moments_pipeline.h", "align_kernels.h", "mk_affine.h", "pipeline.h", "kernels.h")]
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(
            ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
             "-Wno-unused-variable", "-Wno-unknown-pragmas", "-ffp-contract=off",
             os.path.join(_EMU, "emu_moments.cpp"), "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        L.emu_moments_last_error.restype = ctypes.c_char_p
        L.emu_moments_last_kernel.restype = ctypes.c_char_p
        L.emu_moments_last_workspace.restype = ctypes.c_longlong
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _csr(groups):
    atoms = np.ascontiguousarray(np.concatenate([np.asarray(g).reshape(-1) for g in groups]), np.uint32)
    offsets = np.zeros(len(groups) + 1, np.uint32)
    offsets[1:] = np.cumsum([np.asarray(g).size for g in groups])
    return atoms, offsets


def _inputs(xyz, weights, affine):
    xyz = np.ascontiguousarray(xyz, np.float32)
    if weights is not None:
        weights = np.ascontiguousarray(weights, np.float32)
    if affine is not None:
        affine = np.ascontiguousarray(affine, np.float64)
    return xyz, weights, affine


def group_moments(xyz, groups, weights=None, affine=None, out="center", avoid=0, cus=256):
    """xyz float32 [F, N, 3], groups a list of index arrays -> float32 [F, 3 G] / [F, G, 4] / [F, 3] by mode"""
    xyz, weights, affine = _inputs(xyz, weights, affine)
    atoms, offsets = _csr(groups)
    F, N, G = xyz.shape[0], xyz.shape[1], len(groups)
    mode = MODES[out] if isinstance(out, str) else int(out)
    shape = {0: (F, 3 * G), 1: (F, G, 4), 2: (F, 3)}.get(mode, (F, 3 * G))
    res = np.full(shape, -7.0, np.float32)
    st = lib().emu_group_moments(ctypes.c_int(cus), _p(xyz), LL(N), LL(F), _p(affine), _p(atoms), _p(offsets), _p(weights), LL(G),
                                 LL(atoms.size), ctypes.c_int(mode), _p(res), ctypes.c_int(avoid))
    if st:
        raise ValueError(f"emulated group-moment call failed ({st}): {lib().emu_moments_last_error().decode()}")
    return res


def fluctuation(xyz, atoms, ref=None, groups=None, affine=None, avoid=0, cus=256):
    """xyz float32 [F, N, 3], atoms [n_sel], groups None or a list of arrays of POSITIONS in atoms that tile 0 .. n_sel - 1 in order
    -> float64 [F, n_sel] / [F, G]"""
    xyz, _, affine = _inputs(xyz, None, affine)
    atoms = np.ascontiguousarray(atoms, np.uint32)
    offsets = None
    if groups is not None:
        offsets = np.zeros(len(groups) + 1, np.uint32)
        offsets[1:] = np.cumsum([len(g) for g in groups])
    if ref is not None:
        ref = np.ascontiguousarray(ref, np.float64)
    F, N, G = xyz.shape[0], xyz.shape[1], 0 if groups is None else len(groups)
    res = np.full((F, G if groups is not None else atoms.size), -7.0, np.float64)
    st = lib().emu_fluctuation(ctypes.c_int(cus), _p(xyz), LL(N), LL(F), _p(affine), _p(atoms), LL(atoms.size), _p(offsets), LL(G), _p(ref),
                               _p(res), ctypes.c_int(avoid))
    if st:
        raise ValueError(f"emulated fluctuation call failed ({st}): {lib().emu_moments_last_error().decode()}")
    return res


def plan(n_mean, n_max, n_items, cus=256, avoid=0):
    """(glog2, segs, seg_len, blocks_x) of moments_plan"""
    out = (ctypes.c_int * 4)()
    lib().emu_moments_plan(LL(n_mean), LL(n_max), LL(n_items), ctypes.c_int(cus), ctypes.c_int(avoid), out)
    return tuple(out)


def last_kernel():
    return lib().emu_moments_last_kernel().decode()


def last_workspace():
    return int(lib().emu_moments_last_workspace())
