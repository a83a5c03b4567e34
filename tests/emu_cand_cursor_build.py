"""tests/emu_cand_cursor_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_cursor.so, the host
emulation of the product's kernels (tests/emu_build.py) with the walk of a given run table through the product's cand_issue
(tests/emu/emu_cand_cursor.cpp)."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_PATH = os.path.join(_EMU, "libmkamd_emu_cursor.so")
_lib = None

SURV_OFF_BITS = 10                     # kernels.h


def lib():
    global _lib
    if _lib is None:
        srcs = [os.path.join(_EMU, f) for f in ("emu_cand_cursor.cpp", "emu_capi.cpp", "emu_device.h")] + \
               [os.path.join(_CSRC, f) for f in ("kernels.h", "pipeline.h", "mk_diagnostics.h", "dist_kernels.h", "dist_pipeline.h", "xtc_gpu.h", "host_pack.h")]
        if not os.path.exists(_PATH) or any(os.path.getmtime(s) > os.path.getmtime(_PATH) for s in srcs):
            tmp = "%s.%d.tmp" % (_PATH, os.getpid())
            subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
                                   "-Wno-unknown-pragmas", "-ffp-contract=off", srcs[0], "-o", tmp, "-ldl"])
            os.replace(tmp, _PATH)
        _lib = ctypes.CDLL(_PATH)
        _lib.emu_last_error.restype = ctypes.c_char_p
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def walk(r0, length, rec_cls, first=0, stride=1, batch=1, search=None):
    """One wave through cand_issue over the 64 runs (r0[j], length[j]): chunks first, first + stride, ..., `batch` issued together;
    `search`: the per-chunk search instead of the cursor (default: as for_each_candidate decides, stride != 1).
    -> (valid bool [T, 64], record uint32 [T, 64], code uint32 [T, 64], class word uint32 [T, 64], visited bool [T], N, T, codable);
    rows of chunks this wave does not take stay 0xEEEEEEEE."""
    r0 = np.ascontiguousarray(r0, np.uint32); length = np.ascontiguousarray(length, np.uint32)
    rec_cls = np.ascontiguousarray(rec_cls, np.uint32)
    assert r0.shape == (64,) and length.shape == (64,)
    T = (int(length.sum()) + 63) // 64
    out = np.full((max(T, 1), 64, 4), 0xEEEEEEEE, np.uint32)
    meta = np.zeros(3, np.uint32)
    st = lib().emu_cand_cursor_walk(_p(r0), _p(length), _p(rec_cls), ctypes.c_longlong(len(rec_cls)), ctypes.c_uint(first), ctypes.c_uint(stride),
                                    ctypes.c_int(batch), ctypes.c_int(int(stride != 1 if search is None else search)), _p(out), _p(meta))
    assert st == 0
    out = out[:T]
    visited = (out[:, :, 0] != 0xEEEEEEEE).all(axis=1)
    return out[:, :, 0] == 1, out[:, :, 1], out[:, :, 2], out[:, :, 3], visited, int(meta[0]), int(meta[1]), bool(meta[2])

