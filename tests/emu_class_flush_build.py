"""tests/emu_class_flush_build.py -- TEST INFRASTRUCTURE: build + front-end for tests/emu/libmkamd_emu_flush_mut.so, the host emulation
of the product's kernels (tests/emu/emu_cover_fold.cpp, which carries the plain entry points of tests/emu/emu_capi.cpp too) compiled
with -DMK_DIAG=512: mk_min_bits_where (csrc/kernels.h), the masked minimum of the class flush, ignores the cutoff there.  The
unmutated kernels are the libraries of tests/emu_build.py and tests/emu_cover_fold_build.py."""
from __future__ import annotations

import ctypes
import os
import subprocess
from unittest import mock

from tests import emu_build as E
from tests import emu_cover_fold_build as EC

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None


def lib():
    global _lib
    if _lib is None:
        path = os.path.join(_EMU, "libmkamd_emu_flush_mut.so")
        srcs = [os.path.join(_EMU, f) for f in ("emu_cover_fold.cpp", "emu_capi.cpp", "emu_device.h")] + \
               [os.path.join(_CSRC, f) for f in ("kernels.h", "pipeline.h", "mk_diagnostics.h", "dist_kernels.h", "dist_pipeline.h", "xtc_gpu.h", "host_pack.h")]
        if not os.path.exists(path) or any(os.path.getmtime(s) > os.path.getmtime(path) for s in srcs):
            tmp = "%s.%d.tmp" % (path, os.getpid())
            subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
                                   "-Wno-unknown-pragmas", "-ffp-contract=off", "-DMKAMD_DIAGNOSTICS_BUILD", "-DMK_DIAG=512", srcs[0], "-o", tmp, "-ldl"])
            os.replace(tmp, path)
        L = ctypes.CDLL(path)
        L.emu_last_error.restype = ctypes.c_char_p
        L.emu_last_dist_kernel.restype = ctypes.c_char_p
        L.emu_trace_text.restype = ctypes.c_char_p
        _lib = L
    return _lib


def mutant_handle(*args, **kw):
    """tests/emu_cover_fold_build.voxelize (the handle call) through the mutated kernels"""
    L = lib()
    with mock.patch.object(EC, "lib", lambda mutant=False: L):
        return EC.voxelize(*args, **kw)


def mutant_plain(*args, **kw):
    """tests/emu_build.voxelize_lattice (the plain call) through the mutated kernels"""
    L = lib()
    with mock.patch.object(E, "lib", lambda: L):
        return E.voxelize_lattice(*args, **kw)
