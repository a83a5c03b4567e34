"""tests/emu_survivor_regs_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_surv[_mut].so, the host
emulation of the product's kernels with the receiver of MK_SURV_PROBE (tests/emu/emu_survivor_regs.cpp): what every tile of the
one-wave tile kernels counted and kept.  The `mutant` library is the same source with -DMK_DIAG=256: the placement pass reads the kept
x-reach of survivor register 1 for register 0."""
from __future__ import annotations

import ctypes
import os
import subprocess
from unittest import mock

import numpy as np

from tests import emu_cover_fold_build as EC

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_libs = {}


def lib(mutant=False):
    if mutant not in _libs:
        path = os.path.join(_EMU, "libmkamd_emu_surv_mut.so" if mutant else "libmkamd_emu_surv.so")
        srcs = [os.path.join(_EMU, f) for f in ("emu_survivor_regs.cpp", "emu_cover_fold.cpp", "emu_capi.cpp", "emu_device.h")] + \
               [os.path.join(_CSRC, f) for f in ("kernels.h", "pipeline.h", "mk_diagnostics.h", "dist_kernels.h", "dist_pipeline.h", "xtc_gpu.h", "host_pack.h")]
        if not os.path.exists(path) or any(os.path.getmtime(s) > os.path.getmtime(path) for s in srcs):
            tmp = "%s.%d.tmp" % (path, os.getpid())
            knobs = ["-DMKAMD_DIAGNOSTICS_BUILD", "-DMK_SURV_PROBE"] + (["-DMK_DIAG=256"] if mutant else [])
            subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unused-variable",
                                   "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized", "-ffp-contract=off", *knobs, srcs[0], "-o", tmp, "-ldl"])
            os.replace(tmp, path)
        L = ctypes.CDLL(path)
        L.emu_last_error.restype = ctypes.c_char_p
        _libs[mutant] = L
    return _libs[mutant]


def voxelize(*args, mutant=False, **kw):
    """tests/emu_cover_fold_build.voxelize through this library -> its dict plus `tiles`: uint32 rows of (tile of the launch, channel
    group, candidates N, survivors the cull pass counted, 1 = took the survivor list, x-reach values seen: bit 3 j + xr for register j),
    one row per tile of the one-wave tile kernels (a tile that never entered the cull pass, N <= 256, reports 0 survivors)."""
    L = lib(mutant)
    L.emu_surv_probe_reset()
    with mock.patch.object(EC, "lib", lambda mutant=False: L):    # the same entry point and argument packing, from this library
        r = EC.voxelize(*args, **kw)
    rows = np.zeros((L.emu_surv_probe_count(), 6), np.uint32)
    if len(rows):
        L.emu_surv_probe_read(rows.ctypes.data_as(ctypes.c_void_p))
    r["tiles"] = rows
    return r
