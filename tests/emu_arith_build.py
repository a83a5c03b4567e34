"""tests/emu_arith_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_arith.so.

The arithmetic probe kernels (moleculekit_amd/csrc/arith_probe.h) compiled for the HOST on the SIMT emulation of tests/emu/emu_device.h,
with -ffp-contract=off: the CPU-only tier runs the cases of tests/arith_cases.py through them, which proves the vectors, the references
and the emulator's replacements of the device primitives.  ``probe`` has the signature of ``Context.arith_probe``.  Never imported by
the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_arith.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None
LL = ctypes.c_longlong


def build(force=False):
    srcs = [os.path.join(_EMU, "emu_arith.cpp"), os.path.join(_EMU, "emu_device.h")] + \
           [os.path.join(_CSRC, h) for h in ("arith_probe.h", "dist_kernels.h", "ring_kernels.h", "dihedral_kernels.h", "wrap_kernels.h",
                                             "wrap_cell_kernels.h")]
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(
            ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
             "-Wno-unused-variable", "-Wno-unknown-pragmas", "-ffp-contract=off",
             os.path.join(_EMU, "emu_arith.cpp"), "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        L.emu_arith_last_error.restype = ctypes.c_char_p
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def n_ops():
    return int(lib().emu_arith_nops())


def arity(code):
    return int(lib().emu_arith_arity(ctypes.c_int(code)))


def probe(op, a, b=None, c=None):
    """``Context.arith_probe`` on the emulation: the same operations, dtypes, shapes and sentinel"""
    from moleculekit_amd._lib import ARITH_OPS
    code, n_in, in_dt, out_dt, cols = ARITH_OPS[op]
    ins = [np.ascontiguousarray(x, in_dt).ravel() for x in (a, b, c)[:n_in]]
    assert all(x is None for x in (a, b, c)[n_in:]) and all(x.size == ins[0].size for x in ins)
    n = ins[0].size
    out = np.full(n * cols * np.dtype(out_dt).itemsize, 0xA5, np.uint8).view(out_dt)
    ins += [None] * (3 - n_in)
    st = lib().emu_arith_probe(ctypes.c_int(code), LL(n), _p(ins[0]), _p(ins[1]), _p(ins[2]), _p(out))
    if st:
        raise ValueError(f"emulated arithmetic probe failed ({st}): {lib().emu_arith_last_error().decode()}")
    return out.reshape(n, cols) if cols > 1 else out


def libm_acosf(x):
    """the host C library's acosf of a float32 array"""
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    lib().emu_arith_libm_acosf(LL(x.size), _p(x), _p(out))
    return out
