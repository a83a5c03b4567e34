"""tests/emu_xtc_encode_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_xtc_encode.so, and the
build of the stand-alone sanitized driver tests/emu/xtc_encode_main.

The device XTC writer's kernels (moleculekit_amd/csrc/xtc_encode.h) and their launch plan compiled for the HOST on the SIMT emulation
of tests/emu/emu_device.h, with -ffp-contract=off, so that the CPU-only tier checks their bytes against the reference writer's
(tests/golden/xtc_reference/*.xtc).  Never imported by the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_xtc_encode.so")
_MAIN = os.path.join(_EMU, "xtc_encode_main")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None
_SRCS = [os.path.join(_EMU, "emu_xtc_encode.cpp"), os.path.join(_EMU, "emu_device.h"), os.path.join(_CSRC, "xtc_encode.h"),
         os.path.join(_CSRC, "xtc_gpu.h")]
_WARN = ["-Wall", "-Wno-unused-function", "-Wno-unused-variable", "-Wno-unknown-pragmas"]

PLAN_DTYPE = np.dtype([("lo", "<i4", 3), ("hi", "<i4", 3), ("size", "<u4", 3), ("bitsize", "<i4"), ("fieldbits", "<i4", 3), ("smallidx", "<i4"),
                       ("ngroups", "<i4"), ("nbits", "<u4")])          # mkamd::XtcEncPlan
assert PLAN_DTYPE.itemsize == 64
POISON = 0xCD
XE_ATOMS = 85                                                        # csrc/xtc_encode.h: whole atoms of a walk window


def _stale(target, srcs):
    return (not os.path.exists(target)) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in srcs)


def build(force=False):
    if force or _stale(_LIB, _SRCS):
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared"] + _WARN + ["-ffp-contract=off", _SRCS[0], "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def build_main(force=False):
    """The stand-alone driver (its own main), with AddressSanitizer and UBSan; run as a child process, nothing is preloaded."""
    src = os.path.join(_EMU, "xtc_encode_main.cpp")
    if force or _stale(_MAIN, _SRCS + [src]):
        tmp = "%s.%d.tmp" % (_MAIN, os.getpid())
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-fno-omit-frame-pointer"] + _WARN + ["-ffp-contract=off", src, "-o", tmp])
        os.replace(tmp, _MAIN)
    return _MAIN


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        L.emu_xtc_encode_work_bytes.restype = ctypes.c_uint64
        L.emu_xtc_encode_bound.restype = ctypes.c_uint64
        L.emu_xtc_encode_work_bytes.argtypes = L.emu_xtc_encode_bound.argtypes = [ctypes.c_longlong, ctypes.c_longlong]
        L.emu_xtc_encode_layout.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p]
        L.emu_xtc_encode.argtypes = [ctypes.c_void_p, ctypes.c_float] + [ctypes.c_void_p] * 4 + [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_void_p,
                                     ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def per_frame(v, F, dtype):
    a = np.asarray(v, dtype=dtype)
    return np.ascontiguousarray(np.broadcast_to(a, (F,)) if a.ndim == 0 else a.reshape(F))


def encode(coords, box=None, time=None, step=None, precision=1000.0, in_scale=1.0):
    """coords float32 [F, N, 3]; box [F, 3, 3] (zeros when None); time / step per frame (0..F-1 when None, as oracle.xtcref.ref_write_xtc);
    precision a scalar or one per frame -> dict(image uint8 [bound] (poisoned: what lies behind ``offsets[-1]`` must still be poison),
    offsets int64 [F + 1], status int32 [F], plan (PLAN_DTYPE [F]), groups uint32 [F, N, 3] (pos, first atom, meta)).
    Every output buffer goes in poisoned and has exactly the size the two size functions promise."""
    x = np.ascontiguousarray(coords, np.float32)
    F, N = x.shape[:2]
    box = np.zeros((F, 3, 3), np.float32) if box is None else np.ascontiguousarray(np.broadcast_to(np.asarray(box, np.float32), (F, 3, 3)))
    time = per_frame(np.arange(F) if time is None else time, F, np.float32)
    step = per_frame(np.arange(F) if step is None else step, F, np.int32)
    prec = per_frame(precision, F, np.float32)
    L = lib()
    bound, wb = int(L.emu_xtc_encode_bound(F, N)), int(L.emu_xtc_encode_work_bytes(F, N))
    image = np.full(bound, POISON, np.uint8)
    work = np.full(wb // 8 + 1, 0xCDCDCDCDCDCDCDCD, np.uint64).view(np.uint8)[:wb]
    offsets = np.full(F + 1, 0xCDCDCDCDCDCDCDCD, np.uint64)
    status = np.full(F, -7, np.int32)
    st = L.emu_xtc_encode(_p(x), ctypes.c_float(in_scale), _p(prec), _p(box), _p(time), _p(step), F, N, _p(image), bound, _p(offsets), _p(status),
                          _p(work), wb)
    if st:
        raise ValueError(f"emulated encode call failed ({st})")
    lay = np.zeros(5, np.uint64)
    L.emu_xtc_encode_layout(F, N, _p(lay))
    lay = [int(v) for v in lay]
    plan = work[lay[2]:lay[2] + 64 * F].view(PLAN_DTYPE).copy()
    walked = 9 < N < (1 << 21)
    groups = work[lay[3]:lay[3] + 12 * F * N].view(np.uint32).reshape(F, N, 3).copy() if walked else np.zeros((F, N, 3), np.uint32)
    return dict(image=image, offsets=offsets.astype(np.int64), status=status, plan=plan, groups=groups)


def records(out):
    """The image's bytes up to the last record's end, after checking that nothing behind it was touched."""
    total = int(out["offsets"][-1])
    assert (out["image"][total:] == POISON).all(), "the image was written behind the last record"
    return out["image"][:total].tobytes()


def reach(out):
    """What the walk reached in the frames it planned, from its group records."""
    r = dict(max_small=0, swaps=0, idx_lo=99, idx_hi=0, up=0, down=0, flagged=0, unflagged=0, windows=0)
    for f in range(len(out["status"])):
        n = int(out["plan"]["ngroups"][f])
        if out["status"][f] != 0 or n == 0:
            continue
        g = out["groups"][f, :n].astype(np.int64)
        meta = g[:, 2]
        sidx, ns, swap, fv = meta & 0xff, (meta >> 8) & 15, (meta >> 12) & 1, (meta >> 16) & 0xff
        r["max_small"] = max(r["max_small"], int(ns.max()))
        r["swaps"] += int(swap.sum())
        r["idx_lo"], r["idx_hi"] = min(r["idx_lo"], int(sidx.min())), max(r["idx_hi"], int(sidx.max()))
        r["up"] += int(np.count_nonzero(np.diff(sidx) == 1))
        r["down"] += int(np.count_nonzero(np.diff(sidx) == -1))
        r["flagged"] += int(np.count_nonzero(fv != 0xff))
        r["unflagged"] += int(np.count_nonzero(fv == 0xff))
        r["windows"] = max(r["windows"], 1 + int(g[-1, 1]) // XE_ATOMS)   # (a lower bound: a window starts at a group's first atom)
    return r
