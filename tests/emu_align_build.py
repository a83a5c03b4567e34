"""tests/emu_align_build.py -- TEST INFRASTRUCTURE: build + ctypes front-end for tests/emu/libmkamd_emu_align.so.

The alignment kernels (moleculekit_amd/csrc/align_kernels.h) and their launch plans (align_pipeline.h) compiled for the HOST on the
SIMT emulation of tests/emu/emu_device.h, so that the CPU-only tier checks them against a float64 restatement.  Never imported by
the product.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = os.path.join(_EMU, "libmkamd_emu_align.so")
_CSRC = os.path.join(_HERE, "..", "moleculekit_amd", "csrc")
_lib = None


def build(force=False):
    srcs = [os.path.join(_EMU, "emu_align.cpp"), os.path.join(_EMU, "emu_device.h"), os.path.join(_CSRC, "align_kernels.h"),
            os.path.join(_CSRC, "align_pipeline.h"), os.path.join(_CSRC, "mk_affine.h"), os.path.join(_CSRC, "pipeline.h"),
            os.path.join(_CSRC, "kernels.h")]
    stale = (not os.path.exists(_LIB)) or any(os.path.getmtime(s) > os.path.getmtime(_LIB) for s in srcs)
    if force or stale:
        tmp = "%s.%d.tmp" % (_LIB, os.getpid())
        subprocess.check_call(
            ["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
             "-Wno-unused-variable", "-Wno-unknown-pragmas", "-ffp-contract=off",
             os.path.join(_EMU, "emu_align.cpp"), "-o", tmp])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = ctypes.CDLL(_LIB)
        L.emu_align_last_error.restype = ctypes.c_char_p
        L.emu_align_last_kernel.restype = ctypes.c_char_p
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _check(st):
    if st:
        raise RuntimeError(f"emulated alignment call failed ({st}): {lib().emu_align_last_error().decode()}")


def _inputs(xyz, ref, sel, refsel, frames):
    xyz = np.ascontiguousarray(xyz, np.float32)
    ref = np.ascontiguousarray(ref, np.float32)
    if ref.ndim == 2:
        ref = ref[None]
    sel = np.ascontiguousarray(sel, np.uint32)
    refsel = np.ascontiguousarray(refsel, np.uint32)
    fr = None if frames is None else np.ascontiguousarray(frames, np.int64)
    return xyz, ref, sel, refsel, fr


def transforms(xyz, ref, sel, refsel, frames=None, refframe=0, matching=False, cus=256):
    """xyz float32 [F,N,3], ref [Fr,Nr,3] (or [Nr,3]) -> (affine float64 [K,12], fit_rmsd float64 [K])"""
    xyz, ref, sel, refsel, fr = _inputs(xyz, ref, sel, refsel, frames)
    cus = 256 if cus is None else cus
    K = xyz.shape[0] if fr is None else len(fr)
    aff = np.full((K, 12), np.nan)
    rms = np.full(K, np.nan)
    _check(lib().emu_align_transforms(ctypes.c_int(cus), _p(xyz), ctypes.c_longlong(xyz.shape[1]), ctypes.c_longlong(xyz.shape[0]),
                                      _p(ref), ctypes.c_longlong(ref.shape[1]), ctypes.c_longlong(ref.shape[0]), _p(sel), _p(refsel),
                                      ctypes.c_longlong(len(sel)), _p(fr), ctypes.c_longlong(K), ctypes.c_longlong(refframe),
                                      ctypes.c_int(int(bool(matching))), _p(aff), _p(rms)))
    return aff, rms


def apply(xyz, affine, frames=None, out=None):
    """float32(M x + t) of every atom of the listed frames; returns `out` (a copy of xyz unless given; xyz itself: in place)"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    affine = np.ascontiguousarray(affine, np.float64)
    fr = None if frames is None else np.ascontiguousarray(frames, np.int64)
    K = xyz.shape[0] if fr is None else len(fr)
    if out is None:
        out = xyz.copy()
    _check(lib().emu_align_apply(_p(xyz), ctypes.c_longlong(xyz.shape[1]), _p(fr), ctypes.c_longlong(K), _p(affine), _p(out)))
    return out


def apply_raw(xyz_flat, n_atoms, affine, frames, out_flat):
    """the kernel on raw (possibly offset) buffers: xyz_flat / out_flat float32 1-D views"""
    fr = np.ascontiguousarray(frames, np.int64)
    _check(lib().emu_align_apply(_p(xyz_flat), ctypes.c_longlong(n_atoms), _p(fr), ctypes.c_longlong(len(fr)),
                                 _p(np.ascontiguousarray(affine, np.float64)), _p(out_flat)))


def apply_at(base, off_in, outbuf, off_out, n_atoms, n_frames, affine, frames):
    """tests/align_cases.py's driver call: the frames at base[off_in:] moved to outbuf[off_out:] (outbuf None: in place); returns the
    whole output buffer"""
    n = 3 * n_atoms * n_frames
    if outbuf is None:
        outbuf = base
    apply_raw(base[off_in:off_in + n], n_atoms, affine, frames, outbuf[off_out:off_out + n])
    return outbuf


def rmsd_trajectory(xyz, ref, alnsel, rmsdsel, frames=None):
    """align.rmsd_trajectory's sequence: the transforms over alnsel, then the RMSD over rmsdsel"""
    aff, _ = transforms(xyz, ref, alnsel, alnsel, frames=frames)
    return rmsd(xyz, ref, rmsdsel, rmsdsel, aff, frames=frames)


def rmsd(xyz, ref, sel, refsel, affine, frames=None, refframe=0, matching=False, cus=256):
    xyz, ref, sel, refsel, fr = _inputs(xyz, ref, sel, refsel, frames)
    K = xyz.shape[0] if fr is None else len(fr)
    out = np.full(K, np.nan, np.float32)
    _check(lib().emu_align_rmsd(ctypes.c_int(cus), _p(xyz), ctypes.c_longlong(xyz.shape[1]), ctypes.c_longlong(xyz.shape[0]), _p(ref),
                                ctypes.c_longlong(ref.shape[1]), ctypes.c_longlong(ref.shape[0]), _p(sel), _p(refsel),
                                ctypes.c_longlong(len(sel)), _p(fr), ctypes.c_longlong(K), ctypes.c_longlong(refframe),
                                ctypes.c_int(int(bool(matching))), _p(np.ascontiguousarray(affine, np.float64)), _p(out)))
    return out


def last_kernel():
    """The note of the last transforms / rmsd call (run_align_transforms / run_align_rmsd: ctx.last_dist_kernel() on the device)."""
    return lib().emu_align_last_kernel().decode()


def plan(n, n_items, cus=256):
    out = np.zeros(4, np.int32)
    lib().emu_align_plan(ctypes.c_longlong(n), ctypes.c_longlong(n_items), ctypes.c_int(cus), _p(out))
    return dict(glog2=int(out[0]), segs=int(out[1]), seg_len=int(out[2]), blocks_x=int(out[3]))
