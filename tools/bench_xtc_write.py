#!/usr/bin/env python3
"""Times the device XTC writer (moleculekit_amd.xtc.write_xtc_dev / encode_xtc_dev) on two workloads and prints one JSON line each:

    python3 tools/bench_xtc_write.py [--frames-scale 1.0] [--reps 3] [--ref-frames 128]

  water     30 000 water atoms x 2 048 frames
  solvated  a 75 000-atom system (a 4 998-atom chain in 70 002 water atoms) x 256 frames

built from the generators of tests/xtc_cases.py (a few generated frames, repeated on the device with a shift per frame).  Beside the
writer it reports the device->host copy of the raw float32 tensor through pinned memory (the floor any writer pays), the reference's
writer on one CPU thread over the first ``--ref-frames`` frames (through oracle/_ref/libxtcref.so when it is there, skipped otherwise)
and the compressed size of those frames against the reference's, which must be equal byte for byte.  Per-kernel times come from
running this tool under ``rocprofv3 --kernel-trace --stats``."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def workloads(scale):
    from tests import xtc_cases
    rng = np.random.default_rng(2025)
    w = xtc_cases.water(rng, nmol=10000, F=8)
    yield "water", w.coords, w.box, max(8, int(2048 * scale))
    sol = xtc_cases.water(rng, nmol=23334, F=4)
    chain = xtc_cases.dense_chain(rng, N=4998, F=4, spacing=0.15, origin=float(sol.box[0, 0, 0]) / 2)
    yield "solvated", np.concatenate([chain.coords, sol.coords], axis=1), sol.box, max(4, int(256 * scale))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref-frames", type=int, default=128)
    a = ap.parse_args()
    import torch
    from moleculekit_amd import _lib, xtc
    ctx = _lib.default_context()
    dev = torch.device("cuda", ctx.device)
    ref_lib = os.path.join(ROOT, "oracle", "_ref", "libxtcref.so")
    for name, coords, box, F in workloads(a.frames_scale):
        F0, N = coords.shape[:2]
        base = torch.as_tensor(coords).to(dev)
        idx = torch.arange(F, device=dev) % F0
        shift = (torch.arange(F, device=dev, dtype=torch.float32) // F0)[:, None, None] * torch.tensor([0.011, -0.007, 0.005], device=dev)
        xyz = (base[idx] + shift).contiguous()
        bx = np.ascontiguousarray(np.transpose(box[np.arange(F) % F0], (1, 2, 0)))
        t, s = np.arange(F, dtype=np.float32), np.arange(F, dtype=np.int32)
        torch.cuda.synchronize(dev)
        res = {"workload": name, "atoms": N, "frames": F, "raw_MB": round(xyz.numel() * 4 / 1e6, 1)}
        # encode alone
        chunk = xtc.default_chunk(N)
        times = []
        for _ in range(a.reps + 1):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            total = 0
            for lo in range(0, F, chunk):
                image, offsets, status = xtc.encode_xtc_dev(xyz[lo:lo + chunk], bx[:, :, lo:lo + chunk], t[lo:lo + chunk], s[lo:lo + chunk], ctx=ctx)
                assert not status.any()
                total += int(offsets[-1])
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - t0)
        res["encode_ms"] = round(1e3 * float(np.median(times[1:])), 2)
        res["xtc_MB"] = round(total / 1e6, 1)
        # the whole write
        with tempfile.TemporaryDirectory() as tmp:
            fn = os.path.join(tmp, "out.xtc")
            times = []
            for _ in range(a.reps + 1):
                t0 = time.perf_counter()
                xtc.write_xtc_dev(fn, xyz, bx, t, s, ctx=ctx)
                times.append(time.perf_counter() - t0)
            res["write_ms"] = round(1e3 * float(np.median(times[1:])), 2)
            assert os.path.getsize(fn) == total
            # the floor: the raw tensor to the host through pinned memory
            host = torch.empty(xyz.shape, dtype=torch.float32, pin_memory=True)
            times = []
            for _ in range(a.reps + 1):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                host.copy_(xyz, non_blocking=True)
                torch.cuda.synchronize(dev)
                times.append(time.perf_counter() - t0)
            res["raw_d2h_ms"] = round(1e3 * float(np.median(times[1:])), 2)
            # the reference's writer, one thread, on the first frames; its bytes against ours
            if os.path.exists(ref_lib):
                from oracle.xtcref import ref_write_xtc
                K = min(F, a.ref_frames)
                x = host[:K].numpy()
                rf = os.path.join(tmp, "ref.xtc")
                t0 = time.perf_counter()
                ref_write_xtc(rf, x, np.transpose(bx[:, :, :K], (2, 0, 1)), time=t[:K], step=s[:K])
                res["reference_ms_per_frame"] = round(1e3 * (time.perf_counter() - t0) / K, 3)
                res["reference_ms_all_frames"] = round(res["reference_ms_per_frame"] * F, 1)
                with open(rf, "rb") as f1, open(fn, "rb") as f2:
                    want = f1.read()
                    res["reference_bytes"] = len(want)
                    res["equal_to_reference"] = f2.read(len(want)) == want
                assert res["equal_to_reference"], "the device writer's bytes differ from the reference's"
        print(json.dumps(res), flush=True)
        del xyz, base, host


if __name__ == "__main__":
    main()
