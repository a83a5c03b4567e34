#!/usr/bin/env python3
"""Times the device DCD path (moleculekit_amd.dcd) on two workloads and prints one JSON line each:

    python3 tools/bench_dcd.py [--frames-scale 1.0] [--reps 5] [--cpu-frames 32]

  water     30 000 atoms x 2 048 frames (737 MB of float32)
  solvated  75 000 atoms x 256 frames

Random coordinates (the kernels move bit patterns: the values do not matter).  Reported, each as the median of ``--reps`` runs after one
warm-up:
  encode_ms / decode_ms   the two kernels alone (device events around the C ABI call, buffers allocated before), beside clone_ms,
                          ``torch.clone`` of the same [F, N, 3] tensor -- all three move every byte once in and once out;
  write_ms                ``write_dcd_dev`` to a file in a temporary directory, beside raw_d2h_ms, the device-to-host copy of the tensor
                          through pinned memory alone;
  read_ms                 ``read_dcd_frames_dev`` of that file, beside raw_h2d_ms, the pinned host-to-device copy of the same bytes alone;
  cpu_deinterleave_ms     a one-thread numpy restatement of the reference reader's per-frame copy (three planes into [N, 3]) over the first
                          ``--cpu-frames`` frames, scaled to all frames.
The file read back must give the tensor's bits."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def median_ms(fn, reps, dev, events=False):
    import torch
    times = []
    for _ in range(reps + 1):
        torch.cuda.synchronize(dev)
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        else:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            times.append(1e3 * (time.perf_counter() - t0))
    return round(float(np.median(times[1:])), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames-scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-frames", type=int, default=32)
    a = ap.parse_args()
    import torch
    from moleculekit_amd import _lib, dcd
    ctx = _lib.default_context()
    lib = _lib.load()
    dev = torch.device("cuda", ctx.device)
    for name, N, F in (("water", 30000, max(8, int(2048 * a.frames_scale))), ("solvated", 75000, max(4, int(256 * a.frames_scale)))):
        gen = torch.Generator(device=dev).manual_seed(7)
        xyz = torch.randn((F, N, 3), generator=gen, device=dev, dtype=torch.float32) * 30
        lengths = np.full((F, 3), 67.0, np.float32)
        angles = np.full((F, 3), 90.0, np.float32)
        res = {"workload": name, "atoms": N, "frames": F, "raw_MB": round(xyz.numel() * 4 / 1e6, 1)}
        stream = torch.cuda.current_stream(dev).cuda_stream or None
        res["clone_ms"] = median_ms(lambda: xyz.clone(), a.reps, dev, events=True)
        # the encode kernel alone
        bound = int(lib.mkamd_dcd_encode_bound(F, N, 1))
        image = torch.empty(bound, dtype=torch.uint8, device=dev)
        d_cell = torch.as_tensor(dcd.cell_records(lengths, angles, F), device=dev)
        res["encode_ms"] = median_ms(lambda: _lib._check(lib.mkamd_dcd_encode_dev(ctx._h, stream, xyz.data_ptr(), d_cell.data_ptr(), F, N,
                                                                                  image.data_ptr(), bound)), a.reps, dev, events=True)
        res["encode_over_clone"] = round(res["encode_ms"] / res["clone_ms"], 2)
        with tempfile.TemporaryDirectory() as tmp:
            fn = os.path.join(tmp, "out.dcd")
            res["write_ms"] = median_ms(lambda: dcd.write_dcd_dev(fn, xyz, lengths, angles, ctx=ctx), a.reps, dev)
            host = torch.empty(xyz.shape, dtype=torch.float32, pin_memory=True)
            res["raw_d2h_ms"] = median_ms(lambda: host.copy_(xyz, non_blocking=True), a.reps, dev)
            assert os.path.getsize(fn) == dcd.HEADER_BYTES + bound
            # the decode kernel alone, on the image that is already on the device (descriptors of the file just written)
            desc, lo, hi, _ = dcd.chunk_desc(fn, np.arange(F))
            assert hi - lo == bound
            sel, src = dcd.source_table(fn, None, N)
            d_desc, d_sel, d_src = (torch.as_tensor(v, device=dev) for v in (desc, sel, src))
            out = torch.empty_like(xyz)
            d_st = torch.empty(F, dtype=torch.int32, device=dev)
            res["decode_ms"] = median_ms(lambda: _lib._check(lib.mkamd_dcd_decode_dev(ctx._h, stream, image.data_ptr(), bound, d_desc.data_ptr(), F,
                                                                                      d_sel.data_ptr(), d_src.data_ptr(), N, None, N, 1.0,
                                                                                      out.data_ptr(), d_st.data_ptr())), a.reps, dev, events=True)
            res["decode_over_clone"] = round(res["decode_ms"] / res["clone_ms"], 2)
            assert not d_st.any().item() and torch.equal(out.view(torch.int32), xyz.view(torch.int32))
            del out, image
            # the whole read, beside the upload of the same bytes alone
            back = {}
            res["read_ms"] = median_ms(lambda: back.__setitem__("xyz", dcd.read_dcd_frames_dev(fn, ctx=ctx)[0]), a.reps, dev)
            assert torch.equal(back["xyz"].view(torch.int32), xyz.view(torch.int32)), "the file read back differs from the tensor written"
            back.clear()
            raw = torch.empty(bound, dtype=torch.uint8, pin_memory=True)
            d_raw = torch.empty(bound, dtype=torch.uint8, device=dev)
            res["raw_h2d_ms"] = median_ms(lambda: d_raw.copy_(raw, non_blocking=True), a.reps, dev)
            # one host thread: the reference reader's copy of three planes into [N, 3], frame by frame
            K = min(F, a.cpu_frames)
            blob = np.fromfile(fn, np.uint8, count=dcd.HEADER_BYTES + K * (bound // F))[dcd.HEADER_BYTES:].reshape(K, -1)
            dst = np.empty((K, N, 3), np.float32)
            t0 = time.perf_counter()
            for f in range(K):
                planes = blob[f, 56:].view(np.float32).reshape(3, N + 2)[:, 1:N + 1]
                for k in range(3):
                    dst[f, :, k] = planes[k]
            res["cpu_deinterleave_ms"] = round(1e3 * (time.perf_counter() - t0) / K * F, 1)
            assert np.array_equal(dst.view(np.uint32), host[:K].numpy().view(np.uint32))
        print(json.dumps(res), flush=True)
        del xyz, host, raw, d_raw


if __name__ == "__main__":
    main()
