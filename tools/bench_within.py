"""tools/bench_within.py -- time the fused proximity selection (moleculekit_amd.within.within_trajectory) beside the two compositions a
user has without it, and sweep the two launch plans of one frame over n1 x n2, which is what the plan's constant is read from
(DESIGN.md section 18).

    python tools/bench_within.py [--reps 10] [--warmup 2] [--out results.json] [--only NAME] [--no-sweep]

Shapes (cutoff 5 A): 3PTB around its ligand (1 639 atoms, tests/golden/channels_3ptb.npz); 100 000 atoms at water density around a
3 000-atom solute (the atoms nearest the middle of the box), one frame; the same over 256 resident frames (each the first frame
jittered by 0.5 A); 1 000 000 atoms around 100 000, one frame.

The compositions, on the same device and the same resident tensors:
  contacts   the package's own contact list at the same cutoff (Context.contacts_trajectory_dev, non-periodic), its first column
             scattered into a mask: "any" over the list.  Its threshold is <=, not <, and it takes at most 2^32 pairs a call: it is the
             yardstick for what the existing kernels cost, timed where the shape fits
  cdist      (torch.cdist(queries, sources) < cutoff).any(-1), in chunks of at most 2^28 matrix elements, a frame at a time
Neither is bit-exact against the reference; only the NUMBER of selected atoms is printed beside the fused call's.

The sweep: 1 000 000 atoms at water density, one frame; the sources the n2 atoms nearest the middle, the queries a random subset of n1;
each (n1, n2) timed with the all-pairs kernel forced and with the cell list forced.

Device calls are timed with a host clock around work that ends in a device synchronise, alternating, after a warm-up of every variant;
the median and the spread (min .. max) of ``--reps`` repetitions are reported, one JSON line per shape.  Needs a GPU: no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CUTOFF = 5.0
DENSITY = 0.1                                                         # atoms per cubic angstrom


def ptb():
    d = np.load(os.path.join(ROOT, "tests", "golden", "channels_3ptb.npz"))
    xyz = d["coords"].astype(np.float32)
    return xyz[None], np.arange(len(xyz)), np.flatnonzero(d["resname"] == "BEN")


def solvated(n_atoms, n_solute, frames=1, seed=0):
    rng = np.random.default_rng(seed)
    side = (n_atoms / DENSITY) ** (1.0 / 3.0)
    xyz = (rng.random((n_atoms, 3)) * side).astype(np.float32)
    solute = np.argsort(np.linalg.norm(xyz - side / 2, axis=1))[:n_solute]
    xyz = xyz[None] if frames == 1 else xyz[None] + rng.standard_normal((frames, n_atoms, 3), dtype=np.float32) * np.float32(0.5)
    return xyz, np.arange(n_atoms), np.sort(solute)


def timed(fns, warmup, reps):
    counts = {}
    for _ in range(warmup):
        for key, fn in fns:
            counts[key] = fn()
    t = {k: [] for k, _ in fns}
    for _ in range(reps):                                              # alternating: all see the same neighbours on the machine
        for key, fn in fns:
            t0 = time.perf_counter()
            fn()
            t[key].append((time.perf_counter() - t0) * 1e3)
    return counts, t


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(np.min(ts)), 4), "max_ms": round(float(np.max(ts)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="one shape by name")
    ap.add_argument("--no-sweep", action="store_true", help="skip the plan sweep over n1 x n2")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_within: no GPU visible (there is no CPU fallback)")
    from moleculekit_amd import _lib
    from moleculekit_amd import within as W

    ctx = _lib.default_context(0)
    copy = _lib.load().mkamd_copy_dev
    shapes = [("3ptb_ligand", ptb), ("solvated_100k_x_3k", lambda: solvated(100000, 3000)),
              ("solvated_100k_x_3k_256_frames", lambda: solvated(100000, 3000, frames=256)), ("solvated_1m_x_100k", lambda: solvated(1000000, 100000))]
    results = []
    for name, make in shapes:
        if args.only and args.only != name:
            continue
        xyz, sel1, sel2 = make()
        F, N = xyz.shape[0], xyz.shape[1]
        n1, n2 = len(sel1), len(sel2)
        d_xyz = torch.as_tensor(xyz, device="cuda")
        d1, d2 = torch.as_tensor(sel1.astype(np.int64), device="cuda"), torch.as_tensor(sel2.astype(np.int64), device="cuda")

        def fused():
            out = W.within_trajectory(d_xyz, d1, d2, CUTOFF, ctx=ctx)
            torch.cuda.synchronize()
            return int(out.sum())

        fns = [("fused", fused)]
        if n1 * n2 < 2 ** 32:
            d_nf = d_xyz.permute(1, 2, 0).contiguous()                # [N, 3, F]: the layout of the distance calls
            d_box = torch.zeros((3, F), dtype=torch.float32, device="cuda")
            d_chains = torch.zeros(N, dtype=torch.int32, device="cuda")
            u1, u2 = d1.to(torch.int32), d2.to(torch.int32)

            def contacts():
                ctx.set_stream(torch.cuda.current_stream().cuda_stream)
                try:
                    offs, ptr, n = ctx.contacts_trajectory_dev(d_nf, F, d_box, u1, n1, u2, n2, d_chains, False, False, CUTOFF)
                    mask = torch.zeros((F, N), dtype=torch.bool, device="cuda")
                    if n:
                        pairs = torch.empty((n, 2), dtype=torch.int32, device="cuda")
                        _lib._check(copy(ctx._h, pairs.data_ptr(), ptr, n * 8))
                        ctx.synchronize()
                        frame = torch.repeat_interleave(torch.arange(F, device="cuda"), torch.as_tensor(np.diff(offs), device="cuda"))
                        mask[frame, pairs[:, 0].long()] = True
                finally:
                    ctx.set_stream(None)
                torch.cuda.synchronize()
                return int(mask.sum())

            fns.append(("contacts", contacts))

        def cdist():
            total = 0
            step = max(1, 2 ** 28 // n2)
            for f in range(F):
                s = d_xyz[f][d2]
                for a in range(0, n1, step):
                    total += int((torch.cdist(d_xyz[f][d1[a:a + step]], s) < CUTOFF).any(-1).sum())
            torch.cuda.synchronize()
            return total

        fns.append(("cdist", cdist))
        counts, t = timed(fns, args.warmup, args.reps)
        row = {"shape": name, "frames": F, "n1": n1, "n2": n2, "selected": counts}
        for key, _ in fns:
            row[key] = stats(t[key])
        fused()
        row["kernel"] = ctx.last_dist_kernel()
        results.append(row)
        print(json.dumps(row), flush=True)
        del d_xyz

    if not args.no_sweep and not args.only:
        xyz, _, _ = solvated(1000000, 1)
        side = (1000000 / DENSITY) ** (1.0 / 3.0)
        near = np.argsort(np.linalg.norm(xyz[0] - side / 2, axis=1))
        d_xyz = torch.as_tensor(xyz, device="cuda")
        rng = np.random.default_rng(1)
        for n2 in (256, 1024, 4096, 16384, 65536):
            d2 = torch.as_tensor(np.sort(near[:n2]).astype(np.int64), device="cuda")
            for n1 in (4096, 16384, 65536, 262144, 1000000):
                d1 = torch.as_tensor(np.sort(rng.choice(1000000, n1, replace=False)).astype(np.int64), device="cuda")

                def run(avoid):
                    def fn():
                        ctx.set_within_plan(avoid)
                        try:
                            out = W.within_trajectory(d_xyz, d1, d2, CUTOFF, ctx=ctx)
                            torch.cuda.synchronize()
                        finally:
                            ctx.set_within_plan(0)
                        return int(out.sum())
                    return fn

                counts, t = timed([("pairs", run(W.AVOID_CELLS)), ("cells", run(W.AVOID_PAIRS))], args.warmup, args.reps)
                assert counts["pairs"] == counts["cells"]
                row = {"sweep": True, "n1": n1, "n2": n2, "pairs_log2": round(float(np.log2(n1 * n2)), 1), "selected": counts["pairs"],
                       "pairs": stats(t["pairs"]), "cells": stats(t["cells"])}
                results.append(row)
                print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
