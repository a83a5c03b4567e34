#!/usr/bin/env python3
"""Group moments: the fused call (moleculekit_amd.moments, the affine applied in registers) against the composition it replaces on the
same device in the same process: align.align_trajectory (the whole aligned trajectory written), then index_select of the selected
atoms, then torch segment sums -- all on resident tensors.

Shapes, 30 000 atoms x 2 048 frames unless said otherwise: (a) the coordinates of a 3 000-atom C-alpha selection, one group per atom;
(b) the centres of mass of 3 000 residues x 10 atoms; (c) the radius of gyration of one 30 000-atom group; (d) the MetricFluctuation
shape, 4 507 atoms x 200 frames, 277 atoms, from host arrays (the composition: the reference's order of work with align._pp_align on
the whole array); (e) / (f) the few-frames end: (b) on 1 and on 16 frames.  Per shape: the kernels taken, the median time of each
route (events around the call, 3 warm-up calls, 20 timed calls, three rounds with the routes alternating, the median round).  The
two routes are asserted close before anything is timed.

    python tools/bench_moments.py [--json] [--only abcdef]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, calls=20, warmup=3, host=False):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        if host:
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
            continue
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def segment_moments(moved, d_atoms, d_seg, d_w, G, gyration):
    """torch: weighted centres (and radii of gyration) of the groups from an ALIGNED trajectory"""
    import torch
    x = moved.index_select(1, d_atoms).double()
    w = d_w.double()[None, :, None]
    wsum = torch.zeros(G, dtype=torch.float64, device=x.device).index_add_(0, d_seg, d_w.double())
    com = torch.zeros((x.shape[0], G, 3), dtype=torch.float64, device=x.device).index_add_(1, d_seg, x * w) / wsum[None, :, None]
    if not gyration:
        return com.permute(0, 2, 1).reshape(x.shape[0], 3 * G).float()
    sq = (x - com.index_select(1, d_seg)) ** 2 * w
    m = torch.zeros((x.shape[0], G, 3), dtype=torch.float64, device=x.device).index_add_(1, d_seg, sq) / wsum[None, :, None]
    return torch.stack([m.sum(2), m[:, :, 1] + m[:, :, 2], m[:, :, 0] + m[:, :, 2], m[:, :, 0] + m[:, :, 1]], dim=2).sqrt().float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--only", default="abcdef")
    args = ap.parse_args()
    import torch
    from moleculekit_amd import _lib, align, moments
    ctx = _lib.default_context()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    shapes = {"a": ("3 000 CA coordinates", 30000, 2048, 3000, 1, "center"), "b": ("3 000 residues x 10 atoms COM", 30000, 2048, 3000, 10, "center"),
              "c": ("one 30 000-atom gyration group", 30000, 2048, 1, 30000, "gyration"), "d": ("MetricFluctuation 4 507 x 200, host arrays", 4507, 200, 277, 1, "fluct"),
              "e": ("(b) on 1 frame", 30000, 1, 3000, 10, "center"), "f": ("(b) on 16 frames", 30000, 16, 3000, 10, "center")}
    rows = []
    for key in args.only:
        label, N, F, G, size, out = shapes[key]
        g = torch.Generator(device="cuda").manual_seed(17)
        base = torch.rand(N, 3, device=dev, generator=g) * 60
        xyz = (base[None] + 0.5 * torch.randn(F, N, 3, device=dev, generator=g)).contiguous()
        sel = np.sort(rng.choice(N, size=min(3000, N // 2), replace=False))
        ref = base[torch.as_tensor(sel, device=dev)].contiguous()
        refsel = np.arange(sel.size)
        groups = [np.arange(N)] if size == N else [np.sort(rng.choice(N, size=size, replace=False)) for _ in range(G)]
        atoms = np.concatenate(groups)
        csr = (atoms, np.r_[0, np.cumsum([g_.size for g_ in groups])])      # built once: a list of arrays is checked array by array on every call
        w = rng.uniform(1, 32, size=atoms.size).astype(np.float32)
        d_atoms = torch.as_tensor(atoms, device=dev)
        d_seg = torch.as_tensor(np.repeat(np.arange(G), [g_.size for g_ in groups]), device=dev)
        d_w = torch.as_tensor(w, device=dev)
        if out == "fluct":
            coords = np.ascontiguousarray(xyz.cpu().numpy().transpose(1, 2, 0))
            refpos = ref.cpu().numpy()

            def fused():
                return moments.fluctuation(coords, atoms, align=(sel, refpos), ctx=ctx)

            def composed():
                moved = align._pp_align(coords, refpos[:, :, None], sel, refsel, np.arange(F), 0, False, ctx=ctx)[atoms]
                return ((moved - moved.mean(axis=2, keepdims=True)) ** 2).sum(axis=1).T.astype(np.float64)
            close, host = 1e-3, True
        else:
            def fused():
                aff, _ = align.kabsch_transforms(xyz, ref, sel, refsel, ctx=ctx)
                return moments.group_moments_trajectory(xyz, csr, weights=w, affine=aff, out=out, ctx=ctx)

            def composed():
                return segment_moments(align.align_trajectory(xyz, ref, sel, refsel, ctx=ctx), d_atoms, d_seg, d_w, G, out == "gyration")
            close, host = 1e-3, False
        got, want = fused(), composed()
        kernel = ctx.last_dist_kernel()
        torch.cuda.synchronize()
        err = float(np.abs(np.asarray(got.cpu() if hasattr(got, "cpu") else got) - np.asarray(want.cpu() if hasattr(want, "cpu") else want)).max())
        assert err < close, err
        rounds = sorted((timed(fused, host=host), timed(composed, host=host)) for _ in range(3))
        t_f, t_c = rounds[1]
        rows.append(dict(shape=key, label=label, N=N, F=F, G=G, kernel=kernel.replace("mkamd::", ""), fused_ms=t_f, composed_ms=t_c, ratio=t_c / t_f))
        del xyz
    if args.json:
        print(json.dumps(rows))
        return
    print("| shape | N x F, groups | kernel | fused ms | composition ms | composition / fused |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| ({r['shape']}) {r['label']} | {r['N']} x {r['F']}, {r['G']} | {r['kernel']} | {r['fused_ms']:.4f} | {r['composed_ms']:.4f} | {r['ratio']:.1f} |")


if __name__ == "__main__":
    main()
