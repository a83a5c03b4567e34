#!/usr/bin/env python3
"""Dihedral angles: the fused call (moleculekit_amd.dihedral.dihedral_trajectory, sin / cos) against the same computation composed of
torch operations on the device (gather, torch.linalg.cross, atan2, sin / cos) -- both on resident tensors, one process.

Shapes: (a) the real projection, 552 dihedrals x 200 frames; (b) 552 x 2 048; (c) all phi / psi / omega / chi of a 3 000-residue
system (about 3.4 per residue) x 2 048 frames; (d) 1 200 dihedrals x 1 frame.  Per shape: the kernel taken, the median time of each
route (events around the call, 3 warm-up calls, 20 timed calls, three rounds with the routes alternating, the median round), the
effective bandwidth of the fused call over the ALGORITHMIC bytes (unique atoms x 12 B x F read + the result written) and that as a
fraction of 8 TB/s.  (a) is asserted close to (b) before anything is timed.  `--mode` times another output mode of the fused call.

    python tools/bench_dihedral.py [--json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
PEAK = 8.0e12


def backbone_system(n_res, F, seed, chi_per_res=0.0):
    """a chain of n_res residues x 8 atoms (N, CA, C, O and four side-chain atoms): phi / psi (/ omega / chi) quads over it"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    steps = torch.randn(n_res * 8, 3, F, device="cuda", generator=g)
    coords = torch.cumsum(1.5 * steps / steps.norm(dim=1, keepdim=True), dim=0).contiguous()
    quads = []
    rng = np.random.default_rng(seed)
    for r in range(n_res):
        b, nb, pb = 8 * r, 8 * (r + 1), 8 * (r - 1)
        if r > 0:
            quads.append([pb + 2, b, b + 1, b + 2])                  # phi
        if r + 1 < n_res:
            quads.append([b, b + 1, b + 2, nb])                      # psi
            if chi_per_res:
                quads.append([b + 1, b + 2, nb, nb + 1])             # omega
        k = rng.poisson(chi_per_res) if chi_per_res else 0
        for c in range(min(k, 4)):
            quads.append([[b, b + 1, b + 4, b + 5], [b + 1, b + 4, b + 5, b + 6], [b + 4, b + 5, b + 6, b + 7], [b + 5, b + 6, b + 7, b + 3]][c])
    return coords, np.array(quads, np.int64)


def torch_composition(coords, q):
    """the reference's formula in torch operations on [4, 3, D, F] gathers; returns [F, 2 D] sin / cos interleaved"""
    import torch
    x = coords[q.reshape(-1)].reshape(q.shape[0], 4, 3, -1)
    r12, r23, r34 = x[:, 0] - x[:, 1], x[:, 1] - x[:, 2], x[:, 2] - x[:, 3]
    c1, c2 = torch.linalg.cross(r23, r34, dim=1), torch.linalg.cross(r12, r23, dim=1)
    p1 = (r12 * c1).sum(1) * (r23 * r23).sum(1).sqrt()
    p2 = (c1 * c2).sum(1)
    a = -torch.atan2(p1, p2)
    return torch.stack([torch.sin(a), torch.cos(a)], dim=1).reshape(-1, a.shape[1]).t().contiguous()


def timed(fn, calls=20, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--mode", default="sincos", choices=["sincos", "degrees", "radians", "terms"])
    ap.add_argument("--only", default="abcd")
    args = ap.parse_args()
    import torch
    from moleculekit_amd import _lib
    from moleculekit_amd.dihedral import dihedral_trajectory
    ctx = _lib.default_context()
    shapes = {"a": ("real projection 552 x 200", 277, 200, 0.0), "b": ("552 x 2 048", 277, 2048, 0.0),
              "c": ("3 000 residues, all phi/psi/omega/chi x 2 048", 3000, 2048, 1.4), "d": ("1 200 x 1", 601, 1, 0.0)}
    rows = []
    for key in args.only:
        label, n_res, F, chi = shapes[key]
        coords, quads = backbone_system(n_res, F, 17, chi)
        q = torch.as_tensor(quads, device="cuda")
        D = quads.shape[0]
        fused = lambda: dihedral_trajectory(coords, quads, out=args.mode, ctx=ctx)  # noqa: E731
        got = dihedral_trajectory(coords, quads, out="sincos", ctx=ctx)
        kernel = ctx.last_dist_kernel()
        want = torch_composition(coords, q)
        torch.cuda.synchronize()
        assert float((got - want).abs().max()) < 1e-3, float((got - want).abs().max())
        rounds = []
        for _ in range(3):
            rounds.append((timed(fused), timed(lambda: torch_composition(coords, q))))
        t_f, t_t = sorted(rounds)[1]
        width = {"sincos": 2, "terms": 2, "degrees": 1, "radians": 1}[args.mode]
        nbytes = np.unique(quads).size * 12 * F + F * D * width * 4
        bw = nbytes / (t_f * 1e-3)
        rows.append(dict(shape=key, label=label, D=D, F=F, mode=args.mode, kernel=kernel.replace("mkamd::", ""), fused_ms=t_f, torch_ms=t_t,
                         ratio=t_t / t_f, GBps=bw / 1e9, of_peak=bw / PEAK))
    if args.json:
        print(json.dumps(rows))
        return
    print("| shape | D x F | kernel | fused ms | torch ms | torch / fused | GB/s (algorithmic) | of 8 TB/s |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| ({r['shape']}) {r['label']} | {r['D']} x {r['F']} | {r['kernel']} | {r['fused_ms']:.4f} | {r['torch_ms']:.4f} | "
              f"{r['ratio']:.1f} | {r['GBps']:.0f} | {r['of_peak']:.3f} |")


if __name__ == "__main__":
    main()
